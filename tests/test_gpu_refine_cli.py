"""-m gpu: `leann search --refine <FETCH_K> [--refine-rows hbm|host]` through the C++ host CLI, on an int8 index whose exact rows
`leann build --recompute` left beside it as documents.embeddings."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "leann")
N, D, K, FETCH = 400, 96, 8, 20
TOPICS = ["rust ownership borrow checker lifetimes", "python asyncio event loop coroutine", "vector database embedding search",
          "graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]


def _run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory, gpu):
    d = tmp_path_factory.mktemp("cli_refine")
    docs = [dict(id=str(i + 1), text=f"passage {i} about {TOPICS[i % len(TOPICS)]} number {i * 7919 % 1000}", metadata=dict(lines=i))
            for i in range(N)]
    (d / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))
    common = ["--passages-jsonl", str(d / "docs.jsonl"), "--dimensions", str(D), "--graph-degree", "16", "--complexity", "64", "--row-type", "int8"]
    r = _run("build", "--index-dir", str(d / "with"), *common, "--recompute")
    assert r.returncode == 0 and "int8 rows" in r.stdout, r.stderr
    assert os.path.getsize(d / "with" / "documents.embeddings") == N * D * 4
    r = _run("build", "--index-dir", str(d / "without"), *common)
    assert r.returncode == 0 and not (d / "without" / "documents.embeddings").exists(), r.stderr
    rng = np.random.default_rng(3)
    Q = rng.standard_normal((3, D)).astype(np.float32)
    Q /= np.linalg.norm(Q, axis=1, keepdims=True)
    Q[0].tofile(d / "q.f32")
    (d / "queries.txt").write_text("gpu kernel wavefront bandwidth of the lds\nrust lifetimes and the borrow checker\n")
    return d


def _search(index_dir, *extra):
    return _run("search", "any text", "-i", str(index_dir), "--top-k", str(K), "--format", "json", "--auto-hybrid", "false", *extra)


def test_refined_search_prints_the_f32_distances(la, po, dirs):
    qfile = ["--query-vector-file", str(dirs / "q.f32")]
    host = _search(dirs / "with", *qfile, "--refine", str(FETCH))  # --refine-rows defaults to host
    assert host.returncode == 0, host.stderr
    hbm = _search(dirs / "with", *qfile, "--refine", str(FETCH), "--refine-rows", "hbm")
    host2 = _search(dirs / "with", *qfile, "--refine", str(FETCH), "--refine-rows", "host")
    assert hbm.returncode == 0 and host2.returncode == 0, hbm.stderr + host2.stderr
    assert host.stdout.encode() == hbm.stdout.encode() == host2.stdout.encode()  # identical bytes, wherever the rows are
    res = json.loads(host.stdout)
    assert len(res) == K
    # the Python refined call on the same files returns the same ids and the scores printed are its distances
    s = la.HnswSearcher.load(str(dirs / "with" / "documents.leann"), D)
    assert s.row_type() == la.RowType.I8
    rows = la.ExactRows.open(dirs / "with" / "documents.embeddings", D, placement="host")
    assert rows.len() == N
    q = np.fromfile(dirs / "q.f32", np.float32)
    keys, dists, counts = s.search_refined_batch(q[None, :], K, FETCH, 64, rows)  # 64: the CLI's default complexity
    assert counts[0] == K and [int(x["id"]) - 1 for x in res] == [int(k) for k in keys[0]]
    assert np.array([x["score"] for x in res], np.float32).tobytes() == dists[0].tobytes()
    # ... which are the exact rows' distances, not the int8 rows'
    emb = np.fromfile(dirs / "with" / "documents.embeddings", np.float32).reshape(N, D)
    assert all(np.float32(x["score"]) == po.dist_canon(q, emb[int(x["id"]) - 1]) for x in res)
    plain = json.loads(_search(dirs / "with", *qfile).stdout)
    assert [x["score"] for x in plain] != [x["score"] for x in res]
    rows.close()
    s.close()
    # a fetch_k below top_k is raised to it; a filter acts after the refined search
    r = _search(dirs / "with", *qfile, "--refine", "1")
    assert r.returncode == 0 and len(json.loads(r.stdout)) == K
    r = _search(dirs / "with", *qfile, "--refine", str(FETCH), "--filter", "lines>=200")
    assert r.returncode == 0, r.stderr
    kept = json.loads(r.stdout)
    assert 0 < len(kept) <= K and all(x["metadata"]["lines"] >= 200 for x in kept)


def test_refined_batch_of_queries(dirs):
    """--queries-file: one walk and one rerank for the batch; every query answered as it is alone"""
    args = ["--queries-file", str(dirs / "queries.txt"), "--embedding-mode", "synthetic", "--refine", str(FETCH)]
    both = _search(dirs / "with", *args)
    assert both.returncode == 0, both.stderr
    lists = json.loads(both.stdout)
    assert len(lists) == 2 and all(len(x) == K for x in lists)
    for text, want in zip((dirs / "queries.txt").read_text().splitlines(), lists):
        r = _run("search", text, "-i", str(dirs / "with"), "--top-k", str(K), "--format", "json", "--embedding-mode", "synthetic",
                 "--refine", str(FETCH), "--refine-rows", "hbm")
        assert r.returncode == 0 and json.loads(r.stdout) == want, r.stderr


def test_refusals(dirs):
    qfile = ["--query-vector-file", str(dirs / "q.f32")]
    r = _search(dirs / "without", *qfile, "--refine", str(FETCH))
    assert r.returncode != 0 and "--recompute" in r.stderr and "documents.embeddings" in r.stderr
    r = _search(dirs / "with", *qfile, "--refine", str(FETCH), "--hybrid")
    assert r.returncode != 0 and "--refine together with --hybrid" in r.stderr
    r = _search(dirs / "with", "--queries-file", str(dirs / "queries.txt"), "--embedding-mode", "synthetic", "--refine", str(FETCH), "--hybrid")
    assert r.returncode != 0 and "--refine together with --hybrid" in r.stderr
    r = _search(dirs / "with", *qfile, "--refine", str(FETCH), "--refine-rows", "disk")
    assert r.returncode != 0 and "possible values: hbm, host" in r.stderr
    r = _search(dirs / "with", *qfile, "--refine", "0")
    assert r.returncode != 0 and "--refine" in r.stderr
