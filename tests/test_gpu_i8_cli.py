"""-m gpu: the int8 row type through the C++ host CLI — `leann build --row-type int8`, `leann convert --row-type int8`, and
`leann search` (unchanged: leann_backend_open detects the row type from the index file)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import i8_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "leann")
N, D = 600, 96
TOPICS = ["rust ownership borrow checker lifetimes", "python asyncio event loop coroutine", "vector database embedding search",
          "graph traversal beam hnsw neighbours", "gpu kernel wavefront lds bandwidth", "bm25 ranking term frequency"]


def _run(*args):
    return subprocess.run([EXE, *args], capture_output=True, text=True)


def _header(path):
    raw = open(path, "rb").read(128)
    magic, version, kind, n, d, m, m0 = struct.unpack_from("<8sIIQIII", raw)
    nul, = struct.unpack_from("<Q", raw, 56)
    assert magic == b"LEANNGX1"
    return dict(version=version, n=n, d=d, M=m, M0=m0, graph_bytes=n + 4 * n + 4 * n * m0 + 4 * nul * m)


@pytest.fixture(scope="module")
def dirs(tmp_path_factory, gpu):
    d = tmp_path_factory.mktemp("cli_i8")
    docs = [dict(id=str(i + 1), text=f"passage {i} about {TOPICS[i % len(TOPICS)]} number {i * 7919 % 1000}", metadata=dict(lines=i))
            for i in range(N)]
    (d / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in docs))
    common = ["--passages-jsonl", str(d / "docs.jsonl"), "--dimensions", str(D), "--graph-degree", "16", "--complexity", "64"]
    r = _run("build", "--index-dir", str(d / "i8"), *common, "--row-type", "int8")
    assert r.returncode == 0 and "int8 rows" in r.stdout, r.stderr
    r = _run("build", "--index-dir", str(d / "f32"), *common, "--recompute")  # --recompute: documents.embeddings holds the f32 rows
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(3)
    q = rng.standard_normal(D).astype(np.float32)
    q /= np.linalg.norm(q)
    q.tofile(d / "q.f32")
    return d


def _cli_search(index_dir, qfile, k=8):
    r = _run("search", "any text", "-i", str(index_dir), "--top-k", str(k), "--format", "json", "--auto-hybrid", "false",
             "--query-vector-file", str(qfile))
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _rows(raw, graph_bytes):
    """(exps, codes) behind the graph arrays of a version-4 file"""
    return (np.frombuffer(raw[128 + graph_bytes: 128 + graph_bytes + D], np.int8),
            np.frombuffer(raw[128 + graph_bytes + D:], np.int8).reshape(N, D))


def test_build_with_int8_rows_then_search(la, dirs):
    hd = _header(dirs / "i8" / "documents.index")
    assert hd["version"] == 4 and hd["n"] == N and hd["d"] == D
    assert os.path.getsize(dirs / "i8" / "documents.index") == 128 + hd["graph_bytes"] + D + N * D
    meta, meta32 = (json.loads((dirs / x / "documents.leann.meta.json").read_text()) for x in ("i8", "f32"))
    assert set(meta) == set(meta32) and not any("row" in k for k in meta)  # the row type lives in the index file only
    # the stored rows are the quantised embeddings the f32 twin kept
    emb = np.fromfile(dirs / "f32" / "documents.embeddings", np.float32).reshape(N, D)
    exps, codes = _rows((dirs / "i8" / "documents.index").read_bytes(), hd["graph_bytes"])
    re, rc = i8_ref.quantize(emb)
    assert (exps == re).all() and (codes == rc).all()
    res = _cli_search(dirs / "i8", dirs / "q.f32")
    s = la.HnswSearcher.load(str(dirs / "i8" / "documents.leann"), D)
    assert s.row_type() == la.RowType.I8
    q = np.fromfile(dirs / "q.f32", np.float32)
    keys, dists = s.search(q, 8, 64)  # the CLI's default complexity
    s.close()
    assert [int(x["id"]) - 1 for x in res] == [int(k) for k in keys]
    assert np.array([x["score"] for x in res], np.float32).tobytes() == dists.tobytes()
    r = _run("build", "--index-dir", str(dirs / "bad"), "--passages-jsonl", str(dirs / "docs.jsonl"), "--row-type", "fp8")
    assert r.returncode != 0 and "expected f32 or bf16, or int8" in r.stderr


def test_convert_an_f32_index(la, dirs):
    f32 = dirs / "f32" / "documents.index"
    hd = _header(f32)
    size_before = os.path.getsize(f32)
    assert hd["version"] == 1 and size_before == 128 + hd["graph_bytes"] + N * D * 4
    graph_before = f32.read_bytes()[128: 128 + hd["graph_bytes"]]
    before = _cli_search(dirs / "f32", dirs / "q.f32")
    r = _run("convert", str(dirs / "f32"), "--row-type", "int8")
    assert r.returncode == 0 and "rewritten as int8" in r.stdout, r.stderr
    hd2 = _header(f32)
    assert hd2["version"] == 4 and os.path.getsize(f32) == 128 + hd["graph_bytes"] + D + N * D  # a quarter of the row bytes
    raw = f32.read_bytes()
    assert raw[128: 128 + hd["graph_bytes"]] == graph_before  # the graph built on the exact rows is kept
    emb = np.fromfile(dirs / "f32" / "documents.embeddings", np.float32).reshape(N, D)
    exps, codes = _rows(raw, hd["graph_bytes"])
    re, rc = i8_ref.quantize(emb)
    assert (exps == re).all() and (codes == rc).all()
    after = _cli_search(dirs / "f32", dirs / "q.f32")
    assert len(after) == 8 and [x["score"] for x in after] == sorted(x["score"] for x in after)
    # a step is <= 2^-7 of a column's largest value: the scores move in the third decimal and the neighbourhood stays (5 of 8 asked
    # for, where the bf16 twin of this test asks 6 for a step of 2^-9)
    assert len({x["id"] for x in after} & {x["id"] for x in before}) >= 5
    r = _run("convert", str(dirs / "f32"), "--row-type", "int8")  # already converted: nothing to do
    assert r.returncode == 0 and "rows are int8 already" in r.stdout
    for rt in ("f32", "bf16"):
        r = _run("convert", str(dirs / "f32"), "--row-type", rt)
        assert r.returncode != 0 and "f32 -> int8" in r.stderr and "int8 -> " + rt in r.stderr
