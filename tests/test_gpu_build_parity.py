"""-m gpu: the on-device graph builder (csrc/build.hip) against its restatement (tests/build_ref.py), list for list.

The builder takes no atomics that decide content, and on rows whose dot products are exact in f32 (build_ref.grid_rows) the Gram
tile, the wave dot and numpy agree in any summation order — so entry, max_level, levels, upper_off, adj0 and adjU of a device
build must EQUAL the restatement's: select_one (cut, self removal, path-node merge, proposal keys, tail clearing),
reverse_merge_one (run length, append / pend / prune, proposal order, cut, merge sort, pending area, flush), the host schedule
(insertion order, batch sizes, level jobs, entry, medoid), link_dist_kernel + append, and the wide instantiations.  Each case also
asserts the counters of the restatement that show its path ran (build_ref.CASES, validated on the CPU by test_cpu_build_ref.py).
Realistic, inexact rows — where the Gram tile's summation order differs from the wave dot and no exact reference exists — stay
with the quality bars of test_gpu_builder_quality.py."""
import numpy as np
import pytest

import build_ref as br

pytestmark = pytest.mark.gpu


def _upload(la, X):
    """rows on the device, zero padded to a multiple of 4 floats"""
    n, d = X.shape
    ld = (d + 3) & ~3
    Xp = np.zeros((n, ld), np.float32)
    Xp[:, :d] = X
    return la.DeviceArray.from_host(Xp), ld


def _diff(ref, g):
    """-> list of complaints, with the count and the first few differing nodes per level"""
    out = []
    for k in ("entry", "max_level"):
        if int(ref[k]) != int(g[k]):
            out.append(f"{k}: device {g[k]} != reference {ref[k]}")
    for k in ("levels", "upper_off"):
        if not np.array_equal(ref[k], g[k]):
            out.append(f"{k} differ")
    if out:
        return out
    n = len(ref["levels"])
    bad0 = np.flatnonzero((ref["adj0"] != g["adj0"]).any(1))
    if bad0.size:
        out.append(f"level 0: {bad0.size} of {n} lists differ, first {bad0[:4].tolist()}; node {bad0[0]}: device "
                   f"{g['adj0'][bad0[0]][g['adj0'][bad0[0]] != br.EMPTY].tolist()} reference "
                   f"{ref['adj0'][bad0[0]][ref['adj0'][bad0[0]] != br.EMPTY].tolist()}")
    for level in range(1, int(ref["max_level"]) + 1):
        members = np.flatnonzero(ref["levels"] >= level)
        rows = ref["upper_off"][members].astype(np.int64) + level - 1
        bad = members[(ref["adjU"][rows] != g["adjU"][rows]).any(1)]
        if bad.size:
            out.append(f"level {level}: {bad.size} of {members.size} lists differ, first {bad[:4].tolist()}")
    return out


def _device_build(la, c, X, monkeypatch, row_type=None):
    for k, v in c["knobs"].items():
        monkeypatch.setenv(k, v)  # (read once per build)
    dX, ld = _upload(la, X)
    bt = la.BackendType.Hnsw if c["kind"] == br.HN else la.BackendType.DiskAnn
    kw = {} if row_type is None else dict(row_type=row_type)
    s = la.BackendSearcher.build_device(bt, dX.ptr, X.shape[0], X.shape[1], ld, c["M"], c["efc"], **kw)
    g = s.graph_export()
    s.close()
    return g


def _check_case(po, name, g):
    c = br.CASES[name]
    ref = br.case_graph(po, name)
    cn = ref["counters"]
    print(name, {k: v for k, v in cn.items() if v}, "batches", len(ref["batches"]))
    assert all(cn[k] > 0 for k in c["need"]) and all(cn[k] == 0 for k in c["zero"]), cn
    assert g["M"] == c["M"] and g["M0"] == ref["M0"]
    d = _diff(ref, g)
    assert not d, "\n".join(d)


@pytest.mark.parametrize("name", list(br.CASES))
def test_device_build_equals_restatement(la, po, gpu, monkeypatch, name):
    c = br.CASES[name]
    if c["kind"] == br.VA and "LEANN_VAMANA_NAV" not in c["knobs"]:
        assert br.medoid(br.case_rows(c))[1] >= 1e-6  # the device's f32 scan must not be able to pick another medoid
    _check_case(po, name, _device_build(la, c, br.case_rows(c), monkeypatch))


@pytest.mark.parametrize("name", ["hnsw_m8", "vamana_r24"])
def test_bf16_rows_build_the_same_graph(la, po, gpu, monkeypatch, name):
    """build_device_rows with bf16 rows: the grid values are exact in bf16, so the graph is the f32 graph"""
    c = br.CASES[name]
    X = br.case_rows(c)
    assert ((la.round_bf16(X).astype(np.uint32) << 16).view(np.float32) == X).all()
    _check_case(po, name, _device_build(la, c, X, monkeypatch, row_type=la.RowType.BF16))


def test_append_continues_the_build(la, po, gpu, tmp_path):
    """hnsw_m8's rows: 800 built to a file, 400 appended (leann_backend_add: link_dist_kernel recomputes the stored link distances
    of level 0 and of the upper lists, then the batched insertion continues) == build_ref continue_from on the first build's graph"""
    c = br.CASES["hnsw_m8"]
    X = br.case_rows(c)
    n_old, n, d = 800, c["n"], c["d"]
    stem = str(tmp_path / "documents.leann")
    b = la.BackendBuilder(la.BackendType.Hnsw)
    b.build(X[:n_old], [], stem, d, c["M"], c["efc"])
    s = la.HnswSearcher.load(stem, d)
    g_old = s.graph_export()
    s.close()
    first = br.BuildRef(po, br.HN, X[:n_old], c["M"], c["efc"]).build()
    d0 = _diff(first, g_old)
    assert not d0, "\n".join(d0)
    b.add_to_index(X[n_old:], stem, d, n_old)
    s = la.HnswSearcher.load(stem, d)
    g = s.graph_export()
    s.close()
    ref = br.BuildRef(po, br.HN, X, c["M"], c["efc"]).continue_from(g_old, n_old)
    cn = ref["counters"]
    print("append", {k: v for k, v in cn.items() if v}, "batches", ref["batches"])
    assert cn["prunes_merge"] > 0 and cn["prunes_upper"] > 0 and cn["appends_list"] > 0  # old lists pruned on their recomputed distances
    assert ref["batches"][0] == n_old // 8
    dd = _diff(ref, g)
    assert not dd, "\n".join(dd)
    assert (ref["adj0"][:n_old] != g_old["adj0"]).any()  # the appended rows did rewrite lists of the first build
