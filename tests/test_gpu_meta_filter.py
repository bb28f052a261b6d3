"""GPU suite: metadata filters evaluated on the device from a columnar store (csrc/meta.hip, leann_rs_amd.metadata) against
tests/filter_ref.py, a literal restatement of the reference's filter.rs.  Every comparison is exact: bitmaps bit for bit, counts,
keys, f32 distance bits.  The record set and the filters are those of the CPU suite (tests/meta_cases.py): every op x every
right-hand type x every row tag, and the corners named one by one."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as fr
import meta_cases as mc
from util import HipStreams, synth

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 63, 64, 65, 127, 129, 8191, 8192, 8193, 20011]  # the byte, the 64-row step, the wave, the compaction's block
FILTERS = mc.matrix_filters() + mc.CORNERS
FIELDS = sorted(set(x for _, f in FILTERS for x in mc.fields_of(f)))
BASE = mc.MATRIX_RECORDS
# what every filter answers for every base record, computed once; rows of the sized record sets cycle through the base records
TABLE = np.array([[fr.matches(f, r) for r in BASE] for _, f in FILTERS], bool)
GUARD = 0xA5


def _records(n, shift=0):
    return [BASE[(i + shift) % len(BASE)] for i in range(n)]


def _expected(fi, n, shift=0, mask=None):
    bits = TABLE[fi][(np.arange(n) + shift) % len(BASE)]
    if mask is not None:
        bits = bits & mask
    return np.packbits(bits, bitorder="little"), int(bits.sum())


def _unpack(bm, n):
    return np.unpackbits(bm, bitorder="little")[:n].astype(bool)


@pytest.mark.parametrize("n", SIZES)
def test_eval_equals_the_reference_for_every_op_type_and_tag(la, gpu, n):
    rng = np.random.default_rng(n)
    shift = n % 5
    recs = _records(n, shift)
    m = la.MetaColumns.from_records(recs, FIELDS)
    assert m.len() == n and m.has_column("f") and not m.has_column("zzz")
    # unreadable passages: their rows pass no filter, not even Ne / NotIn / one on a missing field
    readable = rng.random(n) < 0.8
    mv = la.MetaColumns.from_records([r if ok else None for r, ok in zip(recs, readable)], FIELDS)
    extra = rng.random(n) < 0.5
    d_and = la.DeviceArray.from_host(np.packbits(extra, bitorder="little"))
    nbytes = (n + 7) // 8
    d_out = la.DeviceArray(nbytes + 8, np.uint8)
    d_cnt = la.DeviceArray(1, np.uint32)
    host = np.zeros(nbytes + 8, np.uint8)
    for fi, (name, f) in enumerate(FILTERS):
        want, cnt = _expected(fi, n, shift)
        host[:] = GUARD
        got_cnt = C.c_size_t(0)
        nodes, k, keep = la.metadata.encode_tree(f)
        la._native.check(la.lib().leann_meta_eval(m._h, nodes, k, host.ctypes.data_as(la._native.u8p), C.byref(got_cnt)))
        assert (host[:nbytes] == want).all() and got_cnt.value == cnt, (name, n)  # (pad bits are zero in `want`)
        assert (host[nbytes:] == GUARD).all(), (name, n)                          # nothing behind ceil(n / 8)
        want_v, cnt_v = _expected(fi, n, shift, readable)
        got_v, got_cnt_v = mv.eval(f, with_count=True)
        assert (got_v == want_v).all() and got_cnt_v == cnt_v, (name, n, "valid")
        # into device memory, ANDed with a caller's bitmap, behind a guard
        d_out.upload(np.full(nbytes + 8, GUARD, np.uint8))
        mv.eval_device(f, d_out.ptr, d_and.ptr, d_cnt.ptr)
        la.sync()
        out = d_out.to_host()
        want_a, cnt_a = _expected(fi, n, shift, readable & extra)
        assert (out[:nbytes] == want_a).all() and int(d_cnt.to_host()[0]) == cnt_a, (name, n, "d_and")
        assert (out[nbytes:] == GUARD).all(), (name, n, "d_and")
    m.close()
    mv.close()


def test_numbers_are_read_only_where_the_tag_says_number(la, gpu):
    """rows of another tag hold NaN in `num`: the answers do not change.  (Codes never cross the ABI — the library builds them from the
    rows' strings — so a poisoned code can only be given to the compiled program on the CPU: test_cpu_meta_plan.py does.)"""
    n = 8193
    recs = _records(n)
    m = la.MetaColumns(n)
    for f in FIELDS:
        tag, num, blob, off = la.metadata.column_arrays(recs, f)
        num[tag != la.metadata.TAG_NUMBER] = np.nan
        m.add_column(f, tag, num, blob, off)
    for fi, (name, f) in enumerate(FILTERS):
        want, cnt = _expected(fi, n)
        got, got_cnt = m.eval(f, with_count=True)
        assert (got == want).all() and got_cnt == cnt, name
    m.close()


def test_dictionary_is_bytewise_and_raw_bytes_work(la, gpu):
    """the library's own dictionary (sort + unique over the rows' strings) under ranges, prefix ranges with 0xFF bytes and bitsets"""
    for recs, filters in ((mc.RANGE_RECORDS, mc.RANGE_FILTERS), (mc.dictionary_records(5000), mc.dictionary_filters(5000)),
                          (mc.dictionary_records(33), mc.dictionary_filters(33))):
        n = len(recs)
        d, tags, nums, _ = mc.column(recs, "s")
        strs = [(r.get("s") if isinstance(r.get("s"), (str, bytes)) else b"") for r in recs]
        strs = [s.encode() if isinstance(s, str) else s for s in strs]
        off = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.uint64)
        m = la.MetaColumns(n)
        m.add_column("s", np.array(tags, np.uint8), np.array(nums), b"".join(strs), off)
        for f in filters:
            want, cnt = fr.bitmap(f, recs)
            got, got_cnt = m.eval(f, with_count=True)
            assert (got == want).all() and got_cnt == cnt, f
        m.close()


def test_add_column_validates_before_any_device_work(la, gpu):
    L = la.lib()
    start = L.leann_debug_device_blocks()
    m = la.MetaColumns(4)
    tag = np.array([4, 5, 0, 1], np.uint8)
    num = np.zeros(4)
    off = np.array([0, 0, 2, 2, 2], np.uint64)
    for kwargs, word in ((dict(tag=np.array([4, 7, 0, 1], np.uint8), num=num, str_blob=b"ab", str_off=off), "tag[1]"),
                         (dict(tag=tag, num=num), "str_off"),
                         (dict(tag=tag, str_blob=b"ab", str_off=off), "num"),
                         (dict(tag=tag, num=num, str_blob=b"ab", str_off=np.array([0, 2, 1, 2, 2], np.uint64)), "monotone")):
        with pytest.raises(la.LeannError) as e:
            m.add_column("f", **kwargs)
        assert e.value.code == 1 and word in str(e.value), (word, str(e.value))
        assert not m.has_column("f")
    m.add_column("f", tag, num, b"ab", off)
    with pytest.raises(la.LeannError) as e:
        m.add_column("f", tag, num, b"ab", off)
    assert e.value.code == 1 and "duplicate field 'f'" in str(e.value)
    out = C.c_void_p()
    assert L.leann_meta_create(1 << 32, None, 0, C.byref(out)) == 1 and b"2^32" in L.leann_last_error() and not out.value
    assert (m.eval(("cond", "f", "eq", "ab")) == np.array([0b0010], np.uint8)).all()
    m.close()
    assert L.leann_debug_device_blocks() == start


# ---- registered filters ----------------------------------------------------------------------------------------------------------
N, D, NQ, K, EF = 20011, 64, 24, 10, 48
REG_FILTERS = ["lines>50", "type=code AND lines<=20", "source:*main1*", "type in [doc,text] OR lines>=190", "type!=code", "lang?",
               "source^/p/3/ AND type not_in [doc]", "lines<0"]


@pytest.fixture(scope="module")
def corpus(po):
    rng = np.random.default_rng(11)
    recs = []
    for i in range(N):
        r = {"type": ["code", "text", "doc"][int(rng.integers(3))], "lines": int(rng.integers(200)), "source": f"/p/{i % 7}/main{i % 3}.{['rs', 'py'][i % 2]}"}
        if i % 11 == 0:
            r["lang"] = None
        if i % 13 == 0:
            del r["lines"]
        recs.append(r)
    X, Q = synth(po, N, D), synth(po, NQ, D, stream=1)
    bitmaps = {t: fr.bitmap(fr.parse(t), recs)[0] for t in REG_FILTERS}
    return recs, X, Q, bitmaps


def _same_answers(s, Q, fm, fb, modes=("walk", "exact", "auto")):
    assert fm.count() == fb.count()
    for mode in modes:
        a, b = s.search_filter_batch(Q, K, EF, fm, mode), s.search_filter_batch(Q, K, EF, fb, mode)
        assert (a[0] == b[0]).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all() and (a[2] == b[2]).all(), mode


def _error(call):
    with pytest.raises(Exception) as e:
        call()
    return getattr(e.value, "code", None), str(e.value)


def test_registered_meta_filter_is_the_bitmap_filter(la, gpu, corpus):
    recs, X, Q, bitmaps = corpus
    L = la.lib()
    start = L.leann_debug_device_blocks()
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, 8, 32, key_offset=5)
    m = la.MetaColumns.from_records(recs, ["type", "lines", "source", "lang"])
    made = []
    for text in REG_FILTERS:
        fm, fb = s.register_meta_filter(m, text), s.register_filter(bitmaps[text])
        assert fm.count() == int(np.unpackbits(bitmaps[text]).sum())
        _same_answers(s, Q, fm, fb)
        made.append((fm, fb))
    # removal of some allowed and some disallowed keys: both kinds of filter made before are stale, both made after agree
    allowed = _unpack(bitmaps["lines>50"], N)
    gone = np.concatenate([np.flatnonzero(allowed)[:300:3], np.flatnonzero(~allowed)[:300:3]]).astype(np.uint64) + np.uint64(5)
    assert s.remove(gone) == len(gone)
    for fm, fb in made[:2]:
        em, eb = _error(lambda: s.search_filter_batch(Q, K, EF, fm, "auto")), _error(lambda: s.search_filter_batch(Q, K, EF, fb, "auto"))
        assert em == eb and em[0] == 1 and "filter predates a removal" in em[1]
    for fm, fb in made:
        fm.close()
        fb.close()
    for text in REG_FILTERS[:4]:
        fm, fb = s.register_meta_filter(m, text), s.register_filter(bitmaps[text])
        live = _unpack(bitmaps[text], N)
        live[(gone - np.uint64(5)).astype(np.int64)] = False
        assert fm.count() == int(live.sum())
        _same_answers(s, Q, fm, fb)
        fm.close()
        fb.close()
    # a filter belongs to the handle it was made on
    s2 = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, 8, 32, key_offset=5)
    fm, fb = s2.register_meta_filter(m, "lines>50"), s2.register_filter(bitmaps["lines>50"])
    em, eb = _error(lambda: s.search_filter_batch(Q, K, EF, fm, "auto")), _error(lambda: s.search_filter_batch(Q, K, EF, fb, "auto"))
    assert em == eb and "filter belongs to another handle" in em[1]
    fm.close()
    fb.close()
    s2.close()
    m.close()
    s.close()
    assert L.leann_debug_device_blocks() == start


def test_registered_meta_filter_on_a_composite_handle(la, gpu, corpus):
    recs, X, Q, bitmaps = corpus
    n0 = 157 * 64  # interior shard boundaries are multiples of 64
    d0, d1 = la.DeviceArray.from_host(X[:n0]), la.DeviceArray.from_host(X[n0:])
    s0 = la.BackendSearcher.build_device(la.BackendType.Hnsw, d0.ptr, n0, D, D, 8, 32)
    s1 = la.BackendSearcher.build_device(la.BackendType.Hnsw, d1.ptr, N - n0, D, D, 8, 32, key_offset=n0)
    s = la.ShardedIndex.from_searchers([s0, s1], take_ownership=True).as_backend()
    m = la.MetaColumns.from_records(recs, ["type", "lines", "source"])
    for text in REG_FILTERS[:4]:
        fm, fb = s.register_meta_filter(m, text), s.register_filter(bitmaps[text])
        _same_answers(s, Q, fm, fb)
        fm.close()
        fb.close()
    m.close()
    s.close()


def test_registered_meta_filter_on_a_bf16_handle(la, gpu, corpus):
    recs, X, Q, bitmaps = corpus
    dX = la.DeviceArray.from_host(X)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, 8, 32, row_type=la.RowType.BF16)
    m = la.MetaColumns.from_records(recs, ["type", "lines"])
    for text in REG_FILTERS[:2]:
        fm, fb = s.register_meta_filter(m, text), s.register_filter(bitmaps[text])
        _same_answers(s, Q, fm, fb, modes=("walk", "auto"))
        em, eb = _error(lambda: s.search_filter_batch(Q, K, EF, fm, "exact")), _error(lambda: s.search_filter_batch(Q, K, EF, fb, "exact"))
        assert em == eb and em[0] == 5  # mode 1 on bf16 rows: refused exactly as for a bitmap filter
        fm.close()
        fb.close()
    m.close()
    s.close()


def test_refusals_leave_the_handle_and_the_store_as_they_were(la, gpu, corpus):
    recs, X, Q, bitmaps = corpus
    L = la.lib()
    start = L.leann_debug_device_blocks()
    n = 4099
    dX = la.DeviceArray.from_host(X[:n])
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, D, D, 8, 32)
    m = la.MetaColumns.from_records(recs[:n], ["type", "lines"])
    want = fr.bitmap(fr.parse("lines>50"), recs[:n])
    before = s.search_batch(Q, K, EF)
    blocks = L.leann_debug_device_blocks()
    short = la.MetaColumns.from_records(recs[: n - 1], ["lines"])
    code, msg = _error(lambda: s.register_meta_filter(short, "lines>50"))
    assert code == 1 and f"{n - 1} rows" in msg and str(n) in msg
    short.close()
    code, msg = _error(lambda: s.register_meta_filter(m, "nowhere>50"))
    assert code == 1 and "no column for field 'nowhere'" in msg
    code, msg = _error(lambda: m.eval("nowhere>50"))
    assert code == 1 and "no column for field 'nowhere'" in msg
    too_many = ("and", [("cond", "lines", "gt", i) for i in range(33)])
    code, msg = _error(lambda: s.register_meta_filter(m, too_many))
    assert code == 1 and "more than 32 conditions" in msg
    deep = ("cond", "lines", "gt", 50)
    for level in range(9):
        deep = ("and" if level % 2 else "or", [deep, ("cond", "type", "eq", "code")])
    code, msg = _error(lambda: m.eval(deep))
    assert code == 1 and "nested deeper than 8" in msg
    if la.device_count() > 1:  # a store on another device than the handle's
        far = la.MetaColumns.from_records(recs[:n], ["lines"], device=1)
        code, msg = _error(lambda: s.register_meta_filter(far, "lines>50"))
        assert code == 1 and "device 1" in msg and "device 0" in msg
        far.close()
    assert L.leann_debug_device_blocks() == blocks
    after = s.search_batch(Q, K, EF)
    assert all((a == b).all() for a, b in zip(before, after))
    got = m.eval("lines>50", with_count=True)
    assert (got[0] == want[0]).all() and got[1] == want[1]
    f = s.register_meta_filter(m, "lines>50")
    assert f.count() == want[1]
    f.close()
    m.close()
    s.close()
    assert L.leann_debug_device_blocks() == start


def test_eval_device_on_a_caller_stream_feeds_the_device_searches(la, gpu, corpus):
    recs, X, Q, bitmaps = corpus
    n = 8193
    dX, dQ = la.DeviceArray.from_host(X[:n]), la.DeviceArray.from_host(Q)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, n, D, D, 8, 32)
    m = la.MetaColumns.from_records(recs[:n], ["type", "lines", "source"])
    nbytes = (n + 7) // 8
    with HipStreams(la, 2) as st:
        for text, stream in (("lines>50", st[0]), ("source:*main1* AND type in [code,doc]", st[1]), ("type=code", st[0])):
            want, cnt = fr.bitmap(fr.parse(text), recs[:n])
            d_bm, d_cnt = la.DeviceArray(nbytes, np.uint8), la.DeviceArray(1, np.uint32)
            dk, dd, dc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
            tk, ts, tc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
            m.eval_device(text, d_bm.ptr, None, d_cnt.ptr, stream)  # enqueued; the searches below are ordered behind it on the same stream
            s.search_filtered_batch_device(dQ.ptr, NQ, K, EF, d_bm.ptr, 0, dk.ptr, dd.ptr, dc.ptr, None, stream)
            la._native.check(la.lib().leann_scan_topk_device(dX.ptr, n, D, D, dQ.ptr, NQ, K, d_bm.ptr, 0, tk.ptr, ts.ptr, tc.ptr, stream))
            st.synchronize(stream)
            assert (d_bm.to_host() == want).all() and int(d_cnt.to_host()[0]) == cnt
            hk, hd, hc = s.search_filtered_batch(Q, K, EF, want)
            assert (dk.to_host() == hk).all() and (dd.to_host().view(np.uint32) == hd.view(np.uint32)).all() and (dc.to_host() == hc).all()
            h_bm = la.DeviceArray.from_host(want)
            uk, us, uc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
            la._native.check(la.lib().leann_scan_topk_device(dX.ptr, n, D, D, dQ.ptr, NQ, K, h_bm.ptr, 0, uk.ptr, us.ptr, uc.ptr, None))
            la.sync()
            assert (tk.to_host() == uk.to_host()).all() and (ts.to_host().view(np.uint32) == us.to_host().view(np.uint32)).all()
            assert (tc.to_host() == uc.to_host()).all()
    m.close()
    s.close()


# ---- the C++ host: `leann search -f ... --device-filter` ---------------------------------------------------------------------------
CLI_FILTERS = ["source=file3.rs", "lines<12", "source in [file1.rs,file2.py,nothing]", "source~e7", "source:file1*", "source:*.py", "lines?",
               "lines!=7 AND source not_in [file1.rs]", "source:*.rs AND lines<100 OR source^file2 AND lines>=500"]


@pytest.fixture(scope="module")
def cli_index(tmp_path_factory, gpu):
    """the fixture index of tests/test_gpu_cli.py: the same documents, the same build"""
    import json
    from test_gpu_cli import _docs, _run
    d = tmp_path_factory.mktemp("meta_cli")
    (d / "docs.jsonl").write_text("\n".join(json.dumps(x) for x in _docs(600)))
    r = _run("build", "--index-dir", str(d / "idx"), "--passages-jsonl", str(d / "docs.jsonl"), "--dimensions", "96",
             "--graph-degree", "16", "--complexity", "64", "--recompute")
    assert r.returncode == 0, r.stderr
    return d


@pytest.mark.parametrize("flt", CLI_FILTERS)
def test_cli_device_filter_prints_the_same_bytes_either_way(cli_index, flt):
    import os
    import subprocess
    from test_gpu_cli import EXE
    args = [EXE, "search", "vector database embedding search and some more words", "-i", str(cli_index / "idx"), "--top-k", "6", "--format", "json",
            "--auto-hybrid", "false", "-f", flt, "--device-filter"]
    env = dict(os.environ, LEANN_LOG="debug")
    env.pop("LEANN_META_DEVICE", None)
    dev = subprocess.run(args, capture_output=True, env=env)
    host = subprocess.run(args, capture_output=True, env=dict(env, LEANN_META_DEVICE="0"))
    assert dev.returncode == 0 and host.returncode == 0, dev.stderr + host.stderr
    assert dev.stdout == host.stdout and len(dev.stdout) > 2
    assert b"filter evaluated on the device" in dev.stderr and b"filter evaluated on the device" not in host.stderr
    assert b"filter evaluated on the host, passage by passage (LEANN_META_DEVICE=0)" in host.stderr
