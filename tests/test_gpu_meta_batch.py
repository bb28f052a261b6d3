"""GPU suite: a batch of metadata filters evaluated in one pass (csrc/meta.hip: meta_eval_batch_kernel; csrc/meta_batch_plan.h) and the
searches under per-query filters built on it, against tests/filter_ref.py, a literal restatement of the reference's filter.rs.  Every
comparison is exact: bitmaps bit for bit, guard bytes, counts, keys, f32 distance bits, stats.  Record sets and filters are those of
the single-filter suites (tests/meta_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as fr
import meta_cases as mc
from test_cpu_meta_batch import _wide_records, wide_filters
from util import HipStreams, synth

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 63, 64, 65, 127, 129, 8191, 8192, 8193, 20011]  # the byte, the 64-row step, the wave, more than one workgroup
FILTERS = mc.matrix_filters() + mc.CORNERS
F = [f for _, f in FILTERS]
FIELDS = sorted(set(x for f in F for x in mc.fields_of(f)))
BASE = mc.MATRIX_RECORDS
TABLE = np.array([[fr.matches(f, r) for r in BASE] for f in F], bool)  # [filter, base record], computed once
GUARD = 0xA5


def _records(n, shift=0):
    return [BASE[(i + shift) % len(BASE)] for i in range(n)]


def _expected(n, shift=0, mask=None, table=TABLE):
    """([filters, ceil(n / 8)] bitmaps with zero pad bits, [filters] counts) for rows cycling through the table's base records"""
    bits = table[:, (np.arange(n) + shift) % table.shape[1]]
    if mask is not None:
        bits = bits & mask[None, :]
    return np.packbits(bits, axis=1, bitorder="little"), bits.sum(axis=1)


def _eval_guarded(la, m, filters, n, stride, d_and=None, stream=None, sync=True):
    """one eval_batch_device call into a block prefilled with GUARD, the bitmaps from a base offset by one byte; returns the block, the
    counts and n_distinct — or, unsynchronised, what to read later"""
    k = len(filters)
    total = 1 + k * stride + 8
    d_out = la.DeviceArray.from_host(np.full(total, GUARD, np.uint8))
    d_cnt = la.DeviceArray.from_host(np.full(k, 0xFFFFFFFF, np.uint32))
    distinct = m.eval_batch_device(filters, d_out.ptr + 1, stride, d_and, d_cnt.ptr, stream)
    if not sync:
        return d_out, d_cnt, distinct
    la.sync()
    return d_out.to_host(), d_cnt.to_host(), distinct


def _check_block(block, counts, want, want_counts, n, stride, what):
    k, nbytes = want.shape[0], (n + 7) // 8
    assert block[0] == GUARD, what
    rows = block[1: 1 + k * stride].reshape(k, stride)
    bad = np.flatnonzero((rows[:, :nbytes] != want).any(axis=1))
    assert bad.size == 0, (what, "bitmaps", bad[:5])
    assert (rows[:, nbytes:] == GUARD).all(), (what, "bytes between rows")
    assert (block[1 + k * stride:] == GUARD).all(), (what, "bytes behind the last row")
    assert (counts == want_counts).all(), (what, "counts", np.flatnonzero(counts != want_counts)[:5])


@pytest.mark.parametrize("n", SIZES)
def test_all_filters_in_one_call_equal_the_reference(la, gpu, n):
    rng = np.random.default_rng(n)
    shift = n % 5
    recs = _records(n, shift)
    readable = rng.random(n) < 0.8  # unreadable passages pass no filter
    mv = la.MetaColumns.from_records([r if ok else None for r, ok in zip(recs, readable)], FIELDS)
    extra = rng.random(n) < 0.5
    d_and = la.DeviceArray.from_host(np.packbits(extra, bitorder="little"))
    nbytes = (n + 7) // 8
    want, want_counts = _expected(n, shift, readable & extra)
    for stride in (nbytes, nbytes + 5):
        block, counts, distinct = _eval_guarded(la, mv, F, n, stride, d_and.ptr)
        _check_block(block, counts, want, want_counts, n, stride, (n, stride))
        assert 0 < distinct <= len(F)
    # the host form (no d_and), into a strided host block behind a guard
    want, want_counts = _expected(n, shift, readable)
    got, got_counts = mv.eval_batch(F, with_count=True)
    assert got.shape == (len(F), nbytes) and (got == want).all() and (got_counts == want_counts).all()
    nodes, off, k, keep = la.metadata.encode_trees(F)
    host = np.full(1 + k * (nbytes + 3) + 8, GUARD, np.uint8)
    cnt = (C.c_size_t * k)()
    distinct = C.c_size_t(0)
    la._native.check(la.lib().leann_meta_eval_batch(mv._h, nodes, off, k, host[1:].ctypes.data_as(la._native.u8p), nbytes + 3, cnt,
                                                    C.byref(distinct)))
    _check_block(host, np.array(cnt[:k]), want, want_counts, n, nbytes + 3, (n, "host"))
    mv.close()


def test_equal_filters_are_evaluated_once_and_written_to_every_output(la, gpu):
    n = 8193
    m = la.MetaColumns.from_records(_records(n), FIELDS)
    nbytes = (n + 7) // 8
    _, _, distinct = _eval_guarded(la, m, F, n, nbytes)
    both = F + F[::-1]
    block, counts, distinct2 = _eval_guarded(la, m, both, n, nbytes + 5)
    want, want_counts = _expected(n)
    _check_block(block, counts, np.concatenate([want, want[::-1]]), np.concatenate([want_counts, want_counts[::-1]]), n, nbytes + 5, "F + reversed(F)")
    assert distinct2 == distinct and distinct < len(F)  # (several of the 106 compile to the same program)
    m.close()


def _string_store(la, recs):
    """a store whose column "s" takes the rows' raw bytes (values no JSON text can hold)"""
    n = len(recs)
    d, tags, nums, _ = mc.column(recs, "s")
    strs = [(r.get("s") if isinstance(r.get("s"), (str, bytes)) else b"") for r in recs]
    strs = [s.encode() if isinstance(s, str) else s for s in strs]
    off = np.concatenate([[0], np.cumsum([len(s) for s in strs])]).astype(np.uint64)
    m = la.MetaColumns(n)
    m.add_column("s", np.array(tags, np.uint8), np.array(nums), b"".join(strs), off)
    return m


def test_bitsets_and_dictionary_ranges_in_one_batch(la, gpu):
    for recs, filters in ((mc.dictionary_records(5000), mc.dictionary_filters(5000)), (mc.RANGE_RECORDS, list(mc.RANGE_FILTERS))):
        m = _string_store(la, recs)
        want = [fr.bitmap(f, recs) for f in filters]
        got, got_counts = m.eval_batch(filters, with_count=True)
        for i, f in enumerate(filters):
            assert (got[i] == want[i][0]).all() and got_counts[i] == want[i][1], f
        m.close()


def test_more_columns_than_a_launch_takes(la, gpu):
    n = 8193
    base, filters = _wide_records(), wide_filters()
    table = np.array([[fr.matches(f, r) for r in base] for f in filters], bool)
    fields = sorted(set(x for f in filters for x in mc.fields_of(f)))
    assert len(fields) == 20
    m = la.MetaColumns.from_records([base[i % len(base)] for i in range(n)], fields)
    want, want_counts = _expected(n, table=table)
    block, counts, distinct = _eval_guarded(la, m, filters, n, (n + 7) // 8 + 5)
    _check_block(block, counts, want, want_counts, n, (n + 7) // 8 + 5, "20 fields")
    assert distinct == len(filters)
    m.close()


def test_two_batches_on_two_streams_of_one_store(la, gpu):
    n = 20011
    m = la.MetaColumns.from_records(_records(n), FIELDS)
    nbytes = (n + 7) // 8
    want, want_counts = _expected(n)
    with HipStreams(la, 2) as st:
        a = _eval_guarded(la, m, F, n, nbytes, stream=st[0], sync=False)
        b = _eval_guarded(la, m, F[::-1], n, nbytes + 5, stream=st[1], sync=False)
        a2 = _eval_guarded(la, m, F[::-1], n, nbytes, stream=st[0], sync=False)  # reuses the first stream's scratch block behind `a`
        st.synchronize(st[0])
        st.synchronize(st[1])
        _check_block(a[0].to_host(), a[1].to_host(), want, want_counts, n, nbytes, "stream 0")
        _check_block(b[0].to_host(), b[1].to_host(), want[::-1], want_counts[::-1], n, nbytes + 5, "stream 1")
        _check_block(a2[0].to_host(), a2[1].to_host(), want[::-1], want_counts[::-1], n, nbytes, "stream 0 again")
    m.close()


# ---- searches under per-query filters ----------------------------------------------------------------------------------------------
N, D, NQ, K, EF = 4096, 64, 70, 10, 48
STRIDE = (N + 7) // 8
QF = [(7 * i) % len(F) for i in range(NQ)]  # all-false, all-true and selective filters


@pytest.fixture(scope="module")
def world(la, gpu, po):
    X, Q = synth(po, N, D), synth(po, NQ, D, stream=1)
    dX, dQ = la.DeviceArray.from_host(X), la.DeviceArray.from_host(Q)
    s = la.BackendSearcher.build_device(la.BackendType.Hnsw, dX.ptr, N, D, D, 16, 48)
    m = la.MetaColumns.from_records(_records(N), FIELDS)
    bitmaps, counts = _expected(N)
    d_allow = la.DeviceArray.from_host(np.ascontiguousarray(bitmaps[QF]))  # [NQ, STRIDE] packed on the host from filter_ref
    yield dict(X=X, Q=Q, dX=dX, dQ=dQ, s=s, m=m, d_allow=d_allow, allowed=counts[QF].astype(np.uint32), filters=[F[i] for i in QF])
    m.close()
    s.close()


def _delegated(la, s, w, mode):
    dk, dd, dc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
    ds = la.DeviceArray.from_host(np.zeros((NQ, 4), np.uint32))
    if mode == "walk":
        s.search_filtered_batch_device(w["dQ"].ptr, NQ, K, EF, w["d_allow"].ptr, STRIDE, dk.ptr, dd.ptr, dc.ptr, ds.ptr)
    else:
        s.search_filtered_exact_batch_device(w["dQ"].ptr, NQ, K, w["d_allow"].ptr, STRIDE, dk.ptr, dd.ptr, dc.ptr)
    la.sync()
    return dk.to_host(), dd.to_host().view(np.uint32), dc.to_host(), ds.to_host()


def _meta_batch(la, s, w, mode):
    dk, dd, dc = la.DeviceArray((NQ, K), np.uint64), la.DeviceArray((NQ, K), np.float32), la.DeviceArray(NQ, np.uint32)
    ds = la.DeviceArray.from_host(np.zeros((NQ, 4), np.uint32))
    da = la.DeviceArray.from_host(np.full(NQ, 0xFFFFFFFF, np.uint32))
    s.search_meta_batch_device(w["m"], w["dQ"].ptr, NQ, w["filters"], K, EF, dk.ptr, dd.ptr, dc.ptr, ds.ptr, da.ptr, mode)
    return dk.to_host(), dd.to_host().view(np.uint32), dc.to_host(), ds.to_host(), da.to_host()


def _same(la, s, w, modes=("walk", "exact")):
    out = {}
    for mode in modes:
        want, got = _delegated(la, s, w, mode), _meta_batch(la, s, w, mode)
        for a, b, what in zip(want, got, ("keys", "distance bits", "counts", "stats")):
            assert (a == b).all(), (mode, what, np.argwhere(a != b)[:3])
        assert (got[4] == w["allowed"]).all(), (mode, "n_allowed")
        out[mode] = got
    return out


def test_search_is_the_delegated_search_under_the_evaluated_bitmaps(la, gpu, world):
    got = _same(la, world["s"], world)
    start = la.lib().leann_debug_device_blocks()  # (the handle's own search scratch exists by now)
    assert (got["exact"][2] == np.minimum(world["allowed"], K)).all()  # nothing removed: the exact scan finds min(allowed, k)
    assert 0 in world["allowed"] and N in world["allowed"]
    # the host form: the same answers through host pointers
    keys, dists, counts, allowed = world["s"].search_meta_batch(world["m"], world["Q"], world["filters"], K, EF, "walk")
    assert (keys == got["walk"][0]).all() and (dists.view(np.uint32) == got["walk"][1]).all() and (counts == got["walk"][2]).all()
    assert (allowed == world["allowed"]).all()
    again = _meta_batch(la, world["s"], world, "exact")
    assert all((x == y).all() for x, y in zip(got["exact"], again))
    assert la.lib().leann_debug_device_blocks() == start  # the bitmaps' scratch went back with each call


def test_search_in_chunks_of_sixteen_queries(la, gpu, world, monkeypatch):
    monkeypatch.setenv("LEANN_DEBUG_META_BATCH_BYTES", str(16 * ((STRIDE + 15) // 16 * 16)))  # 5 chunks, the last holds 6 queries
    la.lib().leann_debug_reload_env()  # (conftest reads the knobs again after the test)
    _same(la, world["s"], world)


def test_search_on_a_bf16_twin(la, gpu, world):
    b = world["s"].to_rows(la.RowType.BF16)
    before = _same(la, b, world, modes=("walk",))["walk"]
    with pytest.raises(la.LeannError) as want:
        _delegated(la, b, world, "exact")
    with pytest.raises(la.LeannError) as got:
        _meta_batch(la, b, world, "exact")
    assert got.value.code == want.value.code == 5 and str(got.value) == str(want.value)
    after = _meta_batch(la, b, world, "walk")
    assert all((x == y).all() for x, y in zip(before, after))
    b.close()


def test_validation_leaves_store_and_handle_as_they_were(la, gpu, world):
    L, s, m = la.lib(), world["s"], world["m"]
    nbytes = STRIDE
    d_out = la.DeviceArray.from_host(np.full(4 * nbytes, GUARD, np.uint8))
    m.eval_batch_device(F[:4], d_out.ptr, nbytes)  # (the store's scratch block of the null stream exists from here on)
    la.sync()
    first = d_out.to_host()
    before = _meta_batch(la, s, world, "walk")
    blocks = L.leann_debug_device_blocks()
    nodes, off, k, keep = la.metadata.encode_trees(F[:4])
    dq, dk, dd, dc = world["dQ"].ptr, la.DeviceArray((4, K), np.uint64), la.DeviceArray((4, K), np.float32), la.DeviceArray(4, np.uint32)

    def refused(rc, *words):
        msg = L.leann_last_error().decode()
        assert rc == 1 and all(x in msg for x in words), (rc, msg)
        assert L.leann_debug_device_blocks() == blocks

    def offsets(*v):
        return (C.c_size_t * len(v))(*v)
    ev, evd = L.leann_meta_eval_batch, L.leann_meta_eval_batch_device
    host = np.zeros(4 * nbytes, np.uint8)
    hp = host.ctypes.data_as(la._native.u8p)
    refused(evd(None, nodes, off, k, None, d_out.ptr, nbytes, None, None, None), "null")
    refused(evd(m._h, None, off, k, None, d_out.ptr, nbytes, None, None, None), "null")
    refused(evd(m._h, nodes, None, k, None, d_out.ptr, nbytes, None, None, None), "null")
    refused(evd(m._h, nodes, off, k, None, None, nbytes, None, None, None), "null")
    refused(ev(None, nodes, off, k, hp, nbytes, None, None), "null")
    refused(ev(m._h, nodes, off, k, None, nbytes, None, None), "null")
    refused(evd(m._h, nodes, offsets(1, 2, 3, 4, 5), k, None, d_out.ptr, nbytes, None, None, None), "node_off[0]")
    refused(evd(m._h, nodes, offsets(0, 2, 1, 3, 4), k, None, d_out.ptr, nbytes, None, None, None), "monotone", "filter 1")
    refused(ev(m._h, nodes, offsets(0, 2, 1, 3, 4), k, hp, nbytes, None, None), "monotone")
    refused(evd(m._h, nodes, off, k, None, d_out.ptr, nbytes - 1, None, None, None), "stride", str(nbytes))
    refused(ev(m._h, nodes, off, k, hp, nbytes - 1, None, None), "stride")
    assert evd(m._h, nodes, off, 0, None, None, 0, None, None, None) == 0 and ev(m._h, None, off, 0, None, 0, None, None) == 0  # n_out == 0
    bad = list(F[:6])
    bad[3] = ("cond", "nowhere", "gt", 50)
    for call in (lambda: m.eval_batch(bad), lambda: m.eval_batch_device(bad, d_out.ptr, nbytes),
                 lambda: s.search_meta_batch_device(m, dq, 6, bad, K, EF, dk.ptr, dd.ptr, dc.ptr)):
        with pytest.raises(la.LeannError) as e:
            call()
        assert e.value.code == 1 and str(e.value) == "filter 3: metadata filter: no column for field 'nowhere'"
        assert L.leann_debug_device_blocks() == blocks
    bad[3] = F[3]
    bad[5] = ("and", [("cond", "f", "gt", i) for i in range(33)])
    with pytest.raises(la.LeannError) as e:
        m.eval_batch_device(bad, d_out.ptr, nbytes)
    assert str(e.value) == "filter 5: metadata filter: more than 32 conditions (the limit)"
    # the searches' own checks
    sm = L.leann_backend_search_meta_batch_device
    args = (dq, 4, K, EF, nodes, off)
    res = (dk.ptr, dd.ptr, dc.ptr, None, None, None)
    refused(sm(None, m._h, *args, 0, *res), "null")
    refused(sm(s._h, None, *args, 0, *res), "null")
    refused(sm(s._h, m._h, None, 4, K, EF, nodes, off, 0, *res), "null")
    refused(sm(s._h, m._h, dq, 4, 0, EF, nodes, off, 0, *res), "zero")
    refused(sm(s._h, m._h, *args, 2, *res), "mode = 2")
    refused(sm(s._h, m._h, *args, -1, *res), "mode = -1")
    refused(sm(s._h, m._h, dq, 4, K, EF, nodes, offsets(0, 2, 1, 3, 4), 0, *res), "monotone")
    short = la.MetaColumns.from_records(_records(N - 1), FIELDS)
    blocks = L.leann_debug_device_blocks()
    refused(sm(s._h, short._h, *args, 0, *res), f"{N - 1} rows", str(N))
    with pytest.raises(la.LeannError) as e:
        s.search_meta_batch(short, world["Q"], world["filters"], K, EF)
    assert e.value.code == 1 and f"{N - 1} rows" in str(e.value) and L.leann_debug_device_blocks() == blocks
    short.close()
    if la.device_count() > 1:  # a store on another device than the handle's
        far = la.MetaColumns.from_records(_records(N), FIELDS, device=1)
        blocks = L.leann_debug_device_blocks()
        refused(sm(s._h, far._h, *args, 0, *res), "device 1", "device 0")
        far.close()
    # nothing was written, and store and handle answer as before
    assert (d_out.to_host() == first).all()
    after = _meta_batch(la, s, world, "walk")
    assert all((x == y).all() for x, y in zip(before, after))
    want, want_counts = _expected(N)
    got, got_counts = m.eval_batch(F, with_count=True)
    assert (got == want).all() and (got_counts == want_counts).all()
    del keep


def test_removed_keys_are_masked_by_the_delegated_search(la, gpu, world):
    """(last: it changes the shared handle)  300 keys removed, not consolidated: the delegated calls AND the live mask themselves"""
    s = world["s"]
    gone = np.arange(0, 3 * 300, 3, dtype=np.uint64)
    assert s.remove(gone) == 300
    got = _same(la, s, world)  # d_n_allowed stays what the filter allows, before the live mask
    for mode in ("walk", "exact"):
        keys, _, counts = got[mode][:3]
        for i in range(NQ):
            assert not np.isin(keys[i, : counts[i]], gone).any(), (mode, i)
    live = np.ones(N, bool)
    live[gone.astype(np.int64)] = False
    allowed_live = (TABLE[QF][:, np.arange(N) % len(BASE)] & live[None, :]).sum(axis=1)
    assert (got["exact"][2] == np.minimum(allowed_live, K)).all()
