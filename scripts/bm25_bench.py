#!/usr/bin/env python3
"""Device BM25 (csrc/bm25.hip) on the synthetic Zipf corpus of tests/bm25_ref.py: prints one JSON line per figure.

  (a) scoring + selection + reset: postings / s and achieved bytes / s (20 B per posting + 8 B per passage and query)
      next to the 8 TB/s HBM peak
  (b) latency of one hybrid query on the device (scoring + injection + rerank on a 50-entry ANN list).  The host figure beside it is
      the CSR list walk of tests/bm25_ref.py in numpy on this CPU, NOT the scorer this index replaces: that one probes one hash map
      per passage and token on top of the same arithmetic, so the list walk is a lower bound for it
  (c) the BM25 + rerank leg for a batch (default 16 384 queries) with BM25 scoring INSIDE the timed region, on random ANN lists resident
      in HBM — WITHOUT the graph walk; `with_walk_queries_per_s` adds --walk-ms-per-batch (default: the 31.6 ms per 16 384 queries of
      the recorded vamana10m1536_r32 --hybrid run, scaled to the batch) and is a derived figure, not a measurement
  (d) the same batch at 64 positives per query through leann_hybrid_rerank_device (the sparse call), to show it did not get slower
  (e) --allow-share S[,S...]: (a) and (c) again under one random allow-bitmap that allows a share S of the passages (the *_filtered
      calls), each next to the unmasked call on the same queries in the same run.  Scoring and reset are the same work in both, so the
      difference of the two (a) times is the selection sweep's; `masked_over_unmasked` is the ratio of the whole calls
  (f) --query-by-query N: the hybrid leg for the first N queries of (c) one call per query — the shape of a host that cannot batch —
      next to one call for the same N queries

  python scripts/bm25_bench.py [--passages 10000000] [--terms 20000] [--batch 16384] [--repeats 5] [--allow-share 1.0,0.1,0.01]
Warm-up runs first, medians of `--repeats` timed runs (host wall clock around calls that return when the device is done; outputs are
allocated before the clock starts).  Every step runs under --step-limit seconds; a step that exceeds it ends the script.  Each line
carries `overflow_fallbacks`: how often a chunk's candidate lists overflowed and the segment sorter selected instead (counted from
the library's debug log)."""
import argparse
import json
import os
import signal
import sys
import tempfile
import time

os.environ["LEANN_LOG"] = "debug"  # read once when the library loads: the overflow fallback is reported there

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import bm25_ref  # noqa: E402
import leann_rs_amd as la  # noqa: E402

HBM_PEAK = 8.0e12


def synth_corpus_blocked(seed, n_docs, n_terms, block=500_000):
    """bm25_ref.synth_corpus in blocks of passages (same law, bounded memory): CSR by (term, passage)"""
    rng = np.random.default_rng(seed)
    cdf = np.cumsum(bm25_ref.zipf_probabilities(n_terms, 1.1))
    cdf[-1] = 1.0
    doc_len = rng.integers(40, 121, size=n_docs).astype(np.uint32)
    parts, counts = [], np.zeros(n_terms, np.int64)
    for d0 in range(0, n_docs, block):
        dl = doc_len[d0:d0 + block]
        term = np.searchsorted(cdf, rng.random(int(dl.sum())), side="right").astype(np.uint64)
        doc = np.repeat(np.arange(d0, d0 + len(dl), dtype=np.uint64), dl)
        pair, tf = np.unique(term * np.uint64(n_docs) + doc, return_counts=True)
        t = (pair // np.uint64(n_docs)).astype(np.int64)
        parts.append((t, (pair % np.uint64(n_docs)).astype(np.uint32), tf.astype(np.uint32)))
        counts += np.bincount(t, minlength=n_terms)
        print(f"bm25_bench: corpus, {min(d0 + block, n_docs)} of {n_docs} passages", file=sys.stderr, flush=True)
    post_off = np.zeros(n_terms + 1, np.uint64)
    post_off[1:] = np.cumsum(counts, dtype=np.uint64)
    post_doc, post_tf = np.empty(int(post_off[-1]), np.uint32), np.empty(int(post_off[-1]), np.uint32)
    fill = post_off[:-1].astype(np.int64).copy()
    for t, d, f in parts:  # blocks ascend in passage id, so lists stay ascending
        c = np.bincount(t, minlength=n_terms)
        start = np.repeat(fill - np.concatenate([[0], np.cumsum(c)[:-1]]), c)
        at = start + np.arange(len(t))
        post_doc[at], post_tf[at] = d, f
        fill += c
    avg = np.float32(doc_len.sum(dtype=np.int64)) / np.float32(n_docs)
    return bm25_ref.Postings(n_docs, post_off, post_doc, post_tf, doc_len, avg)


STEP_LIMIT = 300


def _too_long(signum, frame):
    raise SystemExit("bm25_bench: a step exceeded --step-limit; stopping here")


def timed(fn, warmup, repeats):
    """median seconds of `repeats` runs after `warmup`, and the overflow fallbacks the library logged during all of them"""
    signal.signal(signal.SIGALRM, _too_long)
    signal.alarm(STEP_LIMIT)
    sys.stderr.flush()
    log = tempfile.TemporaryFile()
    saved = os.dup(2)
    os.dup2(log.fileno(), 2)
    try:
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(repeats):
            la.sync()
            t0 = time.perf_counter()
            fn()
            la.sync()
            ts.append(time.perf_counter() - t0)
    finally:
        os.dup2(saved, 2)
        os.close(saved)
        signal.alarm(0)
    log.seek(0)
    return float(np.median(ts)), log.read().count(b"candidate list overflowed") / (warmup + repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passages", type=int, default=10_000_000)
    ap.add_argument("--terms", type=int, default=20_000)
    ap.add_argument("--batch", type=int, default=16_384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-limit", type=int, default=300)
    ap.add_argument("--walk-ms-per-batch", type=float, default=None)
    ap.add_argument("--allow-share", default="", help="comma-separated shares of allowed passages, e.g. 1.0,0.1,0.01")
    ap.add_argument("--query-by-query", type=int, default=0, metavar="N")
    a = ap.parse_args()
    global STEP_LIMIT
    STEP_LIMIT = a.step_limit
    if la.device_count() < 1:
        raise SystemExit("bm25_bench: no HIP device visible")
    t0 = time.perf_counter()
    post = synth_corpus_blocked(20250, a.passages, a.terms)
    idx = la.Bm25Index.from_postings(post.n_docs, post.post_off, post.post_doc, post.post_tf, post.doc_len, post.avg_doc_len)
    print(json.dumps(dict(what="corpus", passages=a.passages, terms=a.terms, postings=int(post.post_off[-1]), slots=idx.slots,
                          build_s=round(time.perf_counter() - t0, 1))), flush=True)
    rng = np.random.default_rng(1)
    fetch_k, top_k = 50, 10

    def pack(queries):
        q_off = np.zeros(len(queries) + 1, np.uint32)
        q_off[1:] = np.cumsum([len(q) for q in queries])
        flat = np.array([t for q in queries for t in q], np.int64)
        df = (post.post_off[flat + 1] - post.post_off[flat]).astype(np.int64)
        idf_of = {}
        for t, d in zip(flat.tolist(), df.tolist()):
            if t not in idf_of:
                idf_of[t] = bm25_ref.idf(post.n_docs, d)
        return (q_off, flat.astype(np.uint32), np.array([idf_of[t] for t in flat.tolist()], np.float32)), int(df.sum())

    def ann_lists(nq):
        keys = rng.integers(0, post.n_docs, size=(nq, fetch_k)).astype(np.uint64)
        dists = np.sort(rng.uniform(0.05, 1.2, size=(nq, fetch_k)).astype(np.float32), axis=1)
        return la.DeviceArray.from_host(keys), la.DeviceArray.from_host(dists), la.DeviceArray.from_host(np.full(nq, fetch_k, np.uint32))

    # (a) a few chunks of queries: scoring + selection + reset
    nqa = 4 * idx.slots
    packed, postings = pack(bm25_ref.synth_queries(13, nqa, a.terms))
    out = idx.search_batch_device(packed, fetch_k)  # results stay in HBM, outputs allocated once
    med, ovf = timed(lambda: idx.search_batch_device(packed, fetch_k, out=out), a.warmup, a.repeats)
    nbytes = 20 * postings + 8 * post.n_docs * nqa
    print(json.dumps(dict(what="a_score_select_reset", queries=nqa, postings_streamed=postings, seconds=med, postings_per_s=postings / med,
                          bytes_per_s=nbytes / med, fraction_of_hbm_peak=nbytes / med / HBM_PEAK, us_per_query=med / nqa * 1e6,
                          overflow_fallbacks=ovf)), flush=True)
    # the same with one-token queries: few distinct scores, so ties with the k-th best crowd the candidate lists
    packed1, postings1 = pack([[q[0]] for q in bm25_ref.synth_queries(16, nqa, a.terms)])
    med, ovf = timed(lambda: idx.search_batch_device(packed1, fetch_k, out=out), a.warmup, a.repeats)
    nbytes = 20 * postings1 + 8 * post.n_docs * nqa
    print(json.dumps(dict(what="a1_one_token_queries", queries=nqa, postings_streamed=postings1, seconds=med, postings_per_s=postings1 / med,
                          bytes_per_s=nbytes / med, fraction_of_hbm_peak=nbytes / med / HBM_PEAK, us_per_query=med / nqa * 1e6,
                          overflow_fallbacks=ovf)), flush=True)
    # (b) one hybrid query
    one, one_postings = pack(bm25_ref.synth_queries(14, 1, a.terms))
    dk, dd, dc = ann_lists(1)
    med, ovf = timed(lambda: idx.hybrid_rerank_device(one, dk, dd, dc, fetch_k, 0.7, True, top_k), 3, max(a.repeats, 9))
    terms = one[1].tolist()
    th = time.perf_counter()
    post.search(terms, fetch_k)
    host = time.perf_counter() - th
    print(json.dumps(dict(what="b_one_hybrid_query", device_ms=med * 1e3, postings=one_postings, host_numpy_list_walk_ms=host * 1e3, overflow_fallbacks=ovf)), flush=True)
    # (c) the batch, BM25 inside the timed region
    packed, postings = pack(bm25_ref.synth_queries(15, a.batch, a.terms))
    dk, dd, dc = ann_lists(a.batch)
    med, ovf = timed(lambda: idx.hybrid_rerank_device(packed, dk, dd, dc, fetch_k, 0.7, True, top_k), 1, max(3, a.repeats // 2))
    walk = (a.walk_ms_per_batch if a.walk_ms_per_batch is not None else 31.6 * a.batch / 16384) * 1e-3
    print(json.dumps(dict(what="c_batch_bm25_plus_rerank_without_walk", queries=a.batch, seconds=med, queries_per_s=a.batch / med,
                          postings_per_s=postings / med, overflow_fallbacks=ovf, assumed_walk_seconds=walk,
                          with_walk_queries_per_s_derived=a.batch / (med + walk))), flush=True)
    # (e) under an allow-bitmap, beside the unmasked call on the same queries
    packed_a, postings_a = pack(bm25_ref.synth_queries(13, nqa, a.terms))
    for share in [float(x) for x in a.allow_share.split(",") if x]:
        member = np.ones(post.n_docs, bool) if share >= 1.0 else rng.random(post.n_docs) < share
        d_allow = la.DeviceArray.from_host(np.packbits(member, bitorder="little"))
        plain, _ = timed(lambda: idx.search_batch_device(packed_a, fetch_k, out=out), a.warmup, a.repeats)
        masked, ovf = timed(lambda: idx.search_batch_device(packed_a, fetch_k, out=out, allow=d_allow), a.warmup, a.repeats)
        print(json.dumps(dict(what="e_score_select_reset_masked", allow_share=share, allowed=int(member.sum()), queries=nqa,
                              unmasked_seconds=plain, masked_seconds=masked, masked_over_unmasked=masked / plain,
                              sweep_difference_us_per_query=(masked - plain) / nqa * 1e6, overflow_fallbacks=ovf)), flush=True)
        plain, _ = timed(lambda: idx.hybrid_rerank_device(packed, dk, dd, dc, fetch_k, 0.7, True, top_k), 1, max(3, a.repeats // 2))
        masked, ovf = timed(lambda: idx.hybrid_rerank_device(packed, dk, dd, dc, fetch_k, 0.7, True, top_k, allow=d_allow), 1,
                            max(3, a.repeats // 2))
        print(json.dumps(dict(what="e_batch_bm25_plus_rerank_masked", allow_share=share, queries=a.batch, unmasked_seconds=plain,
                              masked_seconds=masked, masked_over_unmasked=masked / plain, masked_queries_per_s=a.batch / masked,
                              overflow_fallbacks=ovf)), flush=True)
        d_allow.free()
    # (f) one call per query against one call for all of them
    if a.query_by_query:
        n1 = min(a.query_by_query, a.batch)
        q_off, q_term, q_idf = packed
        singles = [(np.array([0, q_off[i + 1] - q_off[i]], np.uint32), q_term[q_off[i]:q_off[i + 1]], q_idf[q_off[i]:q_off[i + 1]])
                   for i in range(n1)]
        lists1 = [ann_lists(1) for _ in range(n1)]
        head = (q_off[:n1 + 1].copy(), q_term[:q_off[n1]], q_idf[:q_off[n1]])
        dkn, ddn, dcn = ann_lists(n1)

        def one_by_one():
            for qq, (k1, d1, c1) in zip(singles, lists1):
                idx.hybrid_rerank_device(qq, k1, d1, c1, fetch_k, 0.7, True, top_k)
        each, _ = timed(one_by_one, 1, 3)
        together, _ = timed(lambda: idx.hybrid_rerank_device(head, dkn, ddn, dcn, fetch_k, 0.7, True, top_k), 1, 3)
        print(json.dumps(dict(what="f_query_by_query_against_one_call", queries=n1, query_by_query_seconds=each, one_call_seconds=together,
                              query_by_query_queries_per_s=n1 / each, one_call_queries_per_s=n1 / together)), flush=True)
    # (d) the sparse call at 64 positives per query
    stride = 64
    pos = np.sort(rng.integers(0, post.n_docs, size=(a.batch, stride)).astype(np.uint32), axis=1)
    sc = -np.sort(-rng.uniform(0.5, 9.0, size=(a.batch, stride)).astype(np.float32), axis=1)
    dp, ds, dn = la.DeviceArray.from_host(pos), la.DeviceArray.from_host(sc), la.DeviceArray.from_host(np.full(a.batch, stride, np.uint32))
    ok, os_, oc = la.DeviceArray((a.batch, top_k), np.uint64), la.DeviceArray((a.batch, top_k), np.float32), la.DeviceArray(a.batch, np.uint32)

    def sparse():
        la._native.check(la.lib().leann_hybrid_rerank_device(dk.ptr, dd.ptr, dc.ptr, a.batch, fetch_k, dp.ptr, ds.ptr, dn.ptr, stride,
                                                             post.n_docs, 0.7, 1, top_k, ok.ptr, os_.ptr, oc.ptr, None))
        la.sync()
    med, _ = timed(sparse, a.warmup, a.repeats)
    print(json.dumps(dict(what="d_sparse_rerank_64_positives", queries=a.batch, seconds=med, queries_per_s=a.batch / med)), flush=True)
    idx.close()


if __name__ == "__main__":
    main()
