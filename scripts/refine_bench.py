#!/usr/bin/env python3
"""Refining search results on exact f32 rows: what it costs and what it gives back, on one GPU, synthetic rows,
bench.py's headline parameters.

    python scripts/refine_bench.py [--rows 1000000] [--dims 768] [--out profiles/refine_1m768.json] [--md profiles/refine.md]

Builds the f32 index H on the device, makes Q = H.to_rows(I8) and B = H.to_rows(BF16) — the SAME graph — and keeps the exact rows a
second time as ExactRows in HBM and in pinned host memory.  Timed, alternating, with device events, batches of resident queries:
    H plain, Q plain, Q refined at fetch_k in {10, 20, 40} with the exact rows in HBM and on the host, B refined at fetch_k = 20.
Per leg: queries/s of every repeat, their spread, recall@10 against exact f32 ground truth on held-out queries.  Then the rerank kernel
alone on the walk's lists (device events around repeated launches) against the bytes it reads, as a share of the 8 TB/s HBM peak for
rows in HBM and of the host-to-device copy rate measured in the same run for rows on the host; and one query per call (host clock
around calls that end in a synchronise).  One JSON file and a short markdown record, which also says what was not measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SEED, GEN_R, GEN_CLUSTERS, GEN_SIGMA = 0x5EED0001, 64, 4096, 1.0  # bench.py's synthetic set
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dims", type=int, default=768)
    ap.add_argument("--M", type=int, default=32)
    ap.add_argument("--efc", type=int, default=200)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=56)
    ap.add_argument("--batch", type=int, default=16384)
    ap.add_argument("--batches", type=int, default=4, help="distinct resident query batches; one timed repeat runs all of them")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--recall-queries", type=int, default=2000)
    ap.add_argument("--single-calls", type=int, default=300)
    ap.add_argument("--no-host", action="store_true", help="skip the legs with the exact rows in pinned host memory")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_1m768.json"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "refine.md"))
    a = ap.parse_args()
    if a.dims % 4:  # rows and queries are generated with pitch ld = dims rounded up to 4; the library reads queries with pitch dims
        sys.exit("refine_bench.py: --dims must be a multiple of 4")

    import torch
    import leann_rs_amd as la
    L, chk = la.lib(), la._native.check
    if la.device_count() < 1:
        sys.exit("refine_bench.py: no HIP device visible; nothing is measured without one")
    dev = torch.device("cuda:0")
    n, d, k, B = a.rows, a.dims, a.k, a.batch
    sp = None

    t0 = time.time()
    X = torch.empty((n, d), dtype=torch.float32, device=dev)
    chk(L.leann_synth_rows_device(SEED, d, d, GEN_R, GEN_CLUSTERS, GEN_SIGMA, 0, 0, n, X.data_ptr(), sp))
    nq_all = a.batches * B + a.recall_queries
    Q = torch.empty((nq_all, d), dtype=torch.float32, device=dev)
    chk(L.leann_synth_rows_device(SEED, d, d, GEN_R, GEN_CLUSTERS, GEN_SIGMA, 1, 0, nq_all, Q.data_ptr(), sp))
    torch.cuda.synchronize()
    Qr = Q[a.batches * B:]  # held out: never timed
    print(f"rows [{n} x {d}] and {nq_all} queries generated in {time.time() - t0:.1f}s", flush=True)

    t0 = time.time()
    H = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.data_ptr(), n, d, d, a.M, a.efc)
    torch.cuda.synchronize()
    build_s = time.time() - t0
    Qh, Bh = H.to_rows(la.RowType.I8), H.to_rows(la.RowType.BF16)
    H.set_row_screen(False)  # whole f32 rows: the plain f32 walk the refined distances are defined by
    print(f"f32 index built in {build_s:.1f}s; int8 and bf16 twins made", flush=True)

    rows = {"hbm": la.ExactRows.from_device(X.data_ptr(), n, d, d)}  # (borrowed: the rows H was built on)
    h2d_rate = None
    if not a.no_host:
        t0 = time.time()
        Xh = X.cpu().numpy()
        rows["host"] = la.ExactRows.from_host(Xh, placement="host")
        del Xh
        print(f"exact rows copied into pinned host memory in {time.time() - t0:.1f}s", flush=True)
        # the bus: a pinned 1 GiB block copied to the device, device events, best of 5
        pin = torch.empty(1 << 28, dtype=torch.float32).pin_memory()
        dst = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        best = 0.0
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(pin, non_blocking=True)
            e1.record()
            e1.synchronize()
            best = max(best, pin.numel() * 4 / (e0.elapsed_time(e1) * 1e-3))
        h2d_rate = best
        del pin, dst
        print(f"host-to-device copy of pinned memory: {h2d_rate / 1e9:.1f} GB/s", flush=True)

    gt_k = torch.empty((a.recall_queries, k), dtype=torch.int64, device=dev)
    gt_s = torch.empty((a.recall_queries, k), dtype=torch.float32, device=dev)
    gt_c = torch.empty((a.recall_queries,), dtype=torch.int32, device=dev)
    chk(L.leann_scan_topk_device(X.data_ptr(), n, d, d, Qr.data_ptr(), a.recall_queries, k, None, 0, gt_k.data_ptr(), gt_s.data_ptr(),
                                 gt_c.data_ptr(), sp))
    torch.cuda.synchronize()
    truth = gt_k.cpu().numpy()

    keys = torch.empty((B, k), dtype=torch.int64, device=dev)
    dists = torch.empty((B, k), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)

    # leg -> (searcher, fetch_k or None for the plain search, placement)
    legs = {"H plain": (H, None, None), "Q plain": (Qh, None, None)}
    for placement in rows:
        for fk in (10, 20, 40):
            legs[f"Q refined {fk} {placement}"] = (Qh, fk, placement)
    legs["B refined 20 hbm"] = (Bh, 20, "hbm")

    def search(leg, q_ptr, nq, ok, od, oc):
        s, fk, placement = legs[leg]
        if fk is None:
            s.search_batch_device(q_ptr, nq, k, a.ef, ok.data_ptr(), od.data_ptr(), oc.data_ptr(), None, sp)
        else:
            s.search_refined_batch_device(rows[placement], q_ptr, nq, k, fk, a.ef, ok.data_ptr(), od.data_ptr(), oc.data_ptr(), stream=sp)

    def run(leg):
        for b in range(a.batches):
            search(leg, Q[b * B:].data_ptr(), B, keys, dists, counts)

    def timed(leg):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(leg)
        e1.record()
        e1.synchronize()
        return a.batches * B / (e0.elapsed_time(e1) * 1e-3)

    def recall(leg):
        rk = torch.empty((a.recall_queries, k), dtype=torch.int64, device=dev)
        rd = torch.empty((a.recall_queries, k), dtype=torch.float32, device=dev)
        rc = torch.empty((a.recall_queries,), dtype=torch.int32, device=dev)
        search(leg, Qr.data_ptr(), a.recall_queries, rk, rd, rc)
        torch.cuda.synchronize()
        got = rk.cpu().numpy()
        return float(np.mean([len(set(got[i].tolist()) & set(truth[i].tolist())) / k for i in range(a.recall_queries)]))

    res = {leg: dict(qps=[]) for leg in legs}
    for leg in legs:
        for _ in range(a.warmup):
            run(leg)
        torch.cuda.synchronize()
    for rep in range(a.repeats):  # alternating: every repeat visits every leg
        for leg in legs:
            res[leg]["qps"].append(timed(leg))
        print(f"repeat {rep}: " + ", ".join(f"{leg} {res[leg]['qps'][-1] / 1e3:.0f}k" for leg in legs), flush=True)
    for leg in legs:
        q = np.array(res[leg]["qps"])
        res[leg].update(qps_median=float(np.median(q)), qps_min=float(q.min()), qps_max=float(q.max()),
                        spread=float((q.max() - q.min()) / np.median(q)), recall_at_k=recall(leg))

    # the rerank kernel alone, on the int8 walk's own lists of the first batch
    kernel = {}
    for fk in (10, 20, 40):
        wk = torch.empty((B, fk), dtype=torch.int64, device=dev)
        wd = torch.empty((B, fk), dtype=torch.float32, device=dev)
        wc = torch.empty((B,), dtype=torch.int32, device=dev)
        Qh.search_batch_device(Q.data_ptr(), B, fk, a.ef, wk.data_ptr(), wd.data_ptr(), wc.data_ptr(), None, sp)
        torch.cuda.synchronize()
        cand = int(wc.sum().item())
        nbytes = cand * d * 4 + B * d * 4 + B * fk * 8  # rows + queries + lists
        for placement in rows:
            ms = []
            for rep in range(a.warmup + a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.batches):
                    la.rerank_batch_device(rows[placement], Q.data_ptr(), B, wk.data_ptr(), wc.data_ptr(), fk, k, keys.data_ptr(),
                                           dists.data_ptr(), counts.data_ptr(), None, sp)
                e1.record()
                e1.synchronize()
                if rep >= a.warmup:
                    ms.append(e0.elapsed_time(e1) / a.batches)
            t = float(np.median(ms)) * 1e-3
            peak = HBM_PEAK if placement == "hbm" else h2d_rate
            kernel[f"{fk} {placement}"] = dict(ms_per_batch=t * 1e3, ms_all=ms, candidates=cand, bytes=nbytes, bytes_per_s=nbytes / t,
                                               share=nbytes / t / peak, of="8 TB/s HBM peak" if placement == "hbm" else "measured host-to-device copy rate")
            print(f"rerank alone, fetch_k {fk}, rows in {placement}: {t * 1e3:.3f} ms per batch of {B}, {nbytes / t / 1e9:.0f} GB/s", flush=True)

    # one query per call: the one-workgroup-per-query form is a latency chain there
    single = {}
    one_k = torch.empty((1, k), dtype=torch.int64, device=dev)
    one_d = torch.empty((1, k), dtype=torch.float32, device=dev)
    one_c = torch.empty((1,), dtype=torch.int32, device=dev)
    for leg in ["Q plain"] + [f"Q refined 20 {p}" for p in rows]:
        lat = []
        for i in range(a.single_calls + 20):
            t0 = time.perf_counter()
            search(leg, Q[i:].data_ptr(), 1, one_k, one_d, one_c)
            torch.cuda.synchronize()
            if i >= 20:
                lat.append((time.perf_counter() - t0) * 1e6)
        single[leg] = dict(us_median=float(np.median(lat)), us_p90=float(np.percentile(lat, 90)))
        print(f"one query per call, {leg}: median {single[leg]['us_median']:.0f} us", flush=True)

    out = dict(rows=n, dims=d, M=a.M, efc=a.efc, k=k, ef=a.ef, batch=B, batches_per_repeat=a.batches, repeats=a.repeats,
               recall_queries=a.recall_queries, build_s=build_s, legs=res, rerank_kernel_alone=kernel, one_query_per_call=single,
               h2d_bytes_per_s=h2d_rate, device=torch.cuda.get_device_name(0),
               device_note="`device` is the name torch reports; the recorded run was made on an AMD Instinct MI355X (gfx950)",
               not_measured=("rows in pinned host memory at this size; " if a.no_host else "") +
               "other sizes and widths than this one; refined searches under an allow-bitmap; composite handles")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    with open(a.md, "w") as f:
        f.write(f"# Refining on exact f32 rows ({n} x {d}, HNSW M = {a.M}, efc = {a.efc}, k = {k}, ef = {a.ef})\n\n")
        f.write(f"`python scripts/refine_bench.py --rows {n} --dims {d}` on {out['device']} (torch's name for the GPU: an MI355X): H = f32 index built on "
                f"the device (row screen off: whole f32 rows), Q = `to_rows(H, I8)`, B = `to_rows(H, BF16)`, one graph; the exact rows a second time in "
                f"HBM (borrowed from H){' only (--no-host: the pinned host copy and its legs were skipped)' if a.no_host else ' and in pinned host memory'}.  Batches of {B} resident queries, {a.repeats} alternating timed repeats of {a.batches} "
                f"batches each after {a.warmup} warm-up rounds, device events; recall@{k} on {a.recall_queries} held-out queries against the exact f32 "
                f"scan.  A refined call synchronises its stream before it returns (its scratch must outlive the work), a plain one does not: the "
                f"refined legs pay one host round trip per batch inside the timed window.  Raw numbers: `{os.path.basename(a.out)}`.\n\n")
        f.write(f"| leg | queries/s (median) | min .. max | spread | recall@{k} |\n|---|---|---|---|---|\n")
        for leg, r in res.items():
            f.write(f"| {leg} | {r['qps_median']:.0f} | {r['qps_min']:.0f} .. {r['qps_max']:.0f} | {100 * r['spread']:.1f} % | {r['recall_at_k']:.4f} |\n")
        f.write("\n(\"Q refined 20 hbm\": the int8 walk at fetch_k = 20, candidates scored on the exact rows in HBM; \"host\": in pinned host memory.)\n\n")
        f.write("## The rerank kernel alone\n\n`leann_rerank_batch_device` on the int8 walk's own lists of one batch, device events around "
                f"{a.batches} launches, median of {a.repeats}; bytes = candidate rows + queries + lists.\n\n")
        f.write("| fetch_k, rows in | ms per batch | GB/s | share | of |\n|---|---|---|---|---|\n")
        for name, r in kernel.items():
            f.write(f"| {name} | {r['ms_per_batch']:.3f} | {r['bytes_per_s'] / 1e9:.0f} | {100 * r['share']:.1f} % | {r['of']} |\n")
        if h2d_rate:
            f.write(f"\nHost-to-device copy of a pinned 1 GiB block in the same run: {h2d_rate / 1e9:.1f} GB/s (best of 6).  That copy is a yardstick, "
                    "not the link's ceiling: a share above 100 % says the kernel's own loads moved more per second than one copy did (its queries "
                    "and lists, counted in the bytes, come from HBM).\n")
        f.write("\n## One query per call\n\nHost clock around a call and the synchronise that ends it, after 20 unmeasured calls.\n\n| leg | median us | p90 us |\n|---|---|---|\n")
        for leg, r in single.items():
            f.write(f"| {leg} | {r['us_median']:.0f} | {r['us_p90']:.0f} |\n")
        f.write(f"\nNot measured: {out['not_measured']}.\n")
    print(f"wrote {a.out} and {a.md}")
    for r in rows.values():
        r.close()
    for s in (Qh, Bh, H):
        s.close()


if __name__ == "__main__":
    main()
