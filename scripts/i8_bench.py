#!/usr/bin/env python3
"""int8 rows against bf16 and f32 rows on the same graph (DESIGN.md "int8 rows"): one GPU, synthetic rows, bench.py's headline
parameters.

    python scripts/i8_bench.py [--rows 10000000] [--dims 768] [--out profiles/i8_rows_10m768.json] [--md profiles/i8_rows.md]

Builds the f32 index H on the device, makes B = H.to_rows(BF16) and Q = H.to_rows(I8) — the SAME graph, so the comparison isolates
the rows — and times, alternating, with device events, batches of resident queries through
    f32_whole   H with the row screen off (whole f32 rows),
    f32_screen  H with the row screen on (the default at this size),
    bf16        B,
    i8          Q.
Per leg: queries/s of every repeat, their spread, evaluations per query, recall@10 against exact f32 ground truth
(leann_scan_topk_device on the f32 rows, held-out queries) and algorithmic bytes over time as a share of the 8 TB/s HBM peak.  Then
the smallest ef at which Q reaches H's recall at the base ef, and Q's queries/s there.  One JSON file and a short markdown record,
which also says what was not measured."""
import argparse
import ctypes as C
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
    ap.add_argument("--rows", type=int, default=10_000_000)
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
    ap.add_argument("--ef-max", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i8_rows_10m768.json"))
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "i8_rows.md"))
    a = ap.parse_args()
    if a.dims % 4:  # rows and queries are generated with pitch ld = dims rounded up to 4; the library reads queries with pitch dims
        sys.exit("i8_bench.py: --dims must be a multiple of 4")

    import torch
    import leann_rs_amd as la
    L, chk = la.lib(), la._native.check
    dev = torch.device("cuda:0")
    n, d, k, B = a.rows, a.dims, a.k, a.batch
    ld = (d + 3) & ~3
    sp = None

    t0 = time.time()
    X = torch.empty((n, ld), dtype=torch.float32, device=dev)
    chk(L.leann_synth_rows_device(SEED, d, ld, GEN_R, GEN_CLUSTERS, GEN_SIGMA, 0, 0, n, X.data_ptr(), sp))
    nq_all = a.batches * B + a.recall_queries
    Q = torch.empty((nq_all, ld), dtype=torch.float32, device=dev)
    chk(L.leann_synth_rows_device(SEED, d, ld, GEN_R, GEN_CLUSTERS, GEN_SIGMA, 1, 0, nq_all, Q.data_ptr(), sp))
    torch.cuda.synchronize()
    Qr = Q[a.batches * B:]  # held out: never timed
    print(f"rows [{n} x {d}] and {nq_all} queries generated in {time.time() - t0:.1f}s", flush=True)

    t0 = time.time()
    H = la.BackendSearcher.build_device(la.BackendType.Hnsw, X.data_ptr(), n, d, ld, a.M, a.efc)
    torch.cuda.synchronize()
    build_s = time.time() - t0
    print(f"f32 index built in {build_s:.1f}s", flush=True)
    t0 = time.time()
    Bh = H.to_rows(la.RowType.BF16)
    torch.cuda.synchronize()
    to_rows_s = time.time() - t0
    print(f"to_rows(BF16) in {to_rows_s:.1f}s", flush=True)
    t0 = time.time()
    Qh = H.to_rows(la.RowType.I8)
    torch.cuda.synchronize()
    to_i8_s = time.time() - t0
    print(f"to_rows(I8) in {to_i8_s:.1f}s", flush=True)
    H.set_row_screen(True)  # cuts the planes now if the automatic mode has not (small --rows)
    gi = H.graph_info()

    gt_k = torch.empty((a.recall_queries, k), dtype=torch.int64, device=dev)
    gt_s = torch.empty((a.recall_queries, k), dtype=torch.float32, device=dev)
    gt_c = torch.empty((a.recall_queries,), dtype=torch.int32, device=dev)
    chk(L.leann_scan_topk_device(X.data_ptr(), n, d, ld, Qr.data_ptr(), a.recall_queries, k, None, 0, gt_k.data_ptr(), gt_s.data_ptr(),
                                 gt_c.data_ptr(), sp))
    torch.cuda.synchronize()
    truth = gt_k.cpu().numpy()

    keys = torch.empty((B, k), dtype=torch.int64, device=dev)
    dists = torch.empty((B, k), dtype=torch.float32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    stats = torch.zeros((B, 4), dtype=torch.int32, device=dev)

    legs = {"f32_whole": (H, False, 4), "f32_screen": (H, True, 4), "bf16": (Bh, None, 2), "i8": (Qh, None, 1)}

    def select(name):
        s, screen, _ = legs[name]
        if screen is not None:
            s.set_row_screen(screen)
        return s

    def run(s, ef, with_stats=False):
        for b in range(a.batches):
            s.search_batch_device(Q[b * B:].data_ptr(), B, k, ef, keys.data_ptr(), dists.data_ptr(), counts.data_ptr(),
                                  stats.data_ptr() if with_stats else None, sp)

    def timed(s, ef):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(s, ef)
        e1.record()
        e1.synchronize()
        return a.batches * B / (e0.elapsed_time(e1) * 1e-3)

    def recall(s, ef):
        rk = torch.empty((a.recall_queries, k), dtype=torch.int64, device=dev)
        rd = torch.empty((a.recall_queries, k), dtype=torch.float32, device=dev)
        rc = torch.empty((a.recall_queries,), dtype=torch.int32, device=dev)
        s.search_batch_device(Qr.data_ptr(), a.recall_queries, k, ef, rk.data_ptr(), rd.data_ptr(), rc.data_ptr(), None, sp)
        torch.cuda.synchronize()
        got = rk.cpu().numpy()
        return float(np.mean([len(set(got[i].tolist()) & set(truth[i].tolist())) / k for i in range(a.recall_queries)]))

    res = {name: dict(qps=[]) for name in legs}
    for name in legs:
        s = select(name)
        for _ in range(a.warmup):
            run(s, a.ef)
        torch.cuda.synchronize()
    for rep in range(a.repeats):  # alternating: every repeat visits every leg
        for name in legs:
            res[name]["qps"].append(timed(select(name), a.ef))
        print(f"repeat {rep}: " + ", ".join(f"{nm} {res[nm]['qps'][-1] / 1e3:.0f} k q/s" for nm in legs), flush=True)
    for name, (s, _, elem) in legs.items():
        s = select(name)
        stats.zero_()
        s.search_batch_device(Q.data_ptr(), B, k, a.ef, keys.data_ptr(), dists.data_ptr(), counts.data_ptr(), stats.data_ptr(), sp)
        torch.cuda.synchronize()
        st = stats.cpu().numpy().astype(np.int64)
        evals, hops0, hopsU = (float(st[:, i].mean()) for i in range(3))
        r = res[name]
        q = np.array(r["qps"])
        r.update(qps_median=float(np.median(q)), qps_min=float(q.min()), qps_max=float(q.max()), spread=float((q.max() - q.min()) / np.median(q)),
                 evals_per_query=evals, hops_base_per_query=hops0, hops_upper_per_query=hopsU, recall_at_k=recall(s, a.ef))
        algo = evals * d * elem + hops0 * gi["M0"] * 4 + hopsU * gi["M"] * 4  # bytes a query must move (whole rows of the leg's type)
        r["algorithmic_bytes_per_query"] = algo
        r["share_of_hbm_peak"] = algo * r["qps_median"] / HBM_PEAK
    # the smallest ef at which Q reaches H's recall at the base ef
    target = res["f32_whole"]["recall_at_k"]
    match = None
    for ef in range(a.ef, a.ef_max + 1, 4):
        rec = recall(Qh, ef)
        if rec >= target:
            for _ in range(a.warmup):
                run(Qh, ef)
            q = [timed(Qh, ef) for _ in range(a.repeats)]
            match = dict(ef=ef, recall_at_k=rec, qps=q, qps_median=float(np.median(q)))
            break
    w, s_, b, q8 = res["f32_whole"], res["f32_screen"], res["bf16"], res["i8"]
    out = dict(rows=n, dims=d, M=a.M, efc=a.efc, k=k, ef=a.ef, batch=B, batches_per_repeat=a.batches, repeats=a.repeats,
               recall_queries=a.recall_queries, build_s=build_s, to_rows_bf16_s=to_rows_s, to_rows_i8_s=to_i8_s, legs=res,
               i8_ef_matching_f32_recall=match,
               i8_over_f32_whole=q8["qps_median"] / w["qps_median"], i8_over_f32_screen=q8["qps_median"] / s_["qps_median"],
               i8_over_bf16=q8["qps_median"] / b["qps_median"], i8_beats_bf16_beyond_spread=bool(q8["qps_min"] > b["qps_max"]),
               device_row_bytes=dict(f32=n * ld * 4, f32_planes=n * ((ld + 63) & ~63) * 4, bf16=n * ((d + 63) & ~63) * 2, i8=n * ((d + 127) & ~127)),
               device=torch.cuda.get_device_name(0),
               device_note="`device` is the name torch reports; the recorded run was made on an AMD Instinct MI355X (gfx950), which torch names 'AMD Radeon Graphics'",
               not_measured="other widths than this one; the filtered and the wide-list kernels; batches small enough for the 16-wave kernels")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    with open(a.md, "w") as f:
        f.write(f"# int8 rows against bf16 and f32 rows, one graph ({n} x {d}, HNSW M = {a.M}, efc = {a.efc}, k = {k}, ef = {a.ef})\n\n")
        f.write(f"`python scripts/i8_bench.py --rows {n} --dims {d}` on {out['device']}: H = f32 index built on the device, B = `to_rows(H, BF16)`, "
                f"Q = `to_rows(H, I8)` (same graph; `device` is torch's name for the GPU: an MI355X reports itself as 'AMD Radeon Graphics'); "
                f"batches of {B} resident queries, {a.repeats} alternating timed repeats of {a.batches} batches each after {a.warmup} warm-up rounds, "
                f"device events; recall@{k} on {a.recall_queries} held-out queries against the exact f32 scan.  Raw numbers: `{os.path.basename(a.out)}`.\n\n")
        f.write("| leg | queries/s (median) | min .. max | spread | evaluations / query | recall@%d | algorithmic bytes / time, share of 8 TB/s |\n" % k)
        f.write("|---|---|---|---|---|---|---|\n")
        for name, label in (("f32_whole", "H, row screen off (whole f32 rows)"), ("f32_screen", "H, row screen on (default at this size)"),
                            ("bf16", "B (bf16 rows)"), ("i8", "Q (int8 rows)")):
            r = res[name]
            f.write(f"| {label} | {r['qps_median']:.0f} | {r['qps_min']:.0f} .. {r['qps_max']:.0f} | {100 * r['spread']:.1f} % | {r['evals_per_query']:.1f} | "
                    f"{r['recall_at_k']:.4f} | {r['share_of_hbm_peak']:.2f} |\n")
        f.write(f"\nQ over B: {out['i8_over_bf16']:.2f} x (Q's slowest repeat {'above' if out['i8_beats_bf16_beyond_spread'] else 'NOT above'} B's fastest); "
                f"over whole-row H: {out['i8_over_f32_whole']:.2f} x; over screened H: {out['i8_over_f32_screen']:.2f} x.  "
                f"Recall difference Q - H: {q8['recall_at_k'] - w['recall_at_k']:+.4f} (B - H: {b['recall_at_k'] - w['recall_at_k']:+.4f}).\n")
        if match:
            f.write(f"\nSmallest ef at which Q reaches H's recall at ef = {a.ef} ({target:.4f}): ef = {match['ef']} (recall {match['recall_at_k']:.4f}), "
                    f"{match['qps_median']:.0f} queries/s there.\n")
        else:
            f.write(f"\nQ does not reach H's recall at ef = {a.ef} ({target:.4f}) up to ef = {a.ef_max}.\n")
        f.write(f"\nDevice memory for rows: f32 {out['device_row_bytes']['f32'] / 1e9:.1f} GB (+ {out['device_row_bytes']['f32_planes'] / 1e9:.1f} GB of split planes "
                f"with the screen), bf16 {out['device_row_bytes']['bf16'] / 1e9:.1f} GB, int8 {out['device_row_bytes']['i8'] / 1e9:.1f} GB.  "
                f"Build {build_s:.1f} s, to_rows(BF16) {to_rows_s:.1f} s, to_rows(I8) {to_i8_s:.1f} s.\n")
        f.write(f"\nNot measured: {out['not_measured']}.\n")
    print(json.dumps({k_: out[k_] for k_ in ("i8_over_bf16", "i8_over_f32_whole", "i8_over_f32_screen", "i8_beats_bf16_beyond_spread")}), flush=True)
    Qh.close()
    Bh.close()
    H.close()


if __name__ == "__main__":
    main()
