"""CPU suite: how an exhaustive top-k cuts its rows into chunks and sizes its scratch (leann-rs_amd/csrc/topk_plan.h: the one place
where the emission and the slab schedule, the slab and candidate sizes, the list capacity and the emission block's layout are
decided, for the exact scan and for the recompute search).  host/topk_plan_selftest.cpp is built with the host compiler under
AddressSanitizer + UBSan and (a) plans every point of a grid — n in {0, 1, 2047, 2048, 2049, 16383, 16384, 16385, 65535, 65536, 65537,
131072, 131073, 524288, 524289, 10^6, 10^7, 2^32 - 1}, nq in {1, 63, 64, 65, 256, 257, 4096, 16384}, k in {1, 10, 256, 257, 1024}, both
parameter sets, emission wanted and not — and checks: chunks are non-empty, contiguous from 0 and sum to n (n = 0: no chunk, one
segment, k candidates); a slab chunk never exceeds the cap and the scan's slab stays within 2^29 scores; total_segs is the sum over
slab chunks of ceil(rows / 2048), at least 1; cand_len = max(total_segs * k, k); under emission exactly chunk 0 is a slab chunk; the
emission block's pieces do not overlap, are aligned and hold `slots` entries each and slots * emit_cap keys; emit_cap = max(8192, 32 k).
(b) EXPECTED below: plans written by hand from scan_topk_impl and recompute_search_impl as they stood before there was a plan, not
computed by the new header.  The three recompute emission rows are the one intended difference: there the recompute search used to
size its slab by the widest chunk and its candidates by all chunks (slab_rows 16384, 283616 and 507904; 147, 342 and 342 segments),
although only chunk 0 ever wrote either; it now counts slab chunks only, as the exact scan always did.  No GPU, no library."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "topk_plan_selftest")

# (caller, emission wanted, n, nq, k) -> emission in force, chunks (row0, rows), slab_rows, total_segs, cand_len
EXPECTED = [
    (("scan", 0, 1, 1, 10), 0, [(0, 1)], 2048, 1, 10),
    (("scan", 1, 65536, 1, 10), 0, [(0, 65536)], 65536, 32, 320),  # not past the first emission chunk: the slab schedule
    (("scan", 1, 65537, 1, 10), 1, [(0, 65536), (65536, 1)], 65536, 32, 320),
    (("scan", 1, 600000, 5, 10), 1, [(0, 65536), (65536, 458752), (524288, 75712)], 65536, 32, 320),
    (("scan", 0, 80000, 3, 10), 0, [(0, 80000)], 80000, 40, 400),
    (("scan", 0, 1000000, 64, 10), 0, [(0, 131072), (131072, 524288), (655360, 344640)], 524288, 489, 4890),
    # 4096 queries: slab chunks of at most 2^29 / 4096 rows
    (("scan", 0, 1000000, 4096, 10), 0, [(i * 131072, 131072) for i in range(7)] + [(917504, 82496)], 131072, 489, 4890),
    # 16384 queries: the cap of 32768 rows holds for the first emission chunk, not for the emitted ones
    (("scan", 1, 1000000, 16384, 10), 1, [(0, 32768), (32768, 458752), (491520, 508480)], 32768, 16, 160),
    (("recompute", 1, 16384, 9, 10), 0, [(0, 16384)], 16384, 8, 80),  # one chunk: nothing to emit
    (("recompute", 1, 300000, 3, 10), 1, [(0, 16384), (16384, 283616)], 16384, 8, 80),
    (("recompute", 1, 700000, 150, 10), 1, [(0, 16384), (16384, 507904), (524288, 175712)], 16384, 8, 80),
    (("recompute", 0, 700000, 150, 10), 0, [(0, 131072), (131072, 524288), (655360, 44640)], 524288, 342, 3420),
    (("recompute", 0, 10000000, 64, 10), 0, [(0, 131072), (131072, 524288), (655360, 2097152), (2752512, 4194304), (6946816, 3053184)],
     4194304, 4883, 48830),
    # the recompute workload at 10^7 passages: chunks of 16384, 507904 and 9475712 rows, a slab of 16384
    (("recompute", 1, 10000000, 64, 10), 1, [(0, 16384), (16384, 507904), (524288, 9475712)], 16384, 8, 80),
]

# (caller, nq, k) -> emit_cap, slots, byte offsets of cnt / overflow / list (thr at 0), bytes: one layout for both searches,
# [slots f32 thr | slots u32 cnt | u32 overflow | pad to 256 | slots x emit_cap u64 list]
BLOCKS = [
    (("scan", 1, 10), 8192, 64, 256, 512, 768, 768 + 8 * 64 * 8192),
    (("scan", 65, 10), 8192, 128, 512, 1024, 1280, 1280 + 8 * 128 * 8192),
    (("scan", 16384, 10), 8192, 16384, 65536, 131072, 131328, 131328 + 8 * 16384 * 8192),
    (("scan", 64, 1024), 32768, 64, 256, 512, 768, 768 + 8 * 64 * 32768),
    (("recompute", 3, 10), 8192, 256, 1024, 2048, 2304, 2304 + 8 * 256 * 8192),
    (("recompute", 257, 257), 8224, 256, 1024, 2048, 2304, 2304 + 8 * 256 * 8224),
]


@pytest.fixture(scope="module")
def selftest():
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/topk_plan_selftest"])  # a no-op when up to date
    return EXE


def _plans(selftest, cases):
    text = "".join(" ".join(str(v) for v in case) + "\n" for case in cases)
    p = subprocess.run([selftest, "--plans"], input=text.encode(), stdout=subprocess.PIPE, check=True)
    got = [json.loads(line) for line in p.stdout.decode().splitlines()]
    assert len(got) == len(cases)
    return got


def test_invariants_over_the_grid(selftest):
    p = subprocess.run([selftest], stdout=subprocess.PIPE, check=False)
    r = json.loads(p.stdout)
    assert r["cases"] == 18 * 8 * 5 * 2 * 2
    assert 0 < r["emitting"] < r["cases"] // 2
    for key in ("bad_cover", "bad_cap", "bad_slab", "bad_segs", "bad_cand", "bad_emit", "bad_schedule", "bad_block", "bad_emit_cap"):
        assert r[key] == 0, r
    assert p.returncode == 0


def test_plans_written_by_hand(selftest):
    for row, g in zip(EXPECTED, _plans(selftest, [row[0] for row in EXPECTED])):
        got = (g["emit"], [tuple(c) for c in g["chunks"]], g["slab_rows"], g["total_segs"], g["cand_len"])
        assert got == row[1:], (row, g)


def test_emission_block_written_by_hand(selftest):
    for row, g in zip(BLOCKS, _plans(selftest, [(who, 1, 1000000, nq, k) for who, nq, k in (row[0] for row in BLOCKS)])):
        got = (g["emit_cap"], g["slots"], g["cnt_off"], g["overflow_off"], g["list_off"], g["emit_bytes"])
        assert got == row[1:], (row, g)
        # the kernels index the block by slot: `slots` floats, `slots` u32, the flag, then a list aligned to 8 bytes
        assert g["cnt_off"] >= 4 * g["slots"] and g["overflow_off"] >= g["cnt_off"] + 4 * g["slots"]
        assert g["list_off"] >= g["overflow_off"] + 4 and g["list_off"] % 8 == 0


def test_no_plan_for_nothing(selftest):
    (g,) = _plans(selftest, [("recompute", 1, 0, 4, 7)])
    assert (g["emit"], g["chunks"], g["slab_rows"], g["total_segs"], g["cand_len"]) == (0, [], 2048, 1, 7)
