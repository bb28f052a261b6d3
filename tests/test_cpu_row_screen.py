"""CPU suite: the bound of the split-plane row screen (leann-rs_amd/csrc/row_screen.h).  host/row_screen_selftest.cpp restates the
canonical distance chain and the screen's chain in the device code's order and checks, over random and adversarial rows (lower halves
forced to the worst case of the truncation, zero / subnormal elements, norms from 1e-20 to 1e15), that the screen's lower bound never
exceeds the canonical distance; that the two 16-bit planes give every f32 back bit for bit; that the plane layout is a permutation.
The oracle's own statement of the bound (oracle/oracle.c: orc_screen_lb), which the GPU tests count with, is held to the selftest's bit
for bit.  No GPU."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "leann-rs_amd", "host")


def test_lower_bound_never_exceeds_canonical_distance():
    exe = os.path.join(HOST, "row_screen_selftest")
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/row_screen_selftest"])  # a no-op when up to date; never a stale binary
    p = subprocess.run([exe], stdout=subprocess.PIPE, check=False)
    r = json.loads(p.stdout)
    assert r["cases"] >= 5000
    assert r["violations"] == 0 and r["roundtrip_bad"] == 0 and r["layout_bad"] == 0, r
    assert r["min_gap"] >= 0
    assert p.returncode == 0


def _cases():
    """(q, x) pairs in the selftest's families — 0 a random row, 1 a near-duplicate of the query, 2 near the query with the lower halves
    forced to the worst case of the truncation (0xFFFF where the element has the query's sign, 0 elsewhere), 3 the opposite forcing,
    4 as 2 with zero / subnormal / smallest-normal elements sprinkled in, 5 anti-correlated with forcing — at norms 1e-20 .. 1e15 on
    both sides, and at widths of 1 .. 6 chunks with a partial last chunk (516 and 1028: four elements in it)"""
    rng = np.random.default_rng(0x5EED0001)
    scales = (1.0, 1e-3, 37.5, 1e-20, 1e15)
    tiny = np.array([0x00000000, 0x0000FFFF, 0x007FFFFF, 0x0080FFFF], np.uint32)  # zero, subnormals, the smallest normal's neighbour
    out = []
    for d in (1, 37, 516, 768, 1028, 1536):
        for rep in range(60):
            sq, sx = scales[rng.integers(5)], scales[rng.integers(5)]
            q = rng.standard_normal(d)
            q = (q * (sq / np.linalg.norm(q))).astype(np.float32)
            c = rng.standard_normal(d)
            for mode in range(6):
                x = c if mode == 0 else (-1.0 if mode == 5 else 1.0) * q.astype(np.float64) / sq + 1e-3 * c
                x = (x * (sx / np.linalg.norm(x))).astype(np.float32)
                b = x.view(np.uint32)
                if mode >= 2:
                    same = ((b >> 31) != 0) == (q < 0)
                    b[:] = (b & np.uint32(0xFFFF0000)) | np.where(same != (mode == 3), np.uint32(0xFFFF), np.uint32(0))
                if mode == 4:
                    m = len(b[::7])
                    b[::7] = (rng.integers(2, size=m).astype(np.uint32) << 31) | tiny[rng.integers(4, size=m)]
                out.append((q, x.copy()))
    return out


def test_oracle_bound_is_the_bound_the_device_compiles(po, tmp_path):
    """oracle.c restates the screen's lower bound from the definition, with its own constants and without row_screen.h, so that the GPU
    tests can hold the device's ruled-out count to it.  Here that restatement is tied to row_screen.h itself: over the selftest's
    families, po.screen_lb and po.dist_canon equal, bit for bit, what host/row_screen_selftest prints from rs_lane_bound /
    rs_abs_term / rs_lower_bound / rs_hi16 — the functions the device compiles — and lb <= dist in every case."""
    exe = os.path.join(HOST, "row_screen_selftest")
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/row_screen_selftest"])
    cases = _cases()
    assert len(cases) >= 2000
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        for q, x in cases:
            f.write(np.uint32(len(q)).tobytes() + q.tobytes() + x.tobytes())
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, check=True, text=True)
    theirs = np.array([[int(w, 16) for w in line.split()] for line in p.stdout.splitlines()], np.uint32)
    assert theirs.shape == (len(cases), 2)
    lb = np.array([po.screen_lb(q, x) for q, x in cases], np.float32)
    dist = np.array([po.dist_canon(q, x) for q, x in cases], np.float32)
    bad = np.flatnonzero(lb.view(np.uint32) != theirs[:, 0])
    assert bad.size == 0, f"lower bound differs in {bad.size} cases, first: case {bad[0]}, d = {len(cases[bad[0]][0])}"
    assert (dist.view(np.uint32) == theirs[:, 1]).all()
    assert np.isfinite(lb).all() and np.isfinite(dist).all()
    assert (lb <= dist).all()
