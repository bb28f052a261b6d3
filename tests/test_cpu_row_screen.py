"""CPU suite: the bound of the split-plane row screen (leann-rs_amd/csrc/row_screen.h).  host/row_screen_selftest.cpp restates the
canonical distance chain and the screen's chain in the device code's order and checks, over random and adversarial rows (lower halves
forced to the worst case of the truncation, zero / subnormal elements, norms from 1e-20 to 1e15), that the screen's lower bound never
exceeds the canonical distance; that the two 16-bit planes give every f32 back bit for bit; that the plane layout is a permutation.
No GPU."""
import json
import os
import subprocess

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
