"""CPU suite: the owning device-buffer type and the scratch-pool lease of the host side (leann-rs_amd/csrc/device_mem.h).
host/device_mem_selftest.cpp is built with the host compiler under AddressSanitizer + UBSan and defines the header's four functions
(allocation, scratch pool) itself, over malloc / free with counters and a "fail the next N allocations" switch.  It checks: destruction frees exactly once; a move leaves the source empty
and the moved-to buffer frees; grow at or below the capacity asks for nothing and keeps the pointer; grow above it frees the old
block BEFORE it asks for the new one; a failed alloc / grow leaves {nullptr, 0} and LEANN_ERR_DEVICE, and a later grow succeeds;
release() empties the buffer and leaves the block to the caller; a std::map entry made by operator[] and grown twice holds one block
and none after clear(); a converting move hands the same block on under another element type with the capacity rescaled, and it
is freed once; a lease asks the pool for count * sizeof(T) bytes and gives the block back exactly once, a moved-from lease is empty,
an assigned-to lease returns its own block first, reset() twice returns once, a failed acquire leaves the lease empty; nothing is
alive or leased at exit.  A double free, a leak or an overrun is the sanitizer's to report.  No GPU, no
library."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "leann-rs_amd", "host", "device_mem_selftest")


def test_device_buf_selftest_under_sanitizers():
    subprocess.check_call(["make", "-s", "-C", ROOT, "leann-rs_amd/host/device_mem_selftest"])  # a no-op when up to date
    p = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=False)
    out, err = p.stdout.decode(), p.stderr.decode()
    assert p.returncode == 0, out + err
    assert "device_mem_selftest ok" in out
    m = re.search(r"(\d+) blocks allocated and freed, (\d+) leases taken and given back", out)
    assert m and int(m.group(1)) > 0 and int(m.group(2)) > 0, out
    assert "FAIL" not in err and "ERROR: " not in err and "runtime error" not in err and "LeakSanitizer" not in err, err
