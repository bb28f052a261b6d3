"""scripts/device_code_diff.py, without a GPU: a tree against itself is identical, an edited kernel is found by name."""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "scripts", "device_code_diff.py")
UNIT = "shard.hip"  # one small kernel: seconds to compile


def _run(a, b, *more):
    return subprocess.run([sys.executable, TOOL, a, b, "--only", UNIT, *more], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_same_tree_is_identical_and_an_edit_is_named(tmp_path):
    r = _run(ROOT, ROOT)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("IDENTICAL"), r.stdout
    line = next(x for x in r.stdout.splitlines() if x.startswith(UNIT)).split()
    assert int(line[1]) == int(line[3]) >= 1 and int(line[-1]) == 0, line  # the unit's kernels were seen, on both sides

    other = tmp_path / "tree"
    shutil.copytree(os.path.join(ROOT, "leann-rs_amd", "csrc"), other / "leann-rs_amd" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), other / "include")
    shutil.copy(os.path.join(ROOT, "Makefile"), other)
    src = other / "leann-rs_amd" / "csrc" / UNIT
    text = src.read_text()
    k = text.index("{", text.index("__global__"))  # first statement of the unit's first kernel: one more barrier
    src.write_text(text[: k + 1] + " __syncthreads(); " + text[k + 1:])
    r = _run(ROOT, str(other))
    assert r.returncode == 1 and r.stdout.rstrip().endswith("DIFFERENT"), r.stdout
    assert "bytes differ" in r.stdout
    r = _run(ROOT, str(other), "-DLEANN_STAMPS")  # extra -D flags reach both sides
    assert r.returncode == 1 and "-DLEANN_STAMPS" in r.stdout
