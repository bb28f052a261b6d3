#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?

    scripts/device_code_diff.py <tree_a> <tree_b> [-D...] [--only a.hip,b.hip] [--jobs N] [--keep DIR]

For every leann-rs_amd/csrc/*.hip of both trees: compile with the Makefile's HIPFLAGS plus `--cuda-device-only
-Rpass-analysis=kernel-resource-usage`, take the gfx950 code object out of the bundle, and compare
  * per FUNC symbol the SHA-256 of its st_size bytes (per symbol, so a changed emission order is no difference), and
  * per kernel the lines of its resource-usage block with the source position stripped.
Prints one line per translation unit, then the differing functions by name with the differing report lines; exit status 0
only when nothing differs.  Extra -D flags go to both sides.  Needs the ROCm toolchain and no GPU; reads nothing but the two
trees; hashes bytes and diffs report text, nothing else.  The method is the one of profiles/search_plan.md §1.
"""
import argparse
import hashlib
import os
import re
import shlex
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("leann-rs_amd", "csrc")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def tool(name, *dirs):
    root = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in dirs:
        p = os.path.join(root, d, name)
        if os.path.exists(p):
            return p
    return name


HIPCC = os.environ.get("HIPCC") or tool("hipcc", "bin")
BUNDLER = tool("clang-offload-bundler", "llvm/bin", "lib/llvm/bin")
READELF = tool("llvm-readelf", "llvm/bin", "lib/llvm/bin")


def hipflags(tree):
    """HIPFLAGS of the tree's Makefile (continuation lines joined, $(ARCH) expanded)."""
    text = open(os.path.join(tree, "Makefile")).read().replace("\\\n", " ")
    arch = re.search(r"^ARCH\s*\?=\s*(\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS\s*:=\s*(.*)$", text, re.M).group(1)
    return shlex.split(flags.replace("$(ARCH)", arch))


def run(cmd, **kw):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, **kw)


def compile_unit(tree, unit, defines, out):
    """-> (elf path, resource-report text) of one translation unit's gfx950 code object."""
    co, elf = os.path.join(out, unit + ".co"), os.path.join(out, unit + ".elf")
    cmd = [HIPCC, *hipflags(tree), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", *defines,
           "-c", os.path.join(CSRC, unit + ".hip"), "-o", co]
    try:
        rpass = run(cmd, cwd=tree).stderr
    except subprocess.CalledProcessError as e:
        sys.exit("%s: %s failed:\n%s" % (tree, " ".join(cmd), e.stderr[-4000:]))
    run([BUNDLER, "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + co, "--output=" + elf])
    return elf, rpass


def function_hashes(elf):
    """{FUNC symbol: SHA-256 of its st_size bytes at st_value in its section}"""
    sections = {}  # index -> (address, file offset)
    for line in run([READELF, "-SW", elf]).stdout.splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S*)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            sections[int(m.group(1))] = (int(m.group(4), 16), int(m.group(5), 16))
    data = open(elf, "rb").read()
    out = {}
    for line in run([READELF, "-sW", elf]).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6].isdigit():
            addr, off = sections[int(f[6])]
            start = int(f[1], 16) - addr + off
            size = int(f[2], 0)
            out[f[7]] = hashlib.sha256(data[start:start + size]).hexdigest()
    return out


def resource_reports(rpass):
    """{kernel: [report lines, source position stripped]}: `Function Name:` and what follows it up to the next block"""
    out, cur = {}, None
    for line in rpass.splitlines():
        m = re.match(r".*?: remark: (?:.*?:\d+:\d+: )?(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            cur = out.setdefault(text.split(":", 1)[1].strip(), [])
        elif cur is not None:
            cur.append(text)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME[=VALUE]")
    ap.add_argument("--only", default="", help="comma-separated translation units (api.hip,search_bf16.hip); default: all")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--keep", default=None, help="keep the code objects and reports in this directory")
    args = ap.parse_args()
    defines = ["-D" + d for d in args.defines]
    trees = [os.path.abspath(args.tree_a), os.path.abspath(args.tree_b)]
    units = [sorted(f[:-4] for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")) for t in trees]
    if args.only:
        only = {u[:-4] if u.endswith(".hip") else u for u in args.only.split(",")}
        units = [[u for u in us if u in only] for us in units]
    tmp = args.keep or tempfile.mkdtemp(prefix="device_code_diff_")
    jobs = []
    with ThreadPoolExecutor(max_workers=max(1, min(16, args.jobs))) as pool:
        for side, (tree, us) in enumerate(zip(trees, units)):
            out = os.path.join(tmp, "ab"[side])
            os.makedirs(out, exist_ok=True)
            for u in us:
                jobs.append((side, u, pool.submit(compile_unit, tree, u, defines, out)))
        built = {(side, u): fut.result() for side, u, fut in jobs}

    print("# a = %s\n# b = %s\n# flags: Makefile HIPFLAGS %s" % (trees[0], trees[1], " ".join(defines) or "(plain)"))
    print("%-16s %11s %17s %13s %12s %18s %14s" % ("unit", "functions", "beam_search a / b", "one tree only", "bytes differ", "reports a / b", "reports differ"))
    row = "%-16s %5d /%4d %8d /%4d %13d %12d %10d /%4d %14d"
    total = [0] * 9  # the row's columns, summed
    missing, details = 0, []
    for u in sorted(set(units[0]) | set(units[1])):
        if (0, u) not in built or (1, u) not in built:
            print("%-16s only in tree %s" % (u + ".hip", "a" if (0, u) in built else "b"))
            missing += 1
            continue
        ha, hb = function_hashes(built[0, u][0]), function_hashes(built[1, u][0])
        ra, rb = resource_reports(built[0, u][1]), resource_reports(built[1, u][1])
        lone = sorted(set(ha) ^ set(hb))
        bytes_differ = sorted(f for f in set(ha) & set(hb) if ha[f] != hb[f])
        rep_differ = sorted(f for f in set(ra) | set(rb) if ra.get(f) != rb.get(f))
        cols = (len(ha), len(hb), sum("beam_search" in f for f in ha), sum("beam_search" in f for f in hb), len(lone), len(bytes_differ),
                len(ra), len(rb), len(rep_differ))
        print(row % ((u + ".hip",) + cols))
        total = [t + c for t, c in zip(total, cols)]
        for f in lone:
            details.append("%s.hip: %s: in tree %s only" % (u, f, "a" if f in ha else "b"))
        for f in bytes_differ:
            details.append("%s.hip: %s: bytes differ" % (u, f))
        for f in rep_differ:
            la, lb = ra.get(f, []), rb.get(f, [])
            details.append("%s.hip: %s: report differs" % (u, f))
            details += ["    a: " + x for x in la if x not in lb] + ["    b: " + x for x in lb if x not in la]
    print(row % (("total",) + tuple(total)))
    for d in details:
        print(d)
    different = missing or total[4] or total[5] or total[8]
    if not args.keep:
        shutil.rmtree(tmp, ignore_errors=True)
    print("DIFFERENT" if different else "IDENTICAL")
    return 1 if different else 0


if __name__ == "__main__":
    sys.exit(main())
