#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    scripts/compare_device_code.py PARENT_TREE THIS_TREE [--jobs N] [--keep DIR [--reuse-parent]] [--only kernels_pb ...]

The acceptance check of a refactor that must not move an instruction (docs/design/07_measurement.md): every .hip unit of
cuopt_amd/csrc is built alone, device side only, with the HIPFLAGS of that tree's Makefile, and the `llvm-objdump -d` listings
of the two builds are compared
  * per kernel symbol, with the addresses and the branch-target comments stripped (one kernel growing by an instruction shifts
    every address behind it: a plain diff of the listings then reports thousands of lines that say nothing), and
  * as whole listings, without the two header lines that name the file.
Prints one line per unit (kernels, instructions and listing lines on both sides, differing kernels, differing listing lines), one
line per kernel that differs or exists on one side only, and exits 1 when anything differs.  It compares; it does nothing else.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("cuopt_amd", "csrc")


def hipflags(tree):
    """HIPFLAGS of the tree's Makefile, the variables it names expanded from the Makefile's own values (ROOT: the tree)"""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    var["ROOT"] = tree
    flags = var["HIPFLAGS"]
    for _ in range(4):  # (HIPFLAGS names INC, INC names ROOT)
        flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), m.group(0)) if m.group(1) in ("ARCH", "INC", "ROOT") else m.group(0), flags)
    if "$(" in flags:
        sys.exit(f"{tree}: HIPFLAGS has a variable this script does not expand: {flags}")
    return flags.split()


def listing(tree, flags, unit, out_dir, hipcc, objdump):
    obj = os.path.join(out_dir, unit + ".dev.o")
    src = os.path.join(tree, CSRC, unit + ".hip")
    subprocess.run([hipcc, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", src, "-o", obj], check=True)
    return subprocess.run([objdump, "-d", "--demangle", obj], check=True, capture_output=True, text=True).stdout.splitlines()


SYMBOL = re.compile(r"^[0-9a-f]+ <(.*)>:$")
ADDRESS = re.compile(r"//\s*[0-9A-Fa-f]+:")   # "// 000000001900: BF85004C <k+0x134>" -> "// BF85004C"
TARGET = re.compile(r"\s*<[^<>]*(<[^<>]*>[^<>]*)*\+0x[0-9a-f]+>\s*$")


def kernels(lines):
    """symbol -> its instructions, without addresses and branch-target comments (the encodings stay)"""
    out, cur = {}, None
    for line in lines:
        m = SYMBOL.match(line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(ADDRESS.sub("//", TARGET.sub("", line)).strip())
    return out


def differing(a, b):
    return sum(1 for op in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes() if op[0] != "equal"
               for _ in range(max(op[2] - op[1], op[4] - op[3])))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent"), ap.add_argument("this")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--keep", help="directory that keeps the code objects and listings (default: a temporary one)")
    ap.add_argument("--reuse-parent", action="store_true", help="with --keep: take the parent's listings that are already there")
    ap.add_argument("--only", nargs="*", help="unit names without .hip (default: every unit of either tree)")
    args = ap.parse_args()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    hipcc = os.environ.get("HIPCC", os.path.join(rocm, "bin", "hipcc"))
    objdump = os.path.join(rocm, "llvm", "bin", "llvm-objdump")
    trees = [os.path.abspath(args.parent), os.path.abspath(args.this)]
    units = args.only or sorted({f[:-4] for t in trees for f in os.listdir(os.path.join(t, CSRC)) if f.endswith(".hip")})
    tmp = None if args.keep else tempfile.TemporaryDirectory()
    base = args.keep or tmp.name
    dirs = [os.path.join(base, side) for side in ("parent", "this")]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    flags = [hipflags(t) for t in trees]

    def build(job):
        side, unit = job
        if not os.path.exists(os.path.join(trees[side], CSRC, unit + ".hip")):
            return job, None
        kept = os.path.join(dirs[side], unit + ".s")
        if side == 0 and args.reuse_parent and os.path.exists(kept):
            return job, open(kept).read().splitlines()
        lines = listing(trees[side], flags[side], unit, dirs[side], hipcc, objdump)
        with open(kept, "w") as f:
            f.write("\n".join(lines) + "\n")
        return job, lines

    with ThreadPoolExecutor(args.jobs) as pool:
        listings = dict(pool.map(build, [(side, u) for u in units for side in (0, 1)]))

    bad = 0
    print(f"{'unit':30} {'kernels':>9} {'instructions':>17} {'listing lines':>17} {'differing kernels':>18} {'differing lines':>16}")
    detail = []
    for u in units:
        a, b = listings[(0, u)], listings[(1, u)]
        if a is None or b is None:
            print(f"{u:30} only in {'this' if a is None else 'parent'}")
            bad += 1
            continue
        ka, kb = kernels(a), kernels(b)
        diff_k = 0
        for name in list(ka) + [n for n in kb if n not in ka]:
            ia, ib = ka.get(name), kb.get(name)
            if ia == ib:
                continue
            diff_k += 1
            short = name.replace("(anonymous namespace)::", "").split("(")[0]
            detail.append(f"  {u}: {short}: {len(ia) if ia is not None else 'absent'} -> {len(ib) if ib is not None else 'absent'}"
                          f" instructions, {differing(ia or [], ib or [])} differ")
        whole = sum(x != y for x, y in zip(a[2:], b[2:])) + abs(len(a) - len(b))  # (by position: a count, not an alignment)
        bad += diff_k + (whole != 0)
        print(f"{u:30} {len(ka):4}/{len(kb):<4} {sum(map(len, ka.values())):8}/{sum(map(len, kb.values())):<8} "
              f"{len(a):8}/{len(b):<8} {diff_k:18} {whole:16}")
    print("\n".join(detail) if detail else "no kernel differs")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
