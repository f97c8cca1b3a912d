#!/usr/bin/env python3
"""Compares the device code of two source trees kernel by kernel, whatever file a kernel lives in.

    scripts/compare_device_code.py OLD/lidarslam_amd/csrc NEW/lidarslam_amd/csrc [--jobs N] [--table]

Every *.hip of both directories is compiled to gfx950 assembly (device side only, with the HIPFLAGS of that
directory's Makefile).  For each kernel the script takes the code object metadata (VGPRs, AGPRs, SGPRs, LDS bytes,
scratch bytes, spills) and the instruction stream with comments and section directives dropped and the function number
taken out of the local labels and the kernel's own symbol.  It reports kernels that exist on one side only, kernels whose resources differ and kernels whose
instruction stream differs, and exits 1 when there is any of these.  A kernel that exists on one side only is paired
with the one of the other side that has the same demangled signature once the namespace qualifiers are taken out (a
kernel that left an anonymous namespace for a header), and compared like any other.  --table prints the per-kernel
resources of NEW as a Markdown table.  Meant for refactors that move kernels between files: the expected result is no
difference.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def hipflags(csrc):
    for line in open(os.path.join(csrc, "Makefile")):
        if line.startswith("HIPFLAGS"):
            return line.split("=", 1)[1].replace("$(ARCH)", "gfx950").split()
    raise SystemExit(f"{csrc}/Makefile has no HIPFLAGS")


def assemble(job):
    csrc, src, out = job
    cmd = [HIPCC, *hipflags(csrc), "-Wno-unused-command-line-argument", "-Wno-pass-failed", "--cuda-device-only", "-S", src, "-o", out]
    subprocess.check_call(cmd, cwd=csrc)
    return out


def kernels_of(asm_path):
    """{kernel symbol: (resources, instruction stream)} of one assembly file."""
    text = open(asm_path).read()
    meta = {}
    for block in text.split("  - .agpr_count:")[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        meta[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1)) for f in FIELDS)
    out = {}
    for name, res in meta.items():
        body = text.split("\n%s:" % name, 1)[1].split("\n.Lfunc_end", 1)[0]
        lines = []
        for line in body.split("\n")[1:]:
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";", 1)[0]).replace(name, "<self>").strip()
            if line and line != ".text" and not line.startswith(".section"):  # (which section the code lands in is linkage, not code)
                lines.append(line)
        out[name] = (res, lines)
    return out


def demangle(names):
    """{symbol: (name for the report, signature without namespace qualifiers)}"""
    try:
        res = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: (re.sub(r"\(anonymous namespace\)::|\(.*", "", d), re.sub(r"(\(anonymous namespace\)|\w+)::", "", d)) for n, d in zip(names, res)}
    except (OSError, subprocess.CalledProcessError):
        return {n: (n, n) for n in names}


def pair_renamed(old, new, where, plain):
    """Kernels of one side only whose unqualified signature names exactly one kernel of each side: NEW's takes OLD's symbol."""
    alone = {side: {} for side in ("old", "new")}
    for side, mine, other in (("old", old, new), ("new", new, old)):
        for name in set(mine) - set(other):
            alone[side].setdefault(plain[name], []).append(name)
    paired = 0
    for sig, names in alone["old"].items():
        if len(names) == 1 and len(alone["new"].get(sig, ())) == 1:
            was = alone["new"][sig][0]
            new[names[0]] = new.pop(was)
            where["new"][names[0]] = where["new"].pop(was)
            paired += 1
    return paired


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--table", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        jobs = []
        for side, csrc in (("old", os.path.abspath(args.old)), ("new", os.path.abspath(args.new))):
            os.mkdir(os.path.join(tmp, side))
            for src in sorted(glob.glob(os.path.join(csrc, "*.hip"))):
                jobs.append((csrc, src, os.path.join(tmp, side, os.path.basename(src)[:-4] + ".s")))
        with concurrent.futures.ThreadPoolExecutor(args.jobs) as pool:
            list(pool.map(assemble, jobs))
        sides = {"old": {}, "new": {}}
        where = {"old": {}, "new": {}}
        for csrc, src, out in jobs:
            side = os.path.basename(os.path.dirname(out))
            for name, k in kernels_of(out).items():
                if name in sides[side]:
                    raise SystemExit(f"{name} is defined twice on the {side} side")
                sides[side][name] = k
                where[side][name] = os.path.basename(src)
    old, new = sides["old"], sides["new"]
    names = demangle(sorted(set(old) | set(new)))
    pretty = {n: v[0] for n, v in names.items()}
    paired = pair_renamed(old, new, where, {n: v[1] for n, v in names.items()})
    bad = 0
    for name in sorted(set(old) ^ set(new)):
        print(f"ONLY {'old' if name in old else 'new'}: {pretty[name]}")
        bad += 1
    moved = 0
    for name in sorted(set(old) & set(new)):
        moved += where["old"][name] != where["new"][name]
        if old[name][0] != new[name][0]:
            print(f"RESOURCES differ: {pretty[name]}: {dict(zip(FIELDS, old[name][0]))} -> {dict(zip(FIELDS, new[name][0]))}")
            bad += 1
        if old[name][1] != new[name][1]:
            first = next((i for i, (a, b) in enumerate(zip(old[name][1], new[name][1])) if a != b), min(len(old[name][1]), len(new[name][1])))
            print(f"INSTRUCTIONS differ: {pretty[name]}: {len(old[name][1])} -> {len(new[name][1])} lines, first at line {first}")
            bad += 1
    if args.table:
        print("| kernel | file | VGPR | AGPR | SGPR | LDS B | scratch B | spills |")
        print("|---|---|---|---|---|---|---|---|")
        for name in sorted(new, key=lambda n: (where["new"][n], pretty[n])):
            r = new[name][0]
            print(f"| `{pretty[name]}` | {where['new'][name]} | {r[0]} | {r[1]} | {r[2]} | {r[3]} | {r[4]} | {r[5] + r[6]} |")
    print(f"{len(old)} kernels old, {len(new)} kernels new, {moved} in another file, {paired} paired across namespaces, {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
