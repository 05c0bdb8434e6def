#!/usr/bin/env python3
"""Diff the gfx950 kernels of two sets of host objects (no GPU): which kernels each set holds, and per kernel whether the instruction
stream and the kernel descriptor values are the same.  For showing that a source move changed no device code.

    python3 tools/diff_object_kernels.py --a OLD.o [OLD2.o ...] --b NEW1.o [NEW2.o ...] [--match REGEX] > table.md

Instructions are compared without addresses and encodings; branch targets as offsets from the kernel's start; the pc-relative literal
that follows an s_getpc_b64 (the address of a global, which depends on where the linker put it) is blanked.  Exit status 1 on any difference."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def llvm_bin():
    roots = [os.environ["ROCM_PATH"]] if os.environ.get("ROCM_PATH") else []
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    for r in roots:
        if os.path.isdir(os.path.join(r, "llvm", "bin")):
            return os.path.join(r, "llvm", "bin")
    sys.exit("no ROCm llvm/bin found ($ROCM_PATH or next to hipcc)")


def code_object(obj, tmp, llvm):
    base = os.path.join(tmp, f"{abs(hash(obj))}_{os.path.basename(obj)}")
    fb, co = base + ".fatbin", base + ".co"
    run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout
    run(os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", obj, base + ".host.o")
    run(os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={fb}", f"--targets={TARGET}", f"--output={co}")
    return co


def kernels_of(obj, tmp, llvm):
    """{kernel symbol: (normalised instructions, {descriptor field: value})} of one host object"""
    co = code_object(obj, tmp, llvm)
    run = lambda *a: subprocess.run(a, check=True, capture_output=True, text=True).stdout
    meta, name = {}, None
    for line in run(os.path.join(llvm, "llvm-readelf"), "--notes", co).splitlines():
        m = re.match(r"\s*-?\s*(\.\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == ".agpr_count":            # first per-kernel field (keys are sorted): a new kernel record starts
            name = {}
        if name is not None and m.group(1) in META:
            name[m.group(1)] = int(m.group(2))
        if name is not None and m.group(1) == ".name":
            meta[m.group(2).strip("'\"")] = name
        if m.group(1) == ".wavefront_size":        # last per-kernel field
            name = None
    out, cur, after_getpc = {}, None, 0
    for line in run(os.path.join(llvm, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co).splitlines():
        m = re.match(r"^\S*\s*<(\S+)>:$", line)
        if m:
            cur = m.group(1) if m.group(1) in meta else None
            if cur:
                out[cur] = []
            continue
        ins = line.split("//")[0].split(";")[0].strip()
        if not cur or not ins or ins == "...":     # ("...": objdump's mark for zero padding behind the last kernel of a section)
            continue
        ins = re.sub(r"\b\d+ <[^>+]+(\+0x[0-9a-f]+)?>", lambda t: "@" + (t.group(1) or "+0x0"), ins)      # branch target -> offset in kernel
        if ins.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc and re.match(r"s_addc?_u32 .*, (0x[0-9a-f]+|\d+)$", ins):
            ins = re.sub(r", (0x[0-9a-f]+|\d+)$", ", <pcrel>", ins)
            after_getpc -= 1
        out[cur].append(ins)
    return {k: (out.get(k, []), meta[k]) for k in meta}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True, help="objects of the first set")
    ap.add_argument("--b", nargs="+", required=True, help="objects of the second set")
    ap.add_argument("--match", default="", help="only kernels whose symbol matches this regex")
    args = ap.parse_args()
    llvm = llvm_bin()
    sets = []
    with tempfile.TemporaryDirectory() as tmp:
        for objs in (args.a, args.b):
            ks = {}
            for o in objs:
                for k, v in kernels_of(o, tmp, llvm).items():
                    if re.search(args.match, k):
                        assert k not in ks, f"{k} in two objects of one set"
                        ks[k] = (*v, os.path.basename(o))
            sets.append(ks)
    a, b = sets
    bad = 0
    print("| kernel | object (a -> b) | instructions | VGPR | AGPR | SGPR | LDS B | scratch B | identical |")
    print("|---|---|---|---|---|---|---|---|---|")
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"| `{k}` | {'only in ' + ('a' if k in a else 'b')} | | | | | | | **no** |")
            bad += 1
            continue
        (ia, ma, oa), (ib, mb, ob) = a[k], b[k]
        same = ia == ib and ma == mb
        bad += not same
        cols = " | ".join(str(ma.get(f)) if ma.get(f) == mb.get(f) else f"{ma.get(f)} -> {mb.get(f)}" for f in META)
        n = str(len(ia)) if len(ia) == len(ib) else f"{len(ia)} -> {len(ib)}"
        print(f"| `{k}` | {oa} -> {ob} | {n} | {cols} | {'yes' if same else '**no**'} |")
        if ia != ib:
            first = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            print(f"first difference of {k} at instruction {first}: {ia[first:first + 1]} vs {ib[first:first + 1]}", file=sys.stderr)
    print(f"\n{len(set(a) | set(b))} kernels, {bad} different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
