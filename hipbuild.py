#!/usr/bin/env python3
"""The one recipe for libdawn_hip.so and its instrumented variants (standard library only: build_lib.sh runs it without torch).

The source set is every dawn-pytorch_amd/csrc/*.hip, found by glob; a new kernel file needs no list edit.

    python3 hipbuild.py [--force]              the shipped dawn-pytorch_amd/libdawn_hip.so (incremental unless --force)
    python3 hipbuild.py PRESET [-DFLAG ...]    an instrumented library (see PRESETS; tl16debug takes its -D flags here)
    python3 hipbuild.py --source STEM -o OUT -DFLAG [...]
                                               one-off A/B: csrc/STEM.hip recompiled with the flags, the rest shipped objects

A variant is the full source set with extra -D flags on some sources, plus optional extra sources.  Its recompiled objects
live in build/variant-<name>/ and are rebuilt on every call (so the flags in use are always the ones asked for); the other
sources reuse the shipped objects in build/, brought up to date first.  A variant never writes the shipped library."""
import argparse
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent
CSRC = ROOT / "dawn-pytorch_amd" / "csrc"
BUILD = ROOT / "build"
SHIPPED_LIB = ROOT / "dawn-pytorch_amd" / "libdawn_hip.so"
COMPILE = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c"]
LINK = ["--offload-arch=gfx950", "-shared", "-fPIC"]
CLI_FLAGS = None   # marks the source of a preset that takes its -D flags from the command line

# name -> flags: {csrc stem: [-D flags]}, extra: {path relative to the root: [-D flags]}, out: path relative to the root
PRESETS = {
    # s_memtime stamps per wave and phase of temporal_layer_c64_kernel (tools/temporal_phase_timing.py)
    "tltiming": dict(flags={"temporal_layer": ["-DDAWN_TL_TIMING"]}, out="tools/ubench/libdawn_hip_tltiming.bin"),
    # F(2x2,3x3) Winograd stamps / ablations selected by DAWN_WINO_ABL (tools/bench_wino.py --stamps)
    "winotiming": dict(flags={"conv3x3_wino": ["-DDAWN_ABLATION"]}, out="tools/ubench/libdawn_hip_winotiming.bin"),
    # F(4x4,3x3) Winograd stamps / ablations selected by DAWN_WINO4_ABL (tools/bench_wino.py --stamps4)
    "wino4timing": dict(flags={"conv3x3_wino4": ["-DDAWN_ABLATION"]}, out="tools/ubench/libdawn_hip_wino4timing.bin"),
    # round 3's persistent stream-K 3x3 conv, reached through policy bit 0x400 + dawn_conv_desc.sk_ws (tools/conv_sk_phase_timing.py)
    "sktiming": dict(flags={"conv_gemm": ["-DDAWN_WITH_STREAMK"]}, extra={"tools/ubench/conv3x3_sk.hip": ["-DDAWN_ABLATION"]},
                     out="tools/ubench/libdawn_hip_sktiming.bin"),
    # window-tiled temporal layer with -DDAWN_TL16_DUMP (tools/debug_tl16_dump.py) or -DDAWN_TL_TIMING (tools/tl16_phase_timing.py)
    "tl16debug": dict(flags={"temporal_layer16": CLI_FLAGS}, out="tools/ubench/libdawn_hip_tl16debug.bin"),
    # temporal layer stamps + conv ablations / dawn_conv_set_debug / policy 0x40000000 (tools/bench_resample.py).  Every unit of the
    # conv / GEMM family takes the flag: conv_split.h, which all four include, derives the policy mask from it
    "ablation": dict(flags={"temporal_layer": ["-DDAWN_TL_TIMING"],
                            **{u: ["-DDAWN_ABLATION"] for u in ("conv_gemm", "conv3x3_split", "gemm1x1_tiled", "gemm1x1_rows")}},
                     out="tools/ubench/libdawn_hip_ablation.bin"),
}


def sources():
    """The shipped source set: every csrc/*.hip, sorted."""
    return sorted(CSRC.glob("*.hip"))


def headers(root=ROOT):
    """Every header an object may depend on: any *.h under csrc/ or include/."""
    return sorted([*root.joinpath("dawn-pytorch_amd", "csrc").rglob("*.h"), *root.joinpath("include").rglob("*.h")])


def shipped_object(src):
    return BUILD / (src.stem + ".o")


def shipped_units():
    """(source, object, None) of the shipped library: no extra flags."""
    return [(s, shipped_object(s), None) for s in sources()]


def stale(obj, src, hdrs):
    """True when obj is missing or older than its source or any header."""
    if not obj.exists():
        return True
    t = obj.stat().st_mtime
    return any(p.stat().st_mtime > t for p in (src, *hdrs))


def variant_units(name, flags, extra=None):
    """(source, object, -D flags) of every object a variant links: each csrc source once, as its variant object when it has
    flags (in build/variant-<name>/) and as the shipped object (flags None) otherwise; then the extra sources."""
    vdir = BUILD / f"variant-{name}"
    unknown = set(flags) - {s.stem for s in sources()}
    if unknown:
        raise RuntimeError(f"no csrc source for {sorted(unknown)}")
    units = [(s, vdir / (s.stem + ".o"), flags[s.stem]) if s.stem in flags else (s, shipped_object(s), None) for s in sources()]
    return units + [(ROOT / p, vdir / (Path(p).stem + ".o"), f) for p, f in (extra or {}).items()]


def preset_units(name, cli_flags=()):
    p = PRESETS[name]
    flags = {k: list(cli_flags) if v is CLI_FLAGS else v for k, v in p["flags"].items()}
    return variant_units(name, flags, p.get("extra"))


def _hipcc():
    return os.environ.get("HIPCC", "hipcc")


def _compile(job):
    src, obj, flags = job
    obj.parent.mkdir(parents=True, exist_ok=True)
    # root-relative source path: __FILE__ in error messages does not depend on where the tree lives
    r = subprocess.run([_hipcc(), *COMPILE, *flags, str(src.relative_to(ROOT)), "-o", str(obj)], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.stdout:
        print(r.stdout, end="", file=sys.stderr)
    return src, r.returncode


def _build(units, out, force=False):
    hdrs = headers()
    jobs = [(s, o, f or []) for s, o, f in units if f is not None or force or stale(o, s, hdrs)]
    with ThreadPoolExecutor() as ex:
        failed = [str(s.relative_to(ROOT)) for s, rc in ex.map(_compile, jobs) if rc != 0]
    if failed:
        raise RuntimeError(f"hipcc failed on {', '.join(failed)}")
    out.parent.mkdir(parents=True, exist_ok=True)
    subprocess.run([_hipcc(), *LINK, *(str(o) for _, o, _ in units), "-o", str(out)], check=True)
    return out


def build(force=False):
    """The shipped library; returns its path."""
    return _build(shipped_units(), SHIPPED_LIB, force)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("preset", nargs="?", choices=sorted(PRESETS), help="instrumented library to build (default: the shipped one)")
    ap.add_argument("--source", metavar="STEM", help="one-off variant: recompile csrc/STEM.hip with the -D flags given")
    ap.add_argument("-o", dest="out", help="output path of a variant (default: the preset's)")
    ap.add_argument("--force", action="store_true", help="recompile every object")
    args, dflags = ap.parse_known_args(argv)
    bad = [a for a in dflags if not a.startswith("-D")]
    if bad:
        ap.error(f"unrecognised arguments: {' '.join(bad)} (only -D flags pass through to hipcc)")
    takes_flags = args.source or (args.preset and CLI_FLAGS in PRESETS[args.preset]["flags"].values())
    if dflags and not takes_flags:
        ap.error("-D flags apply only to --source or a preset that takes them (tl16debug)")
    if args.preset and args.source:
        ap.error("give a preset or --source, not both")
    if args.source:
        if not args.out:
            ap.error("--source needs -o OUT")
        if args.source not in {s.stem for s in sources()}:
            ap.error(f"no csrc/{args.source}.hip")
        units, out = variant_units(args.source, {args.source: dflags}), Path(args.out)
    elif args.preset:
        units, out = preset_units(args.preset, dflags), Path(args.out or ROOT / PRESETS[args.preset]["out"])
    else:
        if args.out:
            ap.error("-o applies only to a variant")
        units, out = shipped_units(), SHIPPED_LIB
    try:
        _build(units, out.resolve(), args.force)
    except (RuntimeError, subprocess.CalledProcessError) as e:
        sys.exit(f"hipbuild: {e}")
    print(f"built {os.path.relpath(out.resolve(), ROOT)}")


if __name__ == "__main__":
    main()
