#!/usr/bin/env python3
"""GPU box: the HuBERT audio-feature stage at hubert-large widths, seeded random weights.

    python tools/bench_hubert.py [--layers 24] [--reps 20] [--warmup 3] [--stage-reps 5] [--out profiles/hubert.json]

Two A/Bs, each alternating its two sides in one process after a warm-up of both:

  pos    the positional block of one 20 s segment (T = 1000 rows, E = 1024, 16 groups, 128 taps) as HubertFeatures.encode runs it
         (zeroed padded copy + 16 dawn_conv_gemm launches + dawn_add_act) against the one dawn_hubert_pos_conv launch; HIP events
         around each side, median and minimum over --reps; the two results are compared (max |a - b|: the sum orders differ).
  stage  all of process_audio on 20 s of audio (320000 samples -> 500 rows of `cond`) through the Python orchestration and through
         dawn_hubert_features (via_c=True); host wall clock around a call that ends with the rows in host memory.

Prints one JSON line.  A report, not a gate; there is no CPU fallback (no GPU: an error)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONV_K, CONV_STRIDE = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)


def hubert_large_state_dict(layers=24, seed=0, E=1024, D=512, inter=4096, pos_k=128, groups=16):
    """Random weights under transformers.HubertModel's key names (hubert-large-ls960-ft's shapes)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def lin(p, co, ci):
        sd[p + ".weight"] = torch.randn(co, ci, generator=g) * ci ** -0.5
        sd[p + ".bias"] = torch.randn(co, generator=g) * 0.05

    def ln(p, c):
        sd[p + ".weight"] = 1 + 0.1 * torch.randn(c, generator=g)
        sd[p + ".bias"] = 0.1 * torch.randn(c, generator=g)

    for i, k in enumerate(CONV_K):
        ci = 1 if i == 0 else D
        p = f"feature_extractor.conv_layers.{i}."
        sd[p + "conv.weight"] = torch.randn(D, ci, k, generator=g) * (ci * k) ** -0.5
        sd[p + "conv.bias"] = torch.randn(D, generator=g) * 0.05
        ln(p + "layer_norm", D)
    ln("feature_projection.layer_norm", D)
    lin("feature_projection.projection", E, D)
    sd["encoder.pos_conv_embed.conv.weight"] = torch.randn(E, E // groups, pos_k, generator=g) * (E // groups * pos_k) ** -0.5
    sd["encoder.pos_conv_embed.conv.bias"] = torch.randn(E, generator=g) * 0.05
    for i in range(layers):
        p = f"encoder.layers.{i}."
        for n in "qkv":
            lin(p + f"attention.{n}_proj", E, E)
        lin(p + "attention.out_proj", E, E)
        ln(p + "layer_norm", E)
        lin(p + "feed_forward.intermediate_dense", inter, E)
        lin(p + "feed_forward.output_dense", E, inter)
        ln(p + "final_layer_norm", E)
    ln("encoder.layer_norm", E)
    return sd


def pos_block_launches(hf, hid):
    """The positional block as HubertFeatures.encode runs it: padded copy, one GEMM per group, hidden + gelu."""
    ops, T, E = hf.ops, hid.shape[0], hf.E
    pad, gw = hf.pos_k // 2, E // hf.pos_groups
    xp = torch.zeros(T + 2 * pad, E, device=hid.device)
    xp[pad:pad + T].copy_(hid)
    pos = torch.empty(T, E, device=hid.device)
    for g in range(hf.pos_groups):
        ops.conv_gemm(xp[:, g * gw:(g + 1) * gw], hf.pos_w[g], gw, F=1, Hi=1, Wi=T + 2 * pad, Ho=1, Wo=T, KH=1, KW=hf.pos_k, stride=1,
                      pad=0, bias=hf.pos_b[g * gw:(g + 1) * gw], out=pos[:, g * gw:(g + 1) * gw])
    return ops.add_act(hid, pos, 2)


def pos_block_kernel(hf, hid):
    return hf.ops.hubert_pos_conv(hid, hf.pos_w_all, hf.pos_b, hf.pos_groups, hf.pos_k)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def ab(timer, a, b, reps, warmup):
    for _ in range(warmup):
        ra, rb = a(), b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timer(a)[0])
        tb.append(timer(b)[0])
    stat = lambda t: {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4)}   # noqa: E731
    return stat(ta), stat(tb), ra, rb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000, help="T of the positional-block A/B")
    ap.add_argument("--seconds", type=float, default=20.0, help="audio length of the stage A/B")
    ap.add_argument("--out", help="also write the JSON record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_hubert: needs a GPU (a timing taken anywhere else says nothing about it)")
    from dawn_pytorch_amd.hubert import HubertFeatures
    hf = HubertFeatures(hubert_large_state_dict(args.layers), "cuda:0", num_heads=16, conv_stride=CONV_STRIDE, pos_groups=16)
    g = torch.Generator().manual_seed(1)
    hid = torch.randn(args.rows, hf.E, generator=g).cuda()
    old, new, r_old, r_new = ab(event_ms, lambda: pos_block_launches(hf, hid), lambda: pos_block_kernel(hf, hid), args.reps, args.warmup)
    flops = 2.0 * args.rows * hf.E * (hf.E // hf.pos_groups) * hf.pos_k
    rec = {"device": torch.cuda.get_device_name(0), "layers": args.layers,
           "pos": {"T": args.rows, "E": hf.E, "groups": hf.pos_groups, "k": hf.pos_k, "gflop": round(flops / 1e9, 2),
                   "launches16": old, "pos_conv": new, "speedup_median": round(old["median_ms"] / new["median_ms"], 2),
                   "pos_conv_tflops": round(flops / new["median_ms"] / 1e9, 2),
                   "max_abs_diff": float((r_old - r_new).abs().max()), "max_abs": float(r_old.abs().max())}}
    n = int(args.seconds * 16000)
    speech = (torch.randn(n, generator=g) * 0.1).numpy().astype(np.float64)
    py, c, o_py, o_c = ab(wall_ms, lambda: hf.process_audio(speech), lambda: hf.process_audio(speech, via_c=True), args.stage_reps, 2)
    rec["stage"] = {"samples": n, "rows_out": int(o_c.shape[0]), "python": py, "via_c": c,
                    "speedup_median": round(py["median_ms"] / c["median_ms"], 3),
                    "max_abs_diff": float(np.abs(o_py - o_c).max()), "max_abs": float(np.abs(o_py).max())}
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
