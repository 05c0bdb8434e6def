#!/usr/bin/env python3
"""GPU box: the PBnet pose / blink stage at the shipped widths (audio 1024, latent 256, d 64, 4 heads, ff 1024, 4 layers),
seeded random weights.

    python tools/bench_pbnet.py [--reps 20] [--warmup 3] [--stage-reps 5] [--lengths 200 1600] [--out profiles/pbnet_stage_bench.json]

Two A/Bs per clip length, each alternating its two sides in one process after a warm-up of both:

  attn   one attention of the decoder (4 heads of 32, 2 rotary pairs, q | k | v column slices of one tensor) for both windows (100, 200):
         dawn_attn_bias32 on the dense (heads, T, T) table against dawn_attn_win32 on the (heads, 2 win + 1) table; HIP events around each
         side, median and minimum over --reps; the two results are compared bit for bit.
  stage  pose_blink_stage (both decoders, UVG:252-302) through the Python orchestration and through dawn_pose_blink_stage (via_c=True);
         host wall clock around a call that ends with the rows in host memory.  The Python side's per-length tables are cached after
         its first call, so the timed calls do not rebuild them.

And, at the longest length, the peak device memory of one first call of each side on fresh generators (torch's allocator statistics, above
what was allocated before the call: weights excluded, the Python side's dense tables and the C side's workspace included).

Prints one JSON line and writes it to --out.  A report, not a gate; there is no CPU fallback (no GPU: an error)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS, HD = 4, 128


def decoder_state_dict(in_dim, audio_dim=1024, latent=256, d=64, ff=1024, layers=4, heads=HEADS, seed=0):
    """Random weights under the reference decoder's key names, at the widths UVG configures."""
    gn = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=gn) * sc                                # noqa: E731
    lin = lambda o, i: r(o, i, sc=1.2 / i ** 0.5)                                            # noqa: E731
    hd = heads * 32
    freqs = 1.0 / (10000 ** (torch.arange(0, heads, 2).float() / heads))
    sd = {"firstposeEmbedding.weight": lin(d, in_dim), "firstposeEmbedding.bias": r(d, sc=0.2),
          "audioEmbedding.weight": lin(latent, audio_dim), "audioEmbedding.bias": r(latent, sc=0.2),
          "ztimelinear.weight": lin(d, 2 * latent + d), "ztimelinear.bias": r(d, sc=0.2),
          "init_proj.weight": lin(d, d), "init_proj.bias": r(d, sc=0.5),
          "init_temporal_attn.fn.norm.gamma": (1 + r(1, 1, d, sc=0.2)),
          "init_temporal_attn.fn.fn.to_qkv.weight": lin(3 * hd, d), "init_temporal_attn.fn.fn.to_out.weight": lin(d, hd),
          "init_temporal_attn.fn.fn.rotary_emb.freqs": freqs,
          "time_rel_pos_bias_tgt.relative_attention_bias.weight": r(32, heads, sc=1.5),
          "time_rel_pos_bias_mem.relative_attention_bias.weight": r(32, heads, sc=1.5),
          "finallayer.weight": lin(in_dim, d), "finallayer.bias": r(in_dim, sc=0.2)}
    for i in range(layers):
        p = f"seqTransDecoder.decoder_layers.{i}."
        sd.update({p + "self_attn.to_qkv.weight": lin(3 * hd, d), p + "self_attn.to_out.weight": lin(d, hd),
                   p + "multihead_attn.to_q.weight": lin(hd, d), p + "multihead_attn.to_k.weight": lin(hd, d),
                   p + "multihead_attn.to_v.weight": lin(hd, d), p + "multihead_attn.to_out.weight": lin(d, hd),
                   p + "ffn.linear1.weight": lin(ff, d), p + "ffn.linear1.bias": r(ff, sc=0.2),
                   p + "ffn.linear2.weight": lin(d, ff), p + "ffn.linear2.bias": r(d, sc=0.2)})
        for n in (1, 2, 3):
            sd[p + f"layer_norm{n}.weight"] = 1 + r(d, sc=0.2)
            sd[p + f"layer_norm{n}.bias"] = r(d, sc=0.2)
    return sd


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


def attn_ab(ops, T, win, reps, warmup):
    g = torch.Generator().manual_seed(T + win)
    qkv = torch.randn(T, 3 * HD, generator=g).cuda()
    br = torch.randn(HEADS, 2 * win + 1, generator=g) * 1.5
    rel = torch.arange(T)[None, :] - torch.arange(T)[:, None]
    band = rel.abs() <= win
    dense = torch.full((HEADS, T, T), -1e8)
    dense[:, band] = br[:, (rel + win)[band]]
    dense, br = dense.cuda(), br.cuda()
    ang = torch.arange(T).float()[:, None] * (1.0 / 10000 ** (torch.arange(2).float() / 2))[None]
    rc, rs = ang.cos().contiguous().cuda(), ang.sin().contiguous().cuda()
    q, k, v = qkv[:, :HD], qkv[:, HD:2 * HD], qkv[:, 2 * HD:]
    old, new, r_old, r_new = ab(event_ms, lambda: ops.attn_bias32(q, k, v, HEADS, dense, rc, rs, 32 ** -0.5),
                                lambda: ops.attn_win32(q, k, v, HEADS, win, br, rc, rs, 32 ** -0.5), reps, warmup)
    return {"T": T, "win": win, "table_bytes_dense": dense.numel() * 4, "table_bytes_win": br.numel() * 4, "attn_bias32": old,
            "attn_win32": new, "speedup_median": round(old["median_ms"] / new["median_ms"], 2), "bit_equal": bool(torch.equal(r_old, r_new)),
            "max_abs_diff": float((r_old - r_new).abs().max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stage-reps", type=int, default=5)
    ap.add_argument("--lengths", type=int, nargs="+", default=[200, 1600])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pbnet_stage_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pbnet: needs a GPU (a timing taken anywhere else says nothing about it)")
    from dawn_pytorch_amd.ops import HipOps
    from dawn_pytorch_amd.pbnet import PoseBlinkGenerator, pose_blink_stage
    ops = HipOps()
    sdp, sdb = decoder_state_dict(6, seed=1), decoder_state_dict(2, seed=2)

    def gens():
        return (PoseBlinkGenerator(sdp, archiname="transformerreemb6", device="cuda", ops=ops),
                PoseBlinkGenerator(sdb, archiname="transformerreemb5", device="cuda", ops=ops))
    gp, gb = gens()
    init_pose, init_blink = torch.tensor([[3.0, -5.0, 1.0, 4.79e-04, 56.5, 64.9, 9.9]]), torch.tensor([[0.3, 0.28]])

    def stage_runner(T):
        g = torch.Generator().manual_seed(T)
        audio, zp, zb = torch.randn(T, 1024, generator=g), torch.randn(T, 1, 256, generator=g), torch.randn(T, 1, 256, generator=g)
        return lambda via_c, a, b: pose_blink_stage(a, b, audio, init_pose, init_blink, z_pose=zp, z_blink=zb, via_c=via_c)
    rec = {"device": torch.cuda.get_device_name(0), "attn": [], "stage": []}
    for T in args.lengths:
        for win in (100, 200):
            rec["attn"].append(attn_ab(ops, T, win, args.reps, args.warmup))
        run = stage_runner(T)
        py, c, o_py, o_c = ab(wall_ms, lambda: run(False, gp, gb), lambda: run(True, gp, gb), args.stage_reps, 2)
        rec["stage"].append({"T": T, "python": py, "via_c": c, "speedup_median": round(py["median_ms"] / c["median_ms"], 3),
                             "pose_max_abs_diff": float((o_py[0] - o_c[0]).abs().max()), "pose_max_abs": float(o_py[0].abs().max()),
                             "blink_max_abs_diff": float((o_py[1] - o_c[1]).abs().max()), "blink_max_abs": float(o_py[1].abs().max())})
    # peak device memory of a first call at the longest length, on generators that hold no per-length state yet
    T = max(args.lengths)
    peak = {"T": T}
    run = stage_runner(T)
    for side, via_c in (("python", False), ("via_c", True)):
        a, b = gens()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(via_c, a, b)
        torch.cuda.synchronize()
        peak[side + "_peak_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        del a, b
    peak["workspace_bytes_via_c"] = int(ops.L.dawn_pose_blink_workspace_bytes(gp.c_evaluator().h, gb.c_evaluator().h, T))
    rec["peak_memory"] = peak
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
