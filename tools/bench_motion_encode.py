#!/usr/bin/env python3
"""Times the LFG motion encode (dawn_pytorch_amd/motion_encoder.py) on the GPU: a 256 x 256 source and 200 driving frames through
`MotionEncoder.latent` on the shipped architecture (config/hdtf256.yaml: region predictor and background encoder block_expansion 32,
pixelwise predictor 64, max_features 1024, 5 blocks, 10 regions) with random weights -- the times do not depend on the values.

    python tools/bench_motion_encode.py [--res 256] [--frames 200] [--chunk 16] [--repeat 3] [--via-c] [--out profiles/motion_encode.json]

Prints one JSON line: frames/s of the whole call (device events around it, after a warm-up call), and per op the device time of one
call summed over its launches (a second, instrumented call: events around every op, so host gaps are not in it).  For the two
reduction kernels the achieved bytes/s is the bytes each must read (its input once) over its time, against the 8.0 TB/s HBM3E
specification of an MI355X; for the background encoder's first two convolutions the achieved FLOP/s is the algorithm's multiply-adds
(unpadded channels) x 2 over their time, against the 2.5 PFLOP/s dense bf16 specification (the split-operand kernel issues six bf16
products per fp32 product, so 1/6 of it is that kernel's ceiling).  A number that needs a GPU is not produced without one.
--via-c adds the same clip through the C-side stage (`latent(via_c=True)`: dawn_motion_encode_clip, the same launches from C), once from
the uint8 RGB frames and once from I420 frames (driving kind 2), and the yuv420p ingest alone (dawn_yuv420_to_frames on the whole clip:
1.5 bytes read and 3 written per pixel, against the same HBM specification)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC = 8.0e12
BF16_SPEC = 2.5e15


def random_state_dicts(seed=0, R=10, be_rp=32, be_pf=64, mf=1024, nb=5):
    """Random state_dicts with the shipped shapes and key names: (generator's pixelwise predictor, region_predictor, bg_predictor)."""
    g = torch.Generator().manual_seed(seed)

    def conv(sd, p, co, ci, k):
        sd[p + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (ci * k * k) ** -0.5
        sd[p + ".bias"] = torch.randn(co, generator=g) * 0.1

    def bn(sd, p, c):
        sd[p + ".weight"] = 1 + 0.2 * torch.randn(c, generator=g)
        sd[p + ".bias"] = 0.2 * torch.randn(c, generator=g)
        sd[p + ".running_mean"] = 0.2 * torch.randn(c, generator=g)
        sd[p + ".running_var"] = torch.rand(c, generator=g) + 0.5

    def encoder(sd, p, be, cin):
        for i in range(nb):
            ci, co = (cin if i == 0 else min(mf, be * 2 ** i)), min(mf, be * 2 ** (i + 1))
            conv(sd, f"{p}.down_blocks.{i}.conv", co, ci, 3); bn(sd, f"{p}.down_blocks.{i}.norm", co)

    def hourglass(sd, p, be, cin):
        encoder(sd, p + ".encoder", be, cin)
        for j, i in enumerate(reversed(range(nb))):
            ci, co = (1 if i == nb - 1 else 2) * min(mf, be * 2 ** (i + 1)), min(mf, be * 2 ** i)
            conv(sd, f"{p}.decoder.up_blocks.{j}.conv", co, ci, 3); bn(sd, f"{p}.decoder.up_blocks.{j}.norm", co)
        return be + cin

    aa = torch.zeros(3, 1, 13, 13)
    rp, bg, gen = {"down.weight": aa}, {}, {"pixelwise_flow_predictor.down.weight": aa}
    conv(rp, "regions", R, hourglass(rp, "predictor", be_rp, 3), 7)
    rp["regions.weight"] *= 0.3
    encoder(bg, "encoder", be_rp, 6)
    bg["fc.weight"] = torch.randn(6, min(mf, be_rp * 2 ** nb), generator=g) * 0.01
    bg["fc.bias"] = torch.tensor([1.0, 0, 0, 0, 1, 0])
    pf = "pixelwise_flow_predictor"
    of = hourglass(gen, pf + ".hourglass", be_pf, (R + 1) * 4)
    conv(gen, pf + ".mask", R + 1, of, 7)
    conv(gen, pf + ".occlusion", 1, of, 7)
    return gen, rp, bg


class TimedOps:
    """Wraps an op set: device events around every op call, summed per op name (conv_gemm keyed by its shape)."""

    def __init__(self, ops):
        self._ops, self.events = ops, []

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if not callable(fn) or name.startswith("_") or name == "empty":
            return fn

        def timed(*a, **kw):
            key = name
            if name == "conv_gemm":
                key = f"conv_gemm {kw.get('KH', 1)}x{kw.get('KW', 1)}{' up' if kw.get('mode') else ''} {kw['Hi']}x{kw['Wi']} {a[0].shape[1]}" \
                      f"{'+' + str(kw['in1'].shape[1]) if kw.get('in1') is not None else ''}->{a[2]}"
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            self.events.append((key, e0, e1))
            return r
        return timed


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--via-c", action="store_true", help="also time the C-side stage and the yuv420p ingest")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_motion_encode: needs a GPU (nothing here is measured without one)")
    from dawn_pytorch_amd.motion_encoder import MotionEncoder
    from dawn_pytorch_amd.ops import HipOps
    gen, rp, bg = random_state_dicts()
    hip = HipOps()
    me = MotionEncoder(gen, rp, bg, "cuda", ops=hip, chunk=args.chunk)
    H, T = args.res, args.frames
    gd = torch.Generator().manual_seed(1)
    src = torch.rand(3, H, H, generator=gd).cuda()
    drv = torch.randint(0, 256, (T, H, H, 3), generator=gd, dtype=torch.uint8).cuda()
    lat = me.latent(src, drv)                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lat).all())
    times = []
    for _ in range(args.repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        me.latent(src, drv)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    def best_of(fn):
        fn()                                                                    # warm-up
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e-3)
        return out
    via_c = None
    if args.via_c:
        yuv = torch.randint(0, 256, (T, H * H * 3 // 2), generator=gd, dtype=torch.uint8).cuda()
        assert torch.equal(me.latent(src, drv, via_c=True), lat), "the C-side stage must reproduce the Python path's bits"
        t_c = best_of(lambda: me.latent(src, drv, via_c=True))
        t_yuv = best_of(lambda: me.latent(src, yuv, via_c=True))
        t_conv = best_of(lambda: hip.yuv420_to_frames(yuv, H, H))
        byts = T * H * H * 4.5
        via_c = dict(seconds=t_c, frames_per_s=T / min(t_c), i420_seconds=t_yuv, i420_frames_per_s=T / min(t_yuv),
                     yuv420_to_frames=dict(seconds=t_conv, bytes=byts, GBps=byts / min(t_conv) / 1e9, of_hbm_spec=byts / min(t_conv) / HBM_SPEC))
    me.ops = TimedOps(hip)
    me.latent(src, drv)
    torch.cuda.synchronize()
    per_op = {}
    for key, e0, e1 in me.ops.events:
        n, ms = per_op.get(key, (0, 0.0))
        per_op[key] = (n + 1, ms + e0.elapsed_time(e1))
    h = H // me.s
    nb = len(me.bg_enc.downs)
    c_last = me.bg_enc.out_real
    achieved = {}
    if "region_moments" in per_op:
        byts = (T + 1) * h * h * 16 * 4
        achieved["region_moments"] = dict(bytes=byts, GBps=byts / (per_op["region_moments"][1] * 1e-3) / 1e9, of_hbm_spec=byts / (per_op["region_moments"][1] * 1e-3) / HBM_SPEC)
    if "bg_params" in per_op:
        byts = T * (H >> nb) ** 2 * c_last * 4
        achieved["bg_params"] = dict(bytes=byts, GBps=byts / (per_op["bg_params"][1] * 1e-3) / 1e9, of_hbm_spec=byts / (per_op["bg_params"][1] * 1e-3) / HBM_SPEC)
    c1, c2 = me.bg_enc.downs[0].N, me.bg_enc.downs[1].N                           # 64 and 128 in the shipped architecture
    for key, flops in ((f"conv_gemm 3x3 {H}x{H} 16->{c1}", 2.0 * T * H * H * 9 * 3 * c1),          # (the driving half: 3 real input channels)
                       (f"conv_gemm 3x3 {H // 2}x{H // 2} {c1}->{c2}", 2.0 * T * (H // 2) ** 2 * 9 * c1 * c2)):
        if key in per_op:
            achieved[key] = dict(flops=flops, TFLOPs=flops / (per_op[key][1] * 1e-3) / 1e12, of_bf16_spec=flops / (per_op[key][1] * 1e-3) / BF16_SPEC)
    best = min(times)
    res = dict(bench="motion_encode", device=torch.cuda.get_device_name(0), res=H, frames=T, chunk=args.chunk, seconds=times, frames_per_s=T / best,
               op_ms_sum=sum(ms for _, ms in per_op.values()),
               per_op_ms={k: dict(launches=n, ms=round(ms, 3)) for k, (n, ms) in sorted(per_op.items(), key=lambda kv: -kv[1][1])}, achieved=achieved)
    if via_c is not None:
        res["via_c"] = via_c
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
