#!/usr/bin/env python3
"""GPU box: throughput of the LFG flow decode -- `FlowDecoder.decode_clip` on a synthetic clip with
the shipped generator topology (64/128/256 channels, 6 bottleneck blocks) and seeded random weights.

    python tools/bench_decode.py [--res 256] [--frames 200] [--iters 3] [--cpu-frames 2] [--chunk 64]
    python tools/bench_decode.py --u8 [--iters 5] [--chunk 64] [--out profiles/decode_u8.json]
    python tools/bench_decode.py --yuv420 [--iters 5] [--chunk 64] [--out profiles/decode_yuv420.json]

Prints one JSON line: decoded frames/s, algorithmic TFLOP/s of the convolutions (dense math of GEN:138-171 per frame,
encoder excluded -- it runs once per clip here and once per FRAME in the reference), the per-kernel-class time split
measured with HIP events, and the CPU oracle (oracle/lfg_ref.py) timed on `--cpu-frames` frames beside it.

`--u8` times the two ways from a sampled clip to frames in host memory, at 256^2 / 200 frames and at 128^2 / 400 frames, alternating
them in one process: (a) `decode_clip` + `frames_to_u8` + `.cpu()` (two fp32 clips on the device, one conversion launch, one copy)
and (b) `stream_frames_u8` drained to the host (the decoder's last kernel writes the bytes; each chunk's copy overlaps the next
chunk's decode).  Host wall clock around work that ends with the bytes in host memory; peak allocated device bytes of each.

`--yuv420` times `stream_frames_u8` against `stream_frames_yuv420` the same way (alternating in one process, host wall clock until the
last byte is in host memory), plus the device time of the two forms of the final-conv kernel alone (HIP events around one chunk's
launch), and checks the yuv bytes against egress.yuv420_from_rgb_u8 of the RGB ones.  A report, not a gate: from the byte counts the
expectation is device time within noise of the u8 form and half the device->host bytes."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def lfg_state_dict(seed=0, be=64, max_features=512, n_down=2, n_bott=6):
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(p, co, ci, k):
        sd[p + ".weight"] = torch.randn(co, ci, k, k, generator=g) * (ci * k * k) ** -0.5
        sd[p + ".bias"] = torch.randn(co, generator=g) * 0.1

    def bn(p, c):
        sd[p + ".weight"] = 1 + 0.2 * torch.randn(c, generator=g)
        sd[p + ".bias"] = 0.2 * torch.randn(c, generator=g)
        sd[p + ".running_mean"] = 0.2 * torch.randn(c, generator=g)
        sd[p + ".running_var"] = torch.rand(c, generator=g) + 0.5

    conv("first.conv", be, 3, 7); bn("first.norm", be)
    for i in range(n_down):
        ci, co = min(max_features, be * 2 ** i), min(max_features, be * 2 ** (i + 1))
        conv(f"down_blocks.{i}.conv", co, ci, 3); bn(f"down_blocks.{i}.norm", co)
    for i in range(n_down):
        ci, co = min(max_features, be * 2 ** (n_down - i)), min(max_features, be * 2 ** (n_down - i - 1))
        conv(f"up_blocks.{i}.conv", co, ci, 3); bn(f"up_blocks.{i}.norm", co)
    cb = min(max_features, be * 2 ** n_down)
    for i in range(n_bott):
        for j in (1, 2):
            conv(f"bottleneck.r{i}.conv{j}", cb, cb, 3); bn(f"bottleneck.r{i}.norm{j}", cb)
    sd["final.weight"] = torch.randn(3, be, 7, 7, generator=g) * (be * 49) ** -0.5
    sd["final.bias"] = torch.randn(3, generator=g) * 0.1
    return sd


def decode_flops_per_frame(res, be=64, n_bott=6):
    """Dense multiply-adds x2 of the per-frame part of GEN:138-171 (bottleneck, up blocks, final conv)."""
    hb = res // 4
    cb = be * 4
    f = n_bott * 2 * 2.0 * hb * hb * 9 * cb * cb
    f += 2.0 * (2 * hb) ** 2 * 9 * cb * (cb // 2)
    f += 2.0 * (4 * hb) ** 2 * 9 * (cb // 2) * be
    f += 2.0 * res * res * 49 * be * 3
    return f


def synthetic_motion(T, h, device, seed=123):
    g = torch.Generator().manual_seed(seed)
    lin = (torch.arange(h, dtype=torch.float32) + 0.5) / h * 2 - 1
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    grid = torch.stack((xx, yy), 0).view(1, 2, 1, h, h) + torch.randn(1, 2, T, h, h, generator=g) * 0.1
    conf = torch.rand(1, 1, T, h, h, generator=g)
    return grid.to(device), conf.to(device)


def run(res=256, frames=200, iters=3, chunk=64, cpu_frames=2, seed=0):
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.ops import HipOps
    dev = torch.device("cuda:0")
    sd = lfg_state_dict(seed)
    ops = HipOps()
    dec = FlowDecoder(sd, dev, ops=ops, chunk=chunk)
    img = torch.rand(1, 3, res, res, generator=torch.Generator().manual_seed(1)).to(dev)
    grid, conf = synthetic_motion(frames, res // 4, dev)
    dec.decode_clip(img, grid, conf)                       # warm-up (weights resident, attributes set)
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dec.decode_clip(img, grid, conf)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    dt = sorted(ts)[len(ts) // 2]
    fl = decode_flops_per_frame(res) * frames
    # per-class split with HIP events around every op of one more decode
    classes = {}
    real = {}
    for name in ("conv_gemm", "warp_blend", "affine_act", "final_conv_blend", "init_conv_x", "bn_relu_pool2"):
        fn = getattr(ops, name)
        real[name] = fn

        def wrap(*a, _fn=fn, _name=name, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = _fn(*a, **k)
            e1.record()
            classes.setdefault(_name, []).append((e0, e1))
            return r
        setattr(ops, name, wrap)
    dec.decode_clip(img, grid, conf)
    torch.cuda.synchronize()
    for name, fn in real.items():
        setattr(ops, name, fn)
    split = {k: {"launches": len(v), "ms": sum(a.elapsed_time(b) for a, b in v)} for k, v in classes.items()}
    result = {"metric": "decoded frames/sec (LFG flow decode, FD:372-385 batched)", "value": frames / dt, "unit": "frames/s",
              "config": {"workload": f"{res}x{res}, {frames} frames, generator 64/128/256 ch, 6 bottleneck blocks",
                         "chunk": chunk}, "dtype": "f32 (3x3 convs: exact 3-way bf16 operand split, fp32 accumulate)",
              "data": "synthetic", "ms_per_clip": dt * 1e3, "algorithmic_tflop_per_clip": fl / 1e12,
              "algorithmic_tflops": fl / dt / 1e12, "kernel_ms": split, "all_iters_ms": [t * 1e3 for t in ts]}
    if cpu_frames > 0:
        from oracle import lfg_ref
        n = torch.get_num_threads()
        cg, cc = grid[:, :, :cpu_frames].cpu(), conf[:, :, :cpu_frames].cpu()
        t0 = time.perf_counter()
        want = lfg_ref.decode_clip(sd, img.cpu(), cg, cc, chunk=1)
        tc = time.perf_counter() - t0
        err = float((out["sample_out_vid"][:, :, :cpu_frames].cpu() - want["sample_out_vid"]).abs().max())
        result["cpu_baseline"] = {"value": cpu_frames / tc, "unit": "frames/s", "cores": n, "kind": "port",
                                  "sample": f"{cpu_frames} frames of the same clip through oracle/lfg_ref.py "
                                            "(per-frame encoder re-run included, as in the reference)"}
        result["max_abs_err_vs_oracle"] = err
    return result


def run_u8(iters=5, chunk=64, seed=0, cases=((256, 200), (128, 400))):
    """(a) and (b) of the module docstring, alternating a, b, a, b, ... after one warm-up of each; medians and all samples."""
    import numpy as np
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.ops import HipOps
    dev = torch.device("cuda:0")
    ops = HipOps()
    dec = FlowDecoder(lfg_state_dict(seed), dev, ops=ops, chunk=chunk)
    results = []
    for res, frames in cases:
        img = torch.rand(1, 3, res, res, generator=torch.Generator().manual_seed(1)).to(dev)
        grid, conf = synthetic_motion(frames, res // 4, dev)

        def two_step():
            vid = dec.decode_clip(img, grid, conf)["sample_out_vid"][0]
            return ops.frames_to_u8(vid).cpu().numpy()

        def streamed():
            out = np.empty((frames, res, res, 3), dtype=np.uint8)
            for t0, fr in dec.stream_frames_u8(img, grid, conf):
                out[t0:t0 + len(fr)] = fr
            return out

        def timed(fn):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() - base, out

        _, _, a0 = timed(two_step)                     # warm-up of every shape; the two must agree byte for byte
        _, _, b0 = timed(streamed)
        same = bool(np.array_equal(a0, b0))
        del a0, b0
        ta, tb, pa, pb = [], [], 0, 0
        for _ in range(iters):
            ms, peak, _o = timed(two_step)
            ta.append(ms); pa = max(pa, peak)
            ms, peak, _o = timed(streamed)
            tb.append(ms); pb = max(pb, peak)
        med = lambda v: sorted(v)[len(v) // 2]         # noqa: E731
        results.append({"workload": f"{res}x{res}, {frames} frames, chunk {chunk}", "bytes_identical": same,
                        "two_step_ms": med(ta), "streamed_ms": med(tb), "two_step_all_ms": ta, "streamed_all_ms": tb,
                        "two_step_peak_device_bytes": pa, "streamed_peak_device_bytes": pb,
                        "fp32_clip_bytes": 3 * frames * res * res * 4})
    return {"metric": "sampled clip -> uint8 frames in host memory, ms per clip (host wall clock, ends after the last byte arrived)",
            "a": "decode_clip + frames_to_u8 + .cpu()", "b": "stream_frames_u8 drained to the host", "iters": iters,
            "order": "a, b alternating in one process after one warm-up of each", "data": "synthetic", "cases": results}


def run_yuv420(iters=5, chunk=64, seed=0, cases=((256, 200), (128, 400))):
    """stream_frames_u8 (a) against stream_frames_yuv420 (b), alternating a, b, a, b, ... after one warm-up of each."""
    import numpy as np
    from dawn_pytorch_amd.egress import yuv420_from_rgb_u8
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.ops import HipOps
    dev = torch.device("cuda:0")
    ops = HipOps()
    dec = FlowDecoder(lfg_state_dict(seed), dev, ops=ops, chunk=chunk)
    results = []
    for res, frames in cases:
        img = torch.rand(1, 3, res, res, generator=torch.Generator().manual_seed(1)).to(dev)
        grid, conf = synthetic_motion(frames, res // 4, dev)
        fb = res * res * 3 // 2

        def rgb():
            out = np.empty((frames, res, res, 3), dtype=np.uint8)
            for t0, fr in dec.stream_frames_u8(img, grid, conf):
                out[t0:t0 + len(fr)] = fr
            return out

        def yuv():
            out = np.empty((frames, fb), dtype=np.uint8)
            for t0, fr in dec.stream_frames_yuv420(img, grid, conf):
                out[t0:t0 + len(fr)] = fr
            return out

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out

        _, a0 = timed(rgb)                             # warm-up of every shape; b must be the definition applied to a
        _, b0 = timed(yuv)
        same = bool(np.array_equal(yuv420_from_rgb_u8(torch.from_numpy(a0)).numpy(), b0))
        del a0, b0
        ta, tb = [], []
        for _ in range(iters):
            ta.append(timed(rgb)[0])
            tb.append(timed(yuv)[0])
        # the last kernel of a chunk alone, both forms, on the same input
        n = min(chunk, frames)
        C0 = dec.C0
        x = torch.randn(n * res * res, C0, generator=torch.Generator().manual_seed(2)).to(dev)
        g, cf = grid[0, :, :n], conf[0, 0, :n].contiguous()
        fu8 = torch.empty(n, res, res, 3, device=dev, dtype=torch.uint8)
        fyuv = torch.empty(n, fb, device=dev, dtype=torch.uint8)
        ku, ky = [], []
        for i in range(iters + 1):
            for fn, buf, acc in ((ops.final_conv_blend_u8, fu8, ku), (ops.final_conv_blend_yuv420, fyuv, ky)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(x, res, res, dec.final_w7, dec.final_bias, img[0].contiguous(), g, cf, buf)
                e1.record()
                e1.synchronize()
                if i:
                    acc.append(e0.elapsed_time(e1))
        med = lambda v: sorted(v)[len(v) // 2]         # noqa: E731
        results.append({"workload": f"{res}x{res}, {frames} frames, chunk {chunk}", "yuv_is_definition_of_rgb": same,
                        "stream_u8_ms": med(ta), "stream_yuv420_ms": med(tb), "stream_u8_all_ms": ta, "stream_yuv420_all_ms": tb,
                        "d2h_bytes_u8": frames * res * res * 3, "d2h_bytes_yuv420": frames * fb,
                        "final_conv_u8_kernel_ms": med(ku), "final_conv_yuv420_kernel_ms": med(ky), "kernel_frames": n,
                        "final_conv_u8_kernel_all_ms": ku, "final_conv_yuv420_kernel_all_ms": ky})
    return {"metric": "sampled clip -> frames in host memory, ms per clip (host wall clock, ends after the last byte arrived)",
            "a": "stream_frames_u8 drained to the host", "b": "stream_frames_yuv420 drained to the host", "iters": iters,
            "order": "a, b alternating in one process after one warm-up of each", "data": "synthetic", "cases": results}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--iters", type=int, default=None, help="timed repetitions (default 3; 5 with --u8)")
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--cpu-frames", type=int, default=2)
    ap.add_argument("--u8", action="store_true", help="time decode_clip + frames_to_u8 + .cpu() against stream_frames_u8")
    ap.add_argument("--yuv420", action="store_true", help="time stream_frames_u8 against stream_frames_yuv420")
    ap.add_argument("--out", type=str, default=None, help="--u8 / --yuv420: also write the JSON result to this file")
    a = ap.parse_args()
    if a.u8 or a.yuv420:
        r = (run_yuv420 if a.yuv420 else run_u8)(5 if a.iters is None else a.iters, a.chunk)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(r, f, indent=1)
                f.write("\n")
        print(json.dumps(r))
        sys.exit(0)
    print(json.dumps(run(a.res, a.frames, 3 if a.iters is None else a.iters, a.chunk, a.cpu_frames)))
