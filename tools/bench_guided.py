#!/usr/bin/env python3
"""One unguided DDIM step against one guided (cond_scale != 1) step, per host path, at the benchmark shape (256x256 -> 64x64 latent,
200 frames, the shipped architecture), timed with HIP events around whole S-step sampler runs (per step = total / S).

    python tools/bench_guided.py [--frames 200] [--res 256] [--steps 5] [--reps 3] [--out FILE.json]

Paths: the C evaluator (dawn_sampler_run vs dawn_sampler_run_guided), the Python host replaying a HIP graph, the Python host eager.
The guided step runs the condition-free prefix once, so guided / unguided < 2; the prefix's share of an evaluation follows from
the two times: prefix = 2 * unguided - guided (both steps also carry the same sampler tail: x0, threshold, update)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import UNET_KW  # noqa: E402
import dawn_pytorch_amd as D  # noqa: E402
from dawn_pytorch_amd.sampler import ddim_step_scalars  # noqa: E402


def timed(fn, reps):
    fn()                                                     # warm-up (allocator, graph capture, lazy inits)
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scale", type=float, default=2.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, h, S = a.frames, a.res // 4, a.steps
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    unet = D.DynamicNfUnet3D(default_num_frames=T, num_frames=T, init_seed=0, **UNET_KW).to(dev)
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T, denoise_fn=unet, num_frames=T, image_size=h, sampling_timesteps=S,
                                        timesteps=1000, loss_type='l2', use_dynamic_thres=True, null_cond_prob=0.1,
                                        ddim_sampling_eta=1.0).to(dev)
    g = torch.Generator().manual_seed(123)
    fea = torch.randn(1, 256, h, h, generator=g).to(dev)
    bbox = torch.randn(1, 16, h, h, generator=g).to(dev)
    cond = torch.randn(1, T, 1032, generator=g).to(dev)
    x_init = torch.randn(1, 3, T, h, h, generator=g).to(dev)
    diff.noise_seed = 7

    res = {"frames": T, "res": a.res, "latent": h, "ddim_steps_per_run": S, "cond_scale": a.scale, "device": torch.cuda.get_device_name(0)}

    # C evaluator
    ev = unet.ctx_evaluator()
    P = unet.packed()
    rcos, rsin = P.rotary_tables(T + 2 * P.win)
    f272 = torch.cat((fea, bbox), 1)[0].contiguous()
    clip = ev.prepare_clip(f272, cond[0].contiguous(), rcos, rsin)
    null_clip = ev.prepare_null_clip(f272, T, rcos, rsin)
    steps = ddim_step_scalars({k: getattr(diff, k) for k in ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                              "sqrt_recipm1_alphas_cumprod")}, S, 1.0)
    x0 = x_init[0].contiguous()
    paths = {
        "c_evaluator": (lambda: ev.sample(clip, x0, steps, seed=7),
                        lambda: ev.sample(clip, x0, steps, seed=7, null_clip=null_clip, cond_scale=a.scale)),
    }

    def py(graph, scale):
        def run():
            diff.use_graph = graph
            try:
                diff.sample(fea, bbox, cond=cond, cond_scale=scale, x_init=x_init)
            finally:
                diff.use_graph = False
        return run
    paths["python_graph"] = (py(True, 1.0), py(True, a.scale))
    paths["python_eager"] = (py(False, 1.0), py(False, a.scale))
    for name, (unguided, guided) in paths.items():
        tu = timed(unguided, a.reps) / S
        tg = timed(guided, a.reps) / S
        prefix = 2 * tu - tg
        res[name] = {"unguided_step_ms": round(tu, 3), "guided_step_ms": round(tg, 3), "ratio": round(tg / tu, 4),
                     "prefix_ms_implied": round(prefix, 3), "prefix_share_implied": round(prefix / tu, 4)}
        print(f"{name:13s}: unguided {tu:8.3f} ms/step  guided {tg:8.3f} ms/step  ratio {tg / tu:.4f}  "
              f"implied prefix {prefix:.3f} ms ({100 * prefix / tu:.1f} % of a step)", flush=True)
    if unet._ops().graph_error:
        res["graph_error"] = unet._ops().graph_error
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
