#!/usr/bin/env python3
"""One ancestral (DDPM) step against one DDIM step, on the C evaluator and on the Python host replaying a HIP graph, timed with HIP
events around whole sampler runs of `--steps` steps (per step = total / steps).

    python tools/bench_ancestral.py [--case C1|configs2|all] [--steps 20] [--reps 3] [--out FILE.json]

    C1       : 128x128 -> 32x32 latent, 16 frames (the shipped architecture; the C1 fixtures' shape)
    configs2 : 256x256 -> 64x64 latent, 200 frames (the benchmark shape)

The two loops share the evaluation, x0 and the threshold selection; they differ in the step tail only (dawn_ancestral_update in
place vs dawn_ddim_update), so the ratio should be 1 within noise.  The ancestral run takes the first `--steps` steps of the
1000-step schedule (t = 999 ...); a whole ancestral clip costs 1000 such steps."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import UNET_KW  # noqa: E402
import dawn_pytorch_amd as D  # noqa: E402
from dawn_pytorch_amd.sampler import (ancestral_sample_clip, ancestral_step_scalars, ddim_sample_clip,  # noqa: E402
                                      ddim_step_scalars)

CASES = {"C1": (16, 128), "configs2": (200, 256)}


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


def run_case(T, res, S, reps):
    h = res // 4
    dev = torch.device("cuda:0")
    unet = D.DynamicNfUnet3D(default_num_frames=T, num_frames=T, init_seed=0, **UNET_KW).to(dev)
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T, denoise_fn=unet, num_frames=T, image_size=h, sampling_timesteps=S,
                                        timesteps=1000, loss_type='l2', use_dynamic_thres=True, null_cond_prob=0.1,
                                        ddim_sampling_eta=1.0).to(dev)
    g = torch.Generator().manual_seed(123)
    fea = torch.randn(1, 256, h, h, generator=g).to(dev)
    bbox = torch.randn(1, 16, h, h, generator=g).to(dev)
    cond = torch.randn(1, T, 1032, generator=g).to(dev)
    x_init = torch.randn(1, 3, T, h, h, generator=g).to(dev)
    ddim = ddim_step_scalars({k: getattr(diff, k) for k in ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                             "sqrt_recipm1_alphas_cumprod")}, S, 1.0)
    anc = ancestral_step_scalars({k: getattr(diff, k) for k in (
        "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
        "posterior_log_variance_clipped")}, 1000)[:S]
    out = {"frames": T, "res": res, "latent": h, "steps_per_run": S}

    ev = unet.ctx_evaluator()
    P = unet.packed()
    rcos, rsin = P.rotary_tables(T + 2 * P.win)
    f272 = torch.cat((fea, bbox), 1)[0].contiguous()
    clip = ev.prepare_clip(f272, cond[0].contiguous(), rcos, rsin)
    x0 = x_init[0].contiguous()
    ops = unet._ops()
    cs = unet.build_clip(f272, cond[0].contiguous())

    def noise(i):
        return ops.philox_normal(3, T, 0, T, h * h, 7, i + 1, dev).reshape(3, T, h, h)

    paths = {
        "c_evaluator": (lambda: ev.sample(clip, x0, ddim, seed=7), lambda: ev.sample_ancestral(clip, x0, anc, seed=7)),
        "python_graph": (lambda: ddim_sample_clip(ops, P, cs, x0, ddim, noise, use_graph=True),
                         lambda: ancestral_sample_clip(ops, P, cs, x0, anc, noise, use_graph=True)),
    }
    for name, (f_ddim, f_anc) in paths.items():
        td = timed(f_ddim, reps) / S
        ta = timed(f_anc, reps) / S
        out[name] = {"ddim_step_ms": round(td, 3), "ancestral_step_ms": round(ta, 3), "ratio": round(ta / td, 4),
                     "ancestral_1000_step_clip_s": round(ta, 3)}
        print(f"T={T} {res}x{res} {name:12s}: DDIM {td:8.3f} ms/step  ancestral {ta:8.3f} ms/step  ratio {ta / td:.4f}  "
              f"(1000-step clip {ta:.2f} s)", flush=True)
    if ops.graph_error:
        out["graph_error"] = ops.graph_error
    del ev, clip, cs, unet, diff
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="all", choices=sorted(CASES) + ["all"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.set_grad_enabled(False)
    res = {"device": torch.cuda.get_device_name(0)}
    for name in (sorted(CASES) if a.case == "all" else [a.case]):
        res[name] = run_case(*CASES[name], a.steps, a.reps)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
