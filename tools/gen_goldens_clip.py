#!/usr/bin/env python3
"""Trajectories of every x0 clipping mode produced by RUNNING THE REFERENCE sampler in the build container.

    python tools/gen_goldens_clip.py [case ...]        # cases: the names of clip_cases.TINY_CASES and C1 (default: all)

The reference clips the predicted x0 in three ways (MT:1094-1107 in p_mean_variance, MT:1183-1196 in ddim_sample): dynamic
thresholding at `dynamic_thres_percentile` (use_dynamic_thres=True), a static clamp to [-1, 1] (use_dynamic_thres=False, the
constructor default) and no clipping (ddim_sample(clip_denoised=False), DDIM only).  Each case runs the reference's own
`DynamicNfGaussianDiffusion` on the tiny UNet (tiny_unet.npz weights, inputs and initial latent of ddim_tiny.npz):

    ddim_*      : `sample` (-> ddim_sample) at S = 3 (ddim_tiny's S and noise) and S = 50 (seeded noise, clip_cases); `ddim_none`
                  (S = 3 only: clip_cases.NONE_S) calls ddim_sample(fea272, shape, cond=..., clip_denoised=False) with the arguments `sample` forms (MT:1151-1153)
    ancestral_* : `sample` (-> p_sample_loop), 1000 steps, the noise of tests/ancestral_cases.py
    C1          : the shipped architecture (T = 16, h = 32, `init_seed=0` weights, fullsize_cases.build_inputs), DDIM S = 50, static

Each fixture holds the final sample, a few intermediate latents, the per-step quantiles where the mode has any, max|x0| of every
step, and the reference's dynamic(0.9) result on the same inputs and noise.  The conditions that make a fixture able to tell the
modes apart are asserted here and stored, and the tests re-assert them from the stored numbers:

    static : some step has max|x0| > 1 (the clamp acts) and the final sample differs from the dynamic(0.9) one by > 100 x the gate
    none   : differs from the static result by the same margin
    q      : the raw quantile exceeds 1 in some step and the per-step quantiles differ from the 0.9 run's

`x_scale` is the factor applied to the injected initial latent (1.0: the tiny weights produce |x0| > 1 unaided).  Data only; the
reference's Python never leaves this container.
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("DAWN_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(ROOT, "tools", "ref_stubs"))
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")

import DM_3.modules.video_flow_diffusion_multiGPU_v0_crema_plus_faceemb_ca_multi_test as MT  # noqa: E402
from ancestral_cases import ANCESTRAL_NOISE_SEED, ANCESTRAL_STEPS, KEEP, ancestral_noises  # noqa: E402
from clip_cases import (C1, CLIP_NOISE_SEED, DDIM_KEEP, KIND_CODES, MODE_MARGIN, TINY_CASES, ddim_noises_tiny,  # noqa: E402
                        ddim_steps)

torch.set_grad_enabled(False)

X_SCALE = 1.0
TINY = dict(dim=16, cond_dim=24 + 6 + 2, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12,
            channels=3 + 16, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2),
            use_hubert_audio_cond=True, learn_null_cond=False, use_final_activation=False,
            use_deconv=True, padding_mode="zeros", win_width=3)


def run_reference(u, T, h, sampler, mode, cond_scale, fea, bbox, cond, x_init, noises, S, keep):
    """The reference sampler in one clipping mode with the random draws injected (torch.randn -> x_init, torch.randn_like -> noises
    in order).  Returns dict(out, quantiles (per step, empty without dynamic thresholding), x0_absmax (per step), xs {step: latent
    entering it}, seconds)."""
    kind = mode[0]
    kw = dict(use_dynamic_thres=True, dynamic_thres_percentile=mode[1]) if kind == "dynamic" else {}   # else: the constructor default
    steps = ANCESTRAL_STEPS if sampler == "ancestral" else S
    diff = MT.DynamicNfGaussianDiffusion(default_num_frames=T, denoise_fn=u, num_frames=T, image_size=h,
                                         sampling_timesteps=steps, timesteps=1000, loss_type='l2', null_cond_prob=0.1,
                                         ddim_sampling_eta=1.0, **kw)
    diff.update_num_frames(T)
    diff.eval()
    assert diff.is_ddim_sampling == (sampler == "ddim")
    assert diff.use_dynamic_thres == (kind == "dynamic")
    state, calls = {"n": 0}, {"n": 0}
    rr, rl, tq = torch.randn, torch.randn_like, torch.quantile
    qs, xs, amax = [], {}, []

    def frl(t, **k):
        n = noises[state["n"]]
        state["n"] += 1
        return n.clone()

    def fq(*a, **k):
        r = tq(*a, **k)
        qs.append(r.reshape(-1).clone())
        return r

    fwcs, psn = u.forward_with_cond_scale, diff.predict_start_from_noise

    def wrapped(x, *a, **k):
        s = calls["n"]
        calls["n"] += 1
        assert k.get("cond_scale") == cond_scale
        if s in keep:
            xs[s] = x[0, :3].clone()
        return fwcs(x, *a, **k)

    def wrapped_psn(*a, **k):
        r = psn(*a, **k)
        amax.append(r.abs().max().reshape(1).clone())
        return r

    u.forward_with_cond_scale = wrapped
    diff.predict_start_from_noise = wrapped_psn
    torch.randn = lambda *a, **k: x_init.clone()
    torch.randn_like, torch.quantile = frl, fq
    MT.torch.randn, MT.torch.randn_like = torch.randn, frl
    t0 = time.time()
    try:
        if kind == "none":
            fea272 = torch.cat([fea, bbox], dim=1)                                            # MT:1151
            shape = (cond.shape[0], diff.channels, diff.num_frames, fea272.shape[-1], fea272.shape[-1])
            out = diff.ddim_sample(fea272, shape, cond=cond, cond_scale=cond_scale, clip_denoised=False)
        else:
            out = diff.sample(fea, bbox, cond=cond, cond_scale=cond_scale)
    finally:
        torch.randn, torch.randn_like, torch.quantile = rr, rl, tq
        MT.torch.randn, MT.torch.randn_like = rr, rl
        u.forward_with_cond_scale = fwcs
        del diff.predict_start_from_noise
    dt = time.time() - t0
    assert calls["n"] == steps and len(amax) == steps and len(qs) == (steps if kind == "dynamic" else 0), (calls, len(amax), len(qs))
    return dict(out=out, quantiles=torch.cat(qs) if qs else torch.zeros(0), x0_absmax=torch.cat(amax), xs=xs, seconds=dt)


def conditions(name, mode, r, r90, r_static=None):
    """The fixture conditions of the module docstring, asserted on the reference's own numbers; returns what the tests re-assert."""
    kind = mode[0]
    d90 = float((r["out"] - r90["out"]).abs().max())
    if kind == "static":
        assert float(r["x0_absmax"].max()) > 1.0, (name, "the clamp never acts")
        assert d90 > MODE_MARGIN, (name, d90)
    if kind == "none":
        ds = float((r["out"] - r_static["out"]).abs().max())
        assert ds > MODE_MARGIN, (name, ds)
    if kind == "dynamic":
        assert float(r["quantiles"].max()) > 1.0, (name, "s == 1 in every step")
        assert not torch.equal(r["quantiles"], r90["quantiles"]), name
    return d90


def save(name, **arrs):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrs)
    assert os.path.getsize(path) < 1 << 20, path
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.3f} MB")


def tiny_unet():
    g = np.load(os.path.join(OUT, "tiny_unet.npz"))
    sd = {k[len("sd:denoise_fn."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd:denoise_fn.")}
    u = MT.DynamicNfUnet3D(default_num_frames=12, **TINY)
    u.load_state_dict(sd, strict=True)
    u.update_num_frames(12)
    u.eval()
    return u


def gen_tiny(name):
    sampler, mode, cond_scale = TINY_CASES[name]
    d = np.load(os.path.join(OUT, "ddim_tiny.npz"))
    u = tiny_unet()
    T, h = 12, 8
    fea, bbox, cond, x_init = (torch.from_numpy(d[k]) for k in ("fea", "bbox", "cond", "x_init"))
    x_init = x_init * X_SCALE
    arrs = dict(kind=np.array(KIND_CODES[mode[0]]), q=np.float64(mode[1] if mode[0] == "dynamic" else np.nan),
                cond_scale=np.float64(cond_scale), x_scale=np.float64(X_SCALE))
    common = (u, T, h, sampler)
    inputs = (fea, bbox, cond, x_init)
    if sampler == "ancestral":
        noises = ancestral_noises(tuple(x_init.shape))
        r = run_reference(*common, mode, cond_scale, *inputs, noises, None, KEEP)
        # the dynamic(0.9) run on these inputs and this noise is the existing ancestral fixture (tools/gen_goldens_ancestral.py)
        g90 = np.load(os.path.join(OUT, "ancestral_tiny.npz" if cond_scale == 1.0 else "ancestral_guided_tiny.npz"))
        assert float(g90["cond_scale"]) == cond_scale and int(g90["ancestral_noise_seed"]) == ANCESTRAL_NOISE_SEED
        assert np.array_equal(g90["x_init"], x_init.numpy()) and X_SCALE == 1.0
        r90 = dict(out=torch.from_numpy(g90["out"]), quantiles=torch.from_numpy(g90["quantiles"]))
        d90 = conditions(name, mode, r, r90)
        print(f"{name}: {r['seconds']:.1f} s; max|x0| max {float(r['x0_absmax'].max()):.3f}; |out - dynamic(0.9)| = {d90:.4f}; "
              f"quantiles {r['quantiles'][:3].tolist()} max|out| = {float(r['out'].abs().max()):.4f}")
        arrs.update(timesteps=np.array(ANCESTRAL_STEPS), ancestral_noise_seed=np.array(ANCESTRAL_NOISE_SEED), out=r["out"].numpy(),
                    quantiles=r["quantiles"].numpy(), x0_absmax=r["x0_absmax"].numpy(), ref90_out=r90["out"].numpy(),
                    ref90_quantiles=r90["quantiles"].numpy(), keep=np.asarray(KEEP),
                    **{f"x_before_step_{s}": r["xs"][s][None].numpy() for s in KEEP})
    else:
        arrs.update(ddim_noise_seed=np.array(CLIP_NOISE_SEED), S=np.asarray(ddim_steps(name)))
        for S in ddim_steps(name):
            noises = ddim_noises_tiny(tuple(x_init.shape), S, d["noises"])
            keep = DDIM_KEEP[S]
            r = run_reference(*common, mode, cond_scale, *inputs, noises, S, keep)
            r90 = run_reference(*common, ("dynamic", 0.9), cond_scale, *inputs, noises, S, ())
            rs = run_reference(*common, ("static",), cond_scale, *inputs, noises, S, ()) if mode[0] == "none" else None
            d90 = conditions(f"{name} S={S}", mode, r, r90, rs)
            print(f"{name} S={S}: max|x0| max {float(r['x0_absmax'].max()):.3f}; |out - dynamic(0.9)| = {d90:.4f}; quantiles "
                  f"{r['quantiles'][:3].tolist()} ... max {float(r['quantiles'].max()) if len(r['quantiles']) else 0:.3f}; "
                  f"max|out| = {float(r['out'].abs().max()):.4f}")
            arrs.update({f"out_S{S}": r["out"].numpy(), f"quantiles_S{S}": r["quantiles"].numpy(),
                         f"x0_absmax_S{S}": r["x0_absmax"].numpy(), f"ref90_out_S{S}": r90["out"].numpy(),
                         f"ref90_quantiles_S{S}": r90["quantiles"].numpy(), f"keep_S{S}": np.asarray(keep)})
            if rs is not None:
                arrs[f"static_out_S{S}"] = rs["out"].numpy()
            arrs.update({f"x_before_step_{s}_S{S}": r["xs"][s][None].numpy() for s in keep})
    save(f"clip_{name}.npz", **arrs)


def gen_c1():
    import dawn_pytorch_amd as D
    from fullsize_cases import KW, build_inputs, checksum, ddim_noises
    T, h, S, keep = C1["T"], C1["h"], C1["S"], C1["keep"]
    ours = D.DynamicNfUnet3D(default_num_frames=8, **KW, init_seed=0)
    sd = ours.state_dict()
    fea272, cond, x3 = build_inputs(T, h)
    u = MT.DynamicNfUnet3D(default_num_frames=T, **KW)
    u.update_num_frames(T)
    u.load_state_dict(sd, strict=True)
    u.eval()
    inputs = (fea272[:, :256], fea272[:, 256:], cond, x3 * X_SCALE)
    noises = ddim_noises(T, h, S)
    r = run_reference(u, T, h, "ddim", ("static",), 1.0, *inputs, noises, S, keep)
    r90 = run_reference(u, T, h, "ddim", ("dynamic", 0.9), 1.0, *inputs, noises, S, ())
    d90 = conditions("C1", ("static",), r, r90)
    print(f"C1: reference DDIM static T={T} h={h} S={S}: {r['seconds']:.1f} s on {torch.get_num_threads()} threads; max|x0| max "
          f"{float(r['x0_absmax'].max()):.3f}; |out - dynamic(0.9)| = {d90:.4f}; max|out| = {float(r['out'].abs().max()):.4f}")
    save("clip_C1_static.npz", T=T, h=h, S=S, kind=np.array(KIND_CODES["static"]), cond_scale=np.float64(1.0),
         x_scale=np.float64(X_SCALE), ddim_noise_seed=1234, out=r["out"][0].numpy(), x0_absmax=r["x0_absmax"].numpy(),
         ref90_out=r90["out"][0].numpy(), ref90_quantiles=r90["quantiles"].numpy(), weights_checksum=checksum(sd.values()),
         inputs_checksum=checksum([fea272, cond, x3]), ref_seconds=r["seconds"], keep=np.asarray(keep),
         **{f"x_before_step_{s}": r["xs"][s].numpy() for s in keep})


if __name__ == "__main__":
    for name in sys.argv[1:] or [*TINY_CASES, "C1"]:
        gen_c1() if name == "C1" else gen_tiny(name)
