#!/usr/bin/env python3
"""Ancestral (DDPM) trajectories produced by RUNNING THE REFERENCE sampler in the build container.

    python tools/gen_goldens_ancestral.py [case ...]        # cases: tiny guided_tiny C1 (default: all)

The reference `DynamicNfGaussianDiffusion.sample` with sampling_timesteps = timesteps = 1000 takes `p_sample_loop`
(MT:1124-1135, dispatch MT:1150): 1000 evaluations at the integer times 999 ... 0, each followed by the dynamic-threshold
quantile (MT:1097-1106) and the posterior step `mean + (t > 0) * exp(0.5 * log_var) * noise` (MT:1113-1121).

    tiny        : the `ddim_tiny` configuration (tiny_unet.npz weights; inputs and initial latent of ddim_tiny.npz)
    guided_tiny : tiny at cond_scale = 2.5 (forward_with_cond_scale, MT:879-890)
    C1          : T=16, h=32 at the shipped architecture (the deterministic `init_seed=0` weights, fullsize_cases.build_inputs)

The per-step noise (torch.randn_like, MT:1118, 1000 draws: t = 0 draws too) comes from ONE seeded CPU generator that the
tests re-create (tests/ancestral_cases.py, `ancestral_noise_seed`).  Each fixture holds: the final sample, the quantile of
EVERY step, the latents entering steps 1, 500, 900 and 999, and the reference's (coef1, coef2, std) of every step.  Data only;
the reference's Python never leaves this container.
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

torch.set_grad_enabled(False)

TINY = dict(dim=16, cond_dim=24 + 6 + 2, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12,
            channels=3 + 16, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2),
            use_hubert_audio_cond=True, learn_null_cond=False, use_final_activation=False,
            use_deconv=True, padding_mode="zeros", win_width=3)


def run_reference(u, T, h, fea, bbox, cond, x_init, cond_scale):
    """Reference ancestral sampler with the random draws injected: torch.randn (MT:1128) -> x_init, torch.randn_like
    (MT:1118) -> the seeded noise in order.  Returns (out, quantiles, {step: latent entering it}, (coef1, coef2, std), seconds)."""
    diff = MT.DynamicNfGaussianDiffusion(default_num_frames=T, denoise_fn=u, num_frames=T, image_size=h,
                                         sampling_timesteps=ANCESTRAL_STEPS, timesteps=ANCESTRAL_STEPS, loss_type='l2',
                                         use_dynamic_thres=True, null_cond_prob=0.1, ddim_sampling_eta=1.0)
    diff.update_num_frames(T)
    diff.eval()
    assert not diff.is_ddim_sampling
    noises = ancestral_noises(tuple(x_init.shape))
    state = {"n": 0}
    rr, rl, tq = torch.randn, torch.randn_like, torch.quantile
    qs, xs, coefs = [], {}, []

    def frl(t, **k):
        n = noises[state["n"]]
        state["n"] += 1
        return n.clone()

    def fq(*a, **k):
        r = tq(*a, **k)
        qs.append(r.reshape(-1).clone())
        return r

    calls = {"n": 0}
    fwcs = u.forward_with_cond_scale

    def wrapped(x, *a, **k):
        s = calls["n"]
        calls["n"] += 1
        assert k.get("cond_scale") == cond_scale
        if s in KEEP:
            xs[s] = x[0, :3].clone()
        return fwcs(x, *a, **k)

    qpost = diff.q_posterior

    def q_posterior(x_start, x_t, t):
        # the reference's own scalars of this step: extract() of the fp32 buffers, std = (0.5 * log_var).exp() as p_sample forms it
        mean, var, lv = qpost(x_start=x_start, x_t=x_t, t=t)
        c1 = MT.extract(diff.posterior_mean_coef1, t, x_t.shape).reshape(-1)[0]
        c2 = MT.extract(diff.posterior_mean_coef2, t, x_t.shape).reshape(-1)[0]
        coefs.append(torch.stack([c1, c2, (0.5 * lv).exp().reshape(-1)[0]]))
        return mean, var, lv

    u.forward_with_cond_scale = wrapped
    diff.q_posterior = q_posterior
    torch.randn = lambda *a, **k: x_init.clone()
    torch.randn_like, torch.quantile = frl, fq
    MT.torch.randn, MT.torch.randn_like = torch.randn, frl
    t0 = time.time()
    try:
        out = diff.sample(fea, bbox, cond=cond, cond_scale=cond_scale)
    finally:
        torch.randn, torch.randn_like, torch.quantile = rr, rl, tq
        MT.torch.randn, MT.torch.randn_like = rr, rl
        u.forward_with_cond_scale = fwcs
    dt = time.time() - t0
    assert len(qs) == ANCESTRAL_STEPS and calls["n"] == ANCESTRAL_STEPS and state["n"] == ANCESTRAL_STEPS, (len(qs), calls, state)
    return out, torch.cat(qs), xs, torch.stack(coefs), dt


def save(name, **arrs):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.3f} MB")


def _tiny(name, cond_scale):
    g = np.load(os.path.join(OUT, "tiny_unet.npz"))
    d = np.load(os.path.join(OUT, "ddim_tiny.npz"))
    sd = {k[len("sd:denoise_fn."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd:denoise_fn.")}
    u = MT.DynamicNfUnet3D(default_num_frames=12, **TINY)
    u.load_state_dict(sd, strict=True)
    u.update_num_frames(12)
    u.eval()
    T, h = 12, 8
    fea, bbox, cond, x_init = (torch.from_numpy(d[k]) for k in ("fea", "bbox", "cond", "x_init"))
    out, qs, xs, coefs, dt = run_reference(u, T, h, fea, bbox, cond, x_init, cond_scale)
    print(f"{name}: reference ancestral, cond_scale={cond_scale}: {dt:.1f} s; quantiles {qs[:3].tolist()} ... {qs[-3:].tolist()}; "
          f"max|out| = {float(out.abs().max()):.4f}")
    save(f"ancestral_{name}.npz", fea=fea.numpy(), bbox=bbox.numpy(), cond=cond.numpy(), x_init=x_init.numpy(),
         timesteps=np.array(ANCESTRAL_STEPS), ancestral_noise_seed=np.array(ANCESTRAL_NOISE_SEED), cond_scale=np.float64(cond_scale),
         out=out.numpy(), quantiles=qs.numpy(), coefs=coefs.numpy(), ref_seconds=dt, keep=np.asarray(sorted(xs)),
         **{f"x_before_step_{s}": xs[s][None].numpy() for s in xs})


def gen_tiny():
    _tiny("tiny", 1.0)


def gen_guided_tiny():
    _tiny("guided_tiny", 2.5)


def gen_c1():
    import dawn_pytorch_amd as D
    from fullsize_cases import KW, build_inputs, checksum
    T, h = 16, 32
    ours = D.DynamicNfUnet3D(default_num_frames=8, **KW, init_seed=0)
    sd = ours.state_dict()
    fea272, cond, x3 = build_inputs(T, h)
    u = MT.DynamicNfUnet3D(default_num_frames=T, **KW)
    u.update_num_frames(T)
    u.load_state_dict(sd, strict=True)
    u.eval()
    out, qs, xs, coefs, dt = run_reference(u, T, h, fea272[:, :256], fea272[:, 256:], cond, x3, 1.0)
    print(f"C1: reference ancestral T={T} h={h}: {dt:.1f} s on {torch.get_num_threads()} threads; quantiles {qs[:3].tolist()} ... "
          f"{qs[-3:].tolist()}; max|out| = {float(out.abs().max()):.4f}")
    save("ancestral_C1.npz", T=T, h=h, timesteps=np.array(ANCESTRAL_STEPS), ancestral_noise_seed=np.array(ANCESTRAL_NOISE_SEED),
         cond_scale=np.float64(1.0), out=out[0].numpy(), quantiles=qs.numpy(), coefs=coefs.numpy(),
         weights_checksum=checksum(sd.values()), inputs_checksum=checksum([fea272, cond, x3]), ref_seconds=dt,
         keep=np.asarray(sorted(xs)), **{f"x_before_step_{s}": xs[s].numpy() for s in xs})


if __name__ == "__main__":
    cases = {"tiny": gen_tiny, "guided_tiny": gen_guided_tiny, "C1": gen_c1}
    for name in sys.argv[1:] or list(cases):
        cases[name]()
