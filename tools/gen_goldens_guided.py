#!/usr/bin/env python3
"""Guided (classifier-free guidance, cond_scale = 2.5) DDIM trajectories produced by RUNNING THE REFERENCE sampler in the
build container.

    python tools/gen_goldens_guided.py [case ...]        # cases: tiny C1 (default: both)

The reference `DynamicNfGaussianDiffusion.sample(..., cond_scale=2.5)` (MT:1137-1208) calls
`forward_with_cond_scale` (MT:879-890): the conditional evaluation, then the null-condition one (all-zero condition,
`learn_null_cond=False`, MT:917-922), combined as null + (cond - null) * scale.

    tiny : the `ddim_tiny` configuration (tiny_unet.npz weights; inputs, initial latent and per-step noise of ddim_tiny.npz)
    C1   : T=16, h=32, S=10 at the shipped architecture (the deterministic `init_seed=0` weights; inputs and noise exactly as
           tools/gen_goldens_ddim.py draws them for its C1 case)

Each fixture holds outputs only (plus the tiny case's small inputs): the final sample, the latent before a few steps,
and the dynamic-threshold quantile of EVERY step (torch.quantile, MT:1186-1190).  Data only; the reference's Python never
leaves this container.
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

torch.set_grad_enabled(False)

COND_SCALE = 2.5
TINY = dict(dim=16, cond_dim=24 + 6 + 2, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12,
            channels=3 + 16, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2),
            use_hubert_audio_cond=True, learn_null_cond=False, use_final_activation=False,
            use_deconv=True, padding_mode="zeros", win_width=3)


def run_reference(u, T, h, S, fea, bbox, cond, x_init, noises, keep):
    """Reference sampler with the random draws injected: torch.randn (MT:1166) -> x_init, torch.randn_like (MT:1201) ->
    noises in order.  Returns (out, per-step quantiles, {step: latent entering that step}, seconds)."""
    diff = MT.DynamicNfGaussianDiffusion(default_num_frames=T, denoise_fn=u, num_frames=T, image_size=h,
                                         sampling_timesteps=S, timesteps=1000, loss_type='l2', use_dynamic_thres=True,
                                         null_cond_prob=0.1, ddim_sampling_eta=1.0)
    diff.update_num_frames(T)
    diff.eval()
    state = {"n": 0}
    rr, rl, tq = torch.randn, torch.randn_like, torch.quantile
    qs, xs = [], {}

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
        assert k.get("cond_scale") == COND_SCALE
        if s in keep:
            xs[s] = x[0, :3].clone()
        return fwcs(x, *a, **k)
    u.forward_with_cond_scale = wrapped
    torch.randn = lambda *a, **k: x_init.clone()
    torch.randn_like, torch.quantile = frl, fq
    MT.torch.randn, MT.torch.randn_like = torch.randn, frl
    t0 = time.time()
    try:
        out = diff.sample(fea, bbox, cond=cond, cond_scale=COND_SCALE)
    finally:
        torch.randn, torch.randn_like, torch.quantile = rr, rl, tq
        MT.torch.randn, MT.torch.randn_like = rr, rl
        u.forward_with_cond_scale = fwcs
    dt = time.time() - t0
    assert len(qs) == S and calls["n"] == S, (len(qs), calls["n"])
    return out, torch.cat(qs), xs, dt


def save(name, **arrs):
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **arrs)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.3f} MB")


def gen_tiny():
    g = np.load(os.path.join(OUT, "tiny_unet.npz"))
    d = np.load(os.path.join(OUT, "ddim_tiny.npz"))
    sd = {k[len("sd:denoise_fn."):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("sd:denoise_fn.")}
    u = MT.DynamicNfUnet3D(default_num_frames=12, **TINY)
    u.load_state_dict(sd, strict=True)
    u.update_num_frames(12)
    u.eval()
    S = int(d["S"])
    T, h = 12, 8
    fea, bbox, cond, x_init = (torch.from_numpy(d[k]) for k in ("fea", "bbox", "cond", "x_init"))
    noises = [torch.from_numpy(n) for n in d["noises"]]
    keep = (1, 2)
    out, qs, xs, dt = run_reference(u, T, h, S, fea, bbox, cond, x_init, noises, keep)
    print(f"tiny: guided reference DDIM S={S}: quantiles {qs.tolist()}, max|out| = {float(out.abs().max()):.4f}")
    save("ddim_guided_tiny.npz", fea=fea.numpy(), bbox=bbox.numpy(), cond=cond.numpy(), x_init=x_init.numpy(),
         noises=d["noises"], S=np.array(S), cond_scale=np.float64(COND_SCALE), out=out.numpy(), quantiles=qs.numpy(),
         keep=np.asarray(sorted(xs)), **{f"x_before_step_{s}": xs[s][None].numpy() for s in xs})


def gen_c1():
    import dawn_pytorch_amd as D
    from fullsize_cases import DDIM_CASES, KW, build_inputs, checksum, ddim_noises
    T, h, S, keep = DDIM_CASES["C1"]
    ours = D.DynamicNfUnet3D(default_num_frames=8, **KW, init_seed=0)
    sd = ours.state_dict()
    fea272, cond, x3 = build_inputs(T, h)
    u = MT.DynamicNfUnet3D(default_num_frames=T, **KW)
    u.update_num_frames(T)
    u.load_state_dict(sd, strict=True)
    u.eval()
    out, qs, xs, dt = run_reference(u, T, h, S, fea272[:, :256], fea272[:, 256:], cond, x3, ddim_noises(T, h, S), keep)
    print(f"C1: guided reference DDIM T={T} h={h} S={S}: {dt:.1f} s; quantiles {qs[:4].tolist()} ... {qs[-3:].tolist()}; "
          f"max|out| = {float(out.abs().max()):.4f}")
    save("ddim_guided_C1.npz", T=T, h=h, S=S, cond_scale=np.float64(COND_SCALE), out=out[0].numpy(), quantiles=qs.numpy(),
         ddim_noise_seed=1234, weights_checksum=checksum(sd.values()), inputs_checksum=checksum([fea272, cond, x3]),
         ref_seconds=dt, keep=np.asarray(sorted(xs)), **{f"x_before_step_{s}": xs[s].numpy() for s in xs})


if __name__ == "__main__":
    cases = {"tiny": gen_tiny, "C1": gen_c1}
    for name in sys.argv[1:] or list(cases):
        cases[name]()
