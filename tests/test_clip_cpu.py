"""Every x0 clipping mode of the reference sampler, without a GPU: dynamic thresholding at any percentile, the static clamp (the
reference constructor's default) and no clipping.  The Python orchestration on the torch reference op set reproduces the
reference's own trajectories (tools/gen_goldens_clip.py -> clip_*.npz); the fixtures can tell the modes apart (conditions
re-asserted from the stored numbers); the constructor selects the mode as the reference's arguments do; the host's quantile rank
equals torch.quantile's; the C-ABI entries exist and are bound."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from ancestral_cases import ANCESTRAL_STEPS, KEEP, ancestral_noises
from clip_cases import DDIM_KEEP, KIND_CODES, MODE_MARGIN, TINY_CASES, ddim_noises_tiny, ddim_steps
from conftest import GOLDEN, ROOT, load_golden
from oracle.ops_ref import RefOps
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd import sampler as SM

T = torch.from_numpy
CLIP = {"dawn_ddim_step_fixed", "dawn_ancestral_step_fixed", "dawn_sampler_run_clip", "dawn_sampler_run_ancestral_clip"}
TINY_KW = dict(dim=16, cond_dim=32, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12, channels=19,
               out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2), use_hubert_audio_cond=True, learn_null_cond=False,
               use_final_activation=False, use_deconv=True, padding_mode="zeros", win_width=3)
TOL_X = 1e-4          # the gates of tests/test_ancestral_cpu.py for this very comparison
TOL_Q = 2e-5


class ClipRefOps(RefOps):
    """The reference op set plus the fused steps, in plain torch from the reference lines (MT:1074-1076 x0, MT:1095/1107 and
    MT:1184/1196 the clamp with s = 1, MT:1203-1205 and MT:1080-1085/1121 the updates)."""

    def with_comm(self, comm):
        return ClipRefOps(comm)

    def cfg_x0(self, e_null, e_cond, scale, x, recip, recipm1):
        eps = self.cfg_combine(e_null, e_cond, scale)
        x0, hist = self.ddim_x0(x, eps, recip, recipm1)
        return eps, x0, hist

    def ancestral_update(self, x0, x_t, s, noise, c1, c2, std):
        return self.ddim_update(x0, x_t, s, noise, c1, c2, std)

    def ddim_step_fixed(self, x, eps, noise, recip, recipm1, sqrt_alpha_next, c, sigma, clamp=True):
        x0 = recip * x - recipm1 * eps
        if clamp:
            x0 = x0.clamp(-1., 1.) / 1.
        out = x0 * sqrt_alpha_next + c * eps
        return out if noise is None else out + sigma * noise

    def ancestral_step_fixed(self, x_t, eps, noise, recip, recipm1, c1, c2, std, clamp=True):
        assert clamp, "p_sample always clips (MT:1113)"
        x0 = (recip * x_t - recipm1 * eps).clamp(-1., 1.) / 1.
        out = c1 * x0 + c2 * x_t
        return out if noise is None else out + std * noise


def _decls():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dawn_hip.h")).read(), flags=re.S)


def test_clip_symbols_declared_exported_and_bound():
    src = _decls()
    declared = set(re.findall(r"\b(dawn_[a-z0-9_]+)\s*\(", src))
    assert CLIP <= declared
    assert CLIP <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in CLIP:
        assert hasattr(L, n), n
    assert L.dawn_abi_version() == 8                       # additive: nothing that existed changed layout or meaning
    from dawn_pytorch_amd.ctx import CLIP_KINDS, ClipMode
    body = re.search(r"typedef struct dawn_clip_mode \{(.*?)\} dawn_clip_mode;", src, flags=re.S).group(1)
    assert re.findall(r"\b(int|double)\s+([a-z]+)\s*;", body) == [("int", "kind"), ("double", "q")]
    assert [f for f, _ in ClipMode._fields_] == ["kind", "q"]
    assert ctypes.sizeof(ClipMode) == 16 and ClipMode.kind.offset == 0 and ClipMode.q.offset == 8
    enum = re.search(r"enum \{ (DAWN_CLIP_[^}]*)\}", src).group(1)
    assert {k.strip().split(" = ")[0][len("DAWN_CLIP_"):].lower(): int(k.split("=")[1]) for k in enum.split(",")} == CLIP_KINDS
    assert CLIP_KINDS == KIND_CODES


def _tiny_diffusion(sd, mode, sampler="ddim", S=3):
    unet = D.DynamicNfUnet3D(default_num_frames=12, **TINY_KW)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in sd.items()})
    unet.ops = ClipRefOps()
    kw = dict(use_dynamic_thres=True, dynamic_thres_percentile=mode[1]) if mode[0] == "dynamic" else {}   # else: the class default
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=12, denoise_fn=unet, num_frames=12, image_size=8,
                                        sampling_timesteps=1000 if sampler == "ancestral" else S, timesteps=1000, loss_type='l2',
                                        null_cond_prob=0.1, ddim_sampling_eta=1.0, **kw)
    diff.update_num_frames(12)
    unet.update_num_frames(12)
    return diff


def _run(diff, mode, d, cond_scale, noises):
    kw = dict(cond=T(d["cond"]), cond_scale=cond_scale, x_init=T(d["x_init"]), noises=noises, trace=True)
    if mode[0] == "none":                                  # as `sample` forms the arguments (MT:1151-1153)
        fea272 = torch.cat([T(d["fea"]), T(d["bbox"])], dim=1)
        return diff.ddim_sample(fea272, (1, 3, 12, 8, 8), clip_denoised=False, **kw)
    return diff.sample(T(d["fea"]), T(d["bbox"]), **kw)


def _check_trace(tr, mode, qref):
    if mode[0] == "dynamic":
        qs = torch.stack([e["s"][1] for e in tr])
        assert float(((qs - qref).abs() / qref.abs()).max()) < TOL_Q
    elif mode[0] == "static":
        assert all(torch.equal(e["s"], torch.ones(2)) for e in tr)
    else:
        assert all(e["s"] is None for e in tr)


@pytest.mark.parametrize("name", [n for n in TINY_CASES if TINY_CASES[n][0] == "ddim"])
def test_ddim_orchestration_matches_reference(tiny, name):
    """Final sample, intermediate latents and per-step quantiles of the reference's ddim_sample in this mode, S = 3 and S = 50."""
    _, sd = tiny
    _, mode, cond_scale = TINY_CASES[name]
    g, d = load_golden(f"clip_{name}.npz"), load_golden("ddim_tiny.npz")
    assert tuple(g["S"].tolist()) == ddim_steps(name) and int(g["kind"]) == KIND_CODES[mode[0]] and float(g["cond_scale"]) == cond_scale
    for S in ddim_steps(name):
        diff = _tiny_diffusion(sd, mode, "ddim", S)
        assert diff.clip == SM.clip_mode(mode if mode[0] != "none" else ("static",))
        noises = ddim_noises_tiny(tuple(d["x_init"].shape), S, d["noises"], int(g["ddim_noise_seed"]))
        out = _run(diff, mode, d, cond_scale, noises)
        tr = diff.last_trace[0]
        assert len(tr) == S and diff.last_route == "python"
        _check_trace(tr, mode, T(g[f"quantiles_S{S}"]).float())
        for s in DDIM_KEEP[S]:
            assert float((tr[s - 1]["x"] - T(g[f"x_before_step_{s}_S{S}"])[0]).abs().max()) < TOL_X, (S, s)
        err = float((out - T(g[f"out_S{S}"])).abs().max())
        print(f"{name} S={S}: max|out - reference| = {err:.3e}")
        assert err < TOL_X, (S, err)


@pytest.mark.parametrize("name", [n for n in TINY_CASES if TINY_CASES[n][0] == "ancestral"])
def test_ancestral_orchestration_matches_reference(tiny, name):
    _, sd = tiny
    _, mode, cond_scale = TINY_CASES[name]
    g, d = load_golden(f"clip_{name}.npz"), load_golden("ddim_tiny.npz")
    assert int(g["kind"]) == KIND_CODES[mode[0]] and float(g["cond_scale"]) == cond_scale and int(g["timesteps"]) == ANCESTRAL_STEPS
    diff = _tiny_diffusion(sd, mode, "ancestral")
    noises = ancestral_noises(tuple(d["x_init"].shape), ANCESTRAL_STEPS, int(g["ancestral_noise_seed"]))[:-1]
    out = _run(diff, mode, d, cond_scale, noises)
    tr = diff.last_trace[0]
    assert len(tr) == ANCESTRAL_STEPS
    _check_trace(tr, mode, T(g["quantiles"]).float())
    for s in KEEP:
        assert float((tr[s - 1]["x"] - T(g[f"x_before_step_{s}"])[0]).abs().max()) < TOL_X, s
    err = float((out - T(g["out"])).abs().max())
    print(f"{name}: max|out - reference| = {err:.3e}")
    assert err < TOL_X, err


def test_fixtures_can_tell_the_modes_apart():
    """The conditions tools/gen_goldens_clip.py asserted on the reference's numbers, re-asserted from what it stored: no test
    above can pass by running another mode."""
    files = [f"clip_{n}.npz" for n in TINY_CASES] + ["clip_C1_static.npz"]
    for f in files:
        path = os.path.join(GOLDEN, f)
        assert os.path.getsize(path) < 1 << 20
        with np.load(path, allow_pickle=False) as z:
            g = {k: z[k] for k in z.files}
        assert all(v.dtype != object for v in g.values()) and float(g["x_scale"]) == 1.0
        kind = {v: k for k, v in KIND_CODES.items()}[int(g["kind"])]
        sfx = [f"_S{S}" for S in g["S"].tolist()] if "S" in g and g["S"].ndim else [""]
        for s in sfx:
            out, ref90 = g["out" + s], g["ref90_out" + s]
            assert np.isfinite(out).all() and g["x0_absmax" + s].max() > 1.0
            if kind == "static":
                assert np.abs(out).max() <= 1.0 and np.abs(out - ref90.reshape(out.shape)).max() > MODE_MARGIN
            if kind == "none":
                assert np.abs(out - g["static_out" + s]).max() > MODE_MARGIN
            if kind == "dynamic":
                q, q90 = g["quantiles" + s], g["ref90_quantiles" + s]
                assert q.shape == q90.shape and q.max() > 1.0 and not np.array_equal(q, q90)
    # the dynamic(0.9) results the generator compared against are the ones the existing fixtures hold
    assert np.array_equal(load_golden("clip_ddim_static.npz")["ref90_out_S3"], load_golden("ddim_tiny.npz")["out"])
    assert np.array_equal(load_golden("clip_ancestral_static.npz")["ref90_out"], load_golden("ancestral_tiny.npz")["out"])


def test_constructor_selects_the_mode(tiny):
    _, sd = tiny
    unet = D.DynamicNfUnet3D(default_num_frames=12, **TINY_KW)
    diff = D.GaussianDiffusion(unet, image_size=8, num_frames=12)             # nothing else spelled out: the reference's defaults
    assert diff.use_dynamic_thres is False and diff.clip == ("static", None)
    assert D.GaussianDiffusion(unet, image_size=8, num_frames=12, use_dynamic_thres=True).clip == ("dynamic", 0.9) == SM.CLIP_DEFAULT
    assert D.GaussianDiffusion(unet, image_size=8, num_frames=12, use_dynamic_thres=True, dynamic_thres_percentile=0.5).clip == ("dynamic", 0.5)
    assert D.GaussianDiffusion(unet, image_size=8, num_frames=12, dynamic_thres_percentile=1.5).clip == ("static", None)   # unused, as in the reference
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError):
            D.GaussianDiffusion(unet, image_size=8, num_frames=12, use_dynamic_thres=True, dynamic_thres_percentile=bad)
    # the ancestral loop cannot be asked for an unclipped x0: no argument for it, and the loop itself refuses the mode
    assert "clip_denoised" not in inspect.signature(diff.p_sample_loop).parameters
    assert "clip_denoised" in inspect.signature(diff.ddim_sample).parameters
    with pytest.raises(ValueError):
        SM.clip_mode(("none",), ancestral=True)
    with pytest.raises(ValueError):
        SM.ancestral_sample_clip(ClipRefOps(), None, None, torch.zeros(3, 1, 2, 2), [], lambda i: None, clip=("none",))
    from dawn_pytorch_amd.ctx import _clip_struct
    with pytest.raises(ValueError):
        _clip_struct(("none",), True)
    for bad in (("dynamic",), ("static", 0.5), ("median",), ()):
        with pytest.raises(ValueError):
            SM.clip_mode(bad)
    assert SM.clip_mode("static") == SM.clip_mode(("static", None)) == ("static", None)


def test_reference_default_construction_samples(tiny):
    """GaussianDiffusion with the class defaults (static clipping, sampling_timesteps=250 -> DDIM) runs; every value of the last
    step's output is a clamped x0 (alpha_next = 1)."""
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = D.DynamicNfUnet3D(default_num_frames=12, **TINY_KW)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in sd.items()})
    unet.ops = ClipRefOps()
    unet.update_num_frames(12)
    diff = D.GaussianDiffusion(unet, image_size=8, num_frames=12, sampling_timesteps=4)
    out = diff.sample(T(d["fea"]), T(d["bbox"]), cond=T(d["cond"]), x_init=T(d["x_init"]))
    assert out.shape == (1, 3, 12, 8, 8) and torch.isfinite(out).all() and float(out.abs().max()) <= 1.0


@pytest.mark.parametrize("q", [0.0, 0.5, 0.9, 0.99, 1.0])
def test_quantile_rank_and_lerp_equal_torch_quantile_bit_for_bit(q):
    from dawn_pytorch_amd.ops import HipOps
    g = torch.Generator().manual_seed(17)
    vecs = [torch.randn(n, generator=g).abs() for n in (1, 2, 7, 2304, 49152, 100003)]
    vecs += [torch.randint(0, 5, (n,), generator=g).float() for n in (9, 2304)]                 # ties, at the extremes too
    vecs += [torch.cat([torch.full((50,), 3.25), torch.randn(500, generator=g).abs().clamp(max=3.0), torch.zeros(40)])]
    for v in vecs:
        n = v.numel()
        lo, w = HipOps.quantile_rank(n, q)
        sv = torch.sort(v).values
        assert 0 <= lo <= n - 1 and 0.0 <= w < 1.0
        if q == 0.0:
            assert (lo, w) == (0, 0.0)
        if q == 1.0:
            assert (lo, w) == (n - 1, 0.0)
        got = torch.lerp(sv[lo], sv[min(lo + 1, n - 1)], torch.tensor(w))
        assert torch.equal(got, torch.quantile(v, q)), (n, q, float(got), float(torch.quantile(v, q)))
