"""Ancestral (DDPM) sampling without a GPU: the C-ABI entries exist and are bound, the host's step scalars equal the reference's
bit for bit, the dispatch runs `timesteps` evaluations whatever sampling_timesteps >= timesteps is, the Python orchestration
reproduces the reference's 1000-step trajectories on the torch reference op set, and a gloo world-2 T-shard run equals the
unsharded one."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ancestral_cases import ANCESTRAL_STEPS, KEEP, ancestral_noises
from conftest import GOLDEN, ROOT, load_golden
from oracle.ops_ref import RefOps
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd import sampler as SM
from dawn_pytorch_amd.sampler import cosine_schedule_buffers

T = torch.from_numpy
ANCESTRAL = {"dawn_ancestral_update", "dawn_sampler_run_ancestral"}
FIXTURES = {"ancestral_tiny.npz": (12, 8, 1.0), "ancestral_guided_tiny.npz": (12, 8, 2.5), "ancestral_C1.npz": (16, 32, 1.0)}
TINY_KW = dict(dim=16, cond_dim=32, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12, channels=19,
               out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2), use_hubert_audio_cond=True, learn_null_cond=False,
               use_final_activation=False, use_deconv=True, padding_mode="zeros", win_width=3)
TOL_X = 1e-4
TOL_Q = 2e-5


class AncestralRefOps(RefOps):
    """The reference op set plus the fused guidance + x0 step and the ancestral step, composed from reference ops: the ancestral
    step is the DDIM update with eps := x_t (the form dawn_ancestral_update shares with dawn_ddim_update)."""

    def with_comm(self, comm):
        return AncestralRefOps(comm)

    def cfg_x0(self, e_null, e_cond, scale, x, recip, recipm1):
        eps = self.cfg_combine(e_null, e_cond, scale)
        x0, hist = self.ddim_x0(x, eps, recip, recipm1)
        return eps, x0, hist

    def ancestral_update(self, x0, x_t, s, noise, c1, c2, std):
        return self.ddim_update(x0, x_t, s, noise, c1, c2, std)


def _decls():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dawn_hip.h")).read(), flags=re.S)


def test_ancestral_symbols_declared_exported_and_bound():
    src = _decls()
    declared = set(re.findall(r"\b(dawn_[a-z0-9_]+)\s*\(", src))
    assert ANCESTRAL <= declared
    assert ANCESTRAL <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in ANCESTRAL:
        assert hasattr(L, n), n
    assert L.dawn_abi_version() == 8
    # the step struct and its ctypes mirror agree field by field
    from dawn_pytorch_amd.ctx import AncestralStep, CtxEvaluator
    body = re.search(r"typedef struct dawn_ancestral_step \{(.*?)\} dawn_ancestral_step;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [f for f, _ in AncestralStep._fields_] == ["t", "recip", "recipm1", "c1", "c2", "std"]
    assert hasattr(CtxEvaluator, "sample_ancestral")


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_step_scalars_equal_the_references_bit_for_bit(name):
    d = load_golden(name)
    steps = SM.ancestral_step_scalars(cosine_schedule_buffers(1000), 1000)
    assert [st["t"] for st in steps] == list(range(999, -1, -1))
    assert [st["noise"] for st in steps] == [True] * 999 + [False]
    got = np.array([[st["c1"], st["c2"], st["std"]] for st in steps], dtype=np.float32)
    assert d["coefs"].dtype == np.float32 and d["coefs"].shape == (1000, 3)
    assert np.array_equal(got.view(np.uint32), d["coefs"].view(np.uint32)), np.argwhere(got != d["coefs"])[:5]
    # the points that decide parity at t = 0: the clamped x0 is the output; the std is not zero, only masked
    assert steps[-1]["c1"] == 1.0 and steps[-1]["c2"] == 0.0 and 0.0 < steps[-1]["std"] < 1e-9


def test_fixtures_are_read_only_well_formed_data():
    for name, (Tt, h, scale) in FIXTURES.items():
        path = os.path.join(GOLDEN, name)
        assert os.path.getsize(path) < 1 << 20
        with np.load(path, allow_pickle=False) as z:
            d = {k: z[k] for k in z.files}
        assert int(d["timesteps"]) == ANCESTRAL_STEPS and float(d["cond_scale"]) == scale
        assert d["quantiles"].shape == (ANCESTRAL_STEPS,) and np.isfinite(d["quantiles"]).all() and (d["quantiles"] > 0).all()
        out = d["out"].reshape(-1, 3, Tt, h, h)
        assert np.isfinite(out).all() and np.abs(out).max() <= 1.0 + 1e-6          # t = 0 returns the clamped x0
        assert tuple(d["keep"].tolist()) == KEEP
        for s in KEEP:
            assert d[f"x_before_step_{s}"].reshape(-1, 3, Tt, h, h).shape[0] == 1
        for v in d.values():
            assert v.dtype != object


def _tiny_diffusion(sd, ops, sampling_timesteps=1000, timesteps=1000, T_=12):
    unet = D.DynamicNfUnet3D(default_num_frames=T_, **TINY_KW)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in sd.items()})
    unet.ops = ops
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=8,
                                        sampling_timesteps=sampling_timesteps, timesteps=timesteps, loss_type='l2',
                                        use_dynamic_thres=True, null_cond_prob=0.1, ddim_sampling_eta=1.0)
    diff.update_num_frames(T_)
    unet.update_num_frames(T_)
    return unet, diff


@pytest.mark.parametrize("sampling_timesteps", [1000, 1200, None])
def test_dispatch_runs_timesteps_evaluations(tiny, monkeypatch, sampling_timesteps):
    """sampling_timesteps >= timesteps (or None) takes the ancestral loop: exactly `timesteps` evaluations at t = 999 ... 0 (the
    evaluation itself is stubbed here; the trajectory tests below run it)."""
    g, sd = tiny
    _, diff = _tiny_diffusion(sd, AncestralRefOps(), sampling_timesteps)
    assert not diff.is_ddim_sampling
    times = []

    def fake_forward(ops, P, cs, x, t, **k):
        times.append(t)
        return torch.zeros_like(x)
    monkeypatch.setattr(SM, "unet_forward", fake_forward)
    d = load_golden("ddim_tiny.npz")
    out = diff.sample(T(d["fea"]), T(d["bbox"]), cond=T(d["cond"]), x_init=T(d["x_init"]), trace=True)
    assert times == list(range(999, -1, -1))
    assert len(diff.last_trace[0]) == 1000 and out.shape == (1, 3, 12, 8, 8)
    assert diff.last_route == "python"


@pytest.mark.parametrize("name", ["ancestral_tiny.npz", "ancestral_guided_tiny.npz"])
def test_orchestration_matches_reference_trajectory(tiny, name):
    """The whole 1000-step loop on the reference op set against the reference's own p_sample_loop: the quantile of every step,
    the latents entering steps 1 / 500 / 900 / 999 and the output (noises: timesteps - 1 entries, as the contract allows)."""
    g, sd = tiny
    d = load_golden(name)
    _, diff = _tiny_diffusion(sd, AncestralRefOps())
    noises = ancestral_noises(tuple(d["x_init"].shape), int(d["timesteps"]), int(d["ancestral_noise_seed"]))[:-1]
    out = diff.sample(T(d["fea"]), T(d["bbox"]), cond=T(d["cond"]), cond_scale=float(d["cond_scale"]), x_init=T(d["x_init"]),
                      noises=noises, trace=True)
    tr = diff.last_trace[0]
    assert len(tr) == ANCESTRAL_STEPS
    qs = torch.stack([e["s"][1] for e in tr])
    qref = T(d["quantiles"]).float()
    assert float(((qs - qref).abs() / qref.abs()).max()) < TOL_Q
    for s in KEEP:
        assert float((tr[s - 1]["x"] - T(d[f"x_before_step_{s}"])[0]).abs().max()) < TOL_X, s
    assert float((out - T(d["out"])).abs().max()) < TOL_X


def test_flow_diffusion_boundary_with_1000_sampling_steps(monkeypatch):
    """FlowDiffusion(sampling_timesteps=1000) -- what `sampling_step: 1000` / `--sampling_step 1000` builds -- runs the whole
    pre / sample / post path on the ancestral loop (the evaluation stubbed: 1000 full-size evaluations are a GPU's work)."""
    from dawn_pytorch_amd.flow_diffusion import FlowDiffusion
    from test_boundary_cpu import FakeLFG
    fd = FlowDiffusion(generator=FakeLFG(), pose_dim=6, sampling_timesteps=1000, win_width=40, num_frames=5, img_size=16)
    fd.unet.ops = AncestralRefOps()
    fd.update_num_frames(5)                                    # as VideoGenerator does per clip (UVG:370)
    assert not fd.diffusion.is_ddim_sampling
    times = []

    def fake_forward(ops, P, cs, x, t, **k):
        times.append(t)
        return 0.1 * x
    monkeypatch.setattr(SM, "unet_forward", fake_forward)
    d = load_golden("fd_prepost.npz")                          # the boundary test's inputs: a batch of two clips
    out = fd.sample_one_video(T(d["img"]), T(d["hubert"]), T(d["pose"]), T(d["eye"]), T(d["bbox"]), 1.0,
                              init_pose=T(d["init_pose"]), init_eye=T(d["init_eye"]))
    assert times == 2 * list(range(999, -1, -1))
    assert fd.diffusion.last_route == "python"
    assert torch.isfinite(out["sample_out_vid"]).all() and out["sample_out_vid"].shape == (2, 3, 5, 64, 64)


TT, TS = 24, 50


def _shard_build(T_):
    sys.path.insert(0, ROOT)
    d = np.load(os.path.join(ROOT, "tests", "golden", "tiny_unet.npz"))
    sd = {k[len("sd:"):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd:")}
    _, diff = _tiny_diffusion(sd, AncestralRefOps(), None, TS, T_)
    diff.noise_seed = 77
    return diff


def _shard_inputs():
    g = torch.Generator().manual_seed(9)
    return torch.randn(1, 12, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, TT, 32, generator=g)


def _shard_worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from dawn_pytorch_amd.tshard import TShardComm
    F = TT // world
    diff = _shard_build(F)
    fea, bbox, cond = _shard_inputs()
    comm = TShardComm(dist, rank, world, TT, rank * F, F)
    out = diff.sample(fea, bbox, cond=cond[:, rank * F:(rank + 1) * F].contiguous(), comm=comm, trace=True)
    qs = torch.stack([tr["s"][1] for tr in diff.last_trace[0]])
    torch.save({"out": out, "qs": qs, "stats": comm.stats()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_tshard_world2_equals_unsharded(tmp_path):
    """A timesteps=50 schedule (sampling_timesteps=None: ancestral) on a 24-frame clip split 12 + 12 over gloo: the whole-clip
    quantiles and the shard-invariant Philox noise (stream i + 1 for step i) make it equal the unsharded run."""
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out_path = str(tmp_path / "shard")
    mp.spawn(_shard_worker, args=(world, port, out_path), nprocs=world, join=True)
    parts = [torch.load(f"{out_path}.{r}") for r in range(world)]
    diff = _shard_build(TT)
    fea, bbox, cond = _shard_inputs()
    full = diff.sample(fea, bbox, cond=cond, trace=True)
    qs = torch.stack([tr["s"][1] for tr in diff.last_trace[0]])
    assert qs.shape == (TS,)
    torch.testing.assert_close(parts[0]["qs"], parts[1]["qs"], atol=0, rtol=0)
    torch.testing.assert_close(parts[0]["qs"], qs, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(torch.cat([p["out"] for p in parts], dim=2), full, atol=2e-5, rtol=1e-5)
    assert all(p["stats"]["halo_exchanges"] == 6 * TS for p in parts)
