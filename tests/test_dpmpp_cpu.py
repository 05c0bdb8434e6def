"""DPM-Solver++(2M) sampling without a GPU.  The solver is not in the reference, so nothing here is pinned to a golden: its values are the
definition written in include/dawn_hip.h.  The C-ABI entries exist and are bound; the host's step scalars have the structure the
definition gives them; the solver converges at second order on a problem whose exact solution is known; the Python orchestration on the
torch reference op set equals a plain restatement of the definition on the tiny UNet, in every clip mode, guided or not; and a gloo
world-2 T-shard run equals the unsharded one."""
import math
import os
import re
import socket
import sys
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT, load_golden
from oracle.ops_ref import RefOps
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd import sampler as SM
from dawn_pytorch_amd.sampler import cosine_schedule_buffers

T = torch.from_numpy
DPMPP = {"dawn_dpmpp_update", "dawn_dpmpp_step_fixed", "dawn_sampler_run_dpmpp"}
TINY_KW = dict(dim=16, cond_dim=32, cond_aud=24, cond_pose=6, cond_eye=2, num_frames=12, channels=19,
               out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2), use_hubert_audio_cond=True, learn_null_cond=False,
               use_final_activation=False, use_deconv=True, padding_mode="zeros", win_width=3)
TOL_X = 1e-4          # the gate of tests/test_ancestral_cpu.py / test_clip_cpu.py for an orchestration against its restatement
S_TINY = 6
MODES = {"dynamic": ("dynamic", 0.9), "static": ("static",), "none": ("none",)}


class DpmppRefOps(RefOps):
    """The reference op set plus the fused guidance + x0 step and the two DPM-Solver++(2M) step tails in plain torch.  The tails also
    hold the hosts to their contract: the history is handed over exactly when the step's c != 0, and it is updated in place."""

    def with_comm(self, comm):
        return DpmppRefOps(comm)

    def cfg_x0(self, e_null, e_cond, scale, x, recip, recipm1):
        eps = self.cfg_combine(e_null, e_cond, scale)
        x0, hist = self.ddim_x0(x, eps, recip, recipm1)
        return eps, x0, hist

    def ddim_step_fixed(self, x, eps, noise, recip, recipm1, sqrt_alpha_next, c, sigma, clamp=True):     # (the default solver's runs)
        x0 = recip * x - recipm1 * eps
        out = (x0.clamp(-1., 1.) if clamp else x0) * sqrt_alpha_next + c * eps
        return out if noise is None else out + sigma * noise

    @staticmethod
    def _tail(x, v, v_prev, a, b, c, v_out):
        assert (v_prev is None) == (c == 0.0), "the history is passed exactly when c != 0"
        assert v_prev is None or v_prev is v_out, "one history tensor, updated in place"
        out = a * x + b * v
        if v_prev is not None:
            out = out + c * v_prev
        if v_out is None:
            v_out = torch.full_like(v, float("nan"))
        v_out.copy_(v)
        return out, v_out

    def dpmpp_update(self, x0, s, x, v_prev, a, b, c, v_out=None, out=None):
        sv = s[0]
        return self._tail(x, torch.minimum(torch.maximum(x0, -sv), sv) / sv, v_prev, a, b, c, v_out)

    def dpmpp_step_fixed(self, x, eps, v_prev, recip, recipm1, a, b, c, clamp=True, v_out=None, out=None):
        x0 = recip * x - recipm1 * eps
        return self._tail(x, x0.clamp(-1., 1.) if clamp else x0, v_prev, a, b, c, v_out)


def _decls():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dawn_hip.h")).read(), flags=re.S)


# ------------------------------------------------------------------------------------------------------------ 1. symbols and struct
def test_dpmpp_symbols_declared_exported_and_bound():
    src = _decls()
    declared = set(re.findall(r"\b(dawn_[a-z0-9_]+)\s*\(", src))
    assert DPMPP <= declared
    assert DPMPP <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in DPMPP:
        assert hasattr(L, n), n
    assert L.dawn_abi_version() == 8                       # additive: nothing that existed changed layout or meaning
    from dawn_pytorch_amd.ctx import CtxEvaluator, DpmppStep
    body = re.search(r"typedef struct dawn_dpmpp_step \{(.*?)\} dawn_dpmpp_step;", src, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [f for f, _ in DpmppStep._fields_] == ["t", "recip", "recipm1", "a", "b", "c"]
    assert hasattr(CtxEvaluator, "sample_dpmpp")
    from dawn_pytorch_amd.ops import HipOps
    assert hasattr(HipOps, "dpmpp_update") and hasattr(HipOps, "dpmpp_step_fixed")
    assert "DAWN_OPT_DPMPP" not in src and not re.search(r"#define\s+DAWN_DPMPP", src)


# ------------------------------------------------------------------------------------------------------------ 2. scalars
@pytest.mark.parametrize("S", [2, 3, 20, 50, 999])
def test_step_scalars(S):
    bufs = cosine_schedule_buffers(1000)
    steps = SM.dpmpp_step_scalars(bufs, S)
    first = SM.dpmpp_step_scalars(bufs, S, order=1)
    pairs = SM.ddim_time_pairs(S, 1000)
    assert [(st["t"], st["t_next"]) for st in steps] == pairs == [(st["t"], st["t_next"]) for st in first]
    ddim = SM.ddim_step_scalars(bufs, S, 1.0)
    assert [(st["recip"], st["recipm1"]) for st in steps] == [(st["recip"], st["recipm1"]) for st in ddim]
    assert steps[0]["c"] == 0.0 and steps[-1]["c"] == 0.0 and all(st["c"] == 0.0 for st in first)
    assert all(st["c"] < 0.0 for st in steps[1:-1])                      # every inner step of this grid is second order
    assert steps[-1]["a"] == 0.0 and steps[-1]["b"] == 1.0 and first[-1]["a"] == 0.0 and first[-1]["b"] == 1.0
    f32 = lambda v: float(np.float32(v))                                 # noqa: E731
    for st, s1 in zip(steps, first):
        vals = [st[k] for k in ("recip", "recipm1", "a", "b", "c")]
        assert all(math.isfinite(v) and f32(v) == v for v in vals), st   # finite, and already fp32 values
        assert 0.0 <= st["a"] < 1.0 and st["b"] > 0.0
        assert st["a"] == s1["a"] and s1["b"] == st["b0"]                # the first-order solver of the same definition
        # b + c == B0 up to the fp32 roundings of b, c and B0 (half an ulp each)
        assert abs(st["b"] + st["c"] - st["b0"]) <= 2.0 ** -24 * (abs(st["b"]) + abs(st["c"]) + abs(st["b0"])), st
    with pytest.raises(ValueError):
        SM.dpmpp_step_scalars(bufs, S, order=3)


# ------------------------------------------------------------------------------------------------------------ 3. order of convergence
def _analytic_error(S, order, monkeypatch):
    """Data ~ N(0, 0.25), scalar state x_T = 1.3.  The stub denoiser returns the eps for which the formed x0 is the exact posterior
    mean at the state's noise level; the probability-flow solution is then known in closed form.  Runs the Python host loop itself
    (clip mode none) on fp64 tensors."""
    bufs = cosine_schedule_buffers(1000)
    acp = bufs["alphas_cumprod_prev"].double()
    recip, recipm1 = bufs["sqrt_recip_alphas_cumprod"], bufs["sqrt_recipm1_alphas_cumprod"]
    s2, x_T = 0.25, 1.3

    def denoiser(ops, P, cs, x, t, **k):
        ab = float(acp[t])
        Dm = x * math.sqrt(ab) * s2 / (ab * s2 + 1.0 - ab)
        return (float(recip[t]) * x - Dm) / float(recipm1[t])
    monkeypatch.setattr(SM, "unet_forward", denoiser)
    steps = SM.dpmpp_step_scalars(bufs, S, order=order)
    cs = types.SimpleNamespace(Ttotal=1, h=1, w=1, comm=None)
    x = SM.dpmpp_sample_clip(DpmppRefOps(), None, cs, torch.full((3, 1, 1, 1), x_T, dtype=torch.float64), steps, clip=("none",))
    ab0 = float(acp[steps[0]["t"]])
    exact = x_T * math.sqrt(s2) / math.sqrt(ab0 * s2 + 1.0 - ab0)
    assert x.dtype == torch.float64 and float((x - x[0]).abs().max()) == 0.0
    return abs(float(x[0]) - exact)


def test_second_order_convergence(monkeypatch):
    """Errors of this construction in fp64: S = 10: 8.6e-2 (first order) / 2.2e-2 (2M); 40: 2.4e-2 / 1.3e-3; 160: 6.4e-3 / 8.3e-5.
    (Not S = 20: the 2M error changes sign near it.)  A lost or mis-signed history term fails the first condition."""
    e1 = {S: _analytic_error(S, 1, monkeypatch) for S in (10, 40, 160)}
    e2 = {S: _analytic_error(S, 2, monkeypatch) for S in (10, 40, 160)}
    for S in (10, 40, 160):
        print(f"S={S}: first order {e1[S]:.3e}   2M {e2[S]:.3e}")
    assert e2[160] <= e2[40] / 8.0                              # second order gives about 16, first order about 4
    for S in (10, 40, 160):
        assert e2[S] <= e1[S] / 3.0, S
    assert 3.0 <= e1[40] / e1[160] <= 5.0


# ------------------------------------------------------------------------------------------------------------ 4. orchestration
def _tiny_diffusion(sd, mode, S=S_TINY, T_=12, ops=None, timesteps=1000):
    unet = D.DynamicNfUnet3D(default_num_frames=T_, **TINY_KW)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in sd.items()})
    unet.ops = ops if ops is not None else DpmppRefOps()
    kw = dict(use_dynamic_thres=True, dynamic_thres_percentile=mode[1]) if mode[0] == "dynamic" else {}
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=8, sampling_timesteps=S,
                                        timesteps=timesteps, loss_type='l2', null_cond_prob=0.1, ddim_sampling_eta=1.0, **kw)
    diff.update_num_frames(T_)
    unet.update_num_frames(T_)
    return unet, diff


def _sample(diff, mode, d, scale, **kw):
    kw = dict(cond=T(d["cond"]), cond_scale=scale, x_init=T(d["x_init"]), **kw)
    if mode[0] == "none":                                  # as `sample` forms the arguments (MT:1151-1153)
        return diff.ddim_sample(torch.cat([T(d["fea"]), T(d["bbox"])], dim=1), (1, 3, 12, 8, 8), clip_denoised=False, **kw)
    return diff.sample(T(d["fea"]), T(d["bbox"]), **kw)


def restated_trajectory(unet, bufs, d, S, scale, mode, device="cpu"):
    """The definition of include/dawn_hip.h, written out: a loop over unet.forward_with_cond_scale with fp64 coefficients (not
    rounded to fp32), torch.quantile for the dynamic threshold.  -> the latent after every step and the clipped x0 of every step."""
    acp = bufs["alphas_cumprod_prev"].double()
    recip, recipm1 = bufs["sqrt_recip_alphas_cumprod"], bufs["sqrt_recipm1_alphas_cumprod"]
    fea = torch.cat([T(d["fea"]), T(d["bbox"])], dim=1).to(device)
    cond, x = T(d["cond"]).to(device), T(d["x_init"]).to(device)
    xs, vs, v_prev, h_prev = [], [], None, None
    pairs = SM.ddim_time_pairs(S, 1000)
    for i, (t, tn) in enumerate(pairs):
        inp = torch.cat([x, fea[:, :, None].expand(-1, -1, x.shape[2], -1, -1)], dim=1)
        eps = unet.forward_with_cond_scale(inp, torch.tensor([t], device=device), cond=cond, cond_scale=scale)
        x0 = recip[t] * x - recipm1[t] * eps
        if mode[0] == "dynamic":
            s = torch.quantile(x0.abs().flatten(), mode[1]).clamp(min=1.0)
            v = x0.clamp(-s, s) / s
        else:
            v = x0.clamp(-1., 1.) if mode[0] == "static" else x0
        al, sg = math.sqrt(float(acp[t])), math.sqrt(1.0 - float(acp[t]))
        aln, sgn = math.sqrt(float(acp[tn])), math.sqrt(1.0 - float(acp[tn]))
        rho = (sgn * al) / (aln * sg)
        A, B0 = sgn / sg, aln * (1.0 - rho)
        h = -math.log(rho) if sgn > 0 else None
        nxt = A * x.double() + B0 * v.double()
        if not (i == 0 or i == S - 1 or h is None):
            r = h_prev / h
            nxt = A * x.double() + B0 * (1.0 + 1.0 / (2.0 * r)) * v.double() - B0 / (2.0 * r) * v_prev.double()
        x, v_prev, h_prev = nxt.float(), v, h
        xs.append(x)
        vs.append(v)
    return xs, vs


@pytest.fixture(scope="module")
def restated(tiny):
    """One restated trajectory per (clip mode, guidance scale), shared by the checks below and left unchanged."""
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    bufs = cosine_schedule_buffers(1000)
    cache = {}

    def get(mode_name, scale):
        key = (mode_name, scale)
        if key not in cache:
            unet, _ = _tiny_diffusion(sd, MODES[mode_name], ops=RefOps())
            with torch.no_grad():
                cache[key] = restated_trajectory(unet, bufs, d, S_TINY, scale, MODES[mode_name])
        return cache[key]
    return get


@pytest.mark.parametrize("scale", [1.0, 2.5], ids=["unguided", "guided"])
@pytest.mark.parametrize("mode_name", sorted(MODES))
def test_orchestration_equals_the_restated_definition(tiny, restated, monkeypatch, mode_name, scale):
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    mode = MODES[mode_name]
    xs, vs = restated(mode_name, scale)
    _, diff = _tiny_diffusion(sd, mode)
    assert diff.solver == "ddim" and "solver" not in diff.state_dict() and len(diff.state_dict()) - len(diff.denoise_fn.state_dict()) == 12
    times = []
    real, real_g = SM.unet_forward, SM.unet_forward_guided
    monkeypatch.setattr(SM, "unet_forward", lambda ops, P, cs, x, t, **k: (times.append(t), real(ops, P, cs, x, t, **k))[1])
    monkeypatch.setattr(SM, "unet_forward_guided",
                        lambda ops, P, cs, csn, x, t, **k: (times.append(t), real_g(ops, P, cs, csn, x, t, **k))[1])
    noises = [n for n in T(d["noises"])][:1] * S_TINY
    before = _sample(diff, mode, d, scale, noises=noises)               # the default solver, before the attribute was ever set
    ddim_times, times[:] = list(times), []
    diff.solver = "dpmpp2m"
    out = _sample(diff, mode, d, scale, trace=True)
    assert diff.last_route == "python"
    assert times == ddim_times == [t for t, _ in SM.ddim_time_pairs(S_TINY, 1000)]
    tr = diff.last_trace[0]
    assert len(tr) == S_TINY and all(set(e) >= {"eps", "s", "x", "x0c"} for e in tr)
    for i, e in enumerate(tr):
        ex = float((e["x"] - xs[i][0]).abs().max())
        ev = float((e["x0c"] - vs[i][0]).abs().max())
        print(f"{mode_name} scale={scale} step {i}: max|x - restated| = {ex:.3e}   max|x0c - restated| = {ev:.3e}")
        assert ex < TOL_X and ev < TOL_X, (i, ex, ev)
    assert float((out - xs[-1]).abs().max()) < TOL_X and torch.equal(out[0], tr[-1]["x"])
    assert torch.equal(tr[-1]["x"], tr[-1]["x0c"])                      # the last step returns the clipped x0 itself
    if mode_name == "static":
        assert float(out.abs().max()) <= 1.0 and all(torch.equal(e["s"], torch.ones(2)) for e in tr)
    if mode_name == "none":
        assert all(e["s"] is None for e in tr)
    assert not torch.allclose(out, before, atol=1e-3)                    # another solver: another sample
    again = _sample(diff, mode, d, scale)                                # deterministic: no noise is read
    assert torch.equal(again, out)
    diff.solver = "ddim"
    assert torch.equal(_sample(diff, mode, d, scale, noises=noises), before)


def test_solver_attribute_is_validated(tiny):
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    for S in (1000, 1200, None):
        _, diff = _tiny_diffusion(sd, MODES["dynamic"], S=S)
        diff.solver = "dpmpp2m"
        with pytest.raises(ValueError, match="sampling_timesteps < timesteps"):
            diff.sample(T(d["fea"]), T(d["bbox"]), cond=T(d["cond"]), x_init=T(d["x_init"]))
    _, diff = _tiny_diffusion(sd, MODES["dynamic"])
    for bad in ("dpmpp", "DDIM", None, 2):
        diff.solver = bad
        with pytest.raises(ValueError, match="unknown solver"):
            diff.sample(T(d["fea"]), T(d["bbox"]), cond=T(d["cond"]), x_init=T(d["x_init"]))
        with pytest.raises(ValueError, match="unknown solver"):
            diff.ddim_sample(torch.cat([T(d["fea"]), T(d["bbox"])], dim=1), (1, 3, 12, 8, 8), cond=T(d["cond"]), x_init=T(d["x_init"]))
    import inspect
    assert "solver" not in inspect.signature(D.GaussianDiffusion.__init__).parameters
    with pytest.raises(ValueError, match="first step has no history"):
        SM.dpmpp_sample_clip(DpmppRefOps(), None, None, torch.zeros(3, 1, 2, 2), [dict(t=5, recip=1., recipm1=0., a=0., b=1., c=-.5)])
    with pytest.raises(ValueError, match="unknown sampler step kind"):
        SM.ddim_sample_clip(DpmppRefOps(), None, None, torch.zeros(3, 1, 2, 2), [], None, kind="dpmpp3m")


# ------------------------------------------------------------------------------------------------------------ 5. gloo T-shard
TT, TS = 24, 10


def _shard_build(T_):
    sys.path.insert(0, ROOT)
    d = np.load(os.path.join(ROOT, "tests", "golden", "tiny_unet.npz"))
    sd = {k[len("sd:"):]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd:")}
    _, diff = _tiny_diffusion(sd, MODES["dynamic"], TS, T_)
    diff.solver = "dpmpp2m"
    return diff


def _shard_inputs():
    g = torch.Generator().manual_seed(9)
    return (torch.randn(1, 12, 8, 8, generator=g), torch.randn(1, 4, 8, 8, generator=g), torch.randn(1, TT, 32, generator=g),
            torch.randn(1, 3, TT, 8, 8, generator=g))


def _shard_worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from dawn_pytorch_amd.tshard import TShardComm
    F = TT // world
    diff = _shard_build(F)
    fea, bbox, cond, x_init = _shard_inputs()
    comm = TShardComm(dist, rank, world, TT, rank * F, F)
    sl = slice(rank * F, (rank + 1) * F)
    out = diff.sample(fea, bbox, cond=cond[:, sl].contiguous(), x_init=x_init[:, :, sl].contiguous(), comm=comm, trace=True)
    qs = torch.stack([tr["s"][1] for tr in diff.last_trace[0]])
    torch.save({"out": out, "qs": qs, "stats": comm.stats()}, f"{out_path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


def test_tshard_world2_equals_unsharded(tmp_path):
    """S = 10 DPM-Solver++(2M) steps on a 24-frame clip split 12 + 12 over gloo: the whole-clip quantiles make it equal the unsharded
    run; the history is frame-local.  Gates: those of test_ancestral_cpu.py::test_tshard_world2_equals_unsharded."""
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out_path = str(tmp_path / "shard")
    mp.spawn(_shard_worker, args=(world, port, out_path), nprocs=world, join=True)
    parts = [torch.load(f"{out_path}.{r}") for r in range(world)]
    diff = _shard_build(TT)
    fea, bbox, cond, x_init = _shard_inputs()
    full = diff.sample(fea, bbox, cond=cond, x_init=x_init, trace=True)
    qs = torch.stack([tr["s"][1] for tr in diff.last_trace[0]])
    assert qs.shape == (TS,)
    torch.testing.assert_close(parts[0]["qs"], parts[1]["qs"], atol=0, rtol=0)
    torch.testing.assert_close(parts[0]["qs"], qs, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(torch.cat([p["out"] for p in parts], dim=2), full, atol=2e-5, rtol=1e-5)
    assert all(p["stats"]["halo_exchanges"] == 6 * TS for p in parts)
