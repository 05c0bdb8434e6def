"""-m gpu: every x0 clipping mode on every sampler path -- the fused step-tail kernels of the modes without a quantile, Python eager,
HIP graph, the C evaluator (dawn_sampler_run_clip / dawn_sampler_run_ancestral_clip) and T-shard ranks of both hosts.  Pinned to the
reference's own runs (tools/gen_goldens_clip.py -> clip_*.npz); every host must agree bit for bit with the Python eager path."""
import numpy as np
import pytest
import torch

from ancestral_cases import ANCESTRAL_STEPS, KEEP, ancestral_noises
from clip_cases import C1, DDIM_KEEP, TINY_CASES, ddim_noises_tiny, ddim_steps
from conftest import load_golden
from fullsize_cases import KW, build_inputs, checksum, ddim_noises
from inproc_shard import Exchange, InProcComm, run_ranks
from test_hip_end2end import T, log, tiny_unet
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.ctx import CtxEvaluator, ShardCallbacks
from dawn_pytorch_amd.sampler import (ancestral_sample_clip, ancestral_step_scalars, ddim_sample_clip, ddim_step_scalars)
from dawn_pytorch_amd.unet_forward import unet_forward

pytestmark = pytest.mark.gpu

TOL_X = 1e-4          # the gates of tests/test_hip_ancestral.py
TOL_Q = 2e-5
ANC_KEYS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
            "posterior_log_variance_clipped")
DDIM_KEYS = ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")


def _diffusion(unet, T_, h, mode, sampler="ddim", S=3, timesteps=1000):
    kw = dict(use_dynamic_thres=True, dynamic_thres_percentile=mode[1]) if mode[0] == "dynamic" else {}
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=h,
                                        sampling_timesteps=timesteps if sampler == "ancestral" else S, timesteps=timesteps,
                                        loss_type='l2', null_cond_prob=0.1, ddim_sampling_eta=1.0, **kw).cuda()
    diff.update_num_frames(T_)
    assert diff.is_ddim_sampling == (sampler == "ddim")
    return diff


def _steps(diff):
    if diff.is_ddim_sampling:
        return ddim_step_scalars({k: getattr(diff, k) for k in DDIM_KEYS}, diff.sampling_timesteps, diff.ddim_sampling_eta,
                                 diff.num_timesteps)
    return ancestral_step_scalars({k: getattr(diff, k) for k in ANC_KEYS}, diff.num_timesteps)


def _ctx_clips(unet, fea, bbox, cond, guided):
    ev = CtxEvaluator(unet.packed())
    f272 = torch.cat((fea, bbox), 1)[0].contiguous()
    T_ = cond.shape[1]
    rcos, rsin = unet.packed().rotary_tables(T_ + 2 * unet.packed().win)
    clip = ev.prepare_clip(f272, cond[0].contiguous(), rcos, rsin)
    return ev, clip, (ev.prepare_null_clip(f272, T_, rcos, rsin) if guided else None)


def _ctx_run(ev, diff, mode, clip, null_clip, x_init, noises, cond_scale, **kw):
    steps = _steps(diff)
    noisy = [(st["t_next"] if diff.is_ddim_sampling else st["t"]) > 0 for st in steps]
    nz = None if noises is None else [noises[i][0].contiguous() if noisy[i] else None for i in range(len(steps))]
    run = ev.sample if diff.is_ddim_sampling else ev.sample_ancestral
    return run(clip, x_init[0].contiguous(), steps, noises=nz, want_thresholds=True, null_clip=null_clip, cond_scale=cond_scale,
               x0_clip=mode, **kw)


def _trace_s(tr, mode):
    """(S, 2) thresholds of a Python trace the way the C evaluator reports them (static: [1, 1] per step)."""
    if mode[0] == "none":
        return None
    return torch.stack([t["s"] for t in tr])


# ---------------------------------------------------------------------------------------------------------------- kernels
def test_fused_step_kernels_bit_identical_to_the_two_launch_sequence():
    """dawn_ddim_step_fixed / dawn_ancestral_step_fixed against the kernels they fuse.  static: ddim_x0 -> ddim_update /
    ancestral_update with s = [1, 1].  none: ddim_x0 -> ddim_update with s = 2^20 and sqrt_alpha_next * 2^20: clamp(x0, -s, s) / s is
    then x0 / 2^20 exactly (|x0| < 2^20) and the power of two cancels exactly in the product, so that launch computes x0 *
    sqrt_alpha_next + c * eps (+ sigma * noise) in the update kernel's own roundings with no clamp acting.  With and without noise,
    in place, odd n, an unaligned base pointer (the scalar path), with and without the x0 output."""
    from dawn_pytorch_amd.ops import HipOps
    ops = HipOps()
    L = _lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(5)
    one = torch.ones(2, device="cuda")
    big = torch.full((2,), 2.0 ** 20, device="cuda")
    recip, recipm1 = 1.8371, 1.5411
    for n in (3 * 16 * 32 * 32, 3 * 7 * 9 * 9 + 5, 3):
        for off in (0, 1):                                   # off = 1: a slice offset by one float -> not 16-byte aligned
            x, eps, nz = (torch.randn(n + off, generator=g).mul_(m).cuda()[off:] for m in (1.5, 1.0, 1.0))
            assert x.is_contiguous() and (x.data_ptr() % 16 != 0) == bool(off)
            for noise, (a, b, sg) in ((nz, (0.6123, 0.5871, 0.3456)), (None, (1.0, 0.0, 1e-10))):
                x0, _ = ops.ddim_x0(x, eps, recip, recipm1)
                assert float(x0.abs().max()) > 1.0 or n == 3
                want = ops.ddim_update(x0, eps, one, noise, a, b, sg)
                got, x0_got = ops.ddim_step_fixed(x, eps, noise, recip, recipm1, a, b, sg, clamp=True, want_x0=True)
                assert torch.equal(got, want) and torch.equal(x0_got, x0)
                assert torch.equal(ops.ddim_step_fixed(x, eps, noise, recip, recipm1, a, b, sg, clamp=True), want)
                want_none = ops.ddim_update(x0, eps, big, noise, a * 2.0 ** 20, b, sg)
                assert torch.equal(ops.ddim_step_fixed(x, eps, noise, recip, recipm1, a, b, sg, clamp=False), want_none)
                if n > 3:
                    assert not torch.equal(want_none, want)
                want_a = ops.ancestral_update(x0, x, one, noise, a, b, sg)
                got_a, x0_a = ops.ancestral_step_fixed(x, eps, noise, recip, recipm1, a, b, sg, want_x0=True)
                assert torch.equal(got_a, want_a) and torch.equal(x0_a, x0)
                for fn, w in ((ops.ddim_step_fixed, want), (ops.ancestral_step_fixed, want_a)):
                    inplace = x.clone() if not off else torch.cat([x.new_zeros(1), x])[1:]
                    fn(inplace, eps, noise, recip, recipm1, a, b, sg, out=inplace)
                    assert torch.equal(inplace, w)
    # rejected, not run: aliasing, and the ancestral step without the clamp
    p = lambda t: t.data_ptr()                                                               # noqa: E731
    out = torch.empty_like(x)
    for bad in ((p(x), p(eps), None, p(x0), p(eps)), (p(x), p(eps), p(nz), None, p(nz)), (p(x), p(eps), None, p(x), p(out)),
                (p(x), p(eps), None, p(out), p(out)), (p(x), p(eps), None, None, p(x) + 4)):
        xx, ee, nn, x0o, oo = bad
        rc = L.dawn_ddim_step_fixed(xx, ee, nn, recip, recipm1, 1.0, 0.0, 0.0, 1, n - 1, x0o, oo, stream)
        assert rc != 0 and b"alias" in L.dawn_last_error(), bad
    rc = L.dawn_ancestral_step_fixed(p(x), p(eps), None, recip, recipm1, 1.0, 0.0, 0.0, 0, n, None, p(out), stream)
    assert rc != 0 and b"clamp" in L.dawn_last_error()
    rc = L.dawn_ddim_step_fixed(p(x), p(eps), None, recip, recipm1, 1.0, 0.0, 0.0, 7, n, None, p(out), stream)
    assert rc != 0 and b"clamp" in L.dawn_last_error()


def test_quantile_ends_bit_exact():
    """q = 1 (rank n - 1, nothing above it: the hmin == INT_MAX branch of the finalisation) and q = 0 (rank 0, weight 0) through
    ops.quantile_threshold, on a vector with unique extremes and one with tied extremes."""
    from dawn_pytorch_amd.ops import HipOps
    ops = HipOps()
    g = torch.Generator().manual_seed(3)
    v = torch.randn(3 * 16 * 32 * 32, generator=g)
    tied = v.clone()
    tied[:37] = float(v.abs().max()) + 1.0
    tied[100:150] = 0.0
    for vec in (v, tied):
        x = vec.cuda()
        for q in (1.0, 0.0, 0.5, 0.99):
            x0, hist = ops.ddim_x0(x, torch.zeros_like(x), 1.0, 0.0)
            assert torch.equal(x0, x)
            s = ops.quantile_threshold(x0, hist, x.numel(), q).cpu()
            want = torch.quantile(vec.abs(), q)
            assert torch.equal(s[1], want), (q, float(s[1]), float(want))
            assert torch.equal(s[0], want.clamp(min=1.0))
    assert ops.quantile_rank(v.numel(), 1.0) == (v.numel() - 1, 0.0) and ops.quantile_rank(v.numel(), 0.0) == (0, 0.0)


# ---------------------------------------------------------------------------------------------------------------- tiny cases
def _check_vs_reference(name, tr, out, g, sfx, keep, mode):
    if mode[0] == "dynamic":
        qs = torch.stack([t["s"][1] for t in tr]).cpu()
        qref = torch.from_numpy(g["quantiles" + sfx]).float()
        qerr = float(((qs - qref).abs() / qref.abs()).max())
        log(f"clip_{name}{sfx}_quantiles_rel", qs, qref)
        assert qerr < TOL_Q, qerr
    for s in keep:
        want = torch.from_numpy(g[f"x_before_step_{s}{sfx}"]).reshape(tr[s - 1]["x"].shape)
        assert log(f"clip_{name}{sfx}_x_before_step_{s}", tr[s - 1]["x"].cpu(), want) < TOL_X, s
    err = log(f"clip_{name}{sfx}_final_vs_reference", out[0].cpu(), torch.from_numpy(g["out" + sfx]).reshape(out[0].shape))
    assert torch.isfinite(out).all() and err < TOL_X, err


@pytest.mark.parametrize("name", sorted(TINY_CASES))
def test_tiny_python_eager_vs_reference_and_ctx_bit_identical(tiny, name):
    """Python eager against the reference's run in this mode; dawn_sampler_run(_ancestral)_clip and the use_ctx route of
    diffusion.sample bit-identical to it, thresholds included."""
    _, sd = tiny
    sampler, mode, scale = TINY_CASES[name]
    g, d = load_golden(f"clip_{name}.npz"), load_golden("ddim_tiny.npz")
    unet = tiny_unet(sd)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    runs = [(ANCESTRAL_STEPS, "", KEEP)] if sampler == "ancestral" else [(S, f"_S{S}", DDIM_KEEP[S]) for S in ddim_steps(name)]
    for S, sfx, keep in runs:
        diff = _diffusion(unet, 12, 8, mode, sampler, S)
        if sampler == "ancestral":
            noises = [n.cuda() for n in ancestral_noises(tuple(d["x_init"].shape), S, int(g["ancestral_noise_seed"]))[:-1]]
        else:
            noises = [n.cuda() for n in ddim_noises_tiny(tuple(d["x_init"].shape), S, d["noises"], int(g["ddim_noise_seed"]))]
        kw = dict(cond=cond, cond_scale=scale, x_init=x_init, noises=noises)
        if mode[0] == "none":
            sample = lambda **k: diff.ddim_sample(torch.cat([fea, bbox], 1), (1, 3, 12, 8, 8), clip_denoised=False, **kw, **k)  # noqa: E731
        else:
            sample = lambda **k: diff.sample(fea, bbox, **kw, **k)                                                          # noqa: E731
        out = sample(trace=True)
        assert diff.last_route == "python"
        tr = diff.last_trace[0]
        assert len(tr) == S
        _check_vs_reference(name, tr, out, g, sfx, keep, mode)
        ev, clip, null_clip = _ctx_clips(unet, fea, bbox, cond, scale != 1.0)
        got, thr = _ctx_run(ev, diff, mode, clip, null_clip, x_init, noises, scale)
        assert torch.equal(got, out[0]), float((got - out[0]).abs().max())
        if mode[0] != "none":
            assert torch.equal(thr, _trace_s(tr, mode))
        diff.use_ctx = True
        via_ctx = sample()
        assert diff.last_route == "ctx" and torch.equal(via_ctx, out)


# ---------------------------------------------------------------------------------------------------------------- C1
def test_C1_static_every_host_path():
    """Full-size C1, DDIM S = 50, static clipping: Python eager vs the reference; the C evaluator, the use_ctx route and the
    HIP-graph path bit-identical to it."""
    g = load_golden("clip_C1_static.npz")
    T_, h, S = int(g["T"]), int(g["h"]), int(g["S"])
    assert (T_, h, S) == (C1["T"], C1["h"], C1["S"])
    unet = D.DynamicNfUnet3D(default_num_frames=8, **KW, init_seed=0)
    np.testing.assert_allclose(checksum(unet.state_dict().values()), g["weights_checksum"], rtol=1e-12)
    fea272, cond, x3 = build_inputs(T_, h)
    np.testing.assert_allclose(checksum([fea272, cond, x3]), g["inputs_checksum"], rtol=1e-12)
    unet.update_num_frames(T_)
    unet = unet.cuda()
    mode = ("static",)
    diff = _diffusion(unet, T_, h, mode, "ddim", S)
    fea, bbox, cond, x3 = fea272[:, :256].cuda(), fea272[:, 256:].cuda(), cond.cuda(), x3.cuda()
    noises = [n.cuda() for n in ddim_noises(T_, h, S)]
    kw = dict(cond=cond, x_init=x3, noises=noises)
    out = diff.sample(fea, bbox, trace=True, **kw)
    assert diff.last_route == "python"
    tr = diff.last_trace[0]
    _check_vs_reference("C1_static", tr, out, g, "", C1["keep"], mode)
    assert float(out.abs().max()) <= 1.0

    ev, clip, _ = _ctx_clips(unet, fea, bbox, cond, False)
    got, thr = _ctx_run(ev, diff, mode, clip, None, x3, noises, 1.0)
    assert torch.equal(got, out[0]), float((got - out[0]).abs().max())
    assert torch.equal(thr, torch.ones(S, 2, device="cuda"))

    diff.use_ctx = True
    try:
        via_ctx = diff.sample(fea, bbox, **kw)
        assert diff.last_route == "ctx"
    finally:
        diff.use_ctx = False
    assert torch.equal(via_ctx, out)

    diff.use_graph = True
    try:
        graphed = diff.sample(fea, bbox, trace=True, **kw)
    finally:
        diff.use_graph = False
    assert unet._ops().graph_error is None, unet._ops().graph_error
    assert torch.equal(graphed, out), float((graphed - out).abs().max())
    assert all(torch.equal(a["eps"], b["eps"]) for a, b in zip(diff.last_trace[0], tr))


# ---------------------------------------------------------------------------------------------------------------- seeded noise
@pytest.mark.parametrize("mode", [("static",), ("dynamic", 0.5)], ids=["static", "q50"])
@pytest.mark.parametrize("sampler", ["ddim", "ancestral"])
def test_seeded_noise_ctx_equals_python(tiny, mode, sampler):
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8, mode, sampler, S=20, timesteps=1000 if sampler == "ddim" else 60)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    diff.noise_seed = 5
    want = diff.sample(fea, bbox, cond=cond, x_init=x_init)
    assert diff.last_route == "python"
    diff.use_ctx = True
    got = diff.sample(fea, bbox, cond=cond, x_init=x_init)
    assert diff.last_route == "ctx"
    assert torch.equal(got, want), float((got - want).abs().max())
    diff.use_ctx = False
    diff.noise_seed = 6
    assert not torch.equal(diff.sample(fea, bbox, cond=cond, x_init=x_init), want)


# ---------------------------------------------------------------------------------------------------------------- T-shard
class CountingExchange(Exchange):
    """Exchange whose C-host callbacks count the all-reduces they are asked for, per rank."""

    def __init__(self, world):
        super().__init__(world)
        self.n_reduce = [0] * world

    def callbacks(self, rank):
        ex = self

        def halo_begin(xe, hl, F, hh, frame_floats):
            ex.halo(rank, xe.view(hl + F + hh, frame_floats), hl, F, hh)

        def red(op):
            def f(t):
                ex.n_reduce[rank] += 1
                ex.reduce(rank, t, op)
            return f
        return ShardCallbacks(rank, self.world, halo_begin, lambda: None, red(torch.add), red(torch.add), red(torch.minimum))


@pytest.mark.parametrize("mode", [("static",), ("dynamic", 0.5)], ids=["static", "q50"])
@pytest.mark.parametrize("sampler", ["ddim", "ancestral"])
def test_two_tshard_ranks_both_hosts_equal_unsharded(tiny, mode, sampler):
    """A 50-step schedule (DDIM S = 50, or timesteps = 50 ancestral) on a 16-frame clip over two in-process ranks, C host and Python
    host, against the unsharded clip at the shard tests' gate.  static: the step tail issues no collective -- each rank's count
    over the whole loop equals the count of the S evaluations alone on the same rank setup."""
    g, sd = tiny
    unet = tiny_unet(sd)
    ops, P = unet._ops(), unet.packed()
    world, Fr, TS, seed = 2, 8, 50, 21
    Tt = world * Fr
    gen = torch.Generator().manual_seed(11)
    fea272 = T(g["x"])[0, 3:, 0].contiguous().cuda()
    cond = torch.randn(Tt, T(g["cond"]).shape[2], generator=gen).cuda()
    x3 = torch.randn(3, Tt, 8, 8, generator=gen).cuda()
    unet.update_num_frames(Tt)
    diff = _diffusion(unet, Tt, 8, mode, sampler, S=TS, timesteps=1000 if sampler == "ddim" else TS)
    diff.noise_seed = seed
    want = diff.sample(fea272[None, :-4], fea272[None, -4:], cond=cond[None], x_init=x3[None])[0]
    steps = _steps(diff)
    assert len(steps) == TS
    torch.cuda.synchronize()
    loop = ancestral_sample_clip if sampler == "ancestral" else ddim_sample_clip

    ex = CountingExchange(world)
    evs = [CtxEvaluator(P) for _ in range(world)]

    def rank_ctx(r):
        clip = evs[r].prepare_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous())
        run = evs[r].sample_ancestral if sampler == "ancestral" else evs[r].sample
        return run(clip, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, seed=seed, want_thresholds=True, shard=ex.callbacks(r),
                   x0_clip=mode)
    res = run_ranks(world, rank_ctx)
    for _, thr in res[1:]:
        assert torch.equal(thr, res[0][1])
    err = log(f"clip_{sampler}_{mode[0]}_ctx_2ranks_vs_unsharded", torch.cat([o for o, _ in res], dim=1), want)
    assert err < 5e-5, err
    n_loop_ctx = list(ex.n_reduce)

    ex_e = CountingExchange(world)

    def rank_ctx_evals(r):                                   # the S evaluations alone, same rank setup
        clip = evs[r].prepare_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous())
        cb = ex_e.callbacks(r)
        x = x3[:, r * Fr:(r + 1) * Fr].contiguous()
        for st in steps:
            evs[r].forward(clip, x, st["t"], shard=cb)
        return True
    run_ranks(world, rank_ctx_evals)
    assert all(n > 0 for n in ex_e.n_reduce)
    if mode[0] == "static":
        assert n_loop_ctx == ex_e.n_reduce, (n_loop_ctx, ex_e.n_reduce)
    else:
        assert n_loop_ctx == [n + 4 * TS for n in ex_e.n_reduce], (n_loop_ctx, ex_e.n_reduce)

    ex = Exchange(world)
    comms = [InProcComm(ex, r, Fr) for r in range(world)]

    def rank_py(r):
        ops_r = ops.with_comm(comms[r])
        cs = unet.build_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous(), comm=comms[r], Ttotal=Tt, f0=r * Fr)
        noise = lambda i: ops_r.philox_normal(3, Fr, r * Fr, Tt, 64, seed, i + 1, x3.device).reshape(3, Fr, 8, 8)   # noqa: E731
        return loop(ops_r, P, cs, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, noise, clip=mode)
    got = torch.cat(run_ranks(world, rank_py), dim=1)
    err = log(f"clip_{sampler}_{mode[0]}_python_2ranks_vs_unsharded", got, want)
    assert err < 5e-5, err
    n_loop_py = [c.n_allreduce for c in comms]

    ex = Exchange(world)
    comms_e = [InProcComm(ex, r, Fr) for r in range(world)]

    def rank_py_evals(r):
        ops_r = ops.with_comm(comms_e[r])
        cs = unet.build_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous(), comm=comms_e[r], Ttotal=Tt, f0=r * Fr)
        x = x3[:, r * Fr:(r + 1) * Fr].contiguous()
        for st in steps:
            unet_forward(ops_r, P, cs, x, st["t"])
        return True
    run_ranks(world, rank_py_evals)
    n_eval_py = [c.n_allreduce for c in comms_e]
    assert all(n > 0 for n in n_eval_py)
    if mode[0] == "static":
        assert n_loop_py == n_eval_py, (n_loop_py, n_eval_py)
    else:
        assert n_loop_py == [n + 4 * TS for n in n_eval_py], (n_loop_py, n_eval_py)


# ---------------------------------------------------------------------------------------------------------------- regression guard
@pytest.mark.parametrize("scale", [1.0, 2.5], ids=["unguided", "guided"])
@pytest.mark.parametrize("sampler", ["ddim", "ancestral"])
def test_dynamic_090_through_the_new_entries_equals_the_old_entries(tiny, sampler, scale):
    """dawn_sampler_run_clip / dawn_sampler_run_ancestral_clip with {dynamic, 0.9} == dawn_sampler_run(_guided) /
    dawn_sampler_run_ancestral, outputs and thresholds; and the Python loop with clip=("dynamic", 0.9) == its default."""
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8, ("dynamic", 0.9), sampler, S=10, timesteps=1000 if sampler == "ddim" else 40)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    ev, clip, null_clip = _ctx_clips(unet, fea, bbox, cond, scale != 1.0)
    steps = _steps(diff)
    run = ev.sample if sampler == "ddim" else ev.sample_ancestral
    kw = dict(seed=9, want_thresholds=True, null_clip=null_clip, cond_scale=scale)
    old, thr_old = run(clip, x_init[0].contiguous(), steps, **kw)
    new, thr_new = run(clip, x_init[0].contiguous(), steps, x0_clip=("dynamic", 0.9), **kw)
    assert torch.equal(new, old) and torch.equal(thr_new, thr_old)
    other, thr_other = run(clip, x_init[0].contiguous(), steps, x0_clip=("dynamic", 0.5), **kw)
    assert not torch.equal(other, old) and not torch.equal(thr_other, thr_old)
    # error returns of the mode struct: nothing launched
    for bad in (("dynamic", 0.9, 7), ):
        from dawn_pytorch_amd import ctx as CX
        real = CX.CLIP_KINDS["dynamic"]
        CX.CLIP_KINDS["dynamic"] = bad[2]
        try:
            with pytest.raises(_lib.DawnHipError, match="unknown kind"):
                run(clip, x_init[0].contiguous(), steps, x0_clip=("dynamic", 0.9), **kw)
        finally:
            CX.CLIP_KINDS["dynamic"] = real
    diff.noise_seed = 9
    want = diff.sample(fea, bbox, cond=cond, cond_scale=scale, x_init=x_init)
    assert torch.equal(want[0], old)
