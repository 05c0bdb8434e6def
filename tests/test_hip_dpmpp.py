"""-m gpu: DPM-Solver++(2M) on every sampler path -- the two step-tail kernels against the fp64 definition of include/dawn_hip.h, Python
eager, HIP graph, the C evaluator (dawn_sampler_run_dpmpp), the use_ctx route and T-shard ranks of both hosts.  The solver is not in the
reference: the kernels are held to the definition, the hosts to the CPU orchestration of tests/test_dpmpp_cpu.py and to each other bit
for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from guarded import GuardedOps
from inproc_shard import Exchange, InProcComm, run_ranks
from test_dpmpp_cpu import MODES, S_TINY, TOL_X, _tiny_diffusion
from test_hip_end2end import T, log, tiny_unet
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.ctx import ALLREDUCE_FN, CtxEvaluator
from dawn_pytorch_amd.sampler import dpmpp_sample_clip, dpmpp_step_scalars

pytestmark = pytest.mark.gpu

DPMPP_KEYS = ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")
f32 = lambda v: float(np.float32(v))                                     # noqa: E731
RECIP, RECIPM1 = f32(1.8371), f32(1.5411)
A_, B_, C_ = f32(0.8123), f32(0.2871), f32(-0.0931)                       # a second-order step; the first-order one has c = 0
S_DYN = f32(1.7)
U = 2.0 ** -24                                                           # half an ulp, relative: one fp32 rounding

_g = []


@pytest.fixture
def g():
    if not _g:
        _g.append(GuardedOps())
    o = _g[0]
    o.reset()
    try:
        yield o
    finally:
        o.reset()


def plain():
    from dawn_pytorch_amd.ops import HipOps
    return HipOps()


def vec(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def gview(g, t, name, off):
    """The 1-D CPU tensor t as a guarded input (NaN all round); off = 1: a view one float into the buffer, not 16-byte aligned."""
    if t is None:
        return None
    if not off:
        return g.guarded_in(t, name=name)[0]
    v = g.guarded_in(torch.cat((t.new_zeros(1), t)), name=name)[0][1:]
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def gout(g, n, name, off):
    """A caller's output of n floats: poisoned (NaN), between bands; off = 1: one float into it (element 0 must stay poison)."""
    t = g.guarded_out(1, n + off, name=name).view(-1)
    return t[off:]


def finish(g, overwritten=(), offset_outs=()):
    torch.cuda.synchronize()
    for r in g.outs:                              # an offset output: the float before the view belongs to nobody and stays poison
        if r.name in offset_outs:
            first = r.payload.view(-1)[:1]
            assert bool(torch.isnan(first).all()), f"{r.name}: the element before the offset view was written"
            first.zero_()
    g.verify()
    g.inputs_intact(overwritten)


def want_update(x, v, vp, c):
    """fp64 value of the definition's update and its gate: 8 * 2^-24 * (|A x| + |b v| + |c v_prev|) per element -- at most five
    roundings (A*x, b*v, their sum, the fused history term, and the division by s / the formation of x0 behind v), each of relative
    size 2^-24 on a partial sum that the sum of magnitudes bounds."""
    x, v = x.double(), v.double()
    out = A_ * x + B_ * v
    mag = (A_ * x).abs() + (B_ * v).abs()
    if vp is not None:
        out = out + c * vp.double()
        mag = mag + (c * vp.double()).abs()
    return out, 8.0 * U * mag


def x0_fp32(x, eps):
    """x0 with the roundings of dawn_ddim_x0: fma(recip, x, -(recipm1 * eps)).  The product recipm1 * eps is exact in fp64 and rounded
    to fp32 once; recip * x is exact in fp64, and the one fp64 rounding of the difference before the fp32 one can move the result by
    an ulp in rare ties -- the comparison of v allows that ulp."""
    p = (RECIPM1 * eps.double()).float().double()
    return (RECIP * x.double() - p).float()


CASES = [(n, off, hist, inplace) for n in (3 * 12 * 8 * 8, 3 * 7 * 9 * 9 + 5, 3) for off in (0, 1) for hist in (False, True)
         for inplace in (False, True)]


@pytest.mark.parametrize("n,off,hist,inplace", CASES, ids=[f"n{n}-{'offset' if o else 'aligned'}-{'c' if h else 'c0_null'}-{'inplace' if i else 'outofplace'}"
                                                          for n, o, h, i in CASES])
def test_step_tail_kernels_against_the_fp64_definition(g, n, off, hist, inplace):
    """dawn_dpmpp_update (dynamic, s = 1.7 with |x0| up to several s) and dawn_dpmpp_step_fixed (static and none) on guarded, poisoned
    buffers: 128-bit body + scalar tail (aligned; n = 3 is below the body, 1706 has a 2-element tail and, on the scalar path, more than one block;
    2304 has no tail), the scalar path (offset views), c = 0 with v_prev = NULL against c != 0, out of place against in place (out == x, v_out ==
    v_prev; with NULL history the v_out buffer is NaN-poisoned, which must not reach the output).  Then the fused kernel against
    dawn_ddim_x0 -> dawn_dpmpp_update bit for bit, at s = 1 and with the clamp removed."""
    x, eps, x0, vp = vec(n, 1, 1.5), vec(n, 2), vec(n, 3, 2.5), (vec(n, 4) if hist else None)
    c = C_ if hist else 0.0
    s = torch.tensor([S_DYN, S_DYN])
    P = plain()

    def run(call, first_name, first, *scalars, **kw):
        g.reset()
        xg, fg, pg = gview(g, x, "x", off), gview(g, first, first_name, off), gview(g, vp, "v_prev", off)
        sg = g.guarded_in(s, name="s")[0]
        if inplace:
            outs = dict(out=xg, v_out=pg if hist else gout(g, n, "v_out", off))
        elif off:
            outs = dict(out=gout(g, n, "out", off), v_out=gout(g, n, "v_out", off))
        else:
            outs = {}                              # the op's own results: GuardedOps.empty carves and poisons them
        if call == "update":
            out, v = g.dpmpp_update(fg, sg, xg, pg, A_, B_, c, **outs)
        else:
            out, v = g.dpmpp_step_fixed(xg, fg, pg, RECIP, RECIPM1, A_, B_, c, *scalars, **outs, **kw)
        over = (("x",) + (("v_prev",) if hist else ())) if inplace else ()
        finish(g, overwritten=over, offset_outs=("out", "v_out") if off else ())
        if outs:
            assert out.data_ptr() == outs["out"].data_ptr() and v.data_ptr() == outs["v_out"].data_ptr()
        else:
            assert {"_dpmpp_buffers.out", "_dpmpp_buffers.v_out"} <= {r.name for r in g.outs}
        return out.cpu(), v.cpu()

    # ---- dynamic
    out, v = run("update", "x0", x0)
    v64 = x0.double().clamp(-S_DYN, S_DYN) / S_DYN
    assert n == 3 or float(x0.abs().max()) > S_DYN
    assert bool(((v.double() - v64).abs() <= 1.000001 * U * v64.abs()).all())            # one correctly rounded division
    want, gate = want_update(x, v64, vp, c)
    err = (out.double() - want).abs()
    print(f"dpmpp_update n={n}: max err / gate = {float((err / gate).max()):.3f}")
    assert torch.isfinite(out).all() and bool((err <= gate).all()), float((err / gate).max())

    # ---- static and none, fused
    xc, ec, pc = x.cuda(), eps.cuda(), None if vp is None else vp.cuda()
    x0_dev, _ = P.ddim_x0(xc, ec, RECIP, RECIPM1)
    x0_dev = x0_dev.clone()
    x0_ref = x0_fp32(x, eps)
    assert bool(((x0_dev.cpu().double() - x0_ref.double()).abs() <= 2 * U * x0_ref.double().abs()).all())
    for clamp in (True, False):
        out, v = run("fixed", "eps", eps, clamp)
        v_ref = x0_ref.clamp(-1.0, 1.0) if clamp else x0_ref
        assert n == 3 or float(x0_ref.abs().max()) > 1.0
        assert bool(((v.double() - v_ref.double()).abs() <= 2 * U * v_ref.double().abs()).all())
        want, gate = want_update(x, v_ref, vp, c)
        err = (out.double() - want).abs()
        print(f"dpmpp_step_fixed clamp={int(clamp)} n={n}: max err / gate = {float((err / gate).max()):.3f}")
        assert torch.isfinite(out).all() and bool((err <= gate).all()), float((err / gate).max())
        # the two-launch sequence.  static: s = 1.  none: s = 2^20 and b * 2^20 -- clamp(x0, -s, s) / s is then x0 / 2^20 exactly
        # (|x0| < 2^20) and the power of two cancels exactly in b * v, so that launch computes a*x + b*x0 (+ c*v_prev) with no clamp
        if clamp:
            out2, v2 = P.dpmpp_update(x0_dev, torch.ones(2, device="cuda"), xc, pc, A_, B_, c)
        else:
            out2, v2 = P.dpmpp_update(x0_dev, torch.full((2,), 2.0 ** 20, device="cuda"), xc, pc, A_, B_ * 2.0 ** 20, c)
            v2 = v2 * 2.0 ** 20
        assert torch.equal(out, out2.cpu()) and torch.equal(v, v2.cpu()), (clamp, int((out != out2.cpu()).sum()))
        if clamp and n > 3:
            assert not torch.equal(v, x0_dev.cpu())


def test_step_tail_kernels_edges_and_refusals():
    """n = 0 launches nothing and succeeds; a NaN-poisoned history with c = 0 and v_prev = NULL leaves the output finite (handing the
    buffer over would not: 0 * NaN); every forbidden overlap is an error return that names it, nothing written."""
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()                                                                 # noqa: E731
    n = 1000
    x, eps, x0, vp = (vec(n, i).cuda() for i in (1, 2, 3, 4))
    s = torch.tensor([S_DYN, S_DYN], device="cuda")
    out, v = torch.full((n,), 7.0, device="cuda"), torch.full((n,), 7.0, device="cuda")
    assert L.dawn_dpmpp_update(p(x0), p(s), p(x), p(vp), A_, B_, C_, 0, p(v), p(out), st) == 0
    assert L.dawn_dpmpp_step_fixed(p(x), p(eps), p(vp), RECIP, RECIPM1, A_, B_, C_, 1, 0, p(v), p(out), st) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((v == 7.0).all())
    ops = plain()
    hist = torch.full((n,), float("nan"), device="cuda")
    for o, vv in (ops.dpmpp_update(x0, s, x, None, A_, B_, 0.0, v_out=hist),
                  ops.dpmpp_step_fixed(x, eps, None, RECIP, RECIPM1, A_, B_, 0.0, True, v_out=hist.fill_(float("nan")))):
        assert vv is hist and torch.isfinite(o).all() and torch.isfinite(hist).all()
    o_nan, _ = ops.dpmpp_update(x0, s, x, hist.fill_(float("nan")), A_, B_, 0.0, v_out=torch.empty_like(hist))
    assert torch.isnan(o_nan).all()                          # why the hosts pass NULL: the kernel does not test c
    before = [t.clone() for t in (x, eps, x0, vp, out, v)]
    bad_update = [  # (x0, x, v_prev, v_out, out)
        (p(x0), p(x), p(vp), p(v), p(x0)), (p(x0), p(x), p(vp), p(v), p(vp)), (p(x0), p(x), p(vp), p(v), p(v)), (p(x0), p(x), p(vp), p(x), p(out)),
        (p(x0), p(x), p(vp), p(x0), p(out)), (p(x0), p(x), p(vp), p(v), p(x) + 4), (p(x0), p(x), p(vp), p(vp) + 4, p(out)),
        (p(x0), p(x), None, p(v), p(v) + 4)]
    for a0, a1, a2, a3, a4 in bad_update:
        rc = L.dawn_dpmpp_update(a0, p(s), a1, a2, A_, B_, C_, n - 1, a3, a4, st)
        assert rc != 0 and b"alias" in L.dawn_last_error(), (a0, a1, a2, a3, a4)
    rc = L.dawn_dpmpp_update(p(x0), p(out) + 8, p(x), None, A_, B_, 0.0, n, p(v), p(out), st)
    assert rc != 0 and b"alias" in L.dawn_last_error()
    for a0, a1, a2, a3, a4 in ((p(x), p(eps), p(vp), p(v), p(eps)), (p(x), p(eps), p(vp), p(eps), p(out)), (p(x), p(eps), p(vp), p(x), p(x)),
                               (p(x), p(eps), p(vp), p(v), p(vp))):
        rc = L.dawn_dpmpp_step_fixed(a0, a1, a2, RECIP, RECIPM1, A_, B_, C_, 1, n - 1, a3, a4, st)
        assert rc != 0 and b"alias" in L.dawn_last_error(), (a0, a1, a2, a3, a4)
    rc = L.dawn_dpmpp_step_fixed(p(x), p(eps), None, RECIP, RECIPM1, A_, B_, 0.0, 7, n, p(v), p(out), st)
    assert rc != 0 and b"clamp" in L.dawn_last_error()
    rc = L.dawn_dpmpp_update(p(x0), None, p(x), None, A_, B_, 0.0, n, p(v), p(out), st)
    assert rc != 0 and b"null" in L.dawn_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (x, eps, x0, vp, out, v)))
    # the allowed aliases run: out == x and v_out == v_prev at once
    want_o, want_v = ops.dpmpp_update(x0, s, x, vp, A_, B_, C_)
    xi, vi = x.clone(), vp.clone()
    ops.dpmpp_update(x0, s, xi, vi, A_, B_, C_, v_out=vi, out=xi)
    assert torch.equal(xi, want_o) and torch.equal(vi, want_v)


# ---------------------------------------------------------------------------------------------------------------- tiny UNet, every host
def _diffusion(unet, T_, h, mode, S):
    kw = dict(use_dynamic_thres=True, dynamic_thres_percentile=mode[1]) if mode[0] == "dynamic" else {}
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=h, sampling_timesteps=S,
                                        timesteps=1000, loss_type='l2', null_cond_prob=0.1, ddim_sampling_eta=1.0, **kw).cuda()
    diff.update_num_frames(T_)
    diff.solver = "dpmpp2m"
    return diff


def _steps(diff):
    return dpmpp_step_scalars({k: getattr(diff, k) for k in DPMPP_KEYS}, diff.sampling_timesteps, diff.num_timesteps)


@pytest.mark.parametrize("scale", [1.0, 2.5], ids=["unguided", "guided"])
@pytest.mark.parametrize("mode_name", sorted(MODES))
def test_tiny_every_host(tiny, mode_name, scale):
    """S = 6 on the tiny UNet: Python eager on the GPU against the same orchestration on the CPU reference op set (which
    tests/test_dpmpp_cpu.py holds to the restated definition) within TOL_X; dawn_sampler_run_dpmpp, the use_ctx route and the HIP-graph
    route torch.equal to eager, dynamic thresholds too."""
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    mode = MODES[mode_name]
    _, cpu = _tiny_diffusion(sd, mode)
    cpu.solver = "dpmpp2m"
    fea272 = torch.cat([T(d["fea"]), T(d["bbox"])], dim=1)
    kw_cpu = dict(cond=T(d["cond"]), cond_scale=scale, x_init=T(d["x_init"]), trace=True)
    with torch.no_grad():
        want = (cpu.ddim_sample(fea272, (1, 3, 12, 8, 8), clip_denoised=False, **kw_cpu) if mode_name == "none" else
                cpu.sample(T(d["fea"]), T(d["bbox"]), **kw_cpu))
    want_tr = cpu.last_trace[0]

    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8, mode, S_TINY)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    kw = dict(cond=cond, cond_scale=scale, x_init=x_init)
    if mode_name == "none":
        sample = lambda **k: diff.ddim_sample(torch.cat([fea, bbox], 1), (1, 3, 12, 8, 8), clip_denoised=False, **kw, **k)   # noqa: E731
    else:
        sample = lambda **k: diff.sample(fea, bbox, **kw, **k)                                                           # noqa: E731
    out = sample(trace=True)
    assert diff.last_route == "python"
    tr = diff.last_trace[0]
    assert len(tr) == S_TINY
    for i, (e, w) in enumerate(zip(tr, want_tr)):
        assert log(f"dpmpp_{mode_name}_{scale}_x_step_{i}", e["x"], w["x"]) < TOL_X, i
        assert log(f"dpmpp_{mode_name}_{scale}_x0c_step_{i}", e["x0c"], w["x0c"]) < TOL_X, i
    err = log(f"dpmpp_{mode_name}_{scale}_final_vs_cpu", out, want)
    assert torch.isfinite(out).all() and err < TOL_X, err
    thr_py = torch.stack([e["s"] for e in tr]) if mode_name != "none" else None

    ev = CtxEvaluator(unet.packed())
    f272 = torch.cat((fea, bbox), 1)[0].contiguous()
    rcos, rsin = unet.packed().rotary_tables(12 + 2 * unet.packed().win)
    clip = ev.prepare_clip(f272, cond[0].contiguous(), rcos, rsin)
    null_clip = ev.prepare_null_clip(f272, 12, rcos, rsin) if scale != 1.0 else None
    got, thr = ev.sample_dpmpp(clip, x_init[0].contiguous(), _steps(diff), want_thresholds=True, null_clip=null_clip, cond_scale=scale,
                               x0_clip=mode)
    assert torch.equal(got, out[0]), float((got - out[0]).abs().max())
    if mode_name != "none":
        assert torch.equal(thr, thr_py)
    if mode_name == "dynamic":                              # clip = NULL is dynamic at 0.9
        assert torch.equal(ev.sample_dpmpp(clip, x_init[0].contiguous(), _steps(diff), null_clip=null_clip, cond_scale=scale), got)

    diff.use_ctx = True
    try:
        via_ctx = sample()
        assert diff.last_route == "ctx"
    finally:
        diff.use_ctx = False
    assert torch.equal(via_ctx, out)

    diff.use_graph = True
    try:
        graphed = sample(trace=True)
    finally:
        diff.use_graph = False
    assert unet._ops().graph_error is None, unet._ops().graph_error
    assert diff.last_route == "python" and torch.equal(graphed, out), float((graphed - out).abs().max())
    if mode_name != "none":
        assert torch.equal(torch.stack([e["s"] for e in diff.last_trace[0]]), thr_py)

    diff.solver = "ddim"                                    # another solver: another sample (the attribute reaches the GPU hosts)
    diff.noise_seed = 3
    assert not torch.allclose(sample(), out, atol=1e-3)


def test_first_step_with_history_is_refused(tiny):
    _, sd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8, MODES["static"], S_TINY)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    ev = CtxEvaluator(unet.packed())
    clip = ev.prepare_clip(torch.cat((fea, bbox), 1)[0].contiguous(), cond[0].contiguous())
    steps = [dict(st) for st in _steps(diff)]
    steps[0]["c"] = -0.25
    with pytest.raises(_lib.DawnHipError, match="no history"):
        ev.sample_dpmpp(clip, x_init[0].contiguous(), steps, x0_clip=("static",))


# ---------------------------------------------------------------------------------------------------------------- T-shard
@pytest.mark.parametrize("mode_name", ["dynamic", "static"])
def test_two_tshard_ranks_both_hosts_equal_unsharded(tiny, mode_name):
    """S = 10 on a 16-frame clip over two in-process ranks: the C host (dawn_sampler_run_dpmpp with the shard callbacks) and the Python
    host (tshard communicators) equal the unsharded clip within the shard tests' gate.  static: the u32 all-reduce callbacks are NULL."""
    g, sd = tiny
    mode = MODES[mode_name]
    unet = tiny_unet(sd)
    ops, P = unet._ops(), unet.packed()
    world, Fr, TS = 2, 8, 10
    Tt = world * Fr
    gen = torch.Generator().manual_seed(11)
    fea272 = T(g["x"])[0, 3:, 0].contiguous().cuda()
    cond = torch.randn(Tt, T(g["cond"]).shape[2], generator=gen).cuda()
    x3 = torch.randn(3, Tt, 8, 8, generator=gen).cuda()
    unet.update_num_frames(Tt)
    diff = _diffusion(unet, Tt, 8, mode, TS)
    want = diff.sample(fea272[None, :-4], fea272[None, -4:], cond=cond[None], x_init=x3[None])[0]
    steps = _steps(diff)
    assert len(steps) == TS and sum(st["c"] != 0.0 for st in steps) == TS - 2
    torch.cuda.synchronize()

    ex = Exchange(world)
    evs = [CtxEvaluator(P) for _ in range(world)]

    def rank_ctx(r):
        clip = evs[r].prepare_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous())
        cb = ex.callbacks(r)
        if mode_name == "static":
            cb.c.allreduce_sum_u32 = C.cast(None, ALLREDUCE_FN)
            cb.c.allreduce_min_u32 = C.cast(None, ALLREDUCE_FN)
        return evs[r].sample_dpmpp(clip, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, want_thresholds=True, shard=cb, x0_clip=mode)
    res = run_ranks(world, rank_ctx)
    for _, thr in res[1:]:
        assert torch.equal(thr, res[0][1])
    err = log(f"dpmpp_{mode_name}_ctx_2ranks_vs_unsharded", torch.cat([o for o, _ in res], dim=1), want)
    assert err < 5e-5, err

    ex = Exchange(world)
    comms = [InProcComm(ex, r, Fr) for r in range(world)]

    def rank_py(r):
        ops_r = ops.with_comm(comms[r])
        cs = unet.build_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous(), comm=comms[r], Ttotal=Tt, f0=r * Fr)
        return dpmpp_sample_clip(ops_r, P, cs, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, clip=mode)
    got = torch.cat(run_ranks(world, rank_py), dim=1)
    err = log(f"dpmpp_{mode_name}_python_2ranks_vs_unsharded", got, want)
    assert err < 5e-5, err
