"""-m gpu: known-frame conditioning on every sampler path and the chunked driver.  The replacement kernel on guarded, poisoned buffers
against the definition of include/dawn_hip.h formed in fp32 on the CPU (bit for bit), its generator path against dawn_philox_normal, its
refusals; then the tiny UNet on every host -- Python eager against the CPU orchestration that tests/test_known_cpu.py holds to the
restated definition, dawn_sampler_run_known, the use_ctx route and the HIP-graph route bit for bit against eager -- two T-shard ranks of
both hosts, and sample_chunked / iter_chunks against the hand-written loop.  Not in the reference: nothing here is a golden."""
import ctypes as C

import pytest
import torch

from conftest import load_golden
from guarded import GuardedOps
from inproc_shard import Exchange, InProcComm, run_ranks
from test_dpmpp_cpu import TOL_X
from test_hip_end2end import T, log, tiny_unet
from test_known_cpu import KNOWN, MODES, S_TINY, KnownRefOps, _inputs, _tiny_diffusion, known_replace_ref
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd import sampler as SM
from dawn_pytorch_amd.ctx import ALLREDUCE_FN, CtxEvaluator

pytestmark = pytest.mark.gpu

A_, B_ = 0.7779903411865234, 0.6282762289047241           # level 3 of the S = 6 DDIM loop (fp32 values)
SEED = 0x1234567890AB

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


def _gin(g, t, name, off):
    """The CPU tensor t as a guarded input (NaN all round); off: a view one float into the buffer (4 bytes past 16-byte alignment)."""
    if not off:
        return g.guarded_in(t, name=name)[0]
    v = g.guarded_in(torch.cat((t.new_zeros(1), t.flatten())), name=name)[0][1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# (F, hw, masked frames, f0, Ftotal, offsets of (x, known, noise), generator path too)
KERNEL_CASES = {
    "F5-hw16": (5, 16, (0, 3, 4), 0, 5, (0, 0, 0), True),
    "F33-hw64-every-third": (33, 64, tuple(range(0, 33, 3)), 0, 33, (0, 0, 0), True),
    "F33-hw2048-two-blocks-per-plane": (33, 2048, (1, 32), 0, 33, (0, 0, 0), True),
    "F7-hw81-aligned": (7, 81, (0, 2, 5, 6), 0, 7, (0, 0, 0), False),
    "F7-hw81-x-one-float-in": (7, 81, (0, 2, 5, 6), 0, 7, (1, 0, 0), False),
    "F7-hw81-all-one-float-in": (7, 81, (1, 3, 4), 0, 7, (1, 1, 1), False),
    "shard-F4-f0-3-of-11": (4, 64, (0, 1, 3), 3, 11, (0, 0, 0), True),
    "shard-F4-f0-3-of-11-x-one-float-in": (4, 64, (0, 1, 3), 3, 11, (1, 0, 0), True),
}


@pytest.mark.parametrize("case", sorted(KERNEL_CASES))
def test_kernel_against_the_definition(g, case):
    """In place on a guarded x; known and noise hold NaN in every frame outside the mask, so a frame that the kernel touched although
    its mask byte is zero shows.  hw = 81: a 128-bit body with a peeled head and an odd tail when the three pointers are congruent modulo
    16 bytes (aligned: the planes start at every residue; all one float in), the scalar path when they are not (x one float in).
    hw = 2048: more than one block per plane.  Injected noise, the generator (z = ops.philox_normal at the same seed, stream, f0,
    Ftotal), b = 0 with a NaN noise buffer, and out= into a guarded output."""
    F, hw, frames, f0, Ftotal, (ox, ok, on), seeded = KERNEL_CASES[case]
    gen = torch.Generator().manual_seed(F * 1000 + hw)
    x, known, z = (torch.randn(3, F, hw, generator=gen) for _ in range(3))
    mask = torch.zeros(F, dtype=torch.uint8)
    mask[list(frames)] = 1
    m = mask.bool()
    known_nan, z_nan = known.clone(), z.clone()
    known_nan[:, ~m] = float("nan")
    z_nan[:, ~m] = float("nan")

    def run(a, b, noise, **kw):
        g.reset()
        xg, kg, mg = _gin(g, x, "x", ox), _gin(g, known_nan, "known", ok), g.guarded_in(mask, name="mask")[0]
        ng = None if noise is None else _gin(g, noise, "noise", on)
        got = g.known_replace(xg, kg, mg, a, b, noise=ng, f0=f0, Ftotal=Ftotal, **kw)
        torch.cuda.synchronize()
        assert got.data_ptr() == xg.data_ptr()
        g.verify()
        g.inputs_intact(overwritten=("x",))                # known, noise and mask unchanged; the bands of all four untouched
        got = got.cpu()
        assert torch.equal(got[:, ~m], x[:, ~m])           # frames outside the mask: not written (and their NaN inputs not used)
        return got

    got = run(A_, B_, z_nan)
    want = known_replace_ref(x.clone(), known, mask, A_, B_, z)
    assert torch.equal(got, want), int((got != want).sum())
    fused = torch.tensor(A_) * known.double() + torch.tensor(B_).double() * z.double()       # one rounding: what a contracted kernel gives
    assert hw < 64 or not torch.equal(want[:, m], fused.float()[:, m])
    # b == 0: the noise buffer is not read
    got = run(1.0, 0.0, torch.full_like(z, float("nan")))
    assert bool(torch.isfinite(got).all()) and torch.equal(got[:, m], known[:, m])
    got = run(A_, 0.0, None)
    assert torch.equal(got, known_replace_ref(x.clone(), known, mask, A_, 0.0, None))
    if seeded:
        for sid in (0x80000000, 0x80000006):
            zs = g.philox_normal(3, F, f0, Ftotal, hw, SEED, sid, "cuda").cpu()
            whole = g.philox_normal(3, Ftotal, 0, Ftotal, hw, SEED, sid, "cuda").cpu()
            assert torch.equal(zs, whole[:, f0:f0 + F])                                   # keyed by the global element index
            got = run(A_, B_, None, seed=SEED, stream_id=sid)
            assert torch.equal(got, known_replace_ref(x.clone(), known, mask, A_, B_, zs)), sid
    # out=: x stays, the guarded output holds the result
    g.reset()
    xg, kg, mg, ng = _gin(g, x, "x", ox), _gin(g, known_nan, "known", ok), g.guarded_in(mask, name="mask")[0], _gin(g, z_nan, "noise", on)
    out = g.guarded_out(3 * F, hw, name="out").view(3, F, hw)
    res = g.known_replace(xg, kg, mg, A_, B_, noise=ng, f0=f0, Ftotal=Ftotal, out=out)
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    g.verify()
    g.inputs_intact()
    assert torch.equal(res.cpu(), want)


def test_kernel_refusals_write_nothing():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()                                                                 # noqa: E731
    F, hw = 5, 16
    n = 3 * F * hw
    gen = torch.Generator().manual_seed(1)
    x, known, z = (torch.randn(n + 8, generator=gen).cuda() for _ in range(3))
    mask = torch.ones(F, dtype=torch.uint8, device="cuda")
    before = [t.clone() for t in (x, known, z)]
    call = lambda xp, kp, mp, F_, f0, Ft, hw_, b, zp: L.dawn_known_replace(xp, kp, mp, F_, f0, Ft, hw_, A_, b, zp, SEED, 0x80000000, st)   # noqa: E731
    for args, word in (((None, p(known), p(mask), F, 0, F, hw, B_, p(z)), b"null"),
                       ((p(x), None, p(mask), F, 0, F, hw, B_, p(z)), b"null"),
                       ((p(x), p(known), None, F, 0, F, hw, B_, p(z)), b"null"),
                       ((p(x), p(x), p(mask), F, 0, F, hw, B_, p(z)), b"overlap"),
                       ((p(x), p(x) + 4 * (n - 1), p(mask), F, 0, F, hw, B_, p(z)), b"overlap"),
                       ((p(x) + 16, p(known), p(mask), F, 0, F, hw, B_, p(x)), b"overlap"),
                       ((p(x), p(known), p(mask), -1, 0, F, hw, B_, p(z)), b"out of range"),
                       ((p(x), p(known), p(mask), F, 1, F, hw, B_, p(z)), b"out of range"),
                       ((p(x), p(known), p(mask), F, 7, 11, hw, B_, p(z)), b"out of range"),
                       ((p(x), p(known), p(mask), F, 0, F, 15, B_, None), b"multiple of 4")):
        rc = call(*args)
        assert rc != 0 and b"dawn_known_replace" in L.dawn_last_error() and word in L.dawn_last_error(), (args, L.dawn_last_error())
    assert call(p(x), p(known), p(mask), 0, 0, F, hw, B_, p(z)) == 0                          # F == 0: nothing to do, no launch
    assert call(p(x), p(known), p(mask), 0, 11, 11, hw, B_, None) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (x, known, z)))
    # what the refusals protect: the allowed calls next to them run (hw % 4 != 0 with injected noise, and with b == 0 and no noise)
    assert call(p(x), p(known), p(mask), F, 0, F, 15, B_, p(z)) == 0 and call(p(x), p(known), p(mask), F, 0, F, 15, 0.0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(x[3 * F * 15:], before[0][3 * F * 15:]) and torch.equal(x[:3 * F * 15], torch.tensor(A_).cuda() * known[:3 * F * 15])


# ---------------------------------------------------------------------------------------------------------------- tiny UNet, every host
def _diffusion(unet, mode, S, T_=12, timesteps=1000):
    kw = dict(use_dynamic_thres=True, dynamic_thres_percentile=mode[1]) if mode[0] == "dynamic" else {}
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=8, sampling_timesteps=S,
                                        timesteps=timesteps, loss_type='l2', null_cond_prob=0.1, ddim_sampling_eta=1.0, **kw).cuda()
    diff.update_num_frames(T_)
    return diff


def _bufs(diff):
    return {k: getattr(diff, k) for k in ("alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                                          "posterior_mean_coef1", "posterior_mean_coef2", "posterior_log_variance_clipped")}


def _steps_levels(diff, kind):
    """The six steps and seven levels of a loop: DDIM / DPM-Solver++ at S = 6; ancestral: the LAST six of the 1000 steps."""
    bufs = _bufs(diff)
    if kind == "ancestral":
        steps = SM.ancestral_step_scalars(bufs, 1000)
        return steps[-S_TINY:], SM.known_level_scalars(bufs, steps, "ancestral", 1000)[-(S_TINY + 1):]
    steps = SM.ddim_step_scalars(bufs, S_TINY, 1.0) if kind == "ddim" else SM.dpmpp_step_scalars(bufs, S_TINY)
    return steps, SM.known_level_scalars(bufs, steps, kind, 1000)


def _loop(kind, ops, P, cs, csn, x_init, steps, noises, scale, mode, kf, **kw):
    fn = dict(ddim=SM.ddim_sample_clip, ancestral=SM.ancestral_sample_clip)
    if kind == "dpmpp":
        return SM.dpmpp_sample_clip(ops, P, cs, x_init, steps, scale, csn, clip=mode, known=kf, **kw)
    return fn[kind](ops, P, cs, x_init, steps, lambda i: noises[i], scale, csn, clip=mode, known=kf, **kw)


HOST_CASES = [(k, "dynamic", s) for k in ("ddim", "ancestral", "dpmpp") for s in (1.0, 2.5)] + [("ddim", "static", 1.0), ("dpmpp", "none", 2.5),
                                                                                              ("ancestral", "static", 2.5)]


@pytest.mark.parametrize("kind,mode_name,scale", HOST_CASES, ids=[f"{k}-{m}-{'guided' if s != 1.0 else 'unguided'}" for k, m, s in HOST_CASES])
def test_tiny_every_host(tiny, kind, mode_name, scale):
    """S = 6, T = 12, known frames {0, 1, 2, 11}: the loop on the GPU ops against the same loop on the CPU reference op set within TOL_X
    (the project's gate for an orchestration on the GPU against the CPU one); dawn_sampler_run_known, the HIP-graph route and -- DDIM and
    DPM-Solver++, where GaussianDiffusion runs these very steps -- sample() and its use_ctx route torch.equal to eager, thresholds too;
    known = NULL through the new entry torch.equal to the existing entry."""
    _, sd = tiny
    mode = MODES[mode_name]
    d, noises, kz, known, mask = _inputs()
    m = mask.bool()
    assert tuple(m.nonzero().flatten().tolist()) == KNOWN
    fea272 = torch.cat([T(d["fea"]), T(d["bbox"])], dim=1)[0].contiguous()
    cond, x_init = T(d["cond"])[0].contiguous(), T(d["x_init"])[0].contiguous()
    guided = scale != 1.0

    cpu_unet, cpu_diff = _tiny_diffusion(sd, mode, KnownRefOps())
    steps, levels = _steps_levels(cpu_diff, kind)
    cs = cpu_unet.build_clip(fea272, cond)
    csn = cpu_unet.build_clip(fea272, torch.zeros_like(cond)) if guided else None
    kf_cpu = SM.KnownFrames(known[0], mask, levels, lambda i: kz[i][0])
    with torch.no_grad():
        want = _loop(kind, cpu_unet._ops(), cpu_unet.packed(), cs, csn, x_init, steps, [n[0] for n in noises], scale, mode, kf_cpu)
    assert torch.equal(want[:, m], known[0][:, m])

    unet = tiny_unet(sd)
    diff = _diffusion(unet, mode, S_TINY)
    assert (steps, levels) == _steps_levels(diff, kind)
    ops, P = unet._ops(), unet.packed()
    f272, cg, xg = fea272.cuda(), cond.cuda(), x_init.cuda()
    nz, kzg, kg, mg = [n[0].cuda() for n in noises], [z[0].cuda() for z in kz], known[0].cuda().contiguous(), mask.cuda()
    gcs = unet.build_clip(f272, cg)
    gcsn = unet.build_clip(f272, torch.zeros_like(cg)) if guided else None
    kf = SM.KnownFrames(kg, mg, levels, lambda i: kzg[i])
    tr = []
    with torch.no_grad():
        out = _loop(kind, ops, P, gcs, gcsn, xg, steps, nz, scale, mode, kf, trace=tr)
    err = log(f"known_{kind}_{mode_name}_{scale}_eager_vs_cpu", out, want)
    assert torch.isfinite(out).all() and err < TOL_X, err
    assert torch.equal(out[:, m], kg[:, m])                                             # the known frames, bit for bit
    for i, e in enumerate(tr[:-1]):                                                     # the latent entering step i + 1 lies at level i + 1
        a, b = levels[i + 1]
        assert torch.equal(e["x"][:, m], known_replace_ref(e["x"].cpu().clone(), known[0], mask, a, b, kz[i + 1][0])[:, m].cuda()), i
    thr_py = torch.stack([e["s"] for e in tr]) if mode_name != "none" else None

    ev = CtxEvaluator(P)
    rcos, rsin = P.rotary_tables(12 + 2 * P.win)
    clip = ev.prepare_clip(f272, cg, rcos, rsin)
    null_clip = ev.prepare_null_clip(f272, 12, rcos, rsin) if guided else None
    ckw = dict(want_thresholds=True, null_clip=null_clip, cond_scale=scale, x0_clip=mode)
    if kind == "dpmpp":
        run = lambda **k: ev.sample_dpmpp(clip, xg, steps, **ckw, **k)                                              # noqa: E731
    elif kind == "ancestral":
        run = lambda **k: ev.sample_ancestral(clip, xg, steps, noises=nz, **ckw, **k)                               # noqa: E731
    else:
        run = lambda **k: ev.sample(clip, xg, steps, noises=nz, **ckw, **k)                                         # noqa: E731
    got, thr = run(known=kf)
    assert torch.equal(got, out), float((got - out).abs().max())
    if mode_name != "none":
        assert torch.equal(thr, thr_py)
    plain, thr_plain = run()
    via_new, thr_new = run(known_entry=True)                                            # known = NULL through dawn_sampler_run_known
    assert torch.equal(via_new, plain) and (mode_name == "none" or torch.equal(thr_new, thr_plain))
    assert not torch.equal(plain, got)
    zero, _ = run(known=SM.KnownFrames(kg, torch.zeros_like(mg), levels, lambda i: kzg[i]))
    assert torch.equal(zero, plain)                                                     # an empty mask changes nothing

    with torch.no_grad():
        graphed = _loop(kind, ops, P, gcs, gcsn, xg, steps, nz, scale, mode, kf, use_graph=True)
    assert ops.graph_error is None, ops.graph_error
    assert torch.equal(graphed, out), float((graphed - out).abs().max())

    if kind == "ancestral":
        return
    diff.solver = "dpmpp2m" if kind == "dpmpp" else "ddim"
    fea, bbox = T(d["fea"]).cuda(), T(d["bbox"]).cuda()
    kw = dict(cond=cg[None], cond_scale=scale, x_init=xg[None], noises=[n.cuda() for n in noises], known_latent=known.cuda(), known_mask=mg,
              known_noises=[z.cuda() for z in kz])
    if mode_name == "none":
        sample = lambda: diff.ddim_sample(torch.cat([fea, bbox], 1), (1, 3, 12, 8, 8), clip_denoised=False, **kw)          # noqa: E731
    else:
        sample = lambda: diff.sample(fea, bbox, **kw)                                                                   # noqa: E731
    py = sample()
    assert diff.last_route == "python" and torch.equal(py[0], out)
    diff.use_ctx = True
    via_ctx = sample()
    assert diff.last_route == "ctx" and torch.equal(via_ctx, py)
    diff.use_ctx, diff.use_graph = False, True
    via_graph = sample()
    assert unet._ops().graph_error is None and diff.last_route == "python" and torch.equal(via_graph, py)


def test_entry_refusals(tiny):
    """dawn_sampler_run_known: an unknown solver tag, NULL steps, and a known latent without its mask or its levels are refused with a
    message before anything is launched (x_out keeps its fill)."""
    _, sd = tiny
    d, _, _, known, mask = _inputs()
    unet = tiny_unet(sd)
    diff = _diffusion(unet, MODES["dynamic"], S_TINY)
    steps, levels = _steps_levels(diff, "ddim")
    ev = CtxEvaluator(unet.packed())
    f272 = torch.cat([T(d["fea"]), T(d["bbox"])], dim=1)[0].contiguous().cuda()
    clip = ev.prepare_clip(f272, T(d["cond"])[0].contiguous().cuda())
    from dawn_pytorch_amd.ctx import DdimStep
    arr = (DdimStep * S_TINY)()
    for i, st in enumerate(steps):
        arr[i].t, arr[i].t_next, arr[i].recip, arr[i].recipm1 = st["t"], st["t_next"], st["recip"], st["recipm1"]
        arr[i].sqrt_alpha_next, arr[i].c, arr[i].sigma = st["sqrt_alpha_next"], st["c"], st["sigma"]
    ab = (C.c_float * (2 * (S_TINY + 1)))(*[v for lv in levels for v in lv])
    x = T(d["x_init"])[0].contiguous().cuda()
    out = torch.full_like(x, 7.0)
    kg, mg = known[0].contiguous().cuda(), mask.cuda()
    ws = ev.workspace(12, 8, 8)
    L, st_ = ev.L, torch.cuda.current_stream().cuda_stream

    def call(solver, steps_p, known_p, mask_p, ab_p):
        return L.dawn_sampler_run_known(ev.h, 12, 8, 8, clip["mem"].data_ptr(), None, 1.0, x.data_ptr(), S_TINY, solver, steps_p, 3, None,
                                        out.data_ptr(), None, ws.data_ptr(), ws.numel(), None, None, known_p, mask_p, ab_p, None, st_)
    for args, word in (((3, arr, kg.data_ptr(), mg.data_ptr(), ab), b"unknown solver"), ((-1, arr, None, None, None), b"unknown solver"),
                       ((0, None, kg.data_ptr(), mg.data_ptr(), ab), b"null argument"),
                       ((0, arr, kg.data_ptr(), None, ab), b"known_mask"), ((0, arr, kg.data_ptr(), mg.data_ptr(), None), b"known_ab")):
        rc = call(*args)
        assert rc != 0 and b"dawn_sampler_run_known" in L.dawn_last_error() and word in L.dawn_last_error(), (args[0], L.dawn_last_error())
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(0, arr, kg.data_ptr(), mg.data_ptr(), ab) == 0                          # the complete call next to them runs
    torch.cuda.synchronize()
    assert torch.equal(out[:, mask.bool().cuda()], kg[:, mask.bool().cuda()])


@pytest.mark.parametrize("kind", ["ddim", "dpmpp", "ancestral"])
def test_seeded_known_noise_equals_the_same_draws_injected(tiny, kind):
    """noise_seed set and no known_noises: the kernel draws inline for the known frames; equal to injecting
    philox_normal(seed, 0x80000000 + i), on the Python host and through use_ctx.  Ancestral: a 6-step schedule (timesteps = 6), so that
    GaussianDiffusion.sample runs p_sample_loop in six evaluations."""
    _, sd = tiny
    d, _, _, known, mask = _inputs()
    unet = tiny_unet(sd)
    diff = _diffusion(unet, MODES["dynamic"], S_TINY if kind != "ancestral" else None, timesteps=1000 if kind != "ancestral" else S_TINY)
    assert diff.is_ddim_sampling == (kind != "ancestral")
    diff.solver = "dpmpp2m" if kind == "dpmpp" else "ddim"
    diff.noise_seed = 41
    ops = unet._ops()
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    kw = dict(cond=cond, x_init=x_init, known_latent=known.cuda(), known_mask=mask.cuda())
    seeded = diff.sample(fea, bbox, **kw)
    draws = [ops.philox_normal(3, 12, 0, 12, 64, 41, 0x80000000 + i, "cuda").reshape(1, 3, 12, 8, 8) for i in range(S_TINY + 1)]
    assert not torch.equal(draws[0], ops.philox_normal(3, 12, 0, 12, 64, 41, 1, "cuda").reshape(1, 3, 12, 8, 8))
    injected = diff.sample(fea, bbox, known_noises=draws, **kw)
    assert diff.last_route == "python" and torch.equal(seeded, injected)
    assert torch.equal(seeded[0][:, mask.bool()], known[0][:, mask.bool()].cuda())
    diff.use_ctx = True
    via_ctx = diff.sample(fea, bbox, **kw)
    assert diff.last_route == "ctx" and torch.equal(via_ctx, seeded)
    assert torch.equal(diff.sample(fea, bbox, known_noises=draws, **kw), seeded)
    diff.use_ctx = False
    diff.noise_seed = 42
    assert not torch.equal(diff.sample(fea, bbox, **kw)[0][:, ~mask.bool()], seeded[0][:, ~mask.bool()])


# ---------------------------------------------------------------------------------------------------------------- T-shard
@pytest.mark.parametrize("mode_name", ["dynamic", "static"])
def test_two_tshard_ranks_both_hosts_equal_unsharded(tiny, mode_name):
    """S = 6 DDIM steps on a 16-frame clip over two in-process ranks of 8 frames, known frames 6 ... 9 straddling the rank boundary,
    step noise and known-frame noise from the generator (keyed by the global element index): the C host (dawn_sampler_run_known with the
    shard callbacks) and the Python host (tshard communicators) equal the unsharded clip within the shard tests' gate; the thresholds
    are equal across ranks; the known frames are exact on their ranks.  static: the u32 all-reduce callbacks are NULL."""
    g, sd = tiny
    mode = MODES[mode_name]
    unet = tiny_unet(sd)
    ops, P = unet._ops(), unet.packed()
    world, Fr, seed = 2, 8, 21
    Tt = world * Fr
    gen = torch.Generator().manual_seed(11)
    fea272 = T(g["x"])[0, 3:, 0].contiguous().cuda()
    cond = torch.randn(Tt, T(g["cond"]).shape[2], generator=gen).cuda()
    x3 = torch.randn(3, Tt, 8, 8, generator=gen).cuda()
    known = torch.randn(3, Tt, 8, 8, generator=gen).clamp(-1., 1.).cuda()
    mask = torch.zeros(Tt, dtype=torch.uint8)
    mask[6:10] = 1
    mask = mask.cuda()
    unet.update_num_frames(Tt)
    diff = _diffusion(unet, mode, S_TINY, T_=Tt)
    diff.noise_seed = seed
    want = diff.sample(fea272[None, :-4], fea272[None, -4:], cond=cond[None], x_init=x3[None], known_latent=known[None], known_mask=mask)[0]
    assert torch.equal(want[:, 6:10], known[:, 6:10])
    steps, levels = _steps_levels(diff, "ddim")
    torch.cuda.synchronize()
    sl = lambda r: slice(r * Fr, (r + 1) * Fr)                                                 # noqa: E731
    kf = lambda r: SM.KnownFrames(known[:, sl(r)].contiguous(), mask[sl(r)].contiguous(), levels, None, seed)      # noqa: E731

    ex = Exchange(world)
    evs = [CtxEvaluator(P) for _ in range(world)]

    def rank_ctx(r):
        clip = evs[r].prepare_clip(fea272, cond[sl(r)].contiguous())
        cb = ex.callbacks(r)
        if mode_name == "static":
            cb.c.allreduce_sum_u32 = C.cast(None, ALLREDUCE_FN)
            cb.c.allreduce_min_u32 = C.cast(None, ALLREDUCE_FN)
        return evs[r].sample(clip, x3[:, sl(r)].contiguous(), steps, seed=seed, want_thresholds=True, shard=cb, x0_clip=mode, known=kf(r))
    res = run_ranks(world, rank_ctx)
    for _, thr in res[1:]:
        assert torch.equal(thr, res[0][1])
    got = torch.cat([o for o, _ in res], dim=1)
    err = log(f"known_{mode_name}_ctx_2ranks_vs_unsharded", got, want)
    assert err < 5e-5 and torch.equal(got[:, 6:10], known[:, 6:10]), err

    ex = Exchange(world)
    comms = [InProcComm(ex, r, Fr) for r in range(world)]

    def rank_py(r):
        ops_r = ops.with_comm(comms[r])
        cs = unet.build_clip(fea272, cond[sl(r)].contiguous(), comm=comms[r], Ttotal=Tt, f0=r * Fr)
        noise = lambda i: ops_r.philox_normal(3, Fr, r * Fr, Tt, 64, seed, i + 1, x3.device).reshape(3, Fr, 8, 8)   # noqa: E731
        return SM.ddim_sample_clip(ops_r, P, cs, x3[:, sl(r)].contiguous(), steps, noise, clip=mode, known=kf(r))
    got = torch.cat(run_ranks(world, rank_py), dim=1)
    err = log(f"known_{mode_name}_python_2ranks_vs_unsharded", got, want)
    assert err < 5e-5 and torch.equal(got[:, 6:10], known[:, 6:10]), err


# ---------------------------------------------------------------------------------------------------------------- chunked
@pytest.mark.parametrize("use_ctx", [False, True], ids=["python", "ctx"])
def test_chunked_driver(tiny, use_ctx):
    """T = 30, F = 12, K = 4, S = 6, seeded: sample_chunked equals the hand-written loop of sample(known_...) calls; iter_chunks yields
    the same frames in order; every overlapping frame is bit-identical in both chunks that hold it; T = 10 <= F is the plain sample;
    chunking a T-shard is refused."""
    _, sd = tiny
    unet = tiny_unet(sd)
    diff = _diffusion(unet, MODES["dynamic"], S_TINY)
    diff.noise_seed, diff.use_ctx = 5, use_ctx
    gen = torch.Generator().manual_seed(4)
    fea, bbox, cond = (t.cuda() for t in (torch.randn(1, 12, 8, 8, generator=gen), torch.randn(1, 4, 8, 8, generator=gen),
                                          torch.randn(1, 30, 32, generator=gen)))
    plan = SM.chunk_plan(30, 12, 4)
    assert [(s, kn) for s, _, kn in plan] == [(0, 0), (8, 4), (16, 4), (18, 10)]
    whole = diff.sample_chunked(fea, bbox, cond, 1.0, chunk_frames=12, overlap=4)
    assert diff.last_route == ("ctx" if use_ctx else "python")
    assert whole.shape == (1, 3, 30, 8, 8) and bool(torch.isfinite(whole).all()) and diff.num_frames == 12 and diff.noise_seed == 5
    outs, emitted = [], []
    for j, (start, n, kn) in enumerate(plan):
        diff.noise_seed = 5 + (j << 32)
        kl = km = None
        if kn:
            ps = plan[j - 1][0]
            kl = torch.zeros(1, 3, 12, 8, 8, device="cuda")
            kl[:, :, :kn] = outs[-1][:, :, start - ps:start - ps + kn]
            km = torch.cat([torch.ones(kn, dtype=torch.uint8), torch.zeros(12 - kn, dtype=torch.uint8)]).cuda()
        out = diff.sample(fea, bbox, cond=cond[:, start:start + n].contiguous(), known_latent=kl, known_mask=km)
        outs.append(out)
        emitted.append((start + kn, out[:, :, kn:]))
    diff.noise_seed = 5
    assert torch.equal(whole, torch.cat([c for _, c in emitted], dim=2))
    for j in range(1, len(plan)):                                                       # every overlapping frame, in both chunks
        for f in range(plan[j][0], plan[j - 1][0] + 12):
            assert torch.equal(outs[j][:, :, f - plan[j][0]], outs[j - 1][:, :, f - plan[j - 1][0]]), (j, f)
            assert torch.equal(outs[j][:, :, f - plan[j][0]], whole[:, :, f]), (j, f)
    got = list(diff.iter_chunks(fea, bbox, cond, 1.0, chunk_frames=12, overlap=4))
    assert [f for f, _ in got] == [0, 12, 20, 28] and all(torch.equal(a, b) for (_, a), (_, b) in zip(got, emitted))
    diff.update_num_frames(10)
    short = diff.sample_chunked(fea, bbox, cond[:, :10].contiguous(), 1.0, chunk_frames=12, overlap=4)
    assert torch.equal(short, diff.sample(fea, bbox, cond=cond[:, :10].contiguous()))
    with pytest.raises(ValueError, match="T-shard"):
        diff.sample_chunked(fea, bbox, cond, 1.0, chunk_frames=12, overlap=4, comm=object())
