"""-m gpu: classifier-free guidance (cond_scale != 1) on every sampler path -- Python eager, HIP graph, the C evaluator
(dawn_unet_forward_guided / dawn_sampler_run_guided) and T-shard ranks of both hosts -- with the condition-free prefix of the two
branches evaluated once.  Pinned to the reference's own guided sampler (tools/gen_goldens_guided.py -> ddim_guided_{tiny,C1}.npz);
every host must agree bit for bit with the Python eager path, which must agree bit for bit with two separate evaluations."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from fullsize_cases import DDIM_CASES, KW, build_inputs, checksum, ddim_noises
from inproc_shard import Exchange, InProcComm, run_ranks
from test_hip_end2end import T, log, tiny_unet
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.ctx import CtxEvaluator
from dawn_pytorch_amd.sampler import ddim_sample_clip, ddim_step_scalars

pytestmark = pytest.mark.gpu

TOL_X = 1e-4
TOL_Q = 2e-5
SCALE = 2.5
STEP_KEYS = ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod")


def _diffusion(unet, T_, h, S):
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=h, sampling_timesteps=S,
                                        timesteps=1000, loss_type='l2', use_dynamic_thres=True, null_cond_prob=0.1,
                                        ddim_sampling_eta=1.0).cuda()
    diff.update_num_frames(T_)
    return diff


@pytest.fixture(scope="module")
def c1():
    """The reference's guided C1 trajectory (T=16, h=32, S=10) and everything needed to rerun it."""
    g = load_golden("ddim_guided_C1.npz")
    T_, h, S, keep = DDIM_CASES["C1"]
    assert (int(g["T"]), int(g["h"]), int(g["S"])) == (T_, h, S) and float(g["cond_scale"]) == SCALE
    unet = D.DynamicNfUnet3D(default_num_frames=8, **KW, init_seed=0)
    np.testing.assert_allclose(checksum(unet.state_dict().values()), g["weights_checksum"], rtol=1e-12)
    fea272, cond, x3 = build_inputs(T_, h)
    np.testing.assert_allclose(checksum([fea272, cond, x3]), g["inputs_checksum"], rtol=1e-12)
    unet.update_num_frames(T_)
    unet = unet.cuda()
    noises = [n.cuda() for n in ddim_noises(T_, h, S, int(g["ddim_noise_seed"]))] + [None]
    return dict(g=g, unet=unet, T=T_, h=h, S=S, keep=keep, fea=fea272[:, :256].cuda(), bbox=fea272[:, 256:].cuda(), cond=cond.cuda(),
                x3=x3.cuda(), noises=noises, diff=_diffusion(unet, T_, h, S))


def _check_vs_reference(name, diff, out, g, keep):
    tr = diff.last_trace[0]
    qs = torch.stack([t["s"][1] for t in tr]).cpu()
    qref = torch.from_numpy(g["quantiles"]).float()
    log(f"guided_{name}_quantiles_rel", qs, qref)
    qerr = float(((qs - qref).abs() / qref.abs()).max())
    assert qerr < TOL_Q, (qerr, qs, qref)
    for s in keep:
        want = torch.from_numpy(g[f"x_before_step_{s}"]).reshape(tr[s - 1]["x"].shape)
        assert log(f"guided_{name}_x_before_step_{s}", tr[s - 1]["x"].cpu(), want) < TOL_X, s
    err = log(f"guided_{name}_final_vs_reference", out[0].cpu(), torch.from_numpy(g["out"]).reshape(out[0].shape))
    assert torch.isfinite(out).all() and err < TOL_X, err
    return qs


def _ctx_clips(unet, fea, bbox, cond):
    ev = CtxEvaluator(unet.packed())
    f272 = torch.cat((fea, bbox), 1)[0].contiguous()
    T_ = cond.shape[1]
    rcos, rsin = unet.packed().rotary_tables(T_ + 2 * unet.packed().win)
    return ev, ev.prepare_clip(f272, cond[0].contiguous(), rcos, rsin), ev.prepare_null_clip(f272, T_, rcos, rsin)


def test_guided_tiny_python_eager_vs_reference_and_ctx_bit_identical(tiny):
    g, sd = tiny
    d = load_golden("ddim_guided_tiny.npz")
    S = int(d["S"])
    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8, S)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    noises = [n.cuda() for n in T(d["noises"])]
    out = diff.sample(fea, bbox, cond=cond, cond_scale=SCALE, x_init=x_init, noises=noises, trace=True)
    qs = _check_vs_reference("tiny", diff, out, d, d["keep"].tolist())
    ev, clip, null_clip = _ctx_clips(unet, fea, bbox, cond)
    steps = ddim_step_scalars({k: getattr(diff, k) for k in STEP_KEYS}, S, 1.0)
    nz = [noises[i][0].contiguous() if st["t_next"] > 0 else None for i, st in enumerate(steps)]
    got, thr = ev.sample(clip, x_init[0].contiguous(), steps, noises=nz, want_thresholds=True, null_clip=null_clip, cond_scale=SCALE)
    assert torch.equal(got, out[0]), float((got - out[0]).abs().max())
    assert torch.equal(thr[:, 1].cpu(), qs)


def test_guided_C1_every_host_path(c1):
    """Full-size C1 (fused level-0 cross-attention: the conditional branch writes h1 beside the shared c1): Python eager vs the
    reference; dawn_sampler_run_guided, the use_ctx route of diffusion.sample and the HIP-graph path bit-identical to it."""
    c = c1
    diff, unet = c["diff"], c["unet"]
    kw = dict(cond=c["cond"], cond_scale=SCALE, x_init=c["x3"], noises=c["noises"])
    out = diff.sample(c["fea"], c["bbox"], trace=True, **kw)
    assert diff.last_route == "python"
    qs = _check_vs_reference("C1", diff, out, c["g"], c["keep"])

    ev, clip, null_clip = _ctx_clips(unet, c["fea"], c["bbox"], c["cond"])
    steps = ddim_step_scalars({k: getattr(diff, k) for k in STEP_KEYS}, c["S"], 1.0)
    nz = [n[0].contiguous() if n is not None else None for n in c["noises"]]
    got, thr = ev.sample(clip, c["x3"][0].contiguous(), steps, noises=nz, want_thresholds=True, null_clip=null_clip, cond_scale=SCALE)
    assert torch.equal(got, out[0]), float((got - out[0]).abs().max())
    assert torch.equal(thr[:, 1].cpu(), qs)

    diff.use_ctx = True
    try:
        via_ctx = diff.sample(c["fea"], c["bbox"], **kw)
        assert diff.last_route == "ctx"
    finally:
        diff.use_ctx = False
    assert torch.equal(via_ctx, out)

    diff.use_graph = True
    try:
        graphed = diff.sample(c["fea"], c["bbox"], **kw)
    finally:
        diff.use_graph = False
    assert unet._ops().graph_error is None, unet._ops().graph_error
    assert torch.equal(graphed, out), float((graphed - out).abs().max())

    # two runs of the same guided sample are bit-identical (C host, seeded counter-based noise as well)
    again = ev.sample(clip, c["x3"][0].contiguous(), steps, noises=nz, null_clip=null_clip, cond_scale=SCALE)
    assert torch.equal(again, got)


def test_guided_seeded_noise_ctx_equals_python(c1):
    c = c1
    diff = c["diff"]
    diff.noise_seed = 5
    try:
        want = diff.sample(c["fea"], c["bbox"], cond=c["cond"], cond_scale=SCALE, x_init=c["x3"])
        diff.use_ctx = True
        got = diff.sample(c["fea"], c["bbox"], cond=c["cond"], cond_scale=SCALE, x_init=c["x3"])
        assert diff.last_route == "ctx"
        got2 = diff.sample(c["fea"], c["bbox"], cond=c["cond"], cond_scale=SCALE, x_init=c["x3"])
    finally:
        diff.use_ctx = False
        diff.noise_seed = None
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(got2, got)


def test_forward_guided_equals_two_forwards_and_cfg_combine(c1):
    """Sharing the prefix changes no arithmetic: dawn_unet_forward_guided == dawn_cfg_combine(forward(null), forward(cond)), and
    the Python module's forward_with_cond_scale gives the same bits."""
    c = c1
    unet = c["unet"]
    ev, clip, null_clip = _ctx_clips(unet, c["fea"], c["bbox"], c["cond"])
    x3 = c["x3"][0].contiguous()
    e_c = ev.forward(clip, x3, 640.0)
    e_n = ev.forward(null_clip, x3, 640.0)
    want = unet._ops().cfg_combine(e_n, e_c, SCALE)
    got = ev.forward_guided(clip, null_clip, x3, 640.0, SCALE)
    assert torch.equal(got, want), float((got - want).abs().max())
    x = torch.cat((c["x3"], torch.cat((c["fea"], c["bbox"]), 1)[:, :, None].expand(-1, -1, c["T"], -1, -1)), 1)
    y = unet.forward_with_cond_scale(x, torch.tensor([640], device="cuda"), cond=c["cond"], cond_scale=SCALE)
    assert torch.equal(y[0], want), float((y[0] - want).abs().max())
    # cond_scale == 1 through the guided entry is the unguided evaluation
    assert torch.equal(ev.forward_guided(clip, null_clip, x3, 640.0, 1.0), e_c)


def test_cfg_x0_kernel_bit_identical_to_combine_then_x0():
    L = _lib.lib()
    from dawn_pytorch_amd.ops import HipOps
    ops = HipOps()
    g = torch.Generator().manual_seed(3)
    for n in (3 * 16 * 32 * 32, 3 * 7 * 9 * 9 + 5):
        e_n, e_c, x = (torch.randn(n, generator=g).mul_(s).cuda() for s in (1.0, 1.3, 2.0))
        eps = ops.cfg_combine(e_n, e_c, SCALE)
        x0, hist = ops.ddim_x0(x, eps, 1.37, 0.91)
        x0, hist = x0.clone(), hist.clone()
        eps2, x02, hist2 = ops.cfg_x0(e_n, e_c, SCALE, x, 1.37, 0.91)
        assert torch.equal(eps2, eps) and torch.equal(x02, x0) and torch.equal(hist2, hist)
        assert int(hist2.sum()) == n
    # x0_out aliasing x is rejected, not run
    assert L.dawn_cfg_x0(e_n.data_ptr(), e_c.data_ptr(), 2.0, x.data_ptr(), 1.0, 1.0, n, eps.data_ptr(), x.data_ptr(),
                         hist.data_ptr(), torch.cuda.current_stream().cuda_stream) != 0


def test_guided_entry_with_scale_one_equals_sampler_run(tiny):
    g, sd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8, int(d["S"]))
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    ev, clip, null_clip = _ctx_clips(unet, fea, bbox, cond)
    steps = ddim_step_scalars({k: getattr(diff, k) for k in STEP_KEYS}, int(d["S"]), 1.0)
    want = ev.sample(clip, x_init[0].contiguous(), steps, seed=9)
    got = ev.sample(clip, x_init[0].contiguous(), steps, seed=9, null_clip=null_clip, cond_scale=1.0)
    assert torch.equal(got, want)


def test_guided_two_tshard_ranks_both_hosts_equal_unsharded(tiny):
    g, sd = tiny
    unet = tiny_unet(sd)
    ops, P = unet._ops(), unet.packed()
    world, Fr, S, seed = 2, 8, 3, 21
    Tt = world * Fr
    gen = torch.Generator().manual_seed(11)
    fea272 = T(g["x"])[0, 3:, 0].contiguous().cuda()
    cond = torch.randn(Tt, T(g["cond"]).shape[2], generator=gen).cuda()
    x3 = torch.randn(3, Tt, 8, 8, generator=gen).cuda()
    unet.update_num_frames(Tt)
    diff = _diffusion(unet, Tt, 8, S)
    diff.noise_seed = seed
    want = diff.sample(fea272[None, :-4], fea272[None, -4:], cond=cond[None], cond_scale=SCALE, x_init=x3[None])[0]
    steps = ddim_step_scalars({k: getattr(diff, k) for k in STEP_KEYS}, S, 1.0)
    torch.cuda.synchronize()

    # C host: dawn_sampler_run_guided with the shard callbacks
    ex = Exchange(world)
    evs = [CtxEvaluator(P) for _ in range(world)]

    def rank_ctx(r):
        clip = evs[r].prepare_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous())
        null_clip = evs[r].prepare_null_clip(fea272, Fr)
        return evs[r].sample(clip, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, seed=seed, want_thresholds=True,
                             shard=ex.callbacks(r), null_clip=null_clip, cond_scale=SCALE)
    res = run_ranks(world, rank_ctx)
    for _, thr in res[1:]:
        assert torch.equal(thr, res[0][1])
    err = log("guided_ctx_2ranks_vs_unsharded", torch.cat([o for o, _ in res], dim=1), want)
    assert err < 5e-5, err

    # Python host: the guided sampler on tshard communicators
    ex = Exchange(world)
    comms = [InProcComm(ex, r, Fr) for r in range(world)]

    def rank_py(r):
        ops_r = ops.with_comm(comms[r])
        kw = dict(comm=comms[r], Ttotal=Tt, f0=r * Fr)
        cs = unet.build_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous(), **kw)
        cs_null = unet.build_clip(fea272, torch.zeros_like(cond[r * Fr:(r + 1) * Fr]), **kw)
        noise = lambda i: ops_r.philox_normal(3, Fr, r * Fr, Tt, 64, seed, i + 1, x3.device).reshape(3, Fr, 8, 8)   # noqa: E731
        return ddim_sample_clip(ops_r, P, cs, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, noise, SCALE, cs_null)
    got = torch.cat(run_ranks(world, rank_py), dim=1)
    err = log("guided_python_2ranks_vs_unsharded", got, want)
    assert err < 5e-5, err
    for cm in comms:
        # one evaluation = 1 init + 2 x (2 down + 1 mid + 2 up) temporal layers with the prefix shared: the init exchange once
        assert cm.stats()["halo_exchanges"] == S * (1 + 2 * 5), cm.stats()
