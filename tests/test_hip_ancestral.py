"""-m gpu: ancestral (DDPM) sampling on every sampler path -- Python eager, HIP graph, the C evaluator (dawn_sampler_run_ancestral)
and T-shard ranks of both hosts.  Pinned to the reference's own 1000-step p_sample_loop (tools/gen_goldens_ancestral.py ->
ancestral_{tiny,guided_tiny,C1}.npz); every host must agree bit for bit with the Python eager path."""
import numpy as np
import pytest
import torch

from ancestral_cases import KEEP, ancestral_noises
from conftest import load_golden
from fullsize_cases import KW, build_inputs, checksum
from inproc_shard import Exchange, InProcComm, run_ranks
from test_hip_end2end import T, log, tiny_unet
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.ctx import CtxEvaluator
from dawn_pytorch_amd.sampler import ancestral_sample_clip, ancestral_step_scalars

pytestmark = pytest.mark.gpu

TOL_X = 1e-4
TOL_Q = 2e-5
STEP_KEYS = ("sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod", "posterior_mean_coef1", "posterior_mean_coef2",
             "posterior_log_variance_clipped")


def _diffusion(unet, T_, h, timesteps=1000):
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_, denoise_fn=unet, num_frames=T_, image_size=h,
                                        sampling_timesteps=timesteps, timesteps=timesteps, loss_type='l2', use_dynamic_thres=True,
                                        null_cond_prob=0.1, ddim_sampling_eta=1.0).cuda()
    diff.update_num_frames(T_)
    assert not diff.is_ddim_sampling
    return diff


def _steps(diff):
    return ancestral_step_scalars({k: getattr(diff, k) for k in STEP_KEYS}, diff.num_timesteps)


def _noises(d, shape):
    """The reference's per-step draws (seeded CPU generator), t > 0 only: timesteps - 1 entries."""
    return [n.cuda() for n in ancestral_noises(shape, int(d["timesteps"]), int(d["ancestral_noise_seed"]))[:-1]]


def _check_vs_reference(name, diff, out, g):
    tr = diff.last_trace[0]
    assert len(tr) == int(g["timesteps"])
    qs = torch.stack([t["s"][1] for t in tr]).cpu()
    qref = torch.from_numpy(g["quantiles"]).float()
    log(f"ancestral_{name}_quantiles_rel", qs, qref)
    qerr = float(((qs - qref).abs() / qref.abs()).max())
    assert qerr < TOL_Q, qerr
    for s in KEEP:
        want = torch.from_numpy(g[f"x_before_step_{s}"]).reshape(tr[s - 1]["x"].shape)
        assert log(f"ancestral_{name}_x_before_step_{s}", tr[s - 1]["x"].cpu(), want) < TOL_X, s
    err = log(f"ancestral_{name}_final_vs_reference", out[0].cpu(), torch.from_numpy(g["out"]).reshape(out[0].shape))
    assert torch.isfinite(out).all() and err < TOL_X, err
    return qs


def _ctx_clips(unet, fea, bbox, cond, guided):
    ev = CtxEvaluator(unet.packed())
    f272 = torch.cat((fea, bbox), 1)[0].contiguous()
    T_ = cond.shape[1]
    rcos, rsin = unet.packed().rotary_tables(T_ + 2 * unet.packed().win)
    clip = ev.prepare_clip(f272, cond[0].contiguous(), rcos, rsin)
    return ev, clip, (ev.prepare_null_clip(f272, T_, rcos, rsin) if guided else None)


def test_ancestral_update_kernel_bit_identical_to_ddim_update():
    """dawn_ancestral_update == dawn_ddim_update(x0, eps := x_t, san := c1, c := c2, sigma := std) into a separate buffer, out of
    place and in place (out == x_t), with and without noise; out == x0 is rejected, not run."""
    from dawn_pytorch_amd.ops import HipOps
    ops = HipOps()
    L = _lib.lib()
    g = torch.Generator().manual_seed(5)
    s = torch.tensor([1.7, 1.7], device="cuda")
    for n in (3 * 16 * 32 * 32, 3 * 7 * 9 * 9 + 5):
        x0, x_t, nz = (torch.randn(n, generator=g).mul_(m).cuda() for m in (2.5, 1.0, 1.0))
        for noise, (c1, c2, std) in ((nz, (0.0123, 0.9871, 0.0456)), (None, (1.0, 0.0, 1e-10))):
            want = ops.ddim_update(x0, x_t, s, noise, c1, c2, std)
            got = ops.ancestral_update(x0, x_t, s, noise, c1, c2, std)
            assert torch.equal(got, want)
            inplace = x_t.clone()
            ops.ancestral_update(x0, inplace, s, noise, c1, c2, std, out=inplace)
            assert torch.equal(inplace, want)
    rc = L.dawn_ancestral_update(x0.data_ptr(), x_t.data_ptr(), s.data_ptr(), None, 1.0, 0.0, 0.0, n, x0.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc != 0 and b"alias" in L.dawn_last_error()


@pytest.mark.parametrize("name", ["ancestral_tiny.npz", "ancestral_guided_tiny.npz"])
def test_tiny_python_eager_vs_reference_and_ctx_bit_identical(tiny, name):
    g, sd = tiny
    d = load_golden(name)
    scale = float(d["cond_scale"])
    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    noises = _noises(d, tuple(d["x_init"].shape))
    out = diff.sample(fea, bbox, cond=cond, cond_scale=scale, x_init=x_init, noises=noises, trace=True)
    assert diff.last_route == "python"
    qs = _check_vs_reference(name[len("ancestral_"):-4], diff, out, d)
    ev, clip, null_clip = _ctx_clips(unet, fea, bbox, cond, scale != 1.0)
    steps = _steps(diff)
    nz = [noises[i][0].contiguous() if st["t"] > 0 else None for i, st in enumerate(steps)]
    got, thr = ev.sample_ancestral(clip, x_init[0].contiguous(), steps, noises=nz, want_thresholds=True, null_clip=null_clip,
                                   cond_scale=scale)
    assert torch.equal(got, out[0]), float((got - out[0]).abs().max())
    assert torch.equal(thr[:, 1].cpu(), qs)


@pytest.fixture(scope="module")
def c1():
    """The reference's 1000-step ancestral C1 trajectory (T=16, h=32, shipped architecture) and everything needed to rerun it."""
    g = load_golden("ancestral_C1.npz")
    T_, h = int(g["T"]), int(g["h"])
    unet = D.DynamicNfUnet3D(default_num_frames=8, **KW, init_seed=0)
    np.testing.assert_allclose(checksum(unet.state_dict().values()), g["weights_checksum"], rtol=1e-12)
    fea272, cond, x3 = build_inputs(T_, h)
    np.testing.assert_allclose(checksum([fea272, cond, x3]), g["inputs_checksum"], rtol=1e-12)
    unet.update_num_frames(T_)
    unet = unet.cuda()
    return dict(g=g, unet=unet, T=T_, h=h, fea=fea272[:, :256].cuda(), bbox=fea272[:, 256:].cuda(), cond=cond.cuda(),
                x3=x3.cuda(), noises=_noises(g, (1, 3, T_, h, h)), diff=_diffusion(unet, T_, h))


def test_C1_every_host_path(c1):
    """Full-size C1: Python eager vs the reference; dawn_sampler_run_ancestral, the use_ctx route of diffusion.sample and the
    HIP-graph path bit-identical to it (outputs and thresholds)."""
    c = c1
    diff, unet = c["diff"], c["unet"]
    kw = dict(cond=c["cond"], x_init=c["x3"], noises=c["noises"])
    out = diff.sample(c["fea"], c["bbox"], trace=True, **kw)
    assert diff.last_route == "python"
    qs = _check_vs_reference("C1", diff, out, c["g"])

    ev, clip, _ = _ctx_clips(unet, c["fea"], c["bbox"], c["cond"], False)
    steps = _steps(diff)
    nz = [c["noises"][i][0].contiguous() if st["t"] > 0 else None for i, st in enumerate(steps)]
    got, thr = ev.sample_ancestral(clip, c["x3"][0].contiguous(), steps, noises=nz, want_thresholds=True)
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
        graphed = diff.sample(c["fea"], c["bbox"], trace=True, **kw)
    finally:
        diff.use_graph = False
    assert unet._ops().graph_error is None, unet._ops().graph_error
    assert torch.equal(graphed, out), float((graphed - out).abs().max())
    assert torch.equal(torch.stack([t["s"][1] for t in diff.last_trace[0]]).cpu(), qs)


def test_seeded_noise_ctx_equals_python(tiny):
    g, sd = tiny
    d = load_golden("ancestral_tiny.npz")
    unet = tiny_unet(sd)
    diff = _diffusion(unet, 12, 8)
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))
    diff.noise_seed = 5
    want = diff.sample(fea, bbox, cond=cond, x_init=x_init)
    diff.use_ctx = True
    got = diff.sample(fea, bbox, cond=cond, x_init=x_init)
    assert diff.last_route == "ctx"
    got2 = diff.sample(fea, bbox, cond=cond, x_init=x_init)
    assert torch.equal(got, want), float((got - want).abs().max())
    assert torch.equal(got2, got)
    diff.use_ctx = False
    diff.noise_seed = 6                             # the seed reaches the noise: a different sample
    assert not torch.equal(diff.sample(fea, bbox, cond=cond, x_init=x_init), want)


def test_two_tshard_ranks_both_hosts_equal_unsharded(tiny):
    """A timesteps=50 ancestral schedule on a 16-frame clip over two in-process ranks: the C host (dawn_sampler_run_ancestral with
    the shard callbacks) and the Python host (tshard communicators) equal the unsharded clip within the shard tests' gate."""
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
    diff = _diffusion(unet, Tt, 8, TS)
    diff.noise_seed = seed
    want = diff.sample(fea272[None, :-4], fea272[None, -4:], cond=cond[None], x_init=x3[None])[0]
    steps = _steps(diff)
    assert len(steps) == TS
    torch.cuda.synchronize()

    ex = Exchange(world)
    evs = [CtxEvaluator(P) for _ in range(world)]

    def rank_ctx(r):
        clip = evs[r].prepare_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous())
        return evs[r].sample_ancestral(clip, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, seed=seed, want_thresholds=True,
                                       shard=ex.callbacks(r))
    res = run_ranks(world, rank_ctx)
    for _, thr in res[1:]:
        assert torch.equal(thr, res[0][1])
    err = log("ancestral_ctx_2ranks_vs_unsharded", torch.cat([o for o, _ in res], dim=1), want)
    assert err < 5e-5, err

    ex = Exchange(world)
    comms = [InProcComm(ex, r, Fr) for r in range(world)]

    def rank_py(r):
        ops_r = ops.with_comm(comms[r])
        cs = unet.build_clip(fea272, cond[r * Fr:(r + 1) * Fr].contiguous(), comm=comms[r], Ttotal=Tt, f0=r * Fr)
        noise = lambda i: ops_r.philox_normal(3, Fr, r * Fr, Tt, 64, seed, i + 1, x3.device).reshape(3, Fr, 8, 8)   # noqa: E731
        return ancestral_sample_clip(ops_r, P, cs, x3[:, r * Fr:(r + 1) * Fr].contiguous(), steps, noise)
    got = torch.cat(run_ranks(world, rank_py), dim=1)
    err = log("ancestral_python_2ranks_vs_unsharded", got, want)
    assert err < 5e-5, err
