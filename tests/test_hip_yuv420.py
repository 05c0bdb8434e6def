"""-m gpu: decode to yuv420p frames on the HIP kernels.

* `dawn_frames_to_yuv420` (fp32 planes -> I420) against the numpy restatement of the definition applied to RefOps.frames_to_u8's bytes;
* `dawn_final_conv_blend_yuv420` (the final-conv kernel with the yuv420p egress as its store) against the restatement applied to
  `final_conv_blend_u8`'s bytes -- and against the independent kernel above fed `final_conv_blend`'s fp32 frames;
* `FlowDecoder.decode_clip_yuv420` against restatement(`decode_clip_u8`), both hosts of the launch sequence, and the latent form of
  the C entry;
* `stream_frames_yuv420`: the same bytes, and no clip-sized tensor on the device.

Every comparison is integer equality.  Outputs handed to the two kernels come from tests/guarded.py: poisoned, between guard bands."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from guarded import GuardedOps
from oracle.ops_ref import RefOps
from test_hip_decode_u8 import _full_case, _golden
from test_hip_flow_decode import motion
from test_hip_ops import rnd
from test_yuv420_cpu import ANCHORS, planes, yuv420_np

pytestmark = pytest.mark.gpu

T = torch.from_numpy


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def _eq(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ, the first at {np.argwhere(got != want)[0].tolist()}"


# ---------------------------------------------------------------------------------------------- frames_to_yuv420
@pytest.mark.parametrize("H,W", [(2, 4), (16, 32), (18, 36), (32, 64)])
def test_frames_to_yuv420(H, W):
    """fp32 values (k + 0.5)/255 over random byte levels k (every level occurs at the larger sizes, and over the four sizes together),
    a non-zero mean that clips at both ends, anchors in the first pixels of frame 0; a frame range of a longer clip (strided planes)."""
    Tn, Ttot = 3, 4
    mean = (3.0, -2.5, 40.0)
    gen = torch.Generator().manual_seed(H * 100 + W)
    k = torch.randint(0, 256, (3, Ttot, H, W), generator=gen)
    if H * W >= 256:
        k.view(3, Ttot, -1)[:, 2, :256] = torch.stack([torch.randperm(256, generator=gen) for _ in range(3)])      # every level, each channel
    vid = ((k.float() + 0.5) / 255.0).contiguous()
    colours = list(ANCHORS)
    for i in range(min(len(colours), W // 2)):                           # 2x2 blocks of anchor colours, before `mean` moves them
        for ch in range(3):
            vid[ch, 1, 0:2, 2 * i:2 * i + 2] = (colours[i][ch] + 0.5) / 255.0
    part = vid[:, 1:1 + Tn]
    want = yuv420_np(RefOps().frames_to_u8(part, mean=mean, bgr=False).numpy())
    g = GuardedOps()
    out = g.guarded_out(Tn, 3 * H * W // 2, dtype=torch.uint8)
    got = g.frames_to_yuv420(vid.cuda()[:, 1:1 + Tn], mean=mean, out=out)
    torch.cuda.synchronize()
    _eq(got, want)
    g.verify()                                                           # no byte left as poison, none written outside
    _eq(g.frames_to_yuv420(vid.cuda()[:, 1:1 + Tn], mean=mean), want)    # ... and the op's own allocation


def test_frames_to_yuv420_anchors():
    colours = list(ANCHORS)
    vid = torch.empty(3, len(colours), 2, 4)
    for t, c in enumerate(colours):
        for ch in range(3):
            vid[ch, t] = (c[ch] + 0.5) / 255.0
    g = GuardedOps()
    out = g.guarded_out(len(colours), 12, dtype=torch.uint8)
    g.frames_to_yuv420(vid.cuda(), out=out)
    y, u, v = planes(out.cpu().numpy(), 2, 4)
    for t, c in enumerate(colours):
        assert (y[t] == ANCHORS[c][0]).all() and (u[t] == ANCHORS[c][1]).all() and (v[t] == ANCHORS[c][2]).all(), c
    g.verify()


def test_frames_to_yuv420_error_returns(hip):
    from dawn_pytorch_amd._lib import DawnHipError
    for H, W in ((17, 32), (16, 34)):
        out = torch.full((1, 3 * H * W // 2), 9, device="cuda", dtype=torch.uint8)
        with pytest.raises(DawnHipError, match="even H, W % 4 == 0"):
            hip.frames_to_yuv420(torch.rand(3, 1, H, W).cuda(), out=out)
        torch.cuda.synchronize()
        assert bool((out == 9).all())


# ---------------------------------------------------------------------------------------------- final_conv_blend_yuv420
def _inputs(H, W, Cc, h, w, Ttot):
    x = rnd(3 * H * W, Cc, seed=1).cuda()
    w7 = rnd(49, Cc // 4, 3, 4, seed=2, scale=(49 * Cc) ** -0.5).cuda()
    b3 = rnd(3, seed=3).cuda()
    src = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    grid, conf = motion(Ttot, h, w, seed=6)
    return x, w7, b3, src, grid.cuda(), conf.cuda()


@pytest.mark.parametrize("H,W,Cc,h,w", [(16, 32, 8, 4, 8), (32, 64, 16, 8, 16), (24, 40, 8, 6, 10), (18, 36, 8, 5, 9)])
def test_final_conv_blend_yuv420(hip, H, W, Cc, h, w):
    """One full tile; 2x2 full tiles with two channel chunks; tiles cut in x and in y; nine chroma rows with the flow resized by a
    non-integer factor.  T = 3 frames out of a longer clip (strided grid planes), zero mean and one that clips at both ends."""
    Tn, Ttot = 3, 5
    x, w7, b3, src, grid, conf = _inputs(H, W, Cc, h, w, Ttot)
    for mean in ((0.0, 0.0, 0.0), (90.0, 0.5, -110.0)):
        rgb = torch.empty(Tn, H, W, 3, device="cuda", dtype=torch.uint8)
        hip.final_conv_blend_u8(x, H, W, w7, b3, src, grid[:, 1:4], conf[1:4], rgb, mean=mean, bgr=False)
        want = yuv420_np(rgb.cpu().numpy())
        g = GuardedOps()
        frames = g.guarded_out(Tn, 3 * H * W // 2, dtype=torch.uint8, name="frames")
        g.final_conv_blend_yuv420(x, H, W, w7, b3, src, grid[:, 1:4], conf[1:4], frames, mean=mean)
        torch.cuda.synchronize()
        _eq(frames, want)
        g.verify()
        # the second, independent implementation: the fp32 kernel's frames through frames_to_yuv420
        out = torch.zeros(3, Tn, H, W, device="cuda")
        hip.final_conv_blend(x, H, W, w7, b3, src, grid[:, 1:4], conf[1:4], out, torch.zeros_like(out))
        _eq(hip.frames_to_yuv420(out, mean=mean), want)


def test_final_conv_blend_yuv420_byte_boundaries(hip):
    """The construction of test_final_conv_blend_u8_byte_boundaries: identity flow at the image's own resolution and occlusion 1 make the
    blended value the warped source pixel -- k/255, (k + 0.999)/255 and the float below k/255."""
    H = W = 32
    Cc, Tn = 16, 1
    k = torch.arange(0, 256, dtype=torch.float32)
    src = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4))
    src[0, 0] = k[:32] / 255.0
    src[1, 1] = (k[100:132] + 0.999) / 255.0
    src[2, 2] = torch.nextafter(k[200:232] / 255.0, torch.tensor(0.0))
    src[0, 3] = k[224:] / 255.0
    lin = (torch.arange(H, dtype=torch.float32) + 0.5) / H * 2 - 1
    yy, xx = torch.meshgrid(lin, lin, indexing="ij")
    grid = torch.stack((xx, yy), 0).view(2, 1, H, W).contiguous().cuda()
    conf = torch.ones(Tn, H, W).cuda()
    x = rnd(Tn * H * W, Cc, seed=1).cuda()
    w7 = rnd(49, Cc // 4, 3, 4, seed=2, scale=(49 * Cc) ** -0.5).cuda()
    b3 = rnd(3, seed=3).cuda()
    for mean in ((0.0, 0.0, 0.0), (1.5, 0.0, -2.25)):
        rgb = torch.empty(Tn, H, W, 3, device="cuda", dtype=torch.uint8)
        hip.final_conv_blend_u8(x, H, W, w7, b3, src.cuda(), grid, conf, rgb, mean=mean, bgr=False)
        g = GuardedOps()
        frames = g.guarded_out(Tn, 3 * H * W // 2, dtype=torch.uint8, name="frames")
        g.final_conv_blend_yuv420(x, H, W, w7, b3, src.cuda(), grid, conf, frames, mean=mean)
        _eq(frames, yuv420_np(rgb.cpu().numpy()))
        g.verify()


def test_final_conv_blend_yuv420_rejects_bad_sizes(hip):
    from dawn_pytorch_amd._lib import DawnHipError
    Cc, Tn = 8, 1
    for H, W in ((16, 34), (17, 32)):
        frames = torch.full((Tn, 3 * H * W // 2), 9, device="cuda", dtype=torch.uint8)
        grid, conf = motion(Tn, 4, 8, seed=1)
        with pytest.raises(DawnHipError, match="even H, W % 4 == 0"):
            hip.final_conv_blend_yuv420(rnd(Tn * H * W, Cc, seed=1).cuda(), H, W, rnd(49, Cc // 4, 3, 4, seed=2).cuda(),
                                        rnd(3, seed=3).cuda(), torch.rand(3, H, W).cuda(), grid.cuda(), conf.cuda(), frames)
        torch.cuda.synchronize()
        assert bool((frames == 9).all())                                 # nothing was launched


# ---------------------------------------------------------------------------------------------- the decode paths
def _decoders(sd, hip, chunk):
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    py = FlowDecoder(sd, "cuda", ops=hip, chunk=chunk)
    cc = FlowDecoder(sd, "cuda", ops=hip, chunk=chunk)
    cc.use_ctx = True
    return py, cc


@pytest.mark.parametrize("case", ["tiny", 64])
def test_decode_clip_yuv420(hip, case):
    """The tiny golden (32 x 32, T = 5, chunk 3) and the full LFG architecture at 64 x 64, T = 5, chunk 2: restatement(decode_clip_u8),
    and the C-side decoder `torch.equal` to the Python orchestration."""
    if case == "tiny":
        g, sd = _golden()
        img, grid, conf, chunk = T(g["img"]).cuda(), T(g["grid"]).cuda(), T(g["conf"]).cuda(), 3
    else:
        sd, img, grid, conf = _full_case(case, 5)
        chunk = 2
    py, cc = _decoders(sd, hip, chunk)
    H, W = img.shape[2:]
    for mean in ((0.0, 0.0, 0.0), (2.0, 0.0, -3.5)):
        got = py.decode_clip_yuv420(img, grid, conf, mean=mean)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 5, 3 * H * W // 2)
        _eq(got[0], yuv420_np(py.decode_clip_u8(img, grid, conf, mean=mean, bgr=False)[0].cpu().numpy()))
        assert torch.equal(cc.decode_clip_yuv420(img, grid, conf, mean=mean), got)


def test_c_side_yuv420_workspace_and_error_returns(hip):
    """The workspace dawn_decoder_workspace_bytes states is enough (the evaluator hands over exactly that many bytes, inside a guarded
    buffer here); a short one, and an output next to others, are errors with nothing launched."""
    from dawn_pytorch_amd._lib import DawnHipError
    from dawn_pytorch_amd.ctx import DecoderEvaluator
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    g, sd = _golden()
    dec = FlowDecoder(sd, "cuda", ops=hip, chunk=2)
    de = DecoderEvaluator(dec)
    src = T(g["img"]).cuda()[0].contiguous()
    grid, conf = T(g["grid"]).cuda()[0], T(g["conf"]).cuda()[0, 0]
    mem, _ = de.encode(src)
    kw = dict(T=5, h=8, w=8, chunk=2, grid=grid, conf=conf)
    yuv = torch.full((5, 1536), 9, device="cuda", dtype=torch.uint8)
    with pytest.raises(DawnHipError, match="needed"):
        de.decode(src, mem, yuv=yuv, workspace=torch.empty(4096, device="cuda", dtype=torch.uint8), **kw)
    with pytest.raises(DawnHipError, match="only output"):
        de.decode(src, mem, yuv=yuv, frames=torch.empty(5, 32, 32, 3, device="cuda", dtype=torch.uint8), **kw)
    torch.cuda.synchronize()
    assert bool((yuv == 9).all())
    need = de.workspace_bytes(32, 32, 2)
    go = GuardedOps()
    ws = go.guarded_out(1, need, dtype=torch.uint8, name="workspace")
    out = go.guarded_out(5, 1536, dtype=torch.uint8, name="yuv")
    de.decode(src, mem, yuv=out, workspace=ws, **kw)
    torch.cuda.synchronize()
    for r in go.outs:
        r.check_surroundings("write outside the buffer")
    assert torch.equal(out, dec.decode_clip_yuv420(src[None], grid[None], conf[None, None])[0])
    assert not bool((out == 255).any())                                   # no plane reaches 255: every byte was written


def test_latent_from_dawn_sampler_run_decodes_to_the_same_yuv420_bytes(hip, tiny):
    """The (3,T,h,w) output of dawn_sampler_run handed to dawn_decode_clip_yuv420 as is == the conf form fed pred[:, :2] and
    (pred[:, 2] + 1) * 0.5, as in the u8 test of the same name."""
    import dawn_pytorch_amd as D
    from test_hip_end2end import tiny_unet
    from dawn_pytorch_amd.ctx import CtxEvaluator, DecoderEvaluator
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.sampler import ddim_step_scalars
    _, usd = tiny
    d = load_golden("ddim_tiny.npz")
    unet = tiny_unet(usd)
    S = int(d["S"])
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=12, denoise_fn=unet, num_frames=12, image_size=8, sampling_timesteps=S,
                                        timesteps=1000, loss_type='l2', use_dynamic_thres=True, null_cond_prob=0.1,
                                        ddim_sampling_eta=1.0).cuda()
    fea, bbox, cond = T(d["fea"]).cuda(), T(d["bbox"]).cuda(), T(d["cond"]).cuda()
    ev = CtxEvaluator(unet.packed())
    fea272 = torch.cat((fea, bbox), 1)[0].contiguous()
    clip = ev.prepare_clip(fea272, cond[0].contiguous())
    steps = ddim_step_scalars({k: getattr(diff, k) for k in ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                              "sqrt_recipm1_alphas_cumprod")}, S, 1.0)
    latent = ev.sample(clip, T(d["x_init"]).cuda()[0], steps, seed=77)
    Tn, h, w = latent.shape[1:]
    g, sd = _golden()
    dec = FlowDecoder(sd, "cuda", ops=hip, chunk=5)                       # 12 frames: chunks of 5, 5, 2
    img = T(g["img"]).cuda()
    pred = latent[None]
    mean = (1.0, 0.0, -1.0)
    cgrid, cconf = pred[:, :2], (pred[:, 2].unsqueeze(1) + 1) * 0.5
    want = dec.decode_clip_yuv420(img, cgrid, cconf, mean=mean)
    _eq(want[0], yuv420_np(dec.decode_clip_u8(img, cgrid, cconf, mean=mean)[0].cpu().numpy()))
    de = DecoderEvaluator(dec)
    src = img[0].contiguous()
    mem, _ = de.encode(src)
    got = torch.empty(Tn, 1536, device="cuda", dtype=torch.uint8)
    de.decode(src, mem, T=Tn, h=h, w=w, chunk=5, latent=latent, yuv=got, mean=mean)
    assert torch.equal(got, want[0]), int((got != want[0]).sum())
    conf_form = torch.empty_like(got)
    de.decode(src, mem, T=Tn, h=h, w=w, chunk=5, grid=cgrid[0].contiguous(), conf=cconf[0, 0].contiguous(), yuv=conf_form, mean=mean)
    assert torch.equal(conf_form, got)


@pytest.mark.parametrize("use_ctx", [False, True])
def test_stream_frames_yuv420_same_bytes_and_no_clip_sized_tensor(hip, use_ctx):
    """As test_stream_frames_u8_same_bytes_and_no_clip_sized_tensor: 200 frames at 128 x 128 in chunks of 2.  Streaming must stay below
    ONE fp32 clip (39 MB) plus the chunk workspace; the two-step path (decode_clip, then frames_to_yuv420) does not."""
    from dawn_pytorch_amd.ctx import DecoderEvaluator
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    H, Tn, chunk = 128, 200, 2
    sd, img, grid, conf = _full_case(H, Tn)
    dec = FlowDecoder(sd, "cuda", ops=hip, chunk=chunk)
    dec.use_ctx = use_ctx
    mean = (1.0, 0.0, -1.0)
    want = dec.decode_clip_yuv420(img, grid, conf, mean=mean)[0].cpu().numpy()
    ws_bytes = DecoderEvaluator(dec).workspace_bytes(H, H, chunk)
    clip_bytes = 3 * Tn * H * H * 4
    if use_ctx:
        dec._evaluator()._ws = None                                            # its workspace counts as well
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    parts, t0s = [], []
    for t0, fr in dec.stream_frames_yuv420(img, grid, conf, mean=mean):
        assert fr.shape[1:] == (3 * H * H // 2,)
        t0s.append(t0)
        parts.append(fr.copy())                                                # valid until the next next() only
    peak_stream = torch.cuda.max_memory_allocated() - base
    assert t0s == list(range(0, Tn, chunk))
    assert np.array_equal(np.concatenate(parts, 0), want)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    two = hip.frames_to_yuv420(dec.decode_clip(img, grid, conf)["sample_out_vid"][0], mean=mean).cpu().numpy()
    peak_two_step = torch.cuda.max_memory_allocated() - base
    assert np.array_equal(two, want)
    print(f"peak device bytes: streaming {peak_stream}, two-step {peak_two_step}; one fp32 clip {clip_bytes}, chunk workspace {ws_bytes}")
    assert peak_stream < clip_bytes + ws_bytes
    assert peak_two_step > clip_bytes + ws_bytes                               # the bound tells the two apart
