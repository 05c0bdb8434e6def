"""-m gpu: decode to uint8 frames on the HIP kernels (SURVEY.md §8f N1 + N2 as one path).

* `dawn_final_conv_blend_u8` (the final-conv kernel with the frame egress as its store) against the two kernels it replaces,
  `frames_to_u8(final_conv_blend(...))`, bit for bit: the byte form instantiates the same kernel source up to the blended fp32
  value and applies the same `u8_of`, so there is no tolerance here;
* `FlowDecoder.decode_clip_u8` (fused) against the two-step path, and against the reference's own frames (data-derived +-1 rule);
* the C-side decoder (dawn_decoder_* / dawn_decode_clip, `FlowDecoder.use_ctx`) against the Python orchestration: same kernels, same
  arguments, `torch.equal`; its error returns;
* `stream_frames_u8`: same bytes, and no clip-sized fp32 tensor on the device."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle.ops_ref import RefOps
from test_decode_u8_cpu import assert_bytes_within_reference
from test_hip_flow_decode import motion, random_lfg_state_dict
from test_hip_ops import rnd

pytestmark = pytest.mark.gpu

T = torch.from_numpy


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def _two_step(hip, x, H, W, w7, b3, src, grid, conf, Tn, mean, bgr):
    out = torch.zeros(3, Tn, H, W, device="cuda")
    warped = torch.zeros_like(out)
    hip.final_conv_blend(x, H, W, w7, b3, src, grid, conf, out, warped)
    return hip.frames_to_u8(out, mean=mean, bgr=bgr)


@pytest.mark.parametrize("bgr", [False, True])
@pytest.mark.parametrize("H,W,Cc,h,w", [(32, 32, 16, 8, 8), (40, 72, 64, 10, 18), (128, 128, 64, 32, 32)])
def test_final_conv_blend_u8_bit_exact(hip, H, W, Cc, h, w, bgr):
    """The three shapes of test_final_conv_blend (40 x 72 has tiles cut by the right and the bottom edge), on a frame range of a
    longer clip (strided grid planes, bytes into the middle of a longer frame buffer), with zero mean and with one that pushes
    values across 0 and across 1."""
    Tn, Ttot = 2, 5
    x = rnd(Tn * H * W, Cc, seed=1).cuda()
    w7 = rnd(49, Cc // 4, 3, 4, seed=2, scale=(49 * Cc) ** -0.5).cuda()
    b3 = rnd(3, seed=3).cuda()
    src = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4)).cuda()
    grid, conf = motion(Ttot, h, w, seed=6)
    grid, conf = grid.cuda(), conf.cuda()
    for mean in ((0.0, 0.0, 0.0), (90.0, 0.5, -110.0)):
        want = _two_step(hip, x, H, W, w7, b3, src, grid[:, 1:3], conf[1:3], Tn, mean, bgr)
        frames = torch.full((Ttot, H, W, 3), 77, device="cuda", dtype=torch.uint8)
        hip.final_conv_blend_u8(x, H, W, w7, b3, src, grid[:, 1:3], conf[1:3], frames[1:3], mean=mean, bgr=bgr)
        assert torch.equal(frames[1:3], want), int((frames[1:3] != want).sum())
        assert bool((frames[0] == 77).all()) and bool((frames[3:] == 77).all())          # nothing outside the frame range
        if mean[0]:
            c = want[..., 2 if bgr else 0], want[..., 0 if bgr else 2]
            assert bool((c[0] == 255).any()) and bool((c[1] == 0).any())                  # the clip on both sides is exercised


@pytest.mark.parametrize("bgr", [False, True])
def test_final_conv_blend_u8_byte_boundaries(hip, bgr):
    """The byte-boundary rows of test_frames_to_u8_bit_exact reach the egress through the kernel: identity flow at the image's
    own resolution and occlusion 1 make the blended value the warped source pixel, k/255, (k + 0.999)/255 and the float below k/255."""
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
        want = _two_step(hip, x, H, W, w7, b3, src.cuda(), grid, conf, Tn, mean, bgr)
        frames = torch.empty(Tn, H, W, 3, device="cuda", dtype=torch.uint8)
        hip.final_conv_blend_u8(x, H, W, w7, b3, src.cuda(), grid, conf, frames, mean=mean, bgr=bgr)
        assert torch.equal(frames, want), int((frames != want).sum())
    # ... and they are the bytes numpy's arithmetic makes of the fp32 values that arrived: with occlusion 1 the blended value IS
    # the warped source pixel (wv * 1 + s * 0), which the fp32 kernel also writes as `warped_vid`
    out = torch.zeros(3, Tn, H, W, device="cuda")
    warped = torch.zeros_like(out)
    hip.final_conv_blend(x, H, W, w7, b3, src.cuda(), grid, conf, out, warped)
    assert torch.equal(out, warped)
    exact = (warped[0, 0, 0].cpu() == src[0, 0]).sum() + (warped[1, 0, 1].cpu() == src[1, 1]).sum() + (warped[2, 0, 2].cpu() == src[2, 2]).sum()
    print(f"boundary values that came through the warp unchanged: {int(exact)} of 96")
    for mean in ((0.0, 0.0, 0.0), (1.5, 0.0, -2.25)):
        frames = torch.empty(Tn, H, W, 3, device="cuda", dtype=torch.uint8)
        hip.final_conv_blend_u8(x, H, W, w7, b3, src.cuda(), grid, conf, frames, mean=mean, bgr=bgr)
        assert torch.equal(frames.cpu(), RefOps().frames_to_u8(warped.cpu(), mean=mean, bgr=bgr))


def test_final_conv_blend_u8_rejects_unaligned_width(hip):
    from dawn_pytorch_amd._lib import DawnHipError
    H, W, Cc, Tn = 16, 30, 8, 1
    frames = torch.full((Tn, H, W, 3), 9, device="cuda", dtype=torch.uint8)
    grid, conf = motion(Tn, 4, 5, seed=1)
    with pytest.raises(DawnHipError, match="multiple of 4"):
        hip.final_conv_blend_u8(rnd(Tn * H * W, Cc, seed=1).cuda(), H, W, rnd(49, Cc // 4, 3, 4, seed=2).cuda(), rnd(3, seed=3).cuda(),
                                torch.rand(3, H, W).cuda(), grid.cuda(), conf.cuda(), frames)
    torch.cuda.synchronize()
    assert bool((frames == 9).all())


def _golden():
    g = load_golden("lfg_tiny.npz")
    return g, {k[3:]: T(v) for k, v in g.items() if k.startswith("sd/")}


def _two_step_clip(dec, hip, img, grid, conf, mean, bgr):
    vid = dec.decode_clip(img, grid, conf)["sample_out_vid"]
    return torch.stack([hip.frames_to_u8(v, mean=mean, bgr=bgr) for v in vid])


def test_decode_clip_u8_tiny_golden(hip):
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    g, sd = _golden()
    dec = FlowDecoder(sd, "cuda", ops=hip, chunk=3)
    img, grid, conf = T(g["img"]).cuda(), T(g["grid"]).cuda(), T(g["conf"]).cuda()
    for mean, bgr in (((0.0, 0.0, 0.0), False), ((2.0, 0.0, -3.5), True)):
        got = dec.decode_clip_u8(img, grid, conf, mean=mean, bgr=bgr)
        assert torch.equal(got, _two_step_clip(dec, hip, img, grid, conf, mean, bgr))
        # against the reference's own frames: within 1, and different only where 2e-5 on the fp32 value crosses a byte boundary
        assert_bytes_within_reference(got[0].cpu().numpy(), T(g["sample_out_vid"])[0], mean=mean, bgr=bgr)


def _full_case(H, Tn):
    sd = random_lfg_state_dict(seed=3)
    h = H // 4
    img = torch.rand(1, 3, H, H, generator=torch.Generator().manual_seed(1)).cuda()
    grid, conf = motion(Tn, h, h, seed=2, spread=0.15)
    return sd, img, grid.unsqueeze(0).cuda(), conf.view(1, 1, Tn, h, h).cuda()


@pytest.mark.parametrize("H,Tn,chunk", [(128, 3, 2), (256, 2, 2)])
def test_decode_clip_u8_full_architecture(hip, H, Tn, chunk):
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    sd, img, grid, conf = _full_case(H, Tn)
    dec = FlowDecoder(sd, "cuda", ops=hip, chunk=chunk)
    got = dec.decode_clip_u8(img, grid, conf, mean=(1.0, -2.0, 0.0), bgr=True)
    want = _two_step_clip(dec, hip, img, grid, conf, (1.0, -2.0, 0.0), True)
    assert got.shape == (1, Tn, H, H, 3) and torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("case", ["tiny", 128, 256])
def test_c_side_decoder_equals_python_orchestration(hip, case):
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    if case == "tiny":
        g, sd = _golden()
        img, grid, conf, chunk = T(g["img"]).cuda(), T(g["grid"]).cuda(), T(g["conf"]).cuda(), 2
    else:
        sd, img, grid, conf = _full_case(case, 3)
        chunk = 2
    py = FlowDecoder(sd, "cuda", ops=hip, chunk=chunk)
    cc = FlowDecoder(sd, "cuda", ops=hip, chunk=chunk)
    cc.use_ctx = True
    assert torch.equal(cc.compute_fea(img), py.compute_fea(img))
    a, b = cc.decode_clip(img, grid, conf), py.decode_clip(img, grid, conf)
    for k in ("sample_out_vid", "sample_warped_vid"):
        assert torch.equal(a[k], b[k]), (k, float((a[k] - b[k]).abs().max()))
    kw = dict(mean=(2.0, 0.0, -3.5), bgr=True)
    want = py.decode_clip_u8(img, grid, conf, **kw)
    assert torch.equal(cc.decode_clip_u8(img, grid, conf, **kw), want)
    # both kinds of output in one call: the fp32 kernel, then dawn_frames_to_u8 on each chunk
    ev = cc._evaluator()
    src = img[0].contiguous()
    mem, _ = ev.encode(src)
    Tn, (h, w) = grid.shape[2], grid.shape[3:]
    ov = torch.empty(3, Tn, *src.shape[1:], device="cuda")
    wv, fr = torch.empty_like(ov), torch.empty(Tn, *src.shape[1:], 3, device="cuda", dtype=torch.uint8)
    ev.decode(src, mem, T=Tn, h=h, w=w, chunk=chunk, grid=grid[0], conf=conf[0, 0], out_vid=ov, warped_vid=wv, frames=fr, **kw)
    assert torch.equal(ov, b["sample_out_vid"][0]) and torch.equal(wv, b["sample_warped_vid"][0]) and torch.equal(fr, want[0])


def test_latent_from_dawn_sampler_run_decodes_to_the_same_bytes(hip, tiny):
    """sampler -> decode -> bytes with no tensor algebra in between: the (3,T,h,w) output of dawn_sampler_run handed to
    dawn_decode_clip as is == the Python path fed pred[:, :2] and (pred[:, 2] + 1) * 0.5."""
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
    want = dec.decode_clip_u8(img, pred[:, :2], (pred[:, 2].unsqueeze(1) + 1) * 0.5, mean=(1.0, 0.0, -1.0))
    de = DecoderEvaluator(dec)
    src = img[0].contiguous()
    mem, _ = de.encode(src)
    got = torch.empty(Tn, 32, 32, 3, device="cuda", dtype=torch.uint8)
    de.decode(src, mem, T=Tn, h=h, w=w, chunk=5, latent=latent, frames=got, mean=(1.0, 0.0, -1.0))
    assert torch.equal(got, want[0]), int((got != want[0]).sum())


def test_c_side_decoder_error_returns(hip):
    from dawn_pytorch_amd._lib import DawnHipError
    from dawn_pytorch_amd.ctx import DecoderEvaluator, decoder_named_weights
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    g, sd = _golden()
    dec = FlowDecoder(sd, "cuda", ops=hip)
    names = decoder_named_weights(dec)
    with pytest.raises(DawnHipError, match="bott.0.c2.bias"):
        DecoderEvaluator(dec, weights={k: v for k, v in names.items() if k != "bott.0.c2.bias"})
    de = DecoderEvaluator(dec)
    src = T(g["img"]).cuda()[0].contiguous()
    grid, conf = T(g["grid"]).cuda()[0], T(g["conf"]).cuda()[0, 0]
    mem, _ = de.encode(src)
    frames = torch.full((5, 32, 32, 3), 9, device="cuda", dtype=torch.uint8)
    ov = torch.full((3, 5, 32, 32), 9.0, device="cuda")
    kw = dict(T=5, h=8, w=8, chunk=2, grid=grid, conf=conf)
    with pytest.raises(DawnHipError, match="no output requested"):
        de.decode(src, mem, **kw)
    with pytest.raises(DawnHipError, match="needed"):
        de.decode(src, mem, frames=frames, workspace=torch.empty(4096, device="cuda", dtype=torch.uint8), **kw)
    with pytest.raises(DawnHipError, match="pair"):
        de.decode(src, mem, out_vid=ov, **kw)
    with pytest.raises(DawnHipError, match="4-byte aligned"):               # the byte rows leave as 4-byte stores
        odd = torch.full((5 * 32 * 32 * 3 + 4,), 9, device="cuda", dtype=torch.uint8)[1:1 + 5 * 32 * 32 * 3].view(5, 32, 32, 3)
        de.decode(src, mem, frames=odd, **kw)
    torch.cuda.synchronize()
    assert bool((frames == 9).all()) and bool((ov == 9.0).all())            # nothing was launched
    de.decode(src, mem, frames=frames, **kw)                                # ... and the decoder is still usable
    assert torch.equal(frames, dec.decode_clip_u8(src[None], grid[None], conf[None, None])[0])


def test_c_side_decoder_rejects_widths_that_are_not_a_multiple_of_4(hip):
    """`W % 4 != 0` through the decoder entries: an error with a message and nothing launched.  With two down blocks such a width is
    already no multiple of 2^n_down (the image-size check answers); a decoder with ONE down block accepts W = 30, decodes it to fp32
    like the Python orchestration, and refuses the byte output, whose rows leave as 4-byte stores."""
    import os
    import sys
    from conftest import ROOT
    from dawn_pytorch_amd._lib import DawnHipError
    from dawn_pytorch_amd.ctx import DecoderEvaluator
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_decode
    Tn, H, W = 3, 32, 30
    # (a) the tiny golden decoder, n_down = 2
    _, sd = _golden()
    de = DecoderEvaluator(FlowDecoder(sd, "cuda", ops=hip))
    src = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).cuda()
    with pytest.raises(DawnHipError, match="32x30 is not a positive multiple of 4"):
        de.encode(src)
    grid, conf = motion(Tn, 8, 8, seed=3)
    grid, conf = grid.cuda(), conf.cuda()
    frames = torch.full((Tn, H, W, 3), 9, device="cuda", dtype=torch.uint8)
    ov, wv = torch.full((3, Tn, H, W), 9.0, device="cuda"), torch.full((3, Tn, H, W), 9.0, device="cuda")
    mem = torch.zeros(1 << 20, device="cuda", dtype=torch.uint8)
    ws = torch.zeros(1 << 24, device="cuda", dtype=torch.uint8)
    for kw in (dict(frames=frames), dict(out_vid=ov, warped_vid=wv), dict(frames=frames, out_vid=ov, warped_vid=wv)):
        with pytest.raises(DawnHipError, match="32x30 is not a positive multiple of 4"):
            de.decode(src, mem, T=Tn, h=8, w=8, chunk=2, grid=grid, conf=conf, workspace=ws, **kw)
    # (b) one down block: 32 x 30 is a valid image
    sd1 = bench_decode.lfg_state_dict(5, be=16, max_features=64, n_down=1, n_bott=1)
    dec1 = FlowDecoder(sd1, "cuda", ops=hip, chunk=2)
    de1 = DecoderEvaluator(dec1)
    grid, conf = motion(Tn, 16, 15, seed=4)
    grid, conf = grid.cuda(), conf.cuda()
    mem1, _ = de1.encode(src)
    kw = dict(T=Tn, h=16, w=15, chunk=2, grid=grid, conf=conf)
    for out in (dict(frames=frames), dict(frames=frames, out_vid=ov, warped_vid=wv)):
        with pytest.raises(DawnHipError, match=r"frames_u8 needs W % 4 == 0"):
            de1.decode(src, mem1, **kw, **out)
    latent = torch.cat((grid, conf[None] * 2 - 1), 0).contiguous()
    with pytest.raises(DawnHipError, match=r"dawn_decode_clip: frames_u8 needs W % 4 == 0"):
        de1.decode(src, mem1, T=Tn, h=16, w=15, chunk=2, latent=latent, frames=frames)
    torch.cuda.synchronize()
    assert bool((frames == 9).all()) and bool((ov == 9.0).all()) and bool((wv == 9.0).all())      # nothing was launched
    de1.decode(src, mem1, out_vid=ov, warped_vid=wv, **kw)                                       # fp32 outputs have no such limit
    want = dec1.decode_clip(src[None], grid[None], conf[None, None])
    assert torch.equal(ov, want["sample_out_vid"][0]) and torch.equal(wv, want["sample_warped_vid"][0])


@pytest.mark.parametrize("use_ctx", [False, True])
def test_stream_frames_u8_same_bytes_and_no_clip_sized_tensor(hip, use_ctx):
    """200 frames at 128 x 128 in chunks of 2: one fp32 (3,T,H,W) clip is 39 MB, the chunk's activations about as much.  Streaming
    must stay below ONE such clip plus the chunk workspace (what the C side sizes for the same launch sequence; the Python
    orchestration keeps a few more chunk-sized buffers alive, which the clip-sized margin absorbs) -- the two-step path, which
    materialises two fp32 clips, does not."""
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    H, Tn, chunk = 128, 200, 2
    sd, img, grid, conf = _full_case(H, Tn)
    dec = FlowDecoder(sd, "cuda", ops=hip, chunk=chunk)
    dec.use_ctx = use_ctx
    want = dec.decode_clip_u8(img, grid, conf, mean=(1.0, 0.0, -1.0))[0].cpu().numpy()
    from dawn_pytorch_amd.ctx import DecoderEvaluator
    ws_bytes = DecoderEvaluator(dec).workspace_bytes(H, H, chunk)
    clip_bytes = 3 * Tn * H * H * 4
    if use_ctx:
        dec._evaluator()._ws = None                                            # its workspace counts as well
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    parts, t0s = [], []
    for t0, fr in dec.stream_frames_u8(img, grid, conf, mean=(1.0, 0.0, -1.0)):
        t0s.append(t0)
        parts.append(fr.copy())                                                # valid until the next next() only
    peak_stream = torch.cuda.max_memory_allocated() - base
    assert t0s == list(range(0, Tn, chunk))
    assert np.array_equal(np.concatenate(parts, 0), want)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    two = hip.frames_to_u8(dec.decode_clip(img, grid, conf)["sample_out_vid"][0]).cpu()
    peak_two_step = torch.cuda.max_memory_allocated() - base
    del two
    print(f"peak device bytes: streaming {peak_stream}, two-step {peak_two_step}; one fp32 clip {clip_bytes}, chunk workspace {ws_bytes}")
    assert peak_stream < clip_bytes + ws_bytes
    assert peak_two_step > clip_bytes + ws_bytes                               # the bound tells the two apart
