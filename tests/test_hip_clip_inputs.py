"""-m gpu: the clip-input kernels (csrc/clip_inputs.hip), their stage host and the one-call pipeline (csrc/dawn_inputs.hip).

* `dawn_face_loc_embed` against `Face_loc_Encoder(generate_bbox_mask(...))` in float64 through `split_gate.fp32_gate` (file-wide factor
  and floor), written into planes 256..271 of a guarded (272, h, w) buffer; bit-identical run to run.  The cases:
    fallback           UVG:341's default, a 2x2-pixel mask; the shipped 64x64 output
    odd / even phase   rectangle edges on odd / even rows and columns (the two stride-2 phases); 17x17 output, one past a 16-wide tile
    tile edge          a rectangle ending at 33, straddling an output tile boundary; exactly one tile row
    full, smallest     2x2 output, every value touches padding
    beyond             negative and oversize bounds, truncation toward zero; 9x9 partial tile
    empty              an all-zero mask: the interior is relu(conv2(relu(b1))), the border differs (conv2 pads with zero, not relu(b1))
    corner             one pixel at the last row and column
    non-square source  H_src != W_src
* `dawn_cond_rows` against `FlowDiffusion.assemble_cond`, `torch.equal`: separate inputs at wide strides, fully in place, row 0 as the
  subtrahend in place at T = 1025, columns beyond the row untouched, the appended column +0.0.
* `dawn_clip_inputs` / `FlowDiffusion.inputs_via_c`: the same cond bits; latents within 4x what CPU fp32's own error on bbox_mask does
  to them (both numbers go to clip_inputs_parity.txt beside the op-error log; the measured ones are in profiles/clip_inputs_parity.md).
* `dawn_generate_clip` on tiny models of all five stages against the stages run one by one through the existing evaluators."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from clip_inputs_cases import (BBOX_CASES, COND_POSE, COND_T, N_AUD, cond_inits, cond_inputs, cond_want, encoder_refs, encoder_weights)
from conftest import load_golden
from guarded import GuardedOps
from split_gate import fp32_gate
from test_hip_ops import LOG      # the op-error log of the GPU op tests: figures a test prints go beside it

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def dev_weights(seed=0):
    w = encoder_weights(seed)
    return [w[k].cuda() for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")]


# ---------------------------------------------------------------------------------------------- dawn_face_loc_embed
@pytest.mark.parametrize("name,size,bbox6", BBOX_CASES, ids=[c[0] for c in BBOX_CASES])
def test_face_loc_embed_fp64_gate_guarded_and_deterministic(hip, name, size, bbox6):
    want64, base32 = encoder_refs(name)
    s4 = size // 4
    assert want64.shape == (16, s4, s4)
    g = GuardedOps()
    buf = g.guarded_out(272, s4 * s4, name="fea272")
    buf[:256] = 7.0                                          # the decoder's planes: must come back as they are
    out = buf[256:].view(16, s4, s4)
    w = dev_weights()
    hip.face_loc_embed(bbox6, size, *w, out=out)
    torch.cuda.synchronize()
    g.verify()                                               # bands intact, no element of planes 256..271 left as poison
    assert bool((buf[:256] == 7.0).all()), "planes 0..255 were written"
    rec = fp32_gate(f"face_loc_embed/{name}", out, want64, base32)
    print(f"face_loc_embed/{name}: rel err {rec['rel_err']:.3e}, CPU fp32 {rec['rel_err_cpu_fp32']:.3e}")
    assert torch.equal(hip.face_loc_embed(bbox6, size, *w), out)


# ---------------------------------------------------------------------------------------------- dawn_cond_rows
def _wide(t, pad):
    """t as a column slice of a NaN-filled tensor `pad` columns wider on each side (a stride wider than the width)."""
    big = torch.full((t.shape[0], t.shape[1] + 2 * pad), float("nan"), device="cuda")
    big[:, pad:pad + t.shape[1]] = t.cuda()
    return big[:, pad:pad + t.shape[1]]


@pytest.mark.parametrize("T", COND_T)
@pytest.mark.parametrize("n_pose,n_init", COND_POSE)
def test_cond_rows_separate_inputs_at_wide_strides(hip, T, n_pose, n_init):
    audio, pose, eye = cond_inputs(T, n_pose)
    ip, ie = cond_inits(n_init, with_eye=n_init != 0)                  # n_init = 0: both subtrahends are row 0
    want = cond_want(audio, pose, eye, ip, ie)
    g = GuardedOps()
    out = g.guarded_out(T, want.shape[1], col_pad=4, name="cond")       # ld_cond = width + 8
    got = hip.cond_rows(_wide(audio, 3), _wide(pose, 5), _wide(eye, 1), ip, ie, out=out)
    torch.cuda.synchronize()
    g.verify()
    assert torch.equal(got.cpu(), want)
    if n_pose != (n_init or n_pose):
        col = got[:, N_AUD + n_pose].cpu()
        assert bool((col == 0).all()) and not bool(torch.signbit(col).any()), "the appended column is +0.0"


@pytest.mark.parametrize("T", COND_T)
@pytest.mark.parametrize("n_pose,n_init", COND_POSE)
@pytest.mark.parametrize("col_pad", [0, 4])
def test_cond_rows_fully_in_place(hip, T, n_pose, n_init, col_pad):
    """Inputs are the column views of cond they land in (what the HuBERT and PBnet stages leave): ld_cond = the width (1032 at P = 6)
    and the width + 8.  n_init = 0 has both inits NULL: every row subtracts row 0 while row 0 is overwritten."""
    audio, pose, eye = cond_inputs(T, n_pose)
    ip, ie = cond_inits(n_init, with_eye=n_init != 0)
    want = cond_want(audio, pose, eye, ip, ie)
    P = n_init or n_pose
    g = GuardedOps()
    cond = g.guarded_out(T, N_AUD + P + 2, col_pad=col_pad, name="cond")
    va, vp, ve = cond[:, :N_AUD], cond[:, N_AUD:N_AUD + n_pose], cond[:, N_AUD + P:]
    va.copy_(audio); vp.copy_(pose); ve.copy_(eye)                      # (the appended column, if any, stays poison until the kernel)
    got = hip.cond_rows(va, vp, ve, ip, ie, out=cond)
    torch.cuda.synchronize()
    g.verify()                                                          # columns beyond the row and the bands untouched
    assert got.data_ptr() == cond.data_ptr() and torch.equal(got.cpu(), want)
    assert torch.equal(cond[:, :N_AUD].cpu().view(torch.int32), audio.view(torch.int32)), "audio columns changed"
    if n_pose != P:
        col = got[:, N_AUD + n_pose].cpu()
        assert bool((col == 0).all()) and not bool(torch.signbit(col).any())


def test_cond_rows_one_null_init_each(hip):
    audio, pose, eye = cond_inputs(3, 6)
    for ip, ie in ((cond_inits(6, False)[0], None), (None, cond_inits(0, True)[1])):
        want = cond_want(audio, pose, eye, ip, ie)
        assert torch.equal(hip.cond_rows(audio.cuda(), pose.cuda(), eye.cuda(), ip, ie).cpu(), want)


# ---------------------------------------------------------------------------------------------- dawn_clip_inputs, inputs_via_c
class _StubGenerator:
    """What FlowDiffusion asks of its generator when native_decode is off: 256 feature channels and a per-frame decode."""

    def __init__(self, h):
        self.fea = torch.randn(1, 256, h, h, generator=torch.Generator().manual_seed(4)).cuda()

    def compute_fea(self, img):
        return self.fea

    def forward_with_flow(self, source_image, optical_flow, occlusion_map):
        return {"prediction": source_image, "deformed": source_image}


@pytest.fixture(scope="module")
def tiny_fd():
    from dawn_pytorch_amd.flow_diffusion import FlowDiffusion
    torch.manual_seed(0)
    fd = FlowDiffusion(img_size=8, num_frames=5, sampling_timesteps=2, win_width=3, pose_dim=7, dim_mults=(1, 2),
                       generator=_StubGenerator(8), native_decode=False).cuda().eval()
    fd.face_loc_emb.load_state_dict(encoder_weights(3))
    fd.update_num_frames(5)
    return fd


def _fd_inputs(T=5, size=32):
    g = torch.Generator().manual_seed(9)
    img = torch.rand(1, 3, size, size, generator=g).cuda()
    hub = torch.randn(1, T, 1024, generator=g).cuda()
    pose = (torch.randn(1, 6, T, generator=g) * 10).cuda()              # one column fewer than init_pose: FD:348-349
    eye = torch.rand(1, 2, T, generator=g).cuda()
    bbox = torch.tensor([37.0, 190.0, 21.0, 175.0, 256.0, 256.0]).view(1, 6, 1).cuda()
    ip, ie = (torch.randn(1, 7, generator=g) * 10).cuda(), torch.rand(1, 2, generator=g).cuda()
    return img, hub, pose, eye, bbox, ip, ie


def test_inputs_via_c_same_cond_bits_and_latents_within_the_mask_error(tiny_fd):
    fd = tiny_fd
    img, hub, pose, eye, bbox, ip, ie = _fd_inputs()
    with torch.no_grad():
        fd.inputs_via_c = False
        m_t, c_t = fd.clip_inputs(img, hub, pose, eye, bbox, ip, ie)
        fd.inputs_via_c = True
        m_c, c_c = fd.clip_inputs(img, hub, pose, eye, bbox, ip, ie)
    assert m_c.shape == m_t.shape == (1, 16, 8, 8) and torch.equal(c_c, c_t)
    # the mask's own fp32 error, from the CPU: Face_loc_Encoder in float32 against float64
    import copy
    mask = fd.generate_bbox_mask(bbox, size=32).cpu()
    enc = copy.deepcopy(fd.face_loc_emb).cpu()
    with torch.no_grad():
        base32 = enc(mask)
        want64 = enc.double()(mask.double())
    gen = torch.Generator().manual_seed(5)
    x_init = torch.randn(1, 3, 5, 8, 8, generator=gen).cuda()
    noises = [torch.randn(1, 3, 5, 8, 8, generator=gen).cuda() for _ in range(2)]
    fea = fd.generator.compute_fea(img)
    run = lambda m: fd.diffusion.sample(fea, m, cond=c_t, batch_size=1, cond_scale=1.0, x_init=x_init, noises=noises)   # noqa: E731
    lat_t = run(m_t)
    lat_p = run(m_t + (base32.double() - want64).float().cuda())        # the torch path against itself, bbox_mask off by fp32's error
    lat_c = run(m_c)
    e_ref = float((lat_p - lat_t).abs().max())
    e_c = float((lat_c - lat_t).abs().max())
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(os.path.join(os.path.dirname(LOG), "clip_inputs_parity.txt"), "a") as f:
        f.write(f"max|latent(mask + fp32 error) - latent(mask)| = {e_ref:.6e}   max|latent(via_c) - latent(torch)| = {e_c:.6e}   "
                f"max|mask_c - mask_torch| = {float((m_c - m_t).abs().max()):.6e}\n")
    print(f"inputs_via_c: latents move by {e_c:.3e}; the mask's own fp32 error moves them by {e_ref:.3e}")
    assert torch.isfinite(lat_c).all() and e_c <= 4.0 * e_ref, (e_c, e_ref)
    # and sample_one_video itself takes the C stage: the same latent as diffusion.sample fed the C stage's mask and cond
    fd.diffusion.noise_seed = 3
    out = fd.sample_one_video(img, hub, pose, eye, bbox, 1.0, init_pose=ip, init_eye=ie)
    pred = fd.diffusion.sample(fea, m_c, cond=c_c, batch_size=1, cond_scale=1.0)
    fd.diffusion.noise_seed = None
    assert torch.equal(out["sample_vid_grid"], pred[:, :2])
    fd.inputs_via_c = False


def test_clip_inputs_in_place_on_a_host_buffer(tiny_fd):
    """dawn_clip_inputs the way the pipeline calls it: pose / eye are columns of cond, audio apart, fea272 whole."""
    from dawn_pytorch_amd.ctx import InputsEvaluator
    ev = InputsEvaluator(tiny_fd, n_aud=N_AUD)
    T = 7
    audio, pose, eye = cond_inputs(T, 6)
    ip, ie = cond_inits(7, True)
    g = GuardedOps()
    cond = g.guarded_out(T, N_AUD + 9, name="cond")
    cond[:, N_AUD:N_AUD + 6] = pose.cuda()
    cond[:, N_AUD + 7:] = eye.cuda()
    fea = g.guarded_out(272, 64, name="fea272")
    fea[:256] = 1.5
    bbox6 = [37, 190, 21, 175, 256, 256]
    ev.clip_inputs(bbox6, 32, fea.view(272, 8, 8), audio.cuda(), cond[:, N_AUD:N_AUD + 6], cond[:, N_AUD + 7:], ip, ie, cond=cond)
    torch.cuda.synchronize()
    g.verify()
    assert torch.equal(cond.cpu(), cond_want(audio, pose, eye, ip, ie)) and bool((fea[:256] == 1.5).all())
    w = [tiny_fd.state_dict()[f"face_loc_emb.{k}"] for k in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias")]
    from dawn_pytorch_amd.ops import HipOps
    assert torch.equal(fea[256:].view(16, 8, 8), HipOps().face_loc_embed(bbox6, 32, *w))


# ---------------------------------------------------------------------------------------------- dawn_generate_clip
T_PIPE, S_PIPE, H_PIPE, N_SAMPLES, SEED = 5, 3, 32, 5000, 1234          # ~0.3 s of audio: 7 frames at 25 fps, the clip takes 5


@pytest.fixture(scope="module")
def stages(hip):
    """Tiny models of all five stages that fit together: HuBERT (hidden 128), two PBnets (audio 128, latent 32), the LFG decoder
    (64 feature channels at 8x8 from a 32x32 image), the clip inputs and a UNet (80 fea channels, cond 128 + 6 + 2)."""
    import dawn_pytorch_amd as D
    from dawn_pytorch_amd import ctx
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.flow_diffusion import Face_loc_Encoder
    from dawn_pytorch_amd.hubert import HubertFeatures
    from dawn_pytorch_amd.pbnet import PoseBlinkGenerator
    from dawn_pytorch_amd.sampler import ddim_step_scalars
    from test_hip_pbnet import _random_decoder_sd
    gh = load_golden("hubert_tiny.npz")
    hf = HubertFeatures({k[3:]: torch.from_numpy(v) for k, v in gh.items() if k.startswith("sd/")}, "cuda:0",
                        num_heads=int(gh["num_heads"]), pos_groups=int(gh["pos_groups"]))
    gp = PoseBlinkGenerator(_random_decoder_sd(6, audio_dim=128, latent=32, ff=64, layers=1, seed=1), archiname="transformerreemb6", device="cuda")
    gb = PoseBlinkGenerator(_random_decoder_sd(2, audio_dim=128, latent=32, ff=64, layers=1, seed=2), archiname="transformerreemb5", device="cuda")
    gl = load_golden("lfg_tiny.npz")
    dec = FlowDecoder({k[3:]: torch.from_numpy(v) for k, v in gl.items() if k.startswith("sd/")}, "cuda", ops=hip, chunk=2)
    torch.manual_seed(0)
    unet = D.DynamicNfUnet3D(default_num_frames=T_PIPE, dim=16, cond_dim=136, cond_aud=128, cond_pose=6, cond_eye=2, num_frames=T_PIPE,
                             channels=3 + 64 + 16, out_grid_dim=2, out_conf_dim=1, dim_mults=(1, 2), use_hubert_audio_cond=True,
                             learn_null_cond=False, use_final_activation=False, use_deconv=True, padding_mode="zeros", win_width=3).cuda()
    diff = D.DynamicNfGaussianDiffusion(default_num_frames=T_PIPE, denoise_fn=unet, num_frames=T_PIPE, image_size=8,
                                        sampling_timesteps=S_PIPE, timesteps=1000, loss_type='l2', use_dynamic_thres=True,
                                        null_cond_prob=0.1, ddim_sampling_eta=1.0).cuda()
    steps = ddim_step_scalars({k: getattr(diff, k) for k in ("alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
                                                              "sqrt_recipm1_alphas_cumprod")}, S_PIPE, 1.0)

    class Holder(torch.nn.Module):                      # what inputs_named_weights reads: a module with `face_loc_emb` and `pose_dim`
        def __init__(self):
            super().__init__()
            self.face_loc_emb, self.pose_dim = Face_loc_Encoder(), 6
    fl = Holder().cuda()
    fl.face_loc_emb.load_state_dict(encoder_weights(3))
    ev = dict(hub=hf.evaluator(), pose=gp.c_evaluator(), blink=gb.c_evaluator(), dec=ctx.DecoderEvaluator(dec),
              inp=ctx.InputsEvaluator(fl, n_aud=128), unet=ctx.CtxEvaluator(unet.packed()))
    pipe = ctx.PipelineEvaluator(ev["hub"], ev["pose"], ev["blink"], ev["dec"], ev["inp"], ev["unet"])
    samples = torch.from_numpy(np.ascontiguousarray(gh["speech"][:N_SAMPLES], dtype=np.float32)).cuda()
    img = torch.from_numpy(gl["img"])[0].contiguous().cuda()
    return dict(ev=ev, pipe=pipe, samples=samples, img=img, steps=steps, keep=(hf, gp, gb, dec, unet, fl))


BBOX_PIPE = [37, 190, 21, 175, 256, 256]
INIT_POSE6, INIT_BLINK2 = [3.0, -5.0, 1.0, 4.79e-04, 56.5, 64.9], [0.3, 0.28]


def _stage_by_stage(hip, st, fmt, cond_scale, init_pose, init_eye, mean, bgr, chunk):
    """The pipeline's sequence through the existing evaluators, with the Philox keys include/dawn_hip.h states."""
    from dawn_pytorch_amd import ctx
    ev, T, h = st["ev"], T_PIPE, H_PIPE // 4
    _, audio = ev["hub"].features(st["samples"], want_hidden=False)
    assert audio.shape[0] >= T
    zp = hip.philox_normal(1, T, 0, T, 32, SEED, ctx.Z_POSE_STREAM, "cuda").view(T, 32)
    zb = hip.philox_normal(1, T, 0, T, 32, SEED, ctx.Z_BLINK_STREAM, "cuda").view(T, 32)
    cond = torch.full((T, 136), float("nan"), device="cuda")
    ctx.pose_blink_stage_c(ev["pose"], ev["blink"], audio[:T], INIT_POSE6, INIT_BLINK2, zp, zb, dri_pose=cond[:, 128:134],
                           dri_blink=cond[:, 134:136])
    mem, fea = ev["dec"].encode(st["img"], want_fea=True)
    fea272 = torch.cat((fea, torch.full((16, h, h), float("nan"), device="cuda")), 0).contiguous()
    ev["inp"].clip_inputs(BBOX_PIPE, H_PIPE, fea272, audio[:T], cond[:, 128:134], cond[:, 134:136], init_pose, init_eye, cond=cond)
    clip = ev["unet"].prepare_clip(fea272, cond)
    null = ev["unet"].prepare_null_clip(fea272, T) if cond_scale != 1.0 else None
    x_init = hip.philox_normal(3, T, 0, T, h * h, SEED, 0, "cuda").view(3, T, h, h)
    latent = ev["unet"].sample(clip, x_init, st["steps"], seed=SEED, null_clip=null, cond_scale=cond_scale)
    if fmt == "yuv420p":
        frames = torch.empty(T, H_PIPE * H_PIPE * 3 // 2, dtype=torch.uint8, device="cuda")
        ev["dec"].decode(st["img"], mem, T=T, h=h, w=h, chunk=chunk, latent=latent, yuv=frames, mean=mean)
    else:
        frames = torch.empty(T, H_PIPE, H_PIPE, 3, dtype=torch.uint8, device="cuda")
        ev["dec"].decode(st["img"], mem, T=T, h=h, w=h, chunk=chunk, latent=latent, frames=frames, mean=mean, bgr=bgr)
    return frames, latent, cond


@pytest.mark.parametrize("fmt,cond_scale,with_init", [("rgb", 1.0, True), ("rgb", 2.0, False), ("yuv420p", 1.0, False), ("yuv420p", 2.0, True)])
def test_generate_clip_equals_the_stages_one_by_one(hip, stages, fmt, cond_scale, with_init):
    st = stages
    init_pose, init_eye = cond_inits(6, True) if with_init else (None, None)
    mean, bgr, chunk = (2.0, 0.0, -3.5), fmt == "rgb" and with_init, 2
    want_frames, want_latent, want_cond = _stage_by_stage(hip, st, fmt, cond_scale, init_pose, init_eye, mean, bgr, chunk)
    a = st["pipe"].args(st["samples"], st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], init_pose=init_pose,
                        init_eye=init_eye, cond_scale=cond_scale, seed=SEED, fmt=fmt, mean=mean, bgr=bgr, chunk=chunk)
    out = st["pipe"].generate(a, want_latent=True, want_cond=True)
    torch.cuda.synchronize()
    assert torch.equal(out["cond"], want_cond), float((out["cond"] - want_cond).abs().max())
    assert torch.equal(out["latent"], want_latent), float((out["latent"] - want_latent).abs().max())
    assert out["frames"].shape == want_frames.shape and torch.equal(out["frames"], want_frames), int((out["frames"] != want_frames).sum())
    # without the optional outputs: cond and the latent live in the workspace; the same bytes
    b = st["pipe"].args(st["samples"], st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], init_pose=init_pose,
                        init_eye=init_eye, cond_scale=cond_scale, seed=SEED, fmt=fmt, mean=mean, bgr=bgr, chunk=chunk)
    assert torch.equal(st["pipe"].generate(b)["frames"], want_frames)


def test_generate_bytes_sum_rule_and_short_workspace(stages):
    """dawn_generate_bytes >= its fixed buffers + each single stage's own query; one byte less is refused with nothing launched."""
    from dawn_pytorch_amd import _lib
    st, L = stages, _lib.lib()
    ev, T, H, h = st["ev"], T_PIPE, H_PIPE, H_PIPE // 4
    a = st["pipe"].args(st["samples"], st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T, st["steps"], cond_scale=2.0, seed=SEED, chunk=2)
    clip_bytes, need = st["pipe"].sizes(a)
    assert clip_bytes == T * H * H * 3
    nf = int(N_SAMPLES / 16000 * 25)
    fixed = 4 * (T * 136 + 136 + 80 * h * h + nf * 128 + 2 * T * 32 + 2 * 3 * T * h * h) + int(L.dawn_decoder_skip_bytes(ev["dec"].h, H, H)) \
        + 2 * int(L.dawn_clip_bytes(ev["unet"].h, T, h, h))
    for own in (ev["hub"].workspace_bytes(N_SAMPLES), int(L.dawn_pose_blink_workspace_bytes(ev["pose"].h, ev["blink"].h, T)),
                ev["dec"].workspace_bytes(H, H, 2), int(L.dawn_workspace_bytes_guided(ev["unet"].h, T, h, h, 0, 1))):
        assert own > 0 and need >= fixed + own, (need, fixed, own)
    g = GuardedOps()
    frames = g.guarded_out(T, H * H * 3, name="frames", dtype=torch.uint8)
    latent = g.guarded_out(3 * T, h * h, name="latent")
    cond = g.guarded_out(T, 136, name="cond")
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    a.frames_out, a.latent_out, a.cond_out = frames.data_ptr(), latent.data_ptr(), cond.data_ptr()
    _, need2 = st["pipe"].sizes(a)                                       # cond and the latent are the caller's now
    assert need2 < need
    stream = torch.cuda.current_stream().cuda_stream
    assert L.dawn_generate_clip(C.addressof(a), ws.data_ptr(), need2 - 1, stream) != 0
    assert "workspace" in L.dawn_last_error().decode() and "dawn_generate_bytes" in L.dawn_last_error().decode()
    a.T = 8                                                              # above the 7 frames the audio yields
    assert L.dawn_generate_clip(C.addressof(a), ws.data_ptr(), need, stream) != 0 and "audio yields" in L.dawn_last_error().decode()
    a.T = T
    torch.cuda.synchronize()
    for r in g.outs:                                                     # outputs still poison, bands intact, workspace untouched
        r.check_surroundings("write outside the buffer")
        p = r.payload
        assert bool(torch.isnan(p).all()) if p.dtype.is_floating_point else bool((p == 255).all()), r.name
    assert not bool(ws.any())
    assert L.dawn_generate_clip(C.addressof(a), ws.data_ptr(), need2, stream) == 0, L.dawn_last_error().decode()
    torch.cuda.synchronize()
    for r in g.outs:                                                     # everything written (a byte may be 255: only the fp32 outputs
        r.check_surroundings("write outside the buffer")                 # are asked for poison), nothing outside
        assert not r.payload.dtype.is_floating_point or not bool(torch.isnan(r.payload).any()), r.name
    want = st["pipe"].generate(st["pipe"].args(st["samples"], st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T, st["steps"], cond_scale=2.0,
                                               seed=SEED, chunk=2))["frames"]
    assert torch.equal(frames.view(T, H, H, 3), want)
