"""-m gpu: the media ingest (csrc/media_ingest.hip) and the pipeline from decoded media (dawn_generate_clip_media).

* `dawn_image_ingest` on every case of tests/ingest_cases.py: `torch.equal` with the Pillow-made golden bytes / 255 (integers in,
  integers out: no tolerance), written into a guarded buffer, bit-identical run to run; all 256 byte values through the division; the
  byte layouts (BGR, a fourth byte, grey, padded rows, an odd start address); a plane stride wider than the plane; the workspace of
  exactly `dawn_image_ingest_workspace_bytes` between guard bands.
* `dawn_pcm16_to_samples` against `pcm[:, 0].float() / 32768` from a source that is 2- but not 4-byte aligned.
* `dawn_generate_clip_media` on the tiny five-stage models of tests/test_hip_clip_inputs.py: bit-identical to `dawn_generate_clip` fed
  with the two conversions' outputs, and to `dawn_generate_clip` itself without media.
* `VideoGenerator(image_via_c=True)`: the same frames, and the same audio features, as the default path."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden
from guarded import GuardedOps
from ingest_cases import CASES, formula, parts_of, source
from test_hip_clip_inputs import BBOX_PIPE, H_PIPE, INIT_BLINK2, INIT_POSE6, N_SAMPLES, SEED, T_PIPE, hip, stages  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("image_ingest.npz")


def planes(bytes_hwc):
    """(Ho, Wo, 3) uint8 -> the (3, Ho, Wo) fp32 planes ToTensor() makes of them."""
    return (torch.from_numpy(np.ascontiguousarray(bytes_hwc)).permute(2, 0, 1).float() / 255).contiguous()


def device_source(name):
    Hs, Ws, _, _, kind = CASES[name]
    if name == "very_long_support":                          # 25 MB: made on the device by the same formula
        return formula(Hs, Ws, 3, xp=torch, device="cuda").to(torch.uint8)
    return torch.from_numpy(source(name)).cuda()


# ---------------------------------------------------------------------------------------------- dawn_image_ingest
@pytest.mark.parametrize("name", list(CASES))
def test_image_ingest_equals_pillow_guarded_and_deterministic(hip, golden, name):
    Hs, Ws, Ho, Wo, _ = CASES[name]
    src = device_source(name)
    assert src.shape == (Hs, Ws, 3) and src.dtype == torch.uint8
    if name == "very_long_support":                          # the device formula is the host's
        rows = [0, 1, 1079, 2159]
        assert torch.equal(src[rows].cpu(), torch.from_numpy(formula(Hs, Ws)[rows].astype(np.uint8)))
    g = GuardedOps()
    out = g.guarded_out(3, Ho * Wo, name="out3").view(3, Ho, Wo)
    hip.image_ingest(src, Ho, Wo, out=out)
    torch.cuda.synchronize()
    g.verify()                                               # bands intact, no element left as poison
    got = out.cpu()
    for key, part in parts_of(name, got.permute(1, 2, 0)).items():
        want = torch.from_numpy(golden[key]).float() / 255
        assert torch.equal(part, want), (key, int((part != want).sum()), float((part - want).abs().max()) * 255)
    assert torch.equal(hip.image_ingest(src, Ho, Wo), out)


def test_every_byte_value_divides_as_totensor(hip):
    src = torch.arange(256, dtype=torch.uint8).view(16, 16).cuda()
    got = hip.image_ingest(src, 16, 16)
    want = (torch.arange(256, dtype=torch.uint8).float() / 255).view(1, 16, 16).expand(3, 16, 16)
    assert torch.equal(got.cpu(), want)
    # ... times 255 it is the byte again, exactly, on the device too: what VideoGenerator(image_via_c=True) relies on (UVG:325)
    assert torch.equal((got * 255).cpu(), torch.arange(256, dtype=torch.float32).view(1, 16, 16).expand(3, 16, 16))


def test_image_ingest_byte_layouts(hip, golden):
    name = "fractional_shrink"
    Hs, Ws, Ho, Wo, _ = CASES[name]
    a = source(name)
    want = planes(golden[name])
    rgb = torch.from_numpy(a).cuda()
    run = lambda src, **kw: hip.image_ingest(src, Ho, Wo, **kw).cpu()       # noqa: E731
    assert torch.equal(run(rgb), want)
    # BGR bytes, order="bgr": the planes still come out R, G, B
    assert torch.equal(run(rgb.flip(2).contiguous(), order="bgr"), want)
    assert torch.equal(run(rgb, order="bgr"), want.flip(0))
    # a fourth byte, 255 in a pattern: it must not leak into any plane
    y, x = np.arange(Hs).reshape(-1, 1), np.arange(Ws).reshape(1, -1)
    alpha = (((y + x) % 2) * 255).astype(np.uint8)[:, :, None]
    rgbx = torch.from_numpy(np.concatenate((a, alpha), 2)).cuda()
    assert torch.equal(run(rgbx), want)
    bgrx = torch.cat((rgb.flip(2), rgbx[:, :, 3:]), 2).contiguous()
    assert torch.equal(run(bgrx, order="bgr"), want)
    # grey: three equal planes, each what the resample makes of the one channel
    grey = run(rgb[:, :, 1].contiguous())
    assert torch.equal(grey[0], want[1]) and torch.equal(grey[1], want[1]) and torch.equal(grey[2], want[1])
    # rows 5 bytes wider than the pixels, the padding 0xFF: it must not be read into a result
    wide = torch.full((Hs, Ws * 3 + 5), 255, dtype=torch.uint8, device="cuda")
    wide[:, :Ws * 3] = rgb.view(Hs, Ws * 3)
    padded = wide[:, :Ws * 3].view(Hs, Ws, 3)
    assert padded.stride(0) == Ws * 3 + 5
    assert torch.equal(run(padded), want)
    # the source starts at an odd byte inside a larger guarded buffer (0xFF around it) and its rows are 5 bytes apart from dense
    g = GuardedOps()
    flat = torch.full((1 + Hs * (Ws * 3 + 5) + 6,), 255, dtype=torch.uint8)
    body = flat[1:1 + Hs * (Ws * 3 + 5)].view(Hs, Ws * 3 + 5)
    body[:, :Ws * 3] = torch.from_numpy(a).view(Hs, Ws * 3)
    dev, _ = g.guarded_in(flat, name="src")
    odd = dev[1:1 + Hs * (Ws * 3 + 5)].view(Hs, Ws * 3 + 5)[:, :Ws * 3].view(Hs, Ws, 3)
    assert odd.data_ptr() % 2 == 1
    assert torch.equal(run(odd), want)
    dense_odd = g.guarded_in(torch.cat((torch.full((3,), 255, dtype=torch.uint8), torch.from_numpy(a).flatten())), name="src3")[0]
    assert torch.equal(run(dense_odd[3:].view(Hs, Ws, 3)), want)
    torch.cuda.synchronize()
    g.inputs_intact()


def test_image_ingest_plane_stride_wider_than_the_plane(hip, golden):
    for name in ("ragged_out", "identity", "horizontal_only"):
        Hs, Ws, Ho, Wo, _ = CASES[name]
        g = GuardedOps()
        out = g.guarded_out(3, Ho * Wo, col_pad=4, name="out3")          # plane = Ho Wo + 8 floats; the gap holds the pattern
        assert out.stride(0) == Ho * Wo + 8
        hip.image_ingest(torch.from_numpy(source(name)).cuda(), Ho, Wo, out=out.view(3, Ho, Wo))
        torch.cuda.synchronize()
        g.verify()                                                       # the gap floats are as they were
        assert torch.equal(out.view(3, Ho, Wo).cpu(), planes(golden[name])), name


@pytest.mark.parametrize("name", ["fractional_shrink", "long_support", "horizontal_only", "vertical_only", "identity"])
def test_image_ingest_stays_inside_its_workspace(golden, name):
    """The C entry point with a workspace of exactly dawn_image_ingest_workspace_bytes between guard bands."""
    from dawn_pytorch_amd import _lib
    L = _lib.lib()
    Hs, Ws, Ho, Wo, _ = CASES[name]
    need = int(L.dawn_image_ingest_workspace_bytes(Hs, Ws, Ho, Wo))
    g = GuardedOps()
    ws = g.guarded_out(1, need, name="workspace", dtype=torch.uint8)
    out = g.guarded_out(3, Ho * Wo, name="out3")
    src = torch.from_numpy(source(name)).cuda()
    rc = L.dawn_image_ingest(src.data_ptr(), Hs, Ws, Ws * 3, 3, 0, Ho, Wo, out.data_ptr(), Ho * Wo, ws.data_ptr(), need,
                             torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.dawn_last_error().decode()
    torch.cuda.synchronize()
    for r in g.outs:
        r.check_surroundings("write outside the buffer")
    assert torch.equal(out.view(3, Ho, Wo).cpu(), planes(golden[name]))


# ---------------------------------------------------------------------------------------------- dawn_pcm16_to_samples
@pytest.mark.parametrize("n", [1, 3, 1025])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_pcm16_to_samples_channel_0_exact(n, channels):
    i = np.arange(n * channels).reshape(n, channels)
    pcm = ((i * 7919 + 12345) % 65536 - 32768).astype(np.int16)          # the other channels: a pattern that would show
    edge = np.array([-32768, 32767, 0, 1, -1], dtype=np.int16)
    pcm[:, 0] = np.resize(edge, n) if n > 1 else edge[:1]
    if n > 5:
        pcm[5:, 0] = ((np.arange(n - 5) * 977) % 65536 - 32768).astype(np.int16)
    buf = torch.zeros(n * channels + 1, dtype=torch.int16, device="cuda")
    buf[1:] = torch.from_numpy(pcm).flatten().cuda()
    src = buf[1:].view(n, channels) if channels > 1 else buf[1:]
    assert src.data_ptr() % 4 == 2                                       # 2- but not 4-byte aligned
    g = GuardedOps()
    got = g.pcm16_to_samples(src)
    torch.cuda.synchronize()
    g.verify()
    want = torch.from_numpy(pcm)[:, 0].float() / 32768
    assert got.shape == (n,) and torch.equal(got.cpu(), want)
    assert torch.equal(want.double(), torch.from_numpy(pcm)[:, 0].double() / 32768)      # exact in fp32: soundfile's float64 value


# ---------------------------------------------------------------------------------------------- dawn_generate_clip_media
def _media_inputs(st):
    """A 45 x 60 RGB source by the formula and stereo PCM whose channel 0 is the golden speech at 16 bits."""
    image = torch.from_numpy(formula(45, 60).astype(np.uint8)).cuda()
    ch0 = torch.clamp(torch.round(st["samples"].cpu() * 32768), -32768, 32767).to(torch.int16)
    ch1 = ((torch.arange(N_SAMPLES) * 7919) % 65536 - 32768).to(torch.int16)
    return image, torch.stack((ch0, ch1), 1).contiguous().cuda()


def test_generate_clip_media_equals_generate_clip_on_the_converted_inputs(hip, stages):
    st, pipe = stages, stages["pipe"]
    image, pcm = _media_inputs(st)
    img3 = hip.image_ingest(image, H_PIPE, H_PIPE)
    samples = hip.pcm16_to_samples(pcm)
    kw = dict(cond_scale=2.0, seed=SEED, chunk=2)
    want = pipe.generate(pipe.args(samples, img3, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], **kw), want_latent=True,
                         want_cond=True)
    a = pipe.args(None, None, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], H=H_PIPE, **kw)
    m = pipe.from_media(a, image=image, pcm=pcm)
    got = pipe.generate_media(m, want_latent=True, want_cond=True)
    torch.cuda.synchronize()
    for k in ("cond", "latent", "frames"):
        assert torch.equal(got[k], want[k]), k
    # one of the two only: BGR bytes with fp32 samples, PCM with a planar image
    b = pipe.args(samples, None, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], H=H_PIPE, **kw)
    assert torch.equal(pipe.generate_media(pipe.from_media(b, image=image.flip(2).contiguous(), order="bgr"))["frames"], want["frames"])
    c = pipe.args(None, img3, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], **kw)
    assert torch.equal(pipe.generate_media(pipe.from_media(c, pcm=pcm))["frames"], want["frames"])
    # sizes: dawn_generate_bytes plus the three pieces, each rounded up to 256 bytes
    from dawn_pytorch_amd import _lib
    a256 = lambda n: (n + 255) // 256 * 256                              # noqa: E731
    plain = pipe.args(samples, img3, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], **kw)
    ingest = int(_lib.lib().dawn_image_ingest_workspace_bytes(45, 60, H_PIPE, H_PIPE))
    fresh = pipe.args(None, None, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], H=H_PIPE, **kw)
    assert pipe.media_sizes(pipe.from_media(fresh, image=image, pcm=pcm)) == \
        (pipe.sizes(plain)[0], pipe.sizes(plain)[1] + a256(3 * H_PIPE * H_PIPE * 4) + a256(N_SAMPLES * 4) + a256(ingest))


def test_generate_clip_media_without_media_is_generate_clip_and_refusals(stages):
    from dawn_pytorch_amd import _lib
    st, pipe, L = stages, stages["pipe"], _lib.lib()
    mk = lambda: pipe.args(st["samples"], st["img"], BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], seed=SEED, chunk=2)     # noqa: E731
    want = pipe.generate(mk(), want_latent=True, want_cond=True)
    a = mk()
    m = pipe.from_media(a)
    assert pipe.media_sizes(m) == pipe.sizes(a)
    got = pipe.generate_media(m, want_latent=True, want_cond=True)
    torch.cuda.synchronize()
    for k in ("cond", "latent", "frames"):
        assert torch.equal(got[k], want[k]), k
    # a workspace one byte short, and T above what the PCM yields: refused with nothing launched
    image, pcm = _media_inputs(st)
    b = pipe.args(None, None, BBOX_PIPE, INIT_POSE6, INIT_BLINK2, T_PIPE, st["steps"], H=H_PIPE, seed=SEED, chunk=2)
    mb = pipe.from_media(b, image=image, pcm=pcm)
    g = GuardedOps()
    frames = g.guarded_out(T_PIPE, H_PIPE * H_PIPE * 3, name="frames", dtype=torch.uint8)
    b.frames_out = frames.data_ptr()
    _, need = pipe.media_sizes(mb)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert L.dawn_generate_clip_media(C.addressof(mb), ws.data_ptr(), need - 1, stream) != 0
    e = L.dawn_last_error().decode()
    assert "workspace" in e and "dawn_generate_media_bytes" in e and str(need) in e and str(need - 1) in e
    b.T = 8
    assert L.dawn_generate_clip_media(C.addressof(mb), ws.data_ptr(), need, stream) != 0 and "audio yields" in L.dawn_last_error().decode()
    b.T = T_PIPE
    mb.pix_bytes = 2
    assert L.dawn_generate_clip_media(C.addressof(mb), ws.data_ptr(), need, stream) != 0 and "pix_bytes = 2" in L.dawn_last_error().decode()
    mb.pix_bytes = 3
    torch.cuda.synchronize()
    assert not bool(ws.any()) and bool((frames == 255).all())
    assert L.dawn_generate_clip_media(C.addressof(mb), ws.data_ptr(), need, stream) == 0, L.dawn_last_error().decode()
    torch.cuda.synchronize()
    for r in g.outs:
        r.check_surroundings("write outside the buffer")


# ---------------------------------------------------------------------------------------------- VideoGenerator(image_via_c=True)
def rng_features(Tn):
    return np.random.default_rng(7).standard_normal((Tn, 1024)).astype(np.float32)


@pytest.fixture(scope="module")
def vg_runs(tmp_path_factory):
    """One VideoGenerator on the random-init shipped architectures (as tests/test_hip_end2end.py builds it), a 150 x 150 PNG and a stereo
    16 kHz WAV, run with image_via_c off and on: {via_c: (audio features, source image handed to the sampler, frame bytes)}."""
    import argparse
    import os
    import sys
    import wave
    from PIL import Image
    from conftest import ROOT
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_decode
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    from dawn_pytorch_amd.hubert import HubertFeatures
    from dawn_pytorch_amd.video_generator import VideoGenerator
    tmp_path = tmp_path_factory.mktemp("vg")
    res, Tn = 128, 6
    rng = np.random.default_rng(0)
    gh = load_golden("hubert_tiny.npz")
    hub = HubertFeatures({k[3:]: torch.from_numpy(v) for k, v in gh.items() if k.startswith("sd/")}, "cuda:0",
                         num_heads=int(gh["num_heads"]), pos_groups=int(gh["pos_groups"]))
    n = 6000
    pcm = np.stack(((np.sin(np.arange(n) * 0.05) * 9000 + rng.standard_normal(n) * 800).astype("<i2"),
                    (rng.standard_normal(n) * 3000).astype("<i2")), 1)
    pcm[:3, 0] = (-32768, 32767, 0)
    wav = tmp_path / "a.wav"
    with wave.open(str(wav), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(16000); f.writeframes(pcm.tobytes())
    cache, outd = tmp_path / "cache", tmp_path / "out"
    cache.mkdir()
    np.save(cache / "dri_pose.npy", rng.standard_normal((Tn, 6)).astype(np.float32))
    np.save(cache / "dri_blink.npy", rng.random((Tn, 2)).astype(np.float32))
    img = tmp_path / "face.png"
    Image.fromarray(formula(150, 150).astype(np.uint8)).save(img)
    cfg = {"input_size": res, "max_n_frames": 200, "random_seed": 1234, "mean": [0.0, 0.0, 0.0], "win_width": 40,
           "sampling_step": 2, "ddim_sampling_eta": 1.0, "cond_scale": 1.0, "model_config": {"is_train": True, "pose_dim": 6}}
    args = argparse.Namespace(audio_path=str(wav), image_path=str(img), output_path=str(outd), cache_path=str(cache), resolution=res)
    dec = FlowDecoder(bench_decode.lfg_state_dict(0), "cuda:0")
    vg = VideoGenerator(args, generator=dec, config=cfg, device="cuda:0", allow_random_weights=True, hubert=hub)
    assert vg.image_via_c is False and VideoGenerator(args, generator=dec, config=cfg, device="cuda:0", allow_random_weights=True,
                                                      image_via_c=True).image_via_c is True
    seen = []
    inner = vg.video_model.sample_one_video
    vg.video_model.sample_one_video = lambda *a, **kw: (seen.append(kw["sample_img"].clone()), inner(*a, **kw))[1]
    out = {}
    for via_c in (False, True):
        vg.image_via_c = via_c
        vg.process_audio()                                   # the tiny HuBERT's features of the WAV's channel 0
        feats = np.load(cache / "target_audio.npy")
        np.save(cache / "target_audio.npy", rng_features(Tn))            # what the (1024-wide) denoiser is fed: the same both times
        frames = vg.generate_final_video()
        out[via_c] = (feats, seen[-1].cpu(), frames)
    return dict(out=out, n=n, Tn=Tn, res=res, png=str(img))


def test_video_generator_image_via_c_same_features_and_source_image(vg_runs):
    """`image_via_c` changes where the conversions run: the audio features are the same bits, and the source image handed to the sampler
    is the default path's bit for bit -- the bytes of the host resize, through the reference's own `* 255` (UVG:325) and `.cuda() / 255.`
    (UVG:372).  On the device that division by a Python scalar is a multiplication by fl(1 / 255): within one ulp of byte / 255."""
    from PIL import Image
    out, res = vg_runs["out"], vg_runs["res"]
    assert out[True][0].shape[0] == int(vg_runs["n"] / 16000 * 25) and np.array_equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])
    host = torch.from_numpy(np.array(Image.open(vg_runs["png"]).convert("RGB").resize((res, res), Image.BILINEAR))).permute(2, 0, 1)
    assert torch.equal(torch.round(out[True][1] * 255).to(torch.uint8), host.unsqueeze(0))
    assert torch.equal(out[True][1], host.unsqueeze(0).float() * torch.tensor(1.0 / 255.))
    ulp = (out[True][1].view(torch.int32) - (host.float() / 255).unsqueeze(0).view(torch.int32)).abs()
    assert int(ulp.max()) <= 1


def test_video_generator_image_via_c_same_frame_bytes(vg_runs):
    """With a 150 x 150 PNG, `image_via_c=True` yields the same frame bytes as the default path on the same seed."""
    out, Tn, res = vg_runs["out"], vg_runs["Tn"], vg_runs["res"]
    a, b = out[True][2], out[False][2]
    assert a.shape == b.shape == (Tn, res, res, 3)
    d = np.abs(a.astype(int) - b.astype(int))
    print(f"frames: {int((d != 0).sum())} of {d.size} bytes differ, by at most {int(d.max())} levels")
    assert np.array_equal(a, b)
