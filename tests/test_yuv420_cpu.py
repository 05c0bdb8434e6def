"""Decode to yuv420p frames on CPU: `egress.yuv420_from_rgb_u8`, `FlowDecoder.decode_clip_yuv420` / `stream_frames_yuv420`,
`FlowDiffusion.sample_one_video(frames_u8=dict(format="yuv420p"))` and `VideoGenerator(video_egress="yuv420p")`, driven by the torch
op set (oracle/ops_ref.RefOps, which has no yuv kernel: the decoder composes final_conv_blend -> frames_to_u8 -> egress.py), plus the
no-GPU checks of the new C entry points.

Every expected value is `yuv420_np` below, a numpy restatement of the definition (include/dawn_hip.h, dawn_frames_to_yuv420) that shares
nothing with egress.py, applied to RGB bytes of code that predates the format (RefOps.frames_to_u8, decode_clip_u8).  Every comparison
is integer equality.  The kernels run in tests/test_hip_yuv420.py, which imports `yuv420_np` from here."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from oracle.ops_ref import RefOps
from dawn_pytorch_amd.egress import yuv420_from_rgb_u8
from dawn_pytorch_amd.flow_decoder import FlowDecoder

T = torch.from_numpy
NEW_SYMBOLS = ("dawn_frames_to_yuv420", "dawn_final_conv_blend_yuv420", "dawn_decode_clip_yuv420", "dawn_decode_clip_conf_yuv420")
ANCHORS = {(0, 0, 0): (16, 128, 128), (255, 255, 255): (235, 128, 128), (255, 0, 0): (82, 90, 240), (0, 0, 255): (41, 240, 110),
           (0, 255, 0): (144, 54, 34)}


def yuv420_np(rgb):
    """The definition, restated: rgb (T,H,W,3) uint8 in RGB order -> (T, 3HW/2) uint8, per frame Y (H*W), U (H/2*W/2), V (same).
    numpy's >> on signed integers is an arithmetic shift."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 4 and rgb.shape[3] == 3
    n, H, W, _ = rgb.shape
    assert H % 2 == 0 and W % 4 == 0
    c = rgb.astype(np.int32)
    y = ((66 * c[..., 0] + 129 * c[..., 1] + 25 * c[..., 2] + 128) >> 8) + 16
    b = c[:, 0::2, 0::2] + c[:, 0::2, 1::2] + c[:, 1::2, 0::2] + c[:, 1::2, 1::2]          # rows 2i, 2i+1 x cols 2j, 2j+1
    b = (b + 2) >> 2
    u = ((-38 * b[..., 0] - 74 * b[..., 1] + 112 * b[..., 2] + 128) >> 8) + 128
    v = ((112 * b[..., 0] - 94 * b[..., 1] - 18 * b[..., 2] + 128) >> 8) + 128
    for p, lo, hi in ((y, 16, 235), (u, 16, 240), (v, 16, 240)):
        assert p.min() >= lo and p.max() <= hi
    return np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], 1).astype(np.uint8)


def planes(yuv, H, W):
    """(T, 3HW/2) -> Y (T,H,W), U, V (T,H/2,W/2) by the layout's offsets, stated here a second time."""
    n = yuv.shape[0]
    assert yuv.shape == (n, H * W + 2 * (H // 2) * (W // 2))
    q = (H // 2) * (W // 2)
    return (yuv[:, :H * W].reshape(n, H, W), yuv[:, H * W:H * W + q].reshape(n, H // 2, W // 2),
            yuv[:, H * W + q:H * W + 2 * q].reshape(n, H // 2, W // 2))


@pytest.fixture(scope="module")
def lfg():
    g = load_golden("lfg_tiny.npz")
    sd = {k[3:]: T(v) for k, v in g.items() if k.startswith("sd/")}
    return g, sd


def test_restatement_anchors():
    for rgb, yuv in ANCHORS.items():
        img = np.broadcast_to(np.array(rgb, dtype=np.uint8), (1, 2, 4, 3))
        y, u, v = planes(yuv420_np(img), 2, 4)
        assert (int(y[0, 0, 0]), int(u[0, 0, 0]), int(v[0, 0, 0])) == yuv, rgb
        assert (y == yuv[0]).all() and (u == yuv[1]).all() and (v == yuv[2]).all()


def test_all_colours_luma_and_range():
    """All 2^24 colours, one per pixel, laid out along rows (16 frames of 2 x 2^19): Y of every colour, and its range [16,235] (the
    restatement asserts the ranges).  Each 2x2 block holds four different colours, so chroma is compared on them as well."""
    k = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(k >> 16) & 255, (k >> 8) & 255, k & 255], -1).astype(np.uint8).reshape(16, 2, 1 << 19, 3)
    got = yuv420_from_rgb_u8(T(rgb)).numpy()
    want = yuv420_np(rgb)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    y = planes(got, 2, 1 << 19)[0]
    assert y.min() == 16 and y.max() == 235


def test_anchors_and_chroma_extremes():
    """The five anchors as uniform images, and the eight corners of the colour cube (the extremes of every linear form): U and V stay in
    [16,240] and reach both ends."""
    corners = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]
    rgb = np.stack([np.broadcast_to(np.array(c, dtype=np.uint8), (2, 4, 3)) for c in corners])
    got = yuv420_from_rgb_u8(T(rgb)).numpy()
    assert np.array_equal(got, yuv420_np(rgb))
    y, u, v = planes(got, 2, 4)
    for i, c in enumerate(corners):
        if c in ANCHORS:
            assert (int(y[i, 0, 0]), int(u[i, 0, 0]), int(v[i, 0, 0])) == ANCHORS[c], c
    assert set(ANCHORS) <= set(corners)
    assert u.min() == 16 and u.max() == 240 and v.min() == 16 and v.max() == 240


def test_block_sums_hit_every_residue_mod_4():
    """2x2 blocks whose channel sums are 4q + r for every r (and q at both ends of the range): the +2 >> 2 rounding of the average."""
    blocks = []
    for base in (0, 100, 254):
        for r in range(4):
            px = np.full((2, 2, 3), base, dtype=np.uint8)
            px.reshape(4, 3)[:r] += 1                                # r of the four pixels one higher: sum = 4*base + r, every channel
            blocks.append(px)
    for r, g, b in ((0, 1, 2), (1, 2, 3), (2, 3, 0), (3, 0, 1)):    # different residues per channel
        px = np.full((2, 2, 3), 60, dtype=np.uint8)
        for ch, k in enumerate((r, g, b)):
            px.reshape(4, 3)[:k, ch] += 1
        blocks.append(px)
    rgb = np.stack([np.concatenate([b, b], 1) for b in blocks])      # (n, 2, 4, 3): the block twice
    sums = rgb[:, :, :2].astype(int).sum((1, 2))
    assert {int(s) % 4 for s in sums.ravel()} == {0, 1, 2, 3}
    got = yuv420_from_rgb_u8(T(rgb)).numpy()
    assert np.array_equal(got, yuv420_np(rgb))


@pytest.mark.parametrize("H,W", [(2, 4), (6, 12), (32, 32)])
def test_random_images_and_layout(H, W):
    rng = np.random.default_rng(H * 100 + W)
    rgb = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    got = yuv420_from_rgb_u8(T(rgb))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 3 * H * W // 2) and got.is_contiguous()
    got = got.numpy()
    assert np.array_equal(got, yuv420_np(rgb))
    # plane offsets and the frame stride, from single pixels: frame t, Y at y*W + x, U at H*W + (y/2)*(W/2) + x/2, V a quarter-plane on
    flat = got.reshape(-1)
    fs = 3 * H * W // 2
    c = rgb.astype(np.int64)
    for t, y, x in ((0, 0, 0), (1, H - 1, W - 1), (2, H // 2, W // 2 + 1)):
        R, G, B = c[t, y, x]
        assert flat[t * fs + y * W + x] == ((66 * R + 129 * G + 25 * B + 128) >> 8) + 16
        blk = (c[t, y // 2 * 2:y // 2 * 2 + 2, x // 2 * 2:x // 2 * 2 + 2].reshape(4, 3).sum(0) + 2) >> 2
        co = (y // 2) * (W // 2) + x // 2
        assert flat[t * fs + H * W + co] == ((-38 * blk[0] - 74 * blk[1] + 112 * blk[2] + 128) >> 8) + 128
        assert flat[t * fs + H * W + (H // 2) * (W // 2) + co] == ((112 * blk[0] - 94 * blk[1] - 18 * blk[2] + 128) >> 8) + 128


def test_egress_rejects_bad_sizes():
    for shape in ((1, 3, 4, 3), (1, 2, 6, 3), (1, 2, 4, 4)):
        with pytest.raises(ValueError):
            yuv420_from_rgb_u8(torch.zeros(shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        yuv420_from_rgb_u8(torch.zeros(1, 2, 4, 3))


@pytest.mark.parametrize("mean", [(0.0, 0.0, 0.0), (3.0, -2.5, 40.0)])
def test_decode_clip_yuv420_equals_restatement_of_decode_clip_u8(lfg, mean):
    g, sd = lfg
    dec = FlowDecoder(sd, "cpu", ops=RefOps(), chunk=2)                  # T = 5: chunks of 2, 2, 1
    img, grid, conf = T(g["img"]), T(g["grid"]), T(g["conf"])
    got = dec.decode_clip_yuv420(img, grid, conf, mean=mean)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 5, 3 * 32 * 32 // 2)
    want = yuv420_np(dec.decode_clip_u8(img, grid, conf, mean=mean, bgr=False)[0].numpy())
    assert np.array_equal(got[0].numpy(), want)
    assert np.array_equal(dec.decode_clip_yuv420(img, grid, conf, mean=mean, chunk=3)[0].numpy(), want)      # chunk= overrides
    t0s, parts = [], []
    for t0, fr in dec.stream_frames_yuv420(img, grid, conf, mean=mean):
        assert isinstance(fr, np.ndarray) and fr.dtype == np.uint8 and fr.shape[1:] == (3 * 32 * 32 // 2,)
        t0s.append(t0)
        parts.append(fr.copy())
    assert t0s == [0, 2, 4]
    assert np.array_equal(np.concatenate(parts, 0), want)


def test_sample_one_video_yuv420(lfg):
    from test_decode_u8_cpu import _flow_diffusion
    g, sd = lfg
    dec = FlowDecoder(sd, "cpu", ops=RefOps(), chunk=2)
    pred = torch.cat([T(g["grid"]), T(g["conf"]) * 2 - 1], 1)
    fd = _flow_diffusion(dec, pred)
    a = (T(g["img"]), torch.zeros(1, 5, 1024), torch.zeros(1, 6, 5), torch.zeros(1, 2, 5),
         torch.tensor([[4.0], [20.0], [6.0], [28.0], [32.0], [32.0]]).view(1, 6, 1), 1.0)
    mean = (2.0, 0.0, -3.5)
    rgb = fd.sample_one_video(*a, frames_u8=dict(mean=mean))             # no format: today's keys, to the letter
    assert set(rgb) == {"sample_vid_grid", "sample_vid_conf", "ddim_seconds", "sample_frames_u8"}
    assert set(fd.sample_one_video(*a, frames_u8=dict(mean=mean, format="rgb"))) == set(rgb)
    want = yuv420_np(rgb["sample_frames_u8"][0].numpy())
    out = fd.sample_one_video(*a, frames_u8=dict(format="yuv420p", mean=mean))
    assert set(out) == {"sample_vid_grid", "sample_vid_conf", "ddim_seconds", "sample_frames_yuv420"}
    assert tuple(out["sample_frames_yuv420"].shape) == (1, 5, 1536) and np.array_equal(out["sample_frames_yuv420"][0].numpy(), want)
    assert np.array_equal(fd.sample_one_video(*a, frames_u8=dict(format="yuv420p", mean=mean, bgr=False))["sample_frames_yuv420"][0]
                          .numpy(), want)
    chunks = list(fd.sample_one_video(*a, frames_u8=dict(format="yuv420p", mean=mean, stream=True))["sample_frames_yuv420"])
    assert [t0 for t0, _ in chunks] == [0, 2, 4]
    assert np.array_equal(np.concatenate([f for _, f in chunks], 0), want)
    with pytest.raises(ValueError):
        fd.sample_one_video(*a, frames_u8=dict(format="yuv420p", mean=mean, bgr=True))
    with pytest.raises(ValueError):
        fd.sample_one_video(*a, frames_u8=dict(format="nv12"))


def _plumbing(tmp_path, **kw):
    """The RefOps plumbing run of test_decode_u8_cpu.test_video_generator_streams_the_same_frames_and_pngs: 5 frames, 64 x 64."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_decode
    from dawn_pytorch_amd.video_generator import VideoGenerator
    Tn, res = 5, 64
    cache, outd = tmp_path / "cache", tmp_path / "out"
    cache.mkdir(parents=True)
    rng = np.random.default_rng(0)
    np.save(cache / "target_audio.npy", rng.standard_normal((Tn + 2, 1024)).astype(np.float32))
    np.save(cache / "dri_pose.npy", rng.standard_normal((Tn + 2, 6)).astype(np.float32))
    np.save(cache / "dri_blink.npy", rng.random((Tn + 2, 2)).astype(np.float32))
    img = tmp_path / "face.png"
    Image.fromarray((rng.random((80, 80, 3)) * 255).astype(np.uint8)).save(img)
    mean = [3.0, 0.0, -2.0]
    cfg = {"input_size": res, "max_n_frames": Tn, "random_seed": 1234, "mean": mean, "win_width": 40, "sampling_step": 2,
           "ddim_sampling_eta": 1.0, "cond_scale": 1.0, "model_config": {"is_train": True, "pose_dim": 6}}
    args = argparse.Namespace(audio_path="", image_path=str(img), output_path=str(outd), cache_path=str(cache), resolution=res)
    dec = FlowDecoder(bench_decode.lfg_state_dict(0), "cpu", ops=RefOps(), chunk=2)       # 3 chunks: 2 + 2 + 1 frames
    vg = VideoGenerator(args, generator=dec, config=cfg, device="cpu", allow_random_weights=True, **kw)
    vg.video_model.unet.ops = RefOps()
    vg.video_model.native_decode = True

    def want(out):
        src = T(np.array(Image.open(img).convert("RGB").resize((res, res), Image.BILINEAR))).permute(2, 0, 1).float().unsqueeze(0) / 255.
        return yuv420_np(dec.decode_clip_u8(src, out["sample_vid_grid"], out["sample_vid_conf"], mean=tuple(mean), bgr=False)[0].numpy())
    return vg, outd / "face", want, (Tn, res)


def _no_pngs(root):
    return not [f for _, _, fs in os.walk(root) for f in fs if f.endswith(".png")]


def test_video_generator_yuv420p_without_an_encoder_writes_y4m(tmp_path, monkeypatch):
    empty = tmp_path / "nobin"
    empty.mkdir()
    monkeypatch.setenv("PATH", str(empty))                               # no ffmpeg to be found
    vg, root, want, (Tn, res) = _plumbing(tmp_path, video_egress="yuv420p")
    frames = vg.run()
    assert isinstance(frames, np.ndarray) and frames.dtype == np.uint8 and frames.shape == (Tn, 3 * res * res // 2)
    assert np.array_equal(frames, want(vg.last_output))
    assert "sample_frames_yuv420" not in vg.last_output and "sample_out_vid" not in vg.last_output.keys()
    assert _no_pngs(root)
    raw = (root / "video" / "face.y4m").read_bytes()
    head = f"YUV4MPEG2 W{res} H{res} F25:1 Ip A1:1 C420jpeg\n".encode()
    assert raw.startswith(head)
    body, fb = raw[len(head):], 3 * res * res // 2
    assert len(body) == Tn * (6 + fb)
    for i in range(Tn):
        rec = body[i * (6 + fb):(i + 1) * (6 + fb)]
        assert rec[:6] == b"FRAME\n" and rec[6:] == frames[i].tobytes(), i


def test_video_generator_yuv420p_streams_into_the_encoder(tmp_path):
    script = tmp_path / "encoder.py"
    script.write_text("import sys\nopen(sys.argv[-1], 'wb').write(sys.stdin.buffer.read())\n")
    vg, root, want, (Tn, res) = _plumbing(tmp_path, video_egress="yuv420p", encoder_cmd=[sys.executable, str(script), "--opt"])
    frames = vg.run()
    assert frames.shape == (Tn, 3 * res * res // 2) and np.array_equal(frames, want(vg.last_output))
    assert (root / "video" / "face.mp4").read_bytes() == frames.tobytes()
    assert _no_pngs(root) and not (root / "video" / "face.y4m").exists()


def test_video_generator_yuv420p_raises_when_the_encoder_fails(tmp_path):
    script = tmp_path / "encoder.py"
    script.write_text("import sys\nsys.exit(1)\n")
    vg, root, _, _ = _plumbing(tmp_path, video_egress="yuv420p", encoder_cmd=[sys.executable, str(script)])
    with pytest.raises(RuntimeError, match="encoder"):
        vg.run()
    with pytest.raises(ValueError):
        _plumbing(tmp_path / "x", video_egress="h264")


def test_library_exports_the_yuv420_symbols():
    from dawn_pytorch_amd import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    assert L.dawn_abi_version() == 8
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    for n in NEW_SYMBOLS:
        assert f"int {n}(" in src, n


def test_host_side_argument_checks_answer_without_a_gpu():
    """Odd H, W % 4 != 0 and a NULL output are refused before anything is launched: the entries answer on a machine with no GPU.  The
    pointers are never dereferenced on the host."""
    from dawn_pytorch_amd import _lib, ctx
    L = _lib.lib()
    p = 4096
    err = lambda: L.dawn_last_error().decode()      # noqa: E731
    for H, W, out, word in ((17, 32, p, "even H"), (16, 34, p, "W % 4"), (16, 32, None, "non-NULL"), (16, 32, p + 2, "aligned")):
        assert L.dawn_frames_to_yuv420(p, 16 * 32, 1, H, W, 0.0, 0.0, 0.0, out, None) != 0
        assert "dawn_frames_to_yuv420" in err() and word in err() and f"H = {H}, W = {W}" in err()
        assert L.dawn_final_conv_blend_yuv420(p, 1, H, W, 8, p, p, p, p, 16, p, 4, 8, 0.0, 0.0, 0.0, out, None) != 0
        assert "dawn_final_conv_blend_yuv420" in err() and word in err()
    # the decode entries: a decoder without down blocks accepts any size, so the yuv rule itself answers
    names = ["first_w3", "first_bias", "first.a", "first.b", "final_w7", "final_bias"]
    cfg = ctx.DecoderCfg(0, 0, (ctypes.c_int * 8)(8))
    keep = [n.encode() for n in names]
    arr = (ctx.NamedPtr * len(names))(*[ctx.NamedPtr(k, p) for k in keep])
    h = ctypes.c_void_p()
    assert L.dawn_decoder_create(ctypes.addressof(cfg), ctypes.addressof(arr), len(names), ctypes.addressof(h)) == 0
    try:
        need = L.dawn_decoder_workspace_bytes(h, 16, 32, 2)
        assert need > 0
        for H, W, out, ws, word in ((17, 32, p, need, "even H"), (16, 34, p, need, "W % 4"), (16, 32, None, need, "non-NULL"),
                                    (16, 32, p, need - 1, "needed")):
            rc = L.dawn_decode_clip_conf_yuv420(h, H, W, 3, 4, 8, p, p, p, 3 * 4 * 8, p, 2, out, None, p, ws, None)
            assert rc != 0 and "dawn_decode_clip_conf_yuv420" in err() and word in err(), err()
            rc = L.dawn_decode_clip_yuv420(h, H, W, 3, 4, 8, p, p, p, 3 * 4 * 8, 2, out, None, p, ws, None)
            assert rc != 0 and "dawn_decode_clip_yuv420" in err() and word in err(), err()
        assert L.dawn_decode_clip_conf_yuv420(h, 16, 32, 3, 4, 8, p, p, p, 3 * 4 * 8, None, 2, p, None, p, need, None) != 0      # NULL conf
    finally:
        L.dawn_decoder_destroy(h)
    assert L.dawn_decode_clip_yuv420(None, 16, 32, 3, 4, 8, p, p, p, 96, 2, p, None, p, 1 << 20, None) != 0
