"""Decode to uint8 frames (SURVEY.md §8f N1 + N2 as one path) on CPU: `FlowDecoder.decode_clip_u8` / `stream_frames_u8`,
`FlowDiffusion.sample_one_video(frames_u8=...)` and `VideoGenerator.generate_final_video`'s streaming path, driven by the torch op
set (oracle/ops_ref.RefOps, which has no fused byte kernel: the decoder composes final_conv_blend + frames_to_u8 per chunk, the
definition of the expected result), plus the no-GPU checks of the new C entry points.  The fused kernel and the C-side decoder run in
tests/test_hip_decode_u8.py."""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from oracle.ops_ref import RefOps
from dawn_pytorch_amd.flow_decoder import FlowDecoder

T = torch.from_numpy
NEW_SYMBOLS = ("dawn_final_conv_blend_u8", "dawn_decoder_create", "dawn_decoder_destroy", "dawn_decoder_skip_bytes",
               "dawn_decoder_workspace_bytes", "dawn_decoder_encode", "dawn_decode_clip", "dawn_decode_clip_conf")


@pytest.fixture(scope="module")
def lfg():
    g = load_golden("lfg_tiny.npz")
    sd = {k[3:]: T(v) for k, v in g.items() if k.startswith("sd/")}
    return g, sd


def movable_bytes(v, mean=(0.0, 0.0, 0.0), bgr=False, tol=2e-5):
    """Where may a byte of the egress move when the fp32 frame value moves by at most `tol`?  (3,T,H,W) -> bool (T,H,W,3)."""
    ref = RefOps()
    return (ref.frames_to_u8(v - tol, mean=mean, bgr=bgr) != ref.frames_to_u8(v + tol, mean=mean, bgr=bgr)).numpy()


def assert_bytes_within_reference(got, v, mean=(0.0, 0.0, 0.0), bgr=False):
    """`got` (T,H,W,3) against the reference's own fp32 frames v (3,T,H,W): every byte within 1 of frames_to_u8(v), and different
    only where a move of v by 2e-5 (the gate of flow_decoder/golden_out) crosses a byte boundary -- a set computed from the data."""
    want = RefOps().frames_to_u8(v, mean=mean, bgr=bgr).numpy().astype(np.int16)
    got = got.astype(np.int16)
    diff = np.abs(got - want)
    may = movable_bytes(v, mean, bgr)
    print(f"bytes differing from the reference's: {int((diff != 0).sum())} of {diff.size}; allowed to move: {int(may.sum())}; "
          f"max |diff| {int(diff.max())}")
    assert diff.max() <= 1
    assert not ((diff != 0) & ~may).any()


@pytest.mark.parametrize("mean,bgr,chunk", [((0.0, 0.0, 0.0), False, 5), ((0.0, 0.0, 0.0), True, 2), ((3.0, -2.5, 40.0), False, 3),
                                            ((-1.0, 0.5, 7.25), True, 4)])
def test_decode_clip_u8_equals_two_step_path(lfg, mean, bgr, chunk):
    g, sd = lfg
    dec = FlowDecoder(sd, "cpu", ops=RefOps(), chunk=chunk)              # T = 5: chunks 2, 3 and 4 do not divide it
    img, grid, conf = T(g["img"]), T(g["grid"]), T(g["conf"])
    got = dec.decode_clip_u8(img, grid, conf, mean=mean, bgr=bgr)
    assert got.dtype == torch.uint8 and got.shape == (1, 5, 32, 32, 3)
    want = RefOps().frames_to_u8(dec.decode_clip(img, grid, conf)["sample_out_vid"][0], mean=mean, bgr=bgr)
    assert torch.equal(got[0], want)
    assert torch.equal(dec.decode_clip_u8(img, grid, conf, mean=mean, bgr=bgr, chunk=1)[0], want)      # chunk= overrides


def test_decode_clip_u8_against_reference_frames(lfg):
    g, sd = lfg
    dec = FlowDecoder(sd, "cpu", ops=RefOps(), chunk=2)
    got = dec.decode_clip_u8(T(g["img"]), T(g["grid"]), T(g["conf"]))[0].numpy()
    assert_bytes_within_reference(got, T(g["sample_out_vid"])[0])
    got = dec.decode_clip_u8(T(g["img"]), T(g["grid"]), T(g["conf"]), mean=(2.0, 0.0, -3.5), bgr=True)[0].numpy()
    assert_bytes_within_reference(got, T(g["sample_out_vid"])[0], mean=(2.0, 0.0, -3.5), bgr=True)


@pytest.mark.parametrize("chunk", [2, 5, 64])
def test_stream_frames_u8_concatenates_to_decode_clip_u8(lfg, chunk):
    g, sd = lfg
    dec = FlowDecoder(sd, "cpu", ops=RefOps())
    img, grid, conf = T(g["img"]), T(g["grid"]), T(g["conf"])
    want = dec.decode_clip_u8(img, grid, conf, mean=(1.0, 2.0, 3.0), bgr=True)[0].numpy()
    t0s, parts = [], []
    for t0, fr in dec.stream_frames_u8(img, grid, conf, mean=(1.0, 2.0, 3.0), bgr=True, chunk=chunk):
        assert isinstance(fr, np.ndarray) and fr.dtype == np.uint8 and fr.shape[1:] == (32, 32, 3)
        t0s.append(t0)
        parts.append(fr.copy())
    assert t0s == list(range(0, 5, min(chunk, 5)))
    assert np.array_equal(np.concatenate(parts, 0), want)


def _flow_diffusion(dec, pred):
    from dawn_pytorch_amd.flow_diffusion import FlowDiffusion
    fd = FlowDiffusion(img_size=8, num_frames=5, sampling_timesteps=2, pose_dim=6, generator=dec, native_decode=True)
    fd.diffusion.sample = lambda fea, bbox_mask, cond=None, batch_size=None, cond_scale=1.0: pred
    return fd


def test_sample_one_video_frames_u8(lfg):
    g, sd = lfg
    dec = FlowDecoder(sd, "cpu", ops=RefOps(), chunk=2)
    pred = torch.cat([T(g["grid"]), T(g["conf"]) * 2 - 1], 1)
    fd = _flow_diffusion(dec, pred)
    a = (T(g["img"]), torch.zeros(1, 5, 1024), torch.zeros(1, 6, 5), torch.zeros(1, 2, 5),
         torch.tensor([[4.0], [20.0], [6.0], [28.0], [32.0], [32.0]]).view(1, 6, 1), 1.0)
    base = fd.sample_one_video(*a)
    assert set(base) == {"sample_vid_grid", "sample_vid_conf", "ddim_seconds", "sample_out_vid", "sample_warped_vid"}
    assert base["sample_out_vid"].dtype == torch.float32 and base["sample_out_vid"].shape == (1, 3, 5, 32, 32)
    assert set(fd.sample_one_video(*a, None, None, None)) == set(base)            # the reference's positional signature
    out = fd.sample_one_video(*a, frames_u8=dict(mean=(2.0, 0.0, -3.5), bgr=True))
    assert set(out) == {"sample_vid_grid", "sample_vid_conf", "ddim_seconds", "sample_frames_u8"}
    want = RefOps().frames_to_u8(base["sample_out_vid"][0], mean=(2.0, 0.0, -3.5), bgr=True)
    assert out["sample_frames_u8"].shape == (1, 5, 32, 32, 3) and torch.equal(out["sample_frames_u8"][0], want)
    chunks = list(fd.sample_one_video(*a, frames_u8=dict(mean=(2.0, 0.0, -3.5), bgr=True, stream=True))["sample_frames_u8"])
    assert [t0 for t0, _ in chunks] == [0, 2, 4]
    assert np.array_equal(np.concatenate([f for _, f in chunks], 0), want.numpy())
    fd.native_decode = False                                                       # frame-by-frame reference path: no byte decode
    with pytest.raises(ValueError):
        fd.sample_one_video(*a, frames_u8={})


def test_video_generator_streams_the_same_frames_and_pngs(tmp_path):
    """BASELINE-config-0-style plumbing run (random weights, RefOps), native decode: the streamed PNG files and the returned array
    against frames computed the way generate_final_video did before -- decode_clip's fp32 clip, then frames_to_u8 on all of it."""
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_decode
    from dawn_pytorch_amd.video_generator import VideoGenerator
    Tn, res = 5, 64
    cache, outd, old = tmp_path / "cache", tmp_path / "out", tmp_path / "old"
    cache.mkdir()
    old.mkdir()
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
    vg = VideoGenerator(args, generator=dec, config=cfg, device="cpu", allow_random_weights=True)
    vg.video_model.unet.ops = RefOps()
    vg.video_model.native_decode = True
    frames = vg.run()
    assert frames.shape == (Tn, res, res, 3) and frames.dtype == np.uint8
    out = vg.last_output
    assert "sample_frames_u8" not in out and "sample_out_vid" not in out.keys()           # streamed: no fp32 clip was made
    clip = dec.decode_clip(T(np.array(Image.open(img).convert("RGB").resize((res, res), Image.BILINEAR))).permute(2, 0, 1)
                           .float().unsqueeze(0) / 255., out["sample_vid_grid"], out["sample_vid_conf"])["sample_out_vid"]
    want = RefOps().frames_to_u8(clip[0].float().contiguous(), mean=tuple(mean), bgr=False).numpy()
    assert np.array_equal(frames, want)
    assert torch.equal(vg.decode_last_clips()["sample_out_vid"], clip)                    # ... and is there on demand
    assert "sample_warped_vid" in out and torch.equal(out["sample_out_vid"], clip) and "sample_out_vid" in out.keys()
    assert out.get("sample_out_vid") is out["sample_out_vid"] and out.get("nope") is None
    names = sorted(os.listdir(outd / "face" / "img"))
    assert names == [f"{i:03d}.png" for i in range(Tn)]
    for i, n in enumerate(names):
        Image.fromarray(want[i]).save(old / n)
        assert (outd / "face" / "img" / n).read_bytes() == (old / n).read_bytes(), n


def test_new_structs_match_header():
    from dawn_pytorch_amd import ctx
    assert ctypes.sizeof(ctx.DecoderCfg) == 4 * (1 + 1 + 8)                  # int n_down, n_bottleneck; int widths[8]
    assert ctx.DecoderCfg.widths.offset == 8
    assert ctypes.sizeof(ctx.NamedPtr) == 16
    src = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    body = src[src.index("typedef struct dawn_decoder_cfg {"):src.index("} dawn_decoder_cfg;")]
    assert "int n_down;" in body and "int n_bottleneck;" in body and "int widths[8];" in body


def test_library_exports_the_new_symbols():
    from dawn_pytorch_amd import _lib
    L = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    assert L.dawn_abi_version() == 8
    # host-side argument checks answer without a GPU: no decoder, no sizes
    assert L.dawn_decoder_skip_bytes(None, 64, 64) == 0 and L.dawn_decoder_workspace_bytes(None, 64, 64, 4) == 0


def test_decoder_create_and_size_queries_on_the_host():
    """dawn_decoder_create only records pointers, and the size queries are dry passes of the launch sequence: both run without a GPU.
    A missing weight name is an error with the name in the message."""
    from dawn_pytorch_amd import _lib, ctx
    L = _lib.lib()
    names = ["first_w3", "first_bias", "first.a", "first.b", "final_w7", "final_bias"]
    for i in range(2):
        names += [f"{p}.{i}.{f}" for p in ("downs", "ups") for f in ("w", "bias", "a", "b")]
    names += [f"bott.0.{f}" for f in ("a1", "b1", "a2", "b2", "c1.w", "c1.bias", "c2.w", "c2.bias")]

    def create(ns):
        cfg = ctx.DecoderCfg(2, 1, (ctypes.c_int * 8)(64, 128, 256))
        keep = [n.encode() for n in ns]
        arr = (ctx.NamedPtr * len(ns))(*[ctx.NamedPtr(k, 4096) for k in keep])           # never dereferenced on the host
        h = ctypes.c_void_p()
        return L.dawn_decoder_create(ctypes.addressof(cfg), ctypes.addressof(arr), len(ns), ctypes.addressof(h)), h

    rc, h = create([n for n in names if n != "ups.1.a"])
    assert rc != 0 and not h and "ups.1.a" in L.dawn_last_error().decode()
    rc, h = create(names)
    assert rc == 0 and h
    try:
        # skips: 64 ch at 64x64, 128 at 32x32, 256 at 16x16
        assert L.dawn_decoder_skip_bytes(h, 64, 64) == 4 * (64 * 64 * 64 + 32 * 32 * 128 + 16 * 16 * 256)
        assert L.dawn_decoder_skip_bytes(h, 66, 64) == 0 and "66x64" in L.dawn_last_error().decode()
        w1, w4 = L.dawn_decoder_workspace_bytes(h, 64, 64, 1), L.dawn_decoder_workspace_bytes(h, 64, 64, 4)
        # the chunk's largest moment: last up block's upsampled input (128 ch) + its input (128 ch at half size) or output (64 ch)
        assert w1 >= 4 * 64 * 64 * (128 + 64) and 3.5 * w1 <= w4 <= 4 * w1
    finally:
        L.dawn_decoder_destroy(h)
