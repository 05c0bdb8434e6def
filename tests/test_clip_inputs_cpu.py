"""No-GPU checks of the clip-input entry points (csrc/clip_inputs.hip, csrc/dawn_inputs.hip): symbols and signatures, the host-side
rectangle arithmetic against `FlowDiffusion.generate_bbox_mask`, every refusal (an error return with a message; refusals come before
any launch, so they run without a device), and the ctypes mirrors' layout.

`dawn_generate_bytes` needs a `dawn_ctx`, whose creation reads weights back from the device: its sum rule is checked in
tests/test_hip_clip_inputs.py; here only its refusals."""
import ctypes as C
import math

import pytest
import torch

from clip_inputs_cases import BBOX_CASES, mask_from_bounds, mask_of
from dawn_pytorch_amd import _lib, ctx

NEW = ("dawn_face_loc_embed", "dawn_bbox_mask_bounds", "dawn_cond_rows", "dawn_inputs_create", "dawn_inputs_destroy", "dawn_clip_inputs",
       "dawn_generate_bytes", "dawn_generate_clip")
F6 = C.c_float * 6
FAKE = 0x10000          # a non-NULL "device pointer": every call below is refused before anything would read it


def err():
    return _lib.lib().dawn_last_error().decode()


def test_symbols_signatures_and_abi():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    assert L.dawn_abi_version() == 8


@pytest.mark.parametrize("name,size,bbox6", BBOX_CASES, ids=[c[0] for c in BBOX_CASES])
def test_bbox_mask_bounds_reproduce_generate_bbox_mask(name, size, bbox6):
    L = _lib.lib()
    out = (C.c_int * 4)()
    assert L.dawn_bbox_mask_bounds(F6(*bbox6), size, out) == 0, err()
    want = mask_of(bbox6, size)
    assert torch.equal(mask_from_bounds(tuple(out), size), want), (tuple(out), int(want.sum()))
    # and the four numbers themselves, formed as generate_bbox_mask forms them
    b = torch.tensor(bbox6, dtype=torch.float32)
    xs, ys = (b[:2] / b[4]) * size, (b[2:4] / b[5]) * size
    assert tuple(out) == (int(xs[0].to(torch.int32)), int(ys[0].to(torch.int32)), int((xs[1] + 1).to(torch.int32)),
                          int((ys[1] + 1).to(torch.int32)))


def test_face_loc_embed_refusals():
    L = _lib.lib()
    ok = F6(64, 64, 192, 192, 256, 256)

    def call(bbox=ok, size=32, w1=FAKE, b1=FAKE, w2=FAKE, b2=FAKE, out=FAKE, plane=64):
        return L.dawn_face_loc_embed(bbox, size, w1, b1, w2, b2, out, plane, None)
    for size in (0, 2, 3, 30, -4):
        assert call(size=size) != 0 and "multiple of 4" in err(), size
    for k in ("w1", "b1", "w2", "b2", "out"):
        assert call(**{k: None}) != 0 and "NULL" in err(), k
    assert call(bbox=None) != 0 and "NULL" in err()
    assert call(plane=63) != 0 and "plane" in err()
    for i, v in ((0, math.nan), (3, math.inf), (5, -math.inf), (4, 0.0), (5, 0.0)):
        b = [64, 64, 192, 192, 256, 256]
        b[i] = v
        assert call(bbox=F6(*b)) != 0 and "bbox6" in err(), (i, v)
    out = (C.c_int * 4)()
    assert L.dawn_bbox_mask_bounds(F6(1, 2, 3, 4, 0, 5), 32, out) != 0 and "bbox6" in err()
    assert L.dawn_bbox_mask_bounds(ok, 6, out) != 0 and "multiple of 4" in err()
    assert L.dawn_bbox_mask_bounds(ok, 32, None) != 0 and "NULL" in err()


def test_cond_rows_refusals():
    L = _lib.lib()
    ip7, ie = (C.c_float * 7)(*range(7)), (C.c_float * 2)(0.1, 0.2)
    A, P_, E, CO = 0x100000, 0x900000, 0xA00000, 0x2000000          # far apart: no overlap at T = 10

    def call(audio=A, n_aud=1024, ld_audio=1024, pose=P_, n_pose=6, ld_pose=6, eye=E, ld_eye=2, init_pose=ip7, n_init=7, init_eye=ie,
             T=10, cond=CO, ld_cond=1033):
        return L.dawn_cond_rows(audio, n_aud, ld_audio, pose, n_pose, ld_pose, eye, ld_eye, init_pose, n_init, init_eye, T, cond, ld_cond,
                                None)
    for T in (0, -1):
        assert call(T=T) != 0 and "T =" in err()
    for k in ("audio", "pose", "eye", "cond"):
        assert call(**{k: None}) != 0 and "NULL" in err(), k
    for kw in (dict(ld_audio=1023), dict(ld_pose=5), dict(ld_eye=1), dict(ld_cond=1032)):
        assert call(**kw) != 0 and "stride" in err(), kw
    for n_pose, ld in ((5, 5), (8, 8)):
        assert call(n_pose=n_pose, ld_pose=ld) != 0 and "n_pose" in err()
    assert call(init_pose=None, n_init=0, n_pose=6, ld_cond=1031) != 0 and "stride" in err()      # P = 6: width 1032
    ip17 = (C.c_float * 17)(*range(17))
    assert call(init_pose=ip17, n_init=17, n_pose=17, ld_pose=17, ld_cond=2000) != 0 and "n_init" in err()
    for bad in (math.nan, math.inf):
        b = (C.c_float * 7)(0, 1, 2, bad, 4, 5, 6)
        assert call(init_pose=b) != 0 and "finite" in err()
        assert call(init_eye=(C.c_float * 2)(0.1, bad)) != 0 and "finite" in err()
    # overlap: an input inside cond that is not exactly its own columns
    assert call(pose=CO + 4 * 1025, ld_pose=1033) != 0 and "overlaps" in err()
    assert call(audio=CO, ld_audio=1040, ld_cond=1033) != 0 and "overlaps" in err()
    assert call(eye=CO + 4 * 1031, ld_eye=1034) != 0 and "overlaps" in err()


def test_inputs_create_and_clip_inputs_refusals():
    L = _lib.lib()
    names = [b"face_loc_emb.conv1.weight", b"face_loc_emb.conv1.bias", b"face_loc_emb.conv2.weight", b"face_loc_emb.conv2.bias"]
    arr = (ctx.NamedPtr * 4)()
    for i, n in enumerate(names):
        arr[i].name, arr[i].ptr = n, FAKE + 4096 * i
    h = C.c_void_p()
    cfg = ctx.InputsCfg(1024, 7, 2)
    assert L.dawn_inputs_create(None, C.addressof(arr), 4, C.addressof(h)) != 0 and "NULL" in err()
    for bad in (ctx.InputsCfg(0, 7, 2), ctx.InputsCfg(1024, 0, 2), ctx.InputsCfg(1024, 17, 2), ctx.InputsCfg(1024, 7, 3)):
        assert L.dawn_inputs_create(C.addressof(bad), C.addressof(arr), 4, C.addressof(h)) != 0 and "pose_dim" in err()
    assert L.dawn_inputs_create(C.addressof(cfg), C.addressof(arr), 3, C.addressof(h)) != 0
    assert "missing weight 'face_loc_emb.conv2.bias'" in err() and not h.value
    assert L.dawn_inputs_create(C.addressof(cfg), C.addressof(arr), 4, C.addressof(h)) == 0 and h.value
    try:
        ok, ip7, ie = F6(64, 64, 192, 192, 256, 256), (C.c_float * 7)(*range(7)), (C.c_float * 2)(0.1, 0.2)
        A, P_, E, CO, FE = 0x100000, 0x900000, 0xA00000, 0x2000000, 0x4000000

        def call(in_=h, bbox=ok, size=32, fea=FE, fea_ch=272, n_pose=6, init_pose=ip7, n_init=7, T=10, ld_cond=1033, cond=CO):
            return L.dawn_clip_inputs(in_, bbox, size, fea, fea_ch, A, 1024, P_, n_pose, n_pose, E, 2, init_pose, n_init, ie, T, cond, ld_cond,
                                      None)
        assert call(in_=None) != 0 and "NULL" in err()
        assert call(fea=None) != 0 and "NULL" in err()
        assert call(fea_ch=15) != 0 and "fea_ch" in err()
        assert call(size=30) != 0 and "multiple of 4" in err()
        assert call(T=0) != 0 and "T =" in err()                              # the cond rows are checked before the embed is launched
        assert call(ld_cond=1032) != 0 and "stride" in err()
        assert call(init_pose=None, n_init=0) != 0 and "pose_dim" in err()    # P = 6 against a handle of pose_dim 7
    finally:
        L.dawn_inputs_destroy(h)


def test_struct_mirrors_match_the_c_layout():
    assert C.sizeof(ctx.InputsCfg) == 3 * 4
    G = ctx.GenerateArgs
    # dawn_generate_args: 6 handles | samples, n_samples, img3 | H, fea_ch | bbox6, init_pose, init_eye | n_init, latent_dim | init_pose6,
    # init_blink2 | T | S, cond_scale | ddim_steps, ancestral_steps, clip | seed | format, bgr, chunk (+ 4 padding) | mean3, frames_out,
    # latent_out, cond_out
    assert C.sizeof(G) == 6 * 8 + 3 * 8 + 2 * 4 + 3 * 8 + 2 * 4 + 2 * 8 + 8 + 2 * 4 + 3 * 8 + 8 + 4 * 4 + 4 * 8
    assert (G.samples.offset, G.H.offset, G.bbox6.offset, G.n_init.offset, G.init_pose6.offset, G.T.offset, G.S.offset, G.cond_scale.offset,
            G.ddim_steps.offset, G.seed.offset, G.format.offset, G.chunk.offset, G.mean3.offset, G.cond_out.offset) == \
           (48, 72, 80, 104, 112, 128, 136, 140, 144, 168, 176, 184, 192, 216)


def test_generate_refusals_without_handles():
    L = _lib.lib()
    cb, wb = C.c_size_t(7), C.c_size_t(7)
    assert L.dawn_generate_bytes(None, C.byref(cb), C.byref(wb)) != 0 and "NULL" in err()
    a = ctx.GenerateArgs()
    assert L.dawn_generate_bytes(C.addressof(a), C.byref(cb), C.byref(wb)) != 0 and "NULL handle" in err()
    assert L.dawn_generate_clip(C.addressof(a), FAKE, 1 << 20, None) != 0 and "NULL handle" in err()
    assert (cb.value, wb.value) == (7, 7)
