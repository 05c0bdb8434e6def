"""No-GPU checks of the media ingest (csrc/media_ingest.hip; dawn_generate_clip_media in csrc/dawn_inputs.hip): the integer restatement of
the resample against the goldens and the installed Pillow, the pass-order observation, symbols and signatures, the ctypes mirror's layout,
every refusal (refusals come before any launch, so they run without a device) and the workspace helper."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden
from dawn_pytorch_amd import _lib, ctx
from ingest_cases import CASES, PASS_ORDER_SHAPE, formula, parts_of, resample_u8, source

NEW = ("dawn_image_ingest", "dawn_image_ingest_workspace_bytes", "dawn_pcm16_to_samples", "dawn_generate_media_bytes",
       "dawn_generate_clip_media")
# non-NULL "device pointers", far apart: every call below is refused before anything would read them
SRC, OUT, WS, PCM = 0x10000000, 0x40000000, 0x70000000, 0x90000000


def err():
    return _lib.lib().dawn_last_error().decode()


@pytest.fixture(scope="module")
def golden():
    return load_golden("image_ingest.npz")


# ---------------------------------------------------------------------------------------------- the arithmetic
@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_goldens(golden, name):
    Hs, Ws, Ho, Wo, _ = CASES[name]
    got = resample_u8(source(name), Ho, Wo)
    assert got.shape == (Ho, Wo, 3)
    for key, part in parts_of(name, got).items():
        assert np.array_equal(part, golden[key]), (key, int((part != golden[key]).sum()))


def test_saturating_cases_reach_both_clip_ends(golden):
    for name in ("saturating_p1_up", "saturating_p3_up"):
        assert int(golden[name].min()) == 0 and int(golden[name].max()) == 255, name


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_equals_the_installed_pillow(name):
    """What validates the goldens: it holds on a tree without the feature."""
    Image = pytest.importorskip("PIL.Image")
    Hs, Ws, Ho, Wo, _ = CASES[name]
    a = source(name)
    assert np.array_equal(resample_u8(a, Ho, Wo), np.array(Image.fromarray(a).resize((Wo, Ho), Image.BILINEAR)))
    if name == "fractional_shrink":                          # mode "L": one channel, as convert("RGB") would replicate it
        grey = a[:, :, 1].copy()
        assert np.array_equal(resample_u8(grey, Ho, Wo), np.array(Image.fromarray(grey).resize((Wo, Ho), Image.BILINEAR)))


def test_pass_order_observation():
    """On 1023 x 3 -> 8 x 8 Pillow 12.2.0 equals the restatement with the passes SWAPPED (vertical first) and differs from the entry point's
    order by one level.  Informational: pinned to the version it was seen on, so that an upgrade that changes it is noticed there."""
    PIL = pytest.importorskip("PIL")
    from PIL import Image
    Hs, Ws, Ho, Wo = PASS_ORDER_SHAPE
    a = formula(Hs, Ws).astype(np.uint8)
    hv, vh = resample_u8(a, Ho, Wo, "hv"), resample_u8(a, Ho, Wo, "vh")
    assert not np.array_equal(hv, vh) and int(np.abs(hv.astype(int) - vh.astype(int)).max()) == 1
    got = np.array(Image.fromarray(a).resize((Wo, Ho), Image.BILINEAR))
    print(f"Pillow {PIL.__version__} on {Hs} x {Ws} -> {Ho} x {Wo}: equals horizontal-first {np.array_equal(got, hv)}, "
          f"vertical-first {np.array_equal(got, vh)}")
    if PIL.__version__ == "12.2.0":                          # the version the observation was made on
        assert np.array_equal(got, vh) and not np.array_equal(got, hv)


# ---------------------------------------------------------------------------------------------- symbols, signatures, layout
def test_symbols_signatures_and_abi():
    L = _lib.lib()
    for n in NEW:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    assert L.dawn_abi_version() == 8
    assert L.dawn_image_ingest_workspace_bytes.restype is C.c_size_t


def test_media_args_mirror_matches_the_c_layout():
    M = ctx.MediaArgs
    # dawn_media_args: gen, image | Hs, Ws | row_bytes | pix_bytes, order | pcm | n_frames | channels (+ 4 padding)
    assert C.sizeof(M) == 2 * 8 + 2 * 4 + 8 + 2 * 4 + 8 + 8 + 4 + 4
    assert (M.gen.offset, M.image.offset, M.Hs.offset, M.Ws.offset, M.row_bytes.offset, M.pix_bytes.offset, M.order.offset, M.pcm.offset,
            M.n_frames.offset, M.channels.offset) == (0, 8, 16, 20, 24, 32, 36, 40, 48, 56)
    assert (ctx.PIXELS_RGB, ctx.PIXELS_BGR) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "dawn_hip.h")).read()
    assert "DAWN_PIXELS_RGB = 0, DAWN_PIXELS_BGR = 1" in hdr


# ---------------------------------------------------------------------------------------------- refusals
def test_image_ingest_refusals():
    L = _lib.lib()
    need = int(L.dawn_image_ingest_workspace_bytes(37, 23, 8, 8))

    def call(src=SRC, Hs=37, Ws=23, row_bytes=69, pb=3, order=0, Ho=8, Wo=8, out=OUT, plane=64, ws=WS, ws_bytes=need):
        return L.dawn_image_ingest(src, Hs, Ws, row_bytes, pb, order, Ho, Wo, out, plane, ws, ws_bytes, None)
    for k in ("Hs", "Ws", "Ho", "Wo"):
        for v in (0, -3):
            assert call(**{k: v}) != 0 and f"{k} = {v}" in err(), (k, v)
    for pb in (0, 2, 5, -1):
        assert call(pb=pb, row_bytes=200) != 0 and f"pix_bytes = {pb}" in err(), pb
    assert call(row_bytes=68) != 0 and "row_bytes = 68" in err()
    assert call(pb=4, row_bytes=91) != 0 and "row_bytes = 91" in err()
    assert call(plane=63) != 0 and "plane = 63" in err()
    assert call(ws_bytes=need - 1) != 0
    assert "workspace" in err() and str(need - 1) in err() and str(need) in err() and "dawn_image_ingest_workspace_bytes" in err()
    for k in ("src", "out", "ws"):
        assert call(**{k: None}) != 0 and "NULL" in err(), k
    assert call(order=2) != 0 and "order = 2" in err()
    assert call(out=WS + 64) != 0 and "out3 overlaps" in err()
    assert call(Ws=70000, row_bytes=1 << 20) != 0 and "Ws = 70000" in err()


def test_pcm16_refusals():
    L = _lib.lib()

    def call(pcm=PCM, n=100, ch=2, out=OUT):
        return L.dawn_pcm16_to_samples(pcm, n, ch, out, None)
    for ch in (0, 9, -1):
        assert call(ch=ch) != 0 and f"channels = {ch}" in err(), ch
    for n in (0, -5):
        assert call(n=n) != 0 and f"n_frames = {n}" in err(), n
    for k in ("pcm", "out"):
        assert call(**{k: None}) != 0 and "NULL" in err(), k
    assert call(pcm=PCM + 1) != 0 and "2-byte aligned" in err()


def test_generate_clip_media_refusals_without_handles():
    L = _lib.lib()
    cb, wb = C.c_size_t(7), C.c_size_t(7)
    assert L.dawn_generate_media_bytes(None, C.byref(cb), C.byref(wb)) != 0 and "NULL" in err()
    m = ctx.MediaArgs()
    assert L.dawn_generate_clip_media(C.addressof(m), WS, 1 << 20, None) != 0 and "NULL" in err() and "gen" in err()
    a = ctx.GenerateArgs()
    m.gen = C.pointer(a)
    a.samples = PCM
    assert L.dawn_generate_clip_media(C.addressof(m), WS, 1 << 20, None) != 0
    assert "dawn_generate_clip_media" in err() and "image is NULL" in err() and "img3" in err()
    assert L.dawn_generate_media_bytes(C.addressof(m), C.byref(cb), C.byref(wb)) != 0 and "image is NULL" in err()
    a.samples, a.img3 = None, SRC
    assert L.dawn_generate_clip_media(C.addressof(m), WS, 1 << 20, None) != 0 and "pcm is NULL" in err()
    m.pcm, m.n_frames, m.channels = PCM, 16000, 9           # what dawn_pcm16_to_samples refuses, under this entry's name
    assert L.dawn_generate_clip_media(C.addressof(m), WS, 1 << 20, None) != 0
    assert "dawn_generate_clip_media" in err() and "channels = 9" in err()
    m.channels = 2                                           # the media are fine now: the pipeline's own first refusal
    assert L.dawn_generate_clip_media(C.addressof(m), WS, 1 << 20, None) != 0 and "NULL handle" in err()
    assert (cb.value, wb.value) == (7, 7)


# ---------------------------------------------------------------------------------------------- the workspace helper
def test_workspace_helper_is_monotone_and_never_zero():
    L = _lib.lib()
    f = lambda *a: int(L.dawn_image_ingest_workspace_bytes(*a))      # noqa: E731
    for name, (Hs, Ws, Ho, Wo, _) in CASES.items():
        base = f(Hs, Ws, Ho, Wo)
        assert base > 0 and base % 256 == 0, name
        # room for both tables at their tap bound and for the bytes between the passes
        assert base >= 8 * (Wo + Ho) + 4 * (Wo * (2 * -(-Ws // Wo) + 1) + Ho * (2 * -(-Hs // Ho) + 1)) + Hs * Wo * 3, name
        for i in range(4):
            for d in (1, 7, 300):
                a = [Hs, Ws, Ho, Wo]
                a[i] += d
                assert f(*a) >= base, (name, i, d)
    for bad in ((0, 8, 8, 8), (8, 8, 8, -1), (8, 65536, 8, 8)):
        assert f(*bad) == 0, bad
