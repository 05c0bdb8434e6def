"""-m gpu: the kernels of the stages around the UNet and of the sampler between guard bands (tests/guarded.py; tests/test_guarded_cpu.py shows
what the helper catches): the flow decoder (csrc/flow_decode.hip), HuBERT (csrc/hubert.hip), PBnet's attn_bias32 (csrc/pbnet.hip), the sampler
steps (csrc/sampler.hip) and the three C-side hosts that take a caller's workspace.  tests/test_hip_guard.py does the same for the UNet.

Every case asserts three things: the values against the reference and tolerance of the op's existing test (case builders, references, `check`
and gates are imported from those tests, not copied; byte and bit-exact ops keep `torch.equal`); GuardedOps.verify() -- every output element
written, nothing written outside an output; GuardedOps.inputs_intact() -- no operand modified and (through the NaN around every operand)
nothing read outside an operand reached the result.  Every tensor operand is a guarded input; 2-D fp32 operands also run as column slices of a
wider tensor wherever the op accepts ld > C.  The shapes are the smallest that still straddle each kernel's edges: tile edges, the 128-bit body
and its scalar tail, one wrap of a capped grid, a frame range of a longer clip."""
import numpy as np
import pytest
import torch

import stage_gate as S
import test_hip_decode_u8 as U8
import test_hip_hubert as HB
import test_hip_hubert_c as HC
import test_hip_yuv420 as YUV
from conftest import load_golden
from dawn_pytorch_amd import _lib
from guarded import STAGE_BUFFERS, GuardedOps, _poisoned, assert_no_255
from oracle.ops_ref import RefOps
from test_hip_flow_decode import motion
from test_hip_guard import PAD, gin
from test_hip_ops import check, rnd
from test_yuv420_cpu import yuv420_np

pytestmark = pytest.mark.gpu

_g = []
_plain = []
_cache = {}
ref = RefOps()
T_ = torch.from_numpy


@pytest.fixture
def g():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    if not _g:
        _g.append(GuardedOps())
    o = _g[0]
    o.reset()
    try:
        yield o
    finally:
        o.reset()


def plain():
    """The unguarded op set: the launches a guarded launch is compared with bit for bit."""
    from dawn_pytorch_amd.ops import HipOps
    if not _plain:
        _plain.append(HipOps())
    return _plain[0]


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def names(g):
    return {r.name for r in g.outs}


def finish(g, alloc=(), overwritten=(), written=None):
    """After the launches of one run: every buffer of `alloc` was asked for under that name (the names guarded.STAGE_BUFFERS pins in
    ops.py), nothing poisoned is left, nothing outside was written, no operand changed."""
    torch.cuda.synchronize()
    for n in alloc:
        assert n in STAGE_BUFFERS and n in names(g), (n, sorted(names(g)))
    g.verify(written=written)
    g.inputs_intact(overwritten)


def close(name, got, want, tol):
    """`float((got - want).abs().max()) < tol`, the form of tests/test_hip_hubert.py."""
    got = got.detach().cpu()
    assert not torch.isnan(got).any(), f"{name}: NaN"
    err = float((got - want).abs().max())
    assert err < tol, f"{name}: max|diff| {err:.3e} >= {tol:.1e}"


def rows_mask(lead, total, a, b):
    """bool mask over the (lead * total) rows of a clip carved as (lead * total, ...): frames [a, b) of every leading index."""
    m = torch.zeros(lead, total, dtype=torch.bool)
    m[:, a:b] = True
    return m.flatten()


# ---------------------------------------------------------------------------------------------- flow decoder
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("rows,C", [(37, 20), (1, 4)])
def test_affine_act(g, rows, C, act):
    """Values: test_hip_flow_decode.test_affine_act (RefOps, 1e-6).  x contiguous, and a column slice of a tensor 8 columns wider."""
    x, a, b = rnd(rows, C, seed=1), rnd(C, seed=2), rnd(C, seed=3)
    want = ref.affine_act(x, a, b, act)
    for pad in (0, PAD):
        g.reset()
        xg = gin(g, x, "x", pad)
        assert xg.stride(0) == C + 2 * pad
        got = g.affine_act(xg, gin(g, a, "a"), gin(g, b, "b"), act)
        torch.cuda.synchronize()
        check(f"guard/affine_act/{rows}x{C}_act{act}/pad{pad}", got, want, 1e-6)
        finish(g, alloc=("affine_act.out",))


@pytest.mark.parametrize("F,H,W,C", [(2, 6, 10, 12), (1, 2, 2, 4)])
def test_bn_relu_pool2(g, F, H, W, C):
    x, a, b = rnd(F * H * W, C, seed=1), rnd(C, seed=2), rnd(C, seed=3)
    got = g.bn_relu_pool2(gin(g, x, "x"), gin(g, a, "a"), gin(g, b, "b"), F, H, W)
    torch.cuda.synchronize()
    check(f"guard/bn_relu_pool2/{F}x{H}x{W}x{C}", got, ref.bn_relu_pool2(x, a, b, F, H, W), 1e-6)
    finish(g, alloc=("bn_relu_pool2.out",))


@pytest.mark.parametrize("Hs,h,Cc,mode", [(16, 16, 64, "first"), (16, 16, 64, "prev"), (32, 16, 32, "prev_ab_up2"), (24, 8, 20, "prev_up2"),
                                         (40, 16, 8, "prev_ab")])
def test_warp_blend(g, Hs, h, Cc, mode):
    """The non-square construction, seeds and tolerance of test_hip_flow_decode.test_warp_blend, three frames."""
    Tn, Ws = 3, Hs + 8
    w = Ws if Hs == h else h
    skip = rnd(Hs * Ws, Cc, seed=1)
    grid, conf = motion(Tn, h, w, seed=Hs + Cc)
    prev = rnd(Tn * Hs * Ws, Cc, seed=2) if mode != "first" else None
    ab = (rnd(Cc, seed=3), rnd(Cc, seed=4)) if "ab" in mode else None
    up2 = "up2" in mode
    want = ref.warp_blend(skip, Hs, Ws, grid, conf, prev=prev, prev_ab=ab, up2=up2)
    got = g.warp_blend(gin(g, skip, "skip"), Hs, Ws, gin(g, grid, "grid"), gin(g, conf, "conf"), prev=gin(g, prev, "prev"),
                       prev_ab=gin(g, ab, "prev_ab"), up2=up2)
    torch.cuda.synchronize()
    check(f"guard/warp_blend/{Hs}x{Ws}_from_{h}x{w}_C{Cc}_{mode}", got, want, 2e-5)
    finish(g, alloc=("warp_blend.out",))


def test_warp_blend_frame_range_view(g):
    """test_hip_flow_decode.test_warp_blend_frame_range_view: the grid planes of frames [2, 6) of a 7-frame clip.  The whole clip is the
    guarded input: the frames outside the range are in-buffer data that the reference does not see."""
    Ttot, h, w, Hs, Ws, Cc = 7, 8, 8, 16, 16, 32
    grid, conf = motion(Ttot, h, w, seed=5)
    skip = rnd(Hs * Ws, Cc, seed=1)
    gd = gin(g, grid, "grid")[:, 2:6]
    assert gd.stride(0) == Ttot * h * w
    got = g.warp_blend(gin(g, skip, "skip"), Hs, Ws, gd, gin(g, conf[2:6], "conf"))
    torch.cuda.synchronize()
    check("guard/warp_blend/frame_range", got, ref.warp_blend(skip, Hs, Ws, grid[:, 2:6], conf[2:6]), 2e-5)
    finish(g, alloc=("warp_blend.out",))


# the three final_conv_blend forms: T = 3 frames, written into frames [F0, F1) of a 5-frame output, the flow taken from frames [G0, G1) of a
# 7-frame clip
TN, TOUT, F0, F1, TGRID, G0, G1 = 3, 5, 1, 4, 7, 2, 5


def fc_case(H, W, Cc, h, w):
    """Inputs of test_hip_yuv420._inputs (those of test_final_conv_blend / test_final_conv_blend_u8_bit_exact with three frames) on the CPU,
    and RefOps.final_conv_blend of them."""
    def make():
        x, w7, b3, src, grid, conf = (t.cpu() for t in YUV._inputs(H, W, Cc, h, w, TGRID))
        out, warped = torch.zeros(3, TN, H, W), torch.zeros(3, TN, H, W)
        ref.final_conv_blend(x, H, W, w7, b3, src, grid[:, G0:G1], conf[G0:G1], out, warped)
        return dict(x=x, w7=w7, b3=b3, src=src, grid=grid, conf=conf[G0:G1].contiguous(), out=out, warped=warped)
    return cached(("fc", H, W, Cc, h, w), make)


def fc_args(g, c, H, W):
    grid = gin(g, c["grid"], "grid")[:, G0:G1]
    assert grid.stride(0) == TGRID * c["grid"].shape[2] * c["grid"].shape[3]
    return (gin(g, c["x"], "x"), H, W, gin(g, c["w7"], "w7"), gin(g, c["b3"], "bias3"), gin(g, c["src"], "src"), grid, gin(g, c["conf"], "conf"))


def fc_plain(c):
    """The same operands unguarded, for the launches the byte forms are compared with."""
    return (c["x"].cuda(), c["w7"].cuda(), c["b3"].cuda(), c["src"].cuda(), c["grid"].cuda()[:, G0:G1], c["conf"].cuda())


@pytest.mark.parametrize("H,W,Cc,h,w", [(32, 32, 16, 8, 8), (40, 72, 64, 10, 18)])
def test_final_conv_blend(g, H, W, Cc, h, w):
    """(40, 72): tiles cut at the right and at the bottom.  Values: test_hip_flow_decode.test_final_conv_blend (RefOps, 2e-5)."""
    c = fc_case(H, W, Cc, h, w)
    ov = g.guarded_out(3 * TOUT, H * W, name="final_conv_blend.out_vid").view(3, TOUT, H, W)[:, F0:F1]
    wv = g.guarded_out(3 * TOUT, H * W, name="final_conv_blend.warped_vid").view(3, TOUT, H, W)[:, F0:F1]
    g.final_conv_blend(*fc_args(g, c, H, W), ov, wv)
    torch.cuda.synchronize()
    check(f"guard/final_conv_blend/out_{H}x{W}_C{Cc}", ov, c["out"], 2e-5)
    check(f"guard/final_conv_blend/warped_{H}x{W}_C{Cc}", wv, c["warped"], 2e-5)
    m = rows_mask(3, TOUT, F0, F1)
    finish(g, written={"final_conv_blend.out_vid": m, "final_conv_blend.warped_vid": m})


@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("H,W,Cc,h,w", [(32, 32, 16, 8, 8), (40, 72, 64, 10, 18)])
def test_final_conv_blend_u8(g, H, W, Cc, h, w, bgr):
    """Values: test_hip_decode_u8.test_final_conv_blend_u8_bit_exact -- the bytes of frames_to_u8(final_conv_blend(...)), bit for bit.  Zero
    mean and a source image below 1: the expected bytes hold no 255 (asserted on the CPU reference, and on the bytes compared with)."""
    c = fc_case(H, W, Cc, h, w)
    assert_no_255(ref.frames_to_u8(c["out"], bgr=bgr))
    x, w7, b3, src, grid, conf = fc_plain(c)
    want = U8._two_step(plain(), x, H, W, w7, b3, src, grid, conf, TN, (0.0, 0.0, 0.0), bgr)
    assert_no_255(want.cpu())
    frames = g.guarded_out(TOUT, H * W * 3, dtype=torch.uint8, name="final_conv_blend_u8.frames").view(TOUT, H, W, 3)[F0:F1]
    g.final_conv_blend_u8(*fc_args(g, c, H, W), frames, bgr=bgr)
    torch.cuda.synchronize()
    assert torch.equal(frames, want), int((frames != want).sum())
    finish(g, written={"final_conv_blend_u8.frames": slice(F0, F1)})


@pytest.mark.parametrize("H,W,Cc,h,w", [(16, 32, 8, 4, 8), (24, 40, 8, 6, 10), (18, 36, 8, 5, 9)])
def test_final_conv_blend_yuv420(g, H, W, Cc, h, w):
    """Values: test_hip_yuv420.test_final_conv_blend_yuv420 -- the restatement of the I420 definition applied to final_conv_blend_u8's bytes."""
    c = fc_case(H, W, Cc, h, w)
    x, w7, b3, src, grid, conf = fc_plain(c)
    rgb = torch.empty(TN, H, W, 3, device="cuda", dtype=torch.uint8)
    plain().final_conv_blend_u8(x, H, W, w7, b3, src, grid, conf, rgb)
    want = yuv420_np(rgb.cpu().numpy())
    assert_no_255(yuv420_np(ref.frames_to_u8(c["out"]).numpy()))
    assert_no_255(want)
    frames = g.guarded_out(TOUT, 3 * H * W // 2, dtype=torch.uint8, name="final_conv_blend_yuv420.frames")[F0:F1]
    g.final_conv_blend_yuv420(*fc_args(g, c, H, W), frames)
    torch.cuda.synchronize()
    YUV._eq(frames, want)
    finish(g, written={"final_conv_blend_yuv420.frames": slice(F0, F1)})


def _unit_clip(Ttot, H, W, seed):
    """(3, Ttot, H, W) fp32 that clips at 0 and stays below 1: no expected RGB byte is 255."""
    return torch.rand(3, Ttot, H, W, generator=torch.Generator().manual_seed(seed)) * 1.1 - 0.15


@pytest.mark.parametrize("bgr", [False, True], ids=["rgb", "bgr"])
@pytest.mark.parametrize("T,H,W", [(1, 1, 4), (2, 6, 88)], ids=["4_pixels", "1056_pixels"])
def test_frames_to_u8(g, T, H, W, bgr):
    """The smallest pixel count the entry takes (four: one thread) and one that crosses a 256-thread block (264 threads), as a frame range
    of a longer clip.  Values: RefOps.frames_to_u8, bit-exact (test_hip_flow_decode.test_frames_to_u8_bit_exact)."""
    clip = _unit_clip(T + 2, H, W, seed=3)
    want = ref.frames_to_u8(clip[:, 1:1 + T], bgr=bgr)
    assert_no_255(want)
    assert bool((want == 0).any()) or T * H * W == 4
    got = g.frames_to_u8(gin(g, clip, "vid")[:, 1:1 + T], bgr=bgr)
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.shape == (T, H, W, 3) and torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    finish(g, alloc=("frames_to_u8.out",))


def test_frames_to_u8_refuses_a_pixel_count_off_4(g):
    with pytest.raises(_lib.DawnHipError, match="multiples of 4"):
        g.frames_to_u8(gin(g, _unit_clip(1, 3, 2, seed=1), "vid"))
    torch.cuda.synchronize()
    assert names(g) == {"frames_to_u8.out"}
    for r in g.outs:
        r.check_surroundings("refused, yet written")
        assert bool(_poisoned(r.payload).all()), "refused, yet written"
    g.inputs_intact()


@pytest.mark.parametrize("H,W", [(2, 4), (18, 36)])
def test_frames_to_yuv420(g, H, W):
    """Values: test_hip_yuv420.test_frames_to_yuv420 (byte levels (k + 0.5) / 255, a mean that clips at both ends; the numpy restatement of
    the definition on RefOps.frames_to_u8's bytes).  vid = frames [1, 4) of a 5-frame clip; the op's own allocation, and a caller's `out`
    that is frames [1, 4) of a 5-frame I420 clip."""
    Tn, Ttot, mean = 3, 5, (3.0, -2.5, 40.0)
    k = torch.randint(0, 256, (3, Ttot, H, W), generator=torch.Generator().manual_seed(H * 100 + W))
    vid = ((k.float() + 0.5) / 255.0).contiguous()
    want = yuv420_np(ref.frames_to_u8(vid[:, 1:1 + Tn], mean=mean, bgr=False).numpy())
    assert_no_255(want)
    got = g.frames_to_yuv420(gin(g, vid, "vid")[:, 1:1 + Tn], mean=mean)
    torch.cuda.synchronize()
    YUV._eq(got, want)
    finish(g, alloc=("frames_to_yuv420.out",))
    g.reset()
    out = g.guarded_out(Ttot, 3 * H * W // 2, dtype=torch.uint8, name="frames_to_yuv420.out")[1:1 + Tn]
    got = g.frames_to_yuv420(gin(g, vid, "vid")[:, 1:1 + Tn], mean=mean, out=out)
    torch.cuda.synchronize()
    assert got is out
    YUV._eq(got, want)
    finish(g, written={"frames_to_yuv420.out": slice(1, 1 + Tn)})


# ---------------------------------------------------------------------------------------------- HuBERT, PBnet
@pytest.mark.parametrize("n", [1, 2047, 2049])
def test_wave_normalize(g, n):
    """One block of the normalising kernel is 256 x 8 samples.  Values: numpy's float32 statistics at 5e-6 (tests/test_hip_hubert.py); the
    fp64 statistics `st` must be written completely, too."""
    x = HB.rnd(n, seed=3) * 0.2 + 0.05
    xr = x.numpy()
    want = torch.from_numpy((xr - xr.mean()) / np.sqrt(xr.var() + 1e-7))
    got = g.wave_normalize(gin(g, x, "x"))
    torch.cuda.synchronize()
    close(f"wave_normalize/n{n}", got, want, 5e-6)
    finish(g, alloc=("wave_normalize.st", "wave_normalize.out"))


@pytest.mark.parametrize("n", [10, 4014])
def test_hubert_conv0(g, n):
    """stage_gate's geometry and inputs (k = 10, stride = 5, C = 512): n = k is one output row, n = 4014 leaves four samples over.  Values:
    RefOps at 2e-5 (tests/test_hip_hubert.py), and stage_gate's fp64 gate where stage_gate has the case."""
    case = S.Case(f"hubert_conv0/n{n}", "conv0", n=n)
    t = cached(("conv0", n), case.make)
    want = ref.hubert_conv0(t["x"], t["w"], t["bias"], 5)
    got = g.hubert_conv0(gin(g, t["x"], "x"), gin(g, t["w"], "w"), gin(g, t["bias"], "bias"), 5)
    torch.cuda.synchronize()
    assert got.shape == want.shape == ((n - 10) // 5 + 1, 512)
    close(f"hubert_conv0/n{n}", got, want, 2e-5)
    if case.name in [c.name for c in S.CASES]:
        S.fp32_gate("guard/" + case.name, got, case.want64(t), case.base32(t), c=case.c)
    finish(g, alloc=("hubert_conv0.out",))


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("C", [4, 260, 1024])
@pytest.mark.parametrize("rows", [1, 5])
def test_ln_affine_act(g, rows, C, act):
    """One wave per row, four rows per workgroup, 256 channels per pass.  Inputs and tolerance of test_hip_hubert.test_ln_affine_act."""
    x, ga, be = HB.rnd(rows, C, seed=1) * 1.5 + 0.3, HB.rnd(C, seed=2) * 0.3 + 1, HB.rnd(C, seed=3) * 0.2
    got = g.ln_affine_act(gin(g, x, "x"), gin(g, ga, "gamma"), gin(g, be, "beta"), 1e-5, act)
    torch.cuda.synchronize()
    close(f"ln_affine_act/{rows}x{C}_act{act}", got, ref.ln_affine_act(x, ga, be, 1e-5, act), 2e-5)
    finish(g, alloc=("ln_affine_act.out",))


@pytest.mark.parametrize("act", [0, 2])
@pytest.mark.parametrize("n", [4, 1028])
def test_add_act(g, n, act):
    """One 128-bit access, and 257 of them (a second block).  a None and given; the op's allocation, a caller's `out`, and the in-place form
    of stage_gate's `inplace` case (a None, out = b).  Tolerance of tests/test_hip_hubert.py: 2e-6."""
    a, b = HB.rnd(n, seed=1), HB.rnd(n, seed=2) * 2
    for with_a in (False, True):
        want = ref.add_act(a if with_a else None, b, act)
        for mode in ("alloc", "out"):
            g.reset()
            out = g.guarded_out(1, n, name="out").view(n) if mode == "out" else None
            got = g.add_act(gin(g, a, "a") if with_a else None, gin(g, b, "b"), act, out=out)
            torch.cuda.synchronize()
            assert out is None or got is out
            close(f"add_act/n{n}_act{act}_a{int(with_a)}/{mode}", got, want, 2e-6)
            finish(g, alloc=("add_act.out",) if out is None else ())
    g.reset()
    bg = gin(g, b, "b")
    got = g.add_act(None, bg, act, out=bg)
    torch.cuda.synchronize()
    assert got is bg
    close(f"add_act/n{n}_act{act}/inplace", got, ref.add_act(None, b, act), 2e-6)
    finish(g, overwritten=("b",))


@pytest.mark.parametrize("case", HC.CASES, ids=lambda c: "T%d_E%d_g%d_k%d" % c)
def test_hubert_pos_conv(g, case):
    """The table of tests/test_hip_hubert_c.py: T = 63, 64, 65 around the 64-row tile, k = 32 and odd k = 3 / 7 / 5, group widths 16 (E 32 / 2
    groups), 48 (gw % 32 == 16), 64 and 128, the production width.  Inputs, references and the elementwise tolerance 1e-4 * max(1, |ref|)
    of test_pos_conv_vs_torch; the op's own allocation and a caller's `out`."""
    T, E, groups, k = case
    d = HC.inputs(case)
    for mode in ("alloc", "out"):
        g.reset()
        out = g.guarded_out(T, E, name="out") if mode == "out" else None
        got = g.hubert_pos_conv(gin(g, d["hid"], "hid"), gin(g, d["w"], "w"), gin(g, d["bias"], "bias"), groups, k, out=out)
        torch.cuda.synchronize()
        assert (out is None or got is out) and got.shape == d["hid"].shape
        got = got.cpu()
        assert not torch.isnan(got).any()
        for name, r in (("float64", d["want64"]), ("fp32 CPU", d["base32"].double())):
            excess = ((got.double() - r).abs() - 1e-4 * r.abs().clamp_min(1.0)).max()
            assert float(excess) <= 0, (case, mode, name, float(excess))
        finish(g, alloc=("hubert_pos_conv.out",) if out is None else ())


@pytest.mark.parametrize("T", [1, 33, 65])
def test_attn64(g, T):
    """Both sides of the 32-query and 32-key tiles, two heads.  Inputs and tolerance of test_hip_hubert.test_attn64."""
    heads = 2
    qkv = HB.rnd(T, 3 * heads * 64, seed=T) * 1.2
    got = g.attn64(gin(g, qkv, "qkv"), heads)
    torch.cuda.synchronize()
    close(f"attn64/T{T}", got, ref.attn64(qkv, heads), 2e-5)
    finish(g, alloc=("attn64.out",))


def test_interp_linear(g):
    """n = 7 samples of 5 channels at positions that contain 0, n - 1, exact integers and points between them.  Bit-exact against scipy
    (test_hip_hubert.test_interp_linear_bit_exact_vs_scipy)."""
    n, C = 7, 5
    y = HB.rnd(n, C, seed=7)
    xi = torch.tensor([0.0, 0.25, 1.0, 1.5, 2.0, 2.999999, 3.0, 4.75, 5.0, 5.5, float(n - 1)], dtype=torch.float64)
    want = ref.interp_linear(y, xi)
    got = g.interp_linear(gin(g, y, "y"), gin(g, xi, "xi"))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    finish(g, alloc=("interp_linear.out",))


@pytest.mark.parametrize("Tq,Tk", [(1, 5), (65, 64), (64, 65)])
def test_attn_bias32(g, Tq, Tk):
    """stage_gate's attn_bias32 inputs at unit scale (4 heads of 32, one (T, 384) projection, 2 rotary pairs, the eval-mode window mask):
    q | k | v as column slices of the projection, as separate contiguous tensors and as column slices of wider ones; bias None and given;
    with and without the rotary tables.  Values: RefOps at 2e-5 (test_hip_pbnet.test_attn_bias32); with everything present, stage_gate's fp64
    gate as well."""
    case = [c for c in S.CASES if c.name == f"attn_bias32/{Tq}x{Tk}_sigma1"][0]
    t = cached(("attn32", Tq, Tk), case.make)
    q, k, v = case.qkv32(t["qkv"])
    scale = 32 ** -0.5
    for with_bias in (False, True):
        for with_rot in (False, True):
            bias = t["bias"] if with_bias else None
            rc, rs = (t["rc"], t["rs"]) if with_rot else (None, None)
            want = ref.attn_bias32(q, k, v, S.HEADS32, bias, rc, rs, scale)
            for layout in ("projection", "separate", "slices"):
                g.reset()
                if layout == "projection":
                    qg, kg, vg = case.qkv32(gin(g, t["qkv"], "qkv"))
                    assert qg.stride(0) == 384
                else:
                    pad = PAD if layout == "slices" else 0
                    qg, kg, vg = (gin(g, x.contiguous(), n, pad) for x, n in ((q, "q"), (k, "k"), (v, "v")))
                got = g.attn_bias32(qg, kg, vg, S.HEADS32, gin(g, bias, "bias"), gin(g, rc, "rcos"), gin(g, rs, "rsin"), scale)
                torch.cuda.synchronize()
                tag = f"guard/attn_bias32/{Tq}x{Tk}_b{int(with_bias)}_r{int(with_rot)}/{layout}"
                check(tag, got, want, 2e-5)
                if with_bias and with_rot:
                    S.fp32_gate(tag, got, case.want64(t), case.base32(t), c=case.c)
                finish(g, alloc=("attn_bias32.out",))


# ---------------------------------------------------------------------------------------------- sampler
N_WRAP = 2048 * 256 + 3          # grid_for caps at 2048 blocks of 256: the last three elements are the second trip of the first three threads
RECIP, RECIPM1 = 1.8371, 1.5411  # the step scalars of test_hip_clip.test_fused_step_kernels_bit_identical_to_the_two_launch_sequence


def vec(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


def hist_of(x0):
    bits = (x0.abs().cpu().contiguous().view(torch.int32) >> 20).flatten().long()
    return torch.bincount(bits, minlength=2048).to(torch.int32)


@pytest.mark.parametrize("n", [7, 1000, N_WRAP])
def test_ddim_x0(g, n):
    """Values: test_hip_ops.test_ddim_x0_and_histogram (RefOps at 1e-6; the histogram exact against a bincount of the result's bits)."""
    x, e = vec(n, 1), vec(n, 2)
    wx0, _ = ref.ddim_x0(x, e, 1.25, 0.75)
    gx0, gh = g.ddim_x0(gin(g, x, "x"), gin(g, e, "eps"), 1.25, 0.75)
    torch.cuda.synchronize()
    check(f"guard/ddim_x0/n{n}", gx0, wx0, 1e-6)
    assert torch.equal(gh.cpu(), hist_of(gx0)) and int(gh.sum()) == n, "histogram not exact"
    finish(g, alloc=("ddim_x0.x0",))


@pytest.mark.parametrize("n", [7, 1000, N_WRAP])
def test_cfg_x0(g, n):
    """Values: test_hip_guided.test_cfg_x0_kernel_bit_identical_to_combine_then_x0 -- eps, x0 and the histogram bit-identical to cfg_combine
    followed by ddim_x0.  Then eps_out aliasing e_null, through the C entry (the Python entry always allocates eps)."""
    scale = 2.5
    e_n, e_c, x = vec(n, 1), vec(n, 2, 1.3), vec(n, 3, 2.0)
    P = plain()
    eps = P.cfg_combine(e_n.cuda(), e_c.cuda(), scale)
    x0, hist = P.ddim_x0(x.cuda(), eps, 1.37, 0.91)
    x0, hist = x0.clone(), hist.clone()
    check(f"guard/cfg_x0/eps_n{n}", eps, ref.cfg_combine(e_n, e_c, scale), 1e-6)
    eps2, x02, hist2 = g.cfg_x0(gin(g, e_n, "e_null"), gin(g, e_c, "e_cond"), scale, gin(g, x, "x"), 1.37, 0.91)
    torch.cuda.synchronize()
    assert torch.equal(eps2, eps) and torch.equal(x02, x0) and torch.equal(hist2, hist) and int(hist2.sum()) == n
    finish(g, alloc=("cfg_x0.eps", "cfg_x0.x0"))
    g.reset()
    en = gin(g, e_n, "e_null")
    x0o = g.guarded_out(1, n, name="x0").view(n)
    h = g.guarded_out(1, 2048, name="hist", dtype=torch.int32).view(2048)
    h.zero_()
    rc = g.L.dawn_cfg_x0(en.data_ptr(), gin(g, e_c, "e_cond").data_ptr(), scale, gin(g, x, "x").data_ptr(), 1.37, 0.91, n, en.data_ptr(),
                         x0o.data_ptr(), h.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, g.L.dawn_last_error()
    assert torch.equal(en, eps) and torch.equal(x0o, x0) and torch.equal(h, hist)
    finish(g, overwritten=("e_null",))


@pytest.mark.parametrize("n,scale", [(11, 2.0), (100001, 0.5)])
def test_quantile_threshold(g, n, scale):
    """Inputs and tolerance of test_hip_ops.test_quantile_matches_torch.  On the guarded x0 that ddim_x0 returns, with its histogram (the
    selection scratch cached per stream: not guarded); and on a guarded input with a histogram from elsewhere, where the private scratch is
    guarded too and completely written (the reset fills all of it)."""
    v = rnd(n, seed=n % 97) * scale
    want = float(torch.quantile(v.abs(), 0.9))

    def value(s):
        s = s.cpu()
        assert float(s[1]) == pytest.approx(want, rel=0, abs=1e-6 * max(1, want)), (float(s[1]), want)
        assert float(s[0]) == max(1.0, float(s[1]))
    x0, hist = g.ddim_x0(gin(g, v, "x"), gin(g, torch.zeros(n), "eps"), 1.0, 0.0)
    s = g.quantile_threshold(x0, hist, n, 0.9)
    torch.cuda.synchronize()
    value(s)
    assert "quantile_threshold.ws" not in names(g)
    finish(g, alloc=("ddim_x0.x0", "quantile_threshold.out"))
    g.reset()
    elsewhere = hist.clone()
    s = g.quantile_threshold(gin(g, v, "x0"), gin(g, elsewhere.cpu(), "hist1"), n, 0.9)
    torch.cuda.synchronize()
    value(s)
    finish(g, alloc=("quantile_threshold.out", "quantile_threshold.ws"))


@pytest.mark.parametrize("with_noise", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("n", [7, 1000])
def test_ddim_update(g, n, with_noise):
    """Values: test_hip_ops.test_ddim_update_and_cfg (RefOps at 1e-6)."""
    x0, e, nz, s = vec(n, 1, 2.0), vec(n, 2), vec(n, 3) if with_noise else None, torch.tensor([1.7, 1.7])
    a = (0.9, 0.3, 0.2) if with_noise else (1.0, 0.0, 0.0)
    got = g.ddim_update(gin(g, x0, "x0"), gin(g, e, "eps"), gin(g, s, "s"), gin(g, nz, "noise"), *a)
    torch.cuda.synchronize()
    check(f"guard/ddim_update/n{n}_noise{int(with_noise)}", got, ref.ddim_update(x0, e, s, nz, *a), 1e-6)
    finish(g, alloc=("ddim_update.x",))


@pytest.mark.parametrize("with_noise", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("n", [7, 1000])
def test_ancestral_update(g, n, with_noise):
    """Values: test_hip_ancestral.test_ancestral_update_kernel_bit_identical_to_ddim_update -- the bits of ddim_update(x0, eps := x_t, c1, c2,
    std), out of place and in place (out = x_t) -- and RefOps's ddim_update at 1e-6."""
    x0, xt, nz, s = vec(n, 1, 2.5), vec(n, 2), vec(n, 3) if with_noise else None, torch.tensor([1.7, 1.7])
    a = (0.0123, 0.9871, 0.0456) if with_noise else (1.0, 0.0, 1e-10)
    want = plain().ddim_update(x0.cuda(), xt.cuda(), s.cuda(), None if nz is None else nz.cuda(), *a)
    check(f"guard/ancestral_update/n{n}_noise{int(with_noise)}", want, ref.ddim_update(x0, xt, s, nz, *a), 1e-6)
    got = g.ancestral_update(gin(g, x0, "x0"), gin(g, xt, "x_t"), gin(g, s, "s"), gin(g, nz, "noise"), *a)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    finish(g, alloc=("ancestral_update.out",))
    g.reset()
    xg = gin(g, xt, "x_t")
    got = g.ancestral_update(gin(g, x0, "x0"), xg, gin(g, s, "s"), gin(g, nz, "noise"), *a, out=xg)
    torch.cuda.synchronize()
    assert got is xg and torch.equal(got, want)
    finish(g, overwritten=("x_t",))


def off_view(g, t, name, off):
    """The 1-D CPU tensor t as a guarded input; off = 1: as a view that starts one float into a guarded buffer (not 16-byte aligned)."""
    if t is None:
        return None
    if not off:
        return gin(g, t, name)
    v = gin(g, torch.cat((t.new_zeros(1), t)), name)[1:]
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize("with_noise", [False, True], ids=["no_noise", "noise"])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset_one_float"])
@pytest.mark.parametrize("n", [3, 4, 7, 1027])
def test_step_fixed(g, n, off, with_noise):
    """dawn_ddim_step_fixed / dawn_ancestral_step_fixed: aligned operands take the 128-bit body over n // 4 * 4 elements and the scalar tail
    (n = 3: below the body; 4: no tail; 7 and 1027: both, 1027 in a second block), the offset views take the scalar path.  Values:
    bit-identical to the two-launch sequence with s = 1, as test_hip_clip.test_fused_step_kernels_bit_identical_to_the_two_launch_sequence;
    with the x0 output, without it, and in place (out = x)."""
    x, eps, nz = vec(n, 1, 1.5), vec(n, 2), vec(n, 3) if with_noise else None
    a, b, sg = (0.6123, 0.5871, 0.3456) if with_noise else (1.0, 0.0, 1e-10)
    P = plain()
    one = torch.ones(2, device="cuda")
    xc, ec, nc = x.cuda(), eps.cuda(), None if nz is None else nz.cuda()
    x0, _ = P.ddim_x0(xc, ec, RECIP, RECIPM1)
    x0 = x0.clone()
    wants = {"ddim_step_fixed": P.ddim_update(x0, ec, one, nc, a, b, sg), "ancestral_step_fixed": P.ancestral_update(x0, xc, one, nc, a, b, sg)}
    for fn, want in wants.items():
        for form in ("x0", "plain", "inplace"):
            g.reset()
            xg, eg, ng = off_view(g, x, "x", off), off_view(g, eps, "eps", off), off_view(g, nz, "noise", off)
            call = getattr(g, fn)
            if form == "x0":
                got, x0_got = call(xg, eg, ng, RECIP, RECIPM1, a, b, sg, clamp=True, want_x0=True)
                torch.cuda.synchronize()
                assert torch.equal(x0_got, x0), (fn, form)
            else:
                got = call(xg, eg, ng, RECIP, RECIPM1, a, b, sg, clamp=True, out=xg if form == "inplace" else None)
                assert form != "inplace" or got is xg
            torch.cuda.synchronize()
            assert torch.equal(got, want), (fn, form, int((got != want).sum()))
            finish(g, alloc={"x0": ("_step_fixed.out", "_step_fixed.x0"), "plain": ("_step_fixed.out",), "inplace": ()}[form],
                   overwritten=("x",) if form == "inplace" else ())


@pytest.mark.parametrize("n", [7, 1001])
def test_cfg_combine(g, n):
    e_n, e_c = vec(n, 1, 2.0), vec(n, 2)
    got = g.cfg_combine(gin(g, e_n, "e_null"), gin(g, e_c, "e_cond"), 2.5)
    torch.cuda.synchronize()
    check(f"guard/cfg_combine/n{n}", got, ref.cfg_combine(e_n, e_c, 2.5), 1e-6)
    finish(g, alloc=("cfg_combine.out",))


@pytest.mark.parametrize("C,F,f0,Ftotal,hw", [(3, 2, 1, 5, 4), (3, 2, 0, 2, 12)])
def test_philox_normal(g, C, F, f0, Ftotal, hw):
    """One 128-bit store per four elements: a shard of frames [1, 3) of five with one store per frame, and a whole clip with three.  Values:
    the reference generator of test_hip_ops.test_philox_normal at its 2e-5."""
    got = g.philox_normal(C, F, f0, Ftotal, hw, 1234, 1, "cuda")
    torch.cuda.synchronize()
    assert got.shape == (C, F, hw)
    check(f"guard/philox_normal/{C}x{F}x{hw}_f{f0}of{Ftotal}", got, ref.philox_normal(C, F, f0, Ftotal, hw, 1234, 1, "cpu"), 2e-5)
    finish(g, alloc=("philox_normal.out",))


# ---------------------------------------------------------------------------------------------- the C-side hosts
def host_check(go, outputs):
    """The hosts' buffers: every band intact; the outputs hold no poison; the workspace -- scratch that the same call produces and
    consumes -- is checked at its bands only."""
    torch.cuda.synchronize()
    for r in go.outs:
        r.check_surroundings("write outside the buffer")
        if r.name in outputs:
            assert not bool(_poisoned(r.payload).any()), f"{r.name}: elements never written"
    assert set(outputs) <= names(go)
    go.inputs_intact()


def workspace(go, nbytes):
    ws = go.guarded_out(1, nbytes, dtype=torch.uint8, name="workspace").view(nbytes)
    assert ws.numel() == nbytes and ws.data_ptr() % 256 == 0
    return ws


def test_hubert_evaluator_in_an_exact_workspace(g):
    """dawn_hubert_features at the tiny golden's short utterance with a workspace of exactly dawn_hubert_workspace_bytes: the same bits as
    with the evaluator's own workspace, which tests/test_hip_hubert_c.py holds to the reference golden at 3e-4."""
    gd = load_golden("hubert_tiny.npz")
    sd = {k[3:]: T_(v) for k, v in gd.items() if k.startswith("sd/")}
    hf = HC.HubertFeatures(sd, "cuda:0", num_heads=int(gd["num_heads"]), pos_groups=int(gd["pos_groups"]))
    ev = hf.evaluator()
    sp = torch.from_numpy(np.ascontiguousarray(gd["speech"][:int(gd["n_short"])], dtype=np.float32))
    want_hidden, want_target = ev.features(sp.cuda())
    close("hubert_c/hidden_short", want_hidden, T_(gd["hidden_short"]), 3e-4)
    _, eT, nf = ev.segments(sp.numel())
    hidden, target = g.guarded_out(eT, hf.E, name="hidden"), g.guarded_out(nf, hf.E, name="target")
    ev.features(gin(g, sp, "speech"), workspace=workspace(g, ev.workspace_bytes(sp.numel())), hidden=hidden, target=target)
    host_check(g, ("hidden", "target"))
    assert torch.equal(hidden, want_hidden) and torch.equal(target, want_target)


@pytest.mark.parametrize("name", ["pose", "blink"])
def test_pbnet_evaluator_in_an_exact_workspace(g, name):
    """dawn_pbnet_generate at the tiny golden's T = 20 case with a workspace of exactly dawn_pbnet_workspace_bytes: the same bits as
    `generate(via_c=True)`, which tests/test_hip_pbnet_c.py holds to the reference golden at 2e-5."""
    import test_hip_pbnet_c as PC
    gd = load_golden("pbnet_tiny.npz")
    gen = PC.tiny_gen(gd, name)
    init, audio, dur, z = (T_(gd[f"{name}:T20:{k}"]) for k in ("init", "audio", "dur", "z"))
    want = gen.generate(init, audio, dur, fact=1, z=z, via_c=True)["output"][0]
    check(f"guard/pbnet_c/{name}_T20", want, T_(gd[f"{name}:T20:out"])[0], 2e-5)
    ev = gen.c_evaluator()
    Tn = audio.shape[1]
    out = g.guarded_out(Tn, gen.in_dim, name="out")
    ev.generate(gin(g, init[0, 0].float(), "x0"), gin(g, audio[0].float(), "audio"), gin(g, z[:, 0].float().contiguous(), "z"),
                workspace=workspace(g, ev.workspace_bytes(Tn)), out=out)
    host_check(g, ("out",))
    assert torch.equal(out, want)


def test_u8_decoder_in_an_exact_workspace(g):
    """dawn_decode_clip_conf at the tiny golden (32 x 32, T = 5, chunk 2) into guarded RGB frames with a workspace of exactly
    dawn_decoder_workspace_bytes: the bytes of FlowDecoder.decode_clip_u8, as tests/test_hip_decode_u8.py expects of this host.  Zero mean;
    the expected bytes hold no 255 (asserted on the reference golden's own frames and on the bytes compared with)."""
    from dawn_pytorch_amd.ctx import DecoderEvaluator
    from dawn_pytorch_amd.flow_decoder import FlowDecoder
    gd, sd = U8._golden()
    dec = FlowDecoder(sd, "cuda", ops=plain(), chunk=2)
    de = DecoderEvaluator(dec)
    src, grid, conf = T_(gd["img"])[0].contiguous(), T_(gd["grid"])[0].contiguous(), T_(gd["conf"])[0, 0].contiguous()
    assert_no_255(ref.frames_to_u8(T_(gd["sample_out_vid"])[0]))
    want = dec.decode_clip_u8(src[None].cuda(), grid[None].cuda(), conf[None, None].cuda())[0]
    assert_no_255(want.cpu())
    srcg = gin(g, src, "img")
    mem, _ = de.encode(srcg)
    frames = g.guarded_out(5, 32 * 32 * 3, dtype=torch.uint8, name="frames").view(5, 32, 32, 3)
    de.decode(srcg, mem, T=5, h=8, w=8, chunk=2, grid=gin(g, grid, "grid"), conf=gin(g, conf, "conf"), frames=frames,
              workspace=workspace(g, de.workspace_bytes(32, 32, 2)))
    host_check(g, ("frames",))
    assert torch.equal(frames, want), int((frames != want).sum())
