"""No GPU: the use_deconv=False upsampler (nearest x2 + 3x3 conv, MT:169-172) as four output phases of 2x2 folded taps over the
low-resolution input -- the weight folding against the literal form in fp64, the module surface, the host orchestration against
goldens generated from the reference (tools/gen_goldens_upconv.py), and the additive C-ABI pieces."""
import ctypes

import pytest
import torch

from conftest import load_golden
from oracle.ops_ref import RefOps
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.pack import deconv_w_kn_phases, pack_unet, unpack_kn, up_border, upconv_w_kn_phases
from dawn_pytorch_amd.unet_forward import build_clip_state, unet_forward
from upconv_cases import MODES, TINY_KW, literal_upconv, tiny_upconv_sd

T = torch.from_numpy


def eval_phases(img, blocks, border):
    """Gather evaluator of the kernels' mode 1: img (F, Ci, H, W), blocks (4, 4 Ci, Co) in the order of deconv_w_kn_phases
    (phase = 2 py + px, k = (2 ty + tx) Ci + c; tap 0 at offset 0, tap 1 at -1 / +1 by phase bit) -> (F, Co, 2H, 2W).  A tap outside
    the input reads zero (border 0), the edge pixel (1) or the opposite edge (2)."""
    Fr, Ci, H, W = img.shape
    Co = blocks.shape[2]
    out = img.new_zeros(Fr, Co, 2 * H, 2 * W)

    def index(i, n):
        inside = (i >= 0) & (i < n)
        if border == 0:
            return i.clamp(0, n - 1), inside
        return (i.clamp(0, n - 1) if border == 1 else i % n), torch.ones_like(inside)

    for py in range(2):
        for px in range(2):
            blk = blocks[2 * py + px].reshape(2, 2, Ci, Co)
            acc = img.new_zeros(Fr, Co, H, W)
            for ty in range(2):
                for tx in range(2):
                    dy = 0 if ty == 0 else (1 if py else -1)
                    dx = 0 if tx == 0 else (1 if px else -1)
                    iy, vy = index(torch.arange(H) + dy, H)
                    ix, vx = index(torch.arange(W) + dx, W)
                    g = img[:, :, iy][:, :, :, ix] * (vy[:, None] & vx[None, :]).to(img.dtype)
                    acc += torch.einsum("cn,fchw->fnhw", blk[ty, tx], g)
            out[:, :, py::2, px::2] = acc
    return out


class BorderRefOps(RefOps):
    """RefOps whose mode-1 conv honours `border` (the unchanged RefOps rebuilds a transposed 4x4 kernel: exact for zero borders only)."""

    def conv_gemm(self, in0, w, N, *, border=0, **kw):
        if not border:
            return super().conv_gemm(in0, w, N, **kw)
        assert kw.pop("mode") == 1 and kw.pop("KH") == 2 and kw.pop("KW") == 2
        Fr, H, W, bias = kw.pop("F"), kw.pop("Hi"), kw.pop("Wi"), kw.pop("bias", None)
        assert (kw.pop("Ho"), kw.pop("Wo")) == (2 * H, 2 * W) and all(v is None for v in kw.values()), kw
        blocks = torch.stack([unpack_kn(w[i]) for i in range(4)], 0)
        y = eval_phases(in0.reshape(Fr, H, W, -1).permute(0, 3, 1, 2), blocks, border)
        y = y.permute(0, 2, 3, 1).reshape(Fr * 4 * H * W, N)
        return y if bias is None else y + bias


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,W", [(4, 4), (3, 5), (1, 2), (2, 1)])
def test_folded_phases_equal_the_literal_form(mode, H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    img = torch.randn(2, 5, H, W, generator=g, dtype=torch.float64)
    w5 = torch.randn(7, 5, 1, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(7, generator=g, dtype=torch.float64)
    # (the folding itself in fp64: upconv_w_kn_phases rounds its result once to fp32, which a 1e-12 gate would see)
    w32 = w5.float()
    blocks = upconv_w_kn_phases(w32)
    assert blocks.shape == (4, 20, 7) and blocks.dtype == torch.float32
    ksel = (((1, 2), (0,)), ((0, 1), (2,)))
    exact = torch.stack([torch.stack([sum(w5[:, :, 0, ky, kx] for ky in ksel[py][ty] for kx in ksel[px][tx]).t()
                                      for ty in range(2) for tx in range(2)], 0).reshape(20, 7)
                         for py in range(2) for px in range(2)], 0)
    want = literal_upconv(img, w5[:, :, 0], b, mode)
    got = eval_phases(img, exact, up_border(mode)) + b[None, :, None, None]
    assert float((got - want).abs().max()) <= 1e-12
    # ... and the packed function is that folding of the fp32 weights, summed in fp64 and rounded once
    want32 = literal_upconv(img, w32[:, :, 0].double(), b, mode)
    got32 = eval_phases(img, blocks.double(), up_border(mode)) + b[None, :, None, None]
    folded64 = torch.stack([torch.stack([sum(w32.double()[:, :, 0, ky, kx] for ky in ksel[py][ty] for kx in ksel[px][tx]).t()
                                         for ty in range(2) for tx in range(2)], 0).reshape(20, 7)
                            for py in range(2) for px in range(2)], 0)
    assert torch.equal(blocks, folded64.float())
    # one fp32 rounding per folded weight (2^-24 relative), 4 taps x 5 channels of |x| <~ 4, |w| <~ 8 per output
    assert float((got32 - want32).abs().max()) <= 20 * 4 * 8 * 2.0 ** -24


def test_phase_layout_is_that_of_the_transposed_conv():
    """Same block / tap order as deconv_w_kn_phases: a 3x3 kernel with one non-zero entry lands in the taps the derivation names."""
    w5 = torch.zeros(1, 1, 1, 3, 3)
    w5[0, 0, 0, 0, 2] = 1.0                                     # ky = 0, kx = 2
    ph = upconv_w_kn_phases(w5).reshape(2, 2, 2, 2)             # (py, px, ty, tx)
    want = torch.zeros(2, 2, 2, 2)
    want[0, 0, 1, 0] = want[0, 1, 1, 1] = want[1, 0, 0, 0] = want[1, 1, 0, 1] = 1.0
    assert torch.equal(ph, want)
    assert upconv_w_kn_phases(torch.zeros(6, 4, 1, 3, 3)).shape == deconv_w_kn_phases(torch.zeros(4, 6, 1, 4, 4)).shape
    with pytest.raises(ValueError):
        upconv_w_kn_phases(torch.zeros(4, 4, 1, 4, 4))


def test_up_border_values():
    assert [up_border(m) for m in MODES] == [0, 1, 1, 2]
    with pytest.raises(ValueError):
        up_border("bogus")
    with pytest.raises(ValueError):
        D.DynamicNfUnet3D(default_num_frames=12, **TINY_KW, padding_mode="bogus")
    # use_deconv=True ignores padding_mode, as the reference does
    D.DynamicNfUnet3D(default_num_frames=12, **{**TINY_KW, "use_deconv": True}, padding_mode="bogus")


def test_module_state_dict_is_the_reference_variant(tiny):
    g = load_golden("tiny_unet_upconv_reflect.npz")
    unet = D.DynamicNfUnet3D(default_num_frames=12, **TINY_KW, padding_mode="reflect")
    mine = {k: tuple(v.shape) for k, v in unet.state_dict().items() if k.startswith("ups.")}
    ref = {str(k): tuple(int(s) for s in str(v).split(",")) for k, v in zip(g["ups_keys"], g["ups_shapes"])}
    assert mine == ref
    assert mine["ups.0.4.1.weight"] == (16, 16, 1, 3, 3) and mine["ups.0.4.1.bias"] == (16,)
    assert "ups.0.4.weight" not in mine and "ups.0.4.bias" not in mine
    # everything outside the upsampler is the deconv variant's key set; the reference checkpoint loads strictly
    deconv = D.DynamicNfUnet3D(default_num_frames=12, **{**TINY_KW, "use_deconv": True})
    strip = lambda sd: {k: tuple(v.shape) for k, v in sd.items() if not k.startswith("ups.0.4.")}
    assert strip(unet.state_dict()) == strip(deconv.state_dict())
    sd = tiny_upconv_sd(tiny[1], g)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in sd.items()}, strict=True)
    assert unet.packed().up_border == 1
    for mode, b in zip(MODES, (0, 1, 1, 2)):
        assert pack_unet(sd, win=3, device="cpu", padding_mode=mode).up_border == b
    assert pack_unet(tiny[1], win=3, device="cpu", padding_mode="reflect").up_border == 0        # deconv weights: ignored


@pytest.mark.parametrize("mode", ["zeros", "reflect"])
def test_tiny_orchestration_matches_reference_golden(tiny, mode):
    """zeros runs on the unchanged RefOps (unet_forward passes no border there), reflect on the subclass that honours it; the
    tolerance of tests/test_orchestration_cpu.py for tiny_unet.npz."""
    g0, sd0 = tiny
    g = load_golden(f"tiny_unet_upconv_{mode}.npz")
    P = pack_unet(tiny_upconv_sd(sd0, g), win=3, device="cpu", padding_mode=mode)
    ops = RefOps() if mode == "zeros" else BorderRefOps()
    x = T(g0["x"])[0]
    cs = build_clip_state(ops, P, x[3:, 0].contiguous(), T(g0["cond"])[0])
    y = unet_forward(ops, P, cs, x[:3].contiguous(), int(g0["time"][0]))
    torch.testing.assert_close(y, T(g["y"])[0], atol=3e-5, rtol=1e-5)
    # the two goldens differ (the border is observable), and neither is the transposed-conv net
    other = load_golden(f"tiny_unet_upconv_{'reflect' if mode == 'zeros' else 'zeros'}.npz")
    assert float((T(g["y"]) - T(other["y"])).abs().max()) > 1e-3
    assert float((T(g["y"]) - T(g0["y"])).abs().max()) > 1e-2


def test_abi_is_additive():
    assert _lib.ConvDesc._fields_[-1][0] == "border"
    f = _lib.ConvDesc.border
    assert f.size == 4 and f.offset == max(getattr(_lib.ConvDesc, n).offset for n, _ in _lib.ConvDesc._fields_)
    assert ctypes.sizeof(_lib.ConvDesc) == f.offset + 8          # the int + tail padding to the struct's 8-byte alignment
    assert _lib.ConvDesc().border == 0
    L = _lib.lib()
    assert L.dawn_abi_version() == 8
    # the value is checked before anything else: no ctx (and so no GPU) is needed to see it rejected
    for bad in (3, -1):
        assert L.dawn_ctx_set_option(None, 6, bad) != 0
        assert b"DAWN_OPT_UP_BORDER" in L.dawn_last_error()
    assert L.dawn_ctx_set_option(None, 6, 1) != 0 and b"null ctx" in L.dawn_last_error()
    from dawn_pytorch_amd import ctx
    assert ctx.OPT_UP_BORDER == 6
