"""-m gpu: the two device helpers of the C-side evaluator that only end-to-end runs reached (csrc/misc.hip, called by dawn_ctx.hip),
through the ctypes handle: dawn_chw_to_hwc bit-exact against `permute` inside a guard band, dawn_rotary_tables within one fp32 ulp of
cos / sin of the fp32 product and invariant under the T-shard offset pos0."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from dawn_pytorch_amd import _lib
from guarded import GuardedOps

pytestmark = pytest.mark.gpu


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("C", [3, 35, 272])
@pytest.mark.parametrize("HW", [100, 4096])
def test_chw_to_hwc_bit_exact_inside_guard_band(C, HW):
    """(C, HW) planar -> (HW, C): channel counts below, across and far above the 32 x 32 tile (272 = the fea channels of the product),
    pixel counts that are and are not a multiple of it."""
    L = _lib.lib()
    g = GuardedOps()
    x = torch.randn(C, HW, generator=torch.Generator().manual_seed(C + HW))
    xin, _ = g.guarded_in(x)
    out = g.guarded_out(HW, C)
    _lib.check(L.dawn_chw_to_hwc(xin.data_ptr(), C, HW, out.data_ptr(), _stream()), "dawn_chw_to_hwc")
    torch.cuda.synchronize()
    g.verify()
    g.inputs_intact()
    assert torch.equal(out.cpu(), x.t().contiguous())


def _tables(L, freqs, n, pos0):
    c, s = torch.full((n, 16), float("nan"), device="cuda"), torch.full((n, 16), float("nan"), device="cuda")
    _lib.check(L.dawn_rotary_tables(freqs.data_ptr(), n, pos0, c.data_ptr(), s.data_ptr(), _stream()), "dawn_rotary_tables")
    torch.cuda.synchronize()
    return c.cpu().numpy(), s.cpu().numpy()


def _rot_freqs():
    """The 16 rotary frequencies of the temporal attention, as the reference's checkpoint holds them (tests/golden/tiny_unet.npz)."""
    fr = load_golden("tiny_unet.npz")["sd:denoise_fn.init_temporal_attn.fn.fn.fn.rotary_emb.freqs"].astype(np.float32)
    assert fr.shape == (16,)
    return fr


@pytest.mark.parametrize("pos0", [0, 37])
def test_rotary_tables_within_one_ulp(pos0):
    """cos / sin (n, 16) of the fp32 product (pos0 + i) * freqs[j], evaluated in float64 and rounded once."""
    L, fr, n = _lib.lib(), _rot_freqs(), 280
    c, s = _tables(L, torch.from_numpy(fr).cuda(), n, pos0)
    ang = (np.arange(pos0, pos0 + n, dtype=np.float32)[:, None] * fr[None, :]).astype(np.float32).astype(np.float64)
    for got, want64 in ((c, np.cos(ang)), (s, np.sin(ang))):
        want = want64.astype(np.float32)
        assert not np.isnan(got).any()
        ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.float32(2.0 ** -126)))
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), float(np.abs(got - want).max())


def test_rotary_tables_shard_invariance():
    """pos0 = 37, n = 100 == rows 37 .. 136 of the pos0 = 0 table, bit for bit: what the T-sharded evaluator relies on."""
    L = _lib.lib()
    fr = torch.from_numpy(_rot_freqs()).cuda()
    c0, s0 = _tables(L, fr, 280, 0)
    c1, s1 = _tables(L, fr, 100, 37)
    assert np.array_equal(c1.view(np.int32), c0[37:137].view(np.int32)) and np.array_equal(s1.view(np.int32), s0[37:137].view(np.int32))
