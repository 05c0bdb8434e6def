"""No-GPU checks of the folded heads: the library's host function dawn_fold_heads (the heads' res_conv folded into the output
projection, Wf = [Wg.Wr_g ; Wo.Wr_o], bf = [Wg.br_g + bg ; Wo.br_o + bo]) against fp64 torch, and the orchestration's fall-back to the
unfolded sequence for an op set without `heads_eps` (oracle/ops_ref.RefOps)."""
import pytest
import torch

from conftest import load_golden  # noqa: F401  (conftest puts the repository root on sys.path)
from oracle.ops_ref import RefOps
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.pack import fold_heads, pack_unet
from dawn_pytorch_amd.unet_forward import build_clip_state, unet_forward

T = torch.from_numpy


def _weights(Co, Cin, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)     # noqa: E731
    return (r(2, Co) * Co ** -0.5, r(2) * 0.1, r(1, Co) * Co ** -0.5, r(1) * 0.1, r(Co, Cin) * Cin ** -0.5, r(Co) * 0.1,
            r(Co, Cin) * Cin ** -0.5, r(Co) * 0.1)


@pytest.mark.parametrize("Co,Cin", [(64, 128), (8, 12)])
def test_fold_helper_equals_fp64_rounded_once(Co, Cin):
    wg, bg, wo, bo, wr_g, br_g, wr_o, br_o = w = _weights(Co, Cin, 7 + Co)
    wf, bf = fold_heads(*w)
    d = [t.double() for t in w]
    want_wf = torch.cat((d[0] @ d[4], d[2] @ d[6]), 0)
    want_bf = torch.cat((d[0] @ d[5] + d[1], d[2] @ d[7] + d[3]), 0)
    assert wf.dtype == torch.float32 and tuple(wf.shape) == (3, Cin) and tuple(bf.shape) == (3,)
    assert torch.equal(wf, want_wf.float()), float((wf.double() - want_wf).abs().max())
    assert torch.equal(bf, want_bf.float()), float((bf.double() - want_bf).abs().max())
    # reached the way a C host would: raw host pointers into the library, no Python arithmetic in between
    L = _lib.lib()
    host = [t.contiguous() for t in w]
    wf2, bf2 = torch.full((3, Cin), float("nan")), torch.full((3,), float("nan"))
    assert L.dawn_fold_heads(*[t.data_ptr() for t in host], Co, Cin, wf2.data_ptr(), bf2.data_ptr()) == 0
    assert torch.equal(wf2, wf) and torch.equal(bf2, bf)
    assert L.dawn_fold_heads(None, *[t.data_ptr() for t in host[1:]], Co, Cin, wf2.data_ptr(), bf2.data_ptr()) != 0      # refused, not a crash


def test_packer_folds_the_heads_of_the_tiny_unet(tiny):
    g, sd = tiny
    P = pack_unet(sd, win=3, device="cpu")
    dim = P.dim
    assert tuple(P.heads_wf.shape) == (3, 2 * dim) and tuple(P.heads_bf.shape) == (3,)
    p = "denoise_fn."
    wr = sd[p + "final_conv.0.res_conv.weight"].double().reshape(dim, 2 * dim)
    wg = sd[p + "final_conv.1.weight"].double().reshape(2, dim)
    assert torch.equal(P.heads_wf[:2], (wg @ wr).float())


def test_ops_without_heads_eps_fall_back_to_the_unfolded_heads(tiny):
    """fold_heads on, but the injected op set (the torch reference ops) has no heads_eps: the evaluation runs res_conv + head_out as
    before and still reproduces the reference golden."""
    g, sd = tiny
    ops = RefOps()
    ops.fold_heads = True
    assert not hasattr(ops, "heads_eps")
    P = pack_unet(sd, win=3, device="cpu")
    assert P.heads_wf is not None
    x = T(g["x"])[0]
    cs = build_clip_state(ops, P, x[3:, 0].contiguous(), T(g["cond"])[0])
    y = unet_forward(ops, P, cs, x[:3].contiguous(), int(g["time"][0]))
    torch.testing.assert_close(y, T(g["y"])[0], atol=3e-5, rtol=1e-5)
