"""-m gpu: the launches of the LFG flow decoder against a float64 reference at fp32 accuracy (tests/decode_gate.py): the direct split-bf16
3x3 kernel at every distinct conv launch of FlowDecoder (after asserting with dawn_conv3x3_direct_form which instantiation the very
descriptor takes), init_conv_x at the decoder's widths, warp_blend on exact-position motion, the final 7x7 conv without and with its
blend, affine_act and bn_relu_pool2; and, with no tolerance at all, the warps whose result is known bit for bit.

The gate (split_gate.fp32_gate): max|hip - fp64| / max|fp64| <= c x the same for the RefOps op in fp32 on CPU + FLOOR, c = C_GATE = 2 unless
decode_gate.C_WIDE widens it with the MI355X measurement beside it.  tests/test_decode_gate_cpu.py shows that every case rejects the
defects of its kernel.  Each gate appends its errors and its ratio to CPU fp32 to the op-error log."""
import pytest
import torch

import decode_gate as D
from dawn_pytorch_amd.pack import pack_bf3, pack_kn

pytestmark = pytest.mark.gpu

REPEATS = 8


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def cu(t):
    return None if t is None else t.cuda()


def of_kind(*kinds):
    cs = [c for c in D.CASES if c.kind in kinds]
    return pytest.mark.parametrize("case", cs, ids=[c.name for c in cs])


def gate(case, got, T):
    torch.cuda.synchronize()
    want64, base32 = case.want64(T), case.base32(T)
    if case.kind != "final":
        return D.fp32_gate(case.name, got, want64, base32, c=case.c)
    for i, out in enumerate(case.outputs()):
        D.fp32_gate(f"{case.name}/{out}", got[i], want64[i], base32[i], c=case.c)


def conv_call(case, T):
    """The call FlowDecoder._conv3 makes: bias, w_bf3 and no Winograd image, under the shipped policy."""
    kw = dict(case.conv_kw(), bias=cu(T["bias"]), res=cu(T["res"]), w_bf3=pack_bf3(T["w"]).cuda())
    return (cu(T["x"]), pack_kn(T["w"]).cuda(), case.p["N"]), kw


@of_kind("dconv")
def test_direct_conv3x3_fp64_gate(hip, case):
    T = case.make()
    args, kw = conv_call(case, T)
    assert hip.conv_policy == 0
    assert hip.conv_gemm(*args, **kw, form_only="direct") == D.DCONV_FORM[case.name], case.name
    assert hip.conv_gemm(*args, **kw, form_only=True) == (0, 0)
    got = hip.conv_gemm(*args, **kw)
    assert tuple(got.shape) == (case.p["F"] * case.p["H"] * case.p["W"], case.p["N"])
    gate(case, got, T)


DET = [c for c in D.CASES if c.name in ("dconv/up1_256px", "dconv/bott_conv2_res_256px")]     # column-tiled (W = 256); eight waves


@pytest.mark.parametrize("case", DET, ids=[c.name for c in DET])
def test_direct_conv3x3_run_to_run_identical(hip, case):
    """Eight launches on the same input in one process: bit-identical (a race on the register-prefetched patch or on a weight stage would
    show as run-to-run differences)."""
    T = case.make()
    args, kw = conv_call(case, T)
    assert hip.conv_gemm(*args, **kw, form_only="direct") == D.DCONV_FORM[case.name]
    assert (case.p["W"] > 64) != (D.DCONV_FORM[case.name] == D.V2_WN2)
    first = hip.conv_gemm(*args, **kw)
    torch.cuda.synchronize()
    for rep in range(REPEATS - 1):
        again = hip.conv_gemm(*args, **kw)
        assert torch.equal(again, first), f"{case.name}: run {rep + 1} differs from run 0 in {int((again != first).sum())} elements"


@of_kind("first")
def test_init_conv_x_fp64_gate(hip, case):
    T, p = case.make(), case.p
    gate(case, hip.init_conv_x(cu(T["x"]), cu(T["w3"]), cu(T["fea_pre"]), 1, p["h"], p["w"], 64), T)


def warp_call(hip, case, T):
    p = case.p
    grid = T["grid"]
    if "view" in p:                                           # the same frame range of the longer clip, on the device
        Ttot, t0 = p["view"]
        whole, _ = D.dyadic_motion(Ttot, *p["s"], seed=p["S"][0] + p["C"] + len(p["mode"]), max_shift=p["shift"])
        gd = whole.cuda()[:, t0:t0 + 3]
        assert torch.equal(gd.cpu(), grid) and gd.stride(0) == Ttot * p["s"][0] * p["s"][1]
    else:
        gd = grid.cuda()
    return hip.warp_blend(cu(T["skip"]), *p["S"], gd, cu(T["conf"]), prev=cu(T["prev"]),
                          prev_ab=None if T["pa"] is None else (cu(T["pa"]), cu(T["pb"])), up2="up2" in p["mode"])


@of_kind("warp")
def test_warp_blend_fp64_gate(hip, case):
    T = case.make()
    got = warp_call(hip, case, T)
    k = 2 if "up2" in case.p["mode"] else 1
    assert tuple(got.shape) == (3 * case.p["S"][0] * k * case.p["S"][1] * k, case.p["C"])
    gate(case, got, T)


@of_kind("final")
def test_final_conv_blend_fp64_gate(hip, case):
    T, p = case.make(), case.p
    outs = torch.full((2, 3, 2, p["H"], p["W"]), float("nan"), device="cuda")
    hip.final_conv_blend(cu(T["x"]), p["H"], p["W"], cu(T["w7"]), cu(T["b3"]), cu(T["src"]), cu(T["grid"]), cu(T["conf"]), outs[0], outs[1])
    assert bool(torch.isfinite(outs).all()), f"{case.name}: an output pixel was not written"
    gate(case, outs, T)


@of_kind("ew")
def test_affine_and_pool_fp64_gate(hip, case):
    T, p = case.make(), case.p
    if p["op"] == "affine":
        got = hip.affine_act(case.ew_x(T["wide"].cuda()), cu(T["a"]), cu(T["b"]), p["act"])
    else:
        got = hip.bn_relu_pool2(cu(T["x"]), cu(T["a"]), cu(T["b"]), 2, p["H"], p["W"])
    gate(case, got, T)


# ---------------------------------------------------------------------------------------------- exact equality, no tolerance
EXACT_H, EXACT_W = 16, 32
EXACT = ("identity", "whole_pixel", "edge_-1_and_W", "far_outside")


@pytest.mark.parametrize("which", range(4), ids=EXACT)
@pytest.mark.parametrize("Cc", [4, 64])
def test_warp_blend_exact_motion(hip, which, Cc):
    """Mode `first` on a same-size level: identity motion gives skip * conf, whole-pixel shifts the shifted skip with zero fill times conf,
    positions at exactly -1 and W (H) and finite far-outside grids (+-1e30) give zeros -- bit for bit."""
    name, grid, conf, skip, want = D.exact_warp_cases(EXACT_H, EXACT_W, Cc)[which]
    assert name == EXACT[which]
    got = hip.warp_blend(skip.cuda(), EXACT_H, EXACT_W, grid.cuda(), conf.cuda()).cpu()
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {want.numel()} values differ, max {float((got - want).abs().max()):.3e}"


@pytest.mark.parametrize("which", range(4), ids=EXACT)
def test_final_conv_blend_warped_vid_exact_motion(hip, which):
    """The same four motions on warped_vid of final_conv_blend with h == H: the source image itself, shifted, or zeros -- bit for bit."""
    H, W, Cc = EXACT_H, EXACT_W, 8
    name, grid, expect = D.exact_motions(H, W)[which]
    T = grid.shape[1]
    src = torch.rand(3, H, W, generator=torch.Generator().manual_seed(4))
    want = expect(src.permute(1, 2, 0).contiguous()).permute(3, 0, 1, 2)                      # (3, T, H, W)
    conf = torch.rand(T, H, W, generator=torch.Generator().manual_seed(5))
    outs = torch.full((2, 3, T, H, W), float("nan"), device="cuda")
    hip.final_conv_blend(D.rnd(T * H * W, Cc, seed=1).cuda(), H, W, D.rnd(49, Cc // 4, 3, 4, seed=2, scale=0.05).cuda(), D.rnd(3, seed=3).cuda(),
                         src.cuda(), grid.cuda(), conf.cuda(), outs[0], outs[1])
    got = outs[1].cpu()
    assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {want.numel()} values differ"
