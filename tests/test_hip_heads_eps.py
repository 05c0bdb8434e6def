"""-m gpu: heads_eps_kernel (csrc/misc.hip) -- both head blocks' SiLU(GroupNorm(c2)), their res_conv folded into the output projection
(pack.fold_heads) and the projection itself in one streaming pass -- against the UNFUSED formula in fp64 torch, next to the two-kernel
path it replaces (res_conv GEMM with the `tr` epilogue, then head_out) on the same inputs; the shapes at which its indexing can go
wrong; one head at a time with poison and guard bands; determinism; and one tiny evaluation folded / unfolded on both hosts."""
import pytest
import torch

import dawn_pytorch_amd as D
from dawn_pytorch_amd.ctx import CtxEvaluator, OPT_FOLD_HEADS
from dawn_pytorch_amd.ops import HipOps
from dawn_pytorch_amd.pack import fold_heads, pack_bf3, pack_kn
from dawn_pytorch_amd.unet_forward import unet_forward
from test_hip_ops import check

pytestmark = pytest.mark.gpu
TOL = 2e-5                      # what test_hip_ops.py asks of head_out (relative to max(1, max|want|))
POISON = -7.625e11              # an exact fp32 value no head produces


@pytest.fixture(scope="module")
def hip():
    return HipOps()


def _case(rows, Co, C0, C1, seed=0):
    """Realistic magnitudes: c2 is a conv output (O(1), offset), a2 / b2 = rstd * gamma / beta - mean * a of a GroupNorm, [x | r] O(1)
    activations, weights at 1 / sqrt(fan-in) like the checkpoint's."""
    g = torch.Generator().manual_seed(1000 * seed + rows + Co + C0 + C1)
    r = lambda *s: torch.randn(*s, generator=g)     # noqa: E731
    Cin = C0 + C1
    t = dict(c2g=r(rows, Co) * 1.7 + 0.3, c2o=r(rows, Co) * 0.8 - 0.2, a2g=r(Co) * 0.2 + 0.6, b2g=r(Co) * 0.3, a2o=r(Co) * 0.3 + 1.2,
             b2o=r(Co) * 0.3, x=r(rows, C0) * 1.5, r=r(rows, C1) * 0.9 + 0.1, wg=r(2, Co) * Co ** -0.5, bg=r(2) * 0.1,
             wo=r(1, Co) * Co ** -0.5, bo=r(1) * 0.1, wr_g=r(Co, Cin) * Cin ** -0.5, br_g=r(Co) * 0.1, wr_o=r(Co, Cin) * Cin ** -0.5,
             br_o=r(Co) * 0.1)
    t["wf"], t["bf"] = fold_heads(t["wg"], t["bg"], t["wo"], t["bo"], t["wr_g"], t["br_g"], t["wr_o"], t["br_o"])
    return t


def _want(t):
    """The unfused formula in fp64: h = SiLU(a2 * c2 + b2) + Wr.[x|r] + br per head, eps = [Wg.hg + bg ; Wo.ho + bo] -> (3, rows)."""
    d = {k: v.double() for k, v in t.items()}
    xr = torch.cat((d["x"], d["r"]), 1)
    hg = torch.nn.functional.silu(d["c2g"] * d["a2g"] + d["b2g"]) + xr @ d["wr_g"].t() + d["br_g"]
    ho = torch.nn.functional.silu(d["c2o"] * d["a2o"] + d["b2o"]) + xr @ d["wr_o"].t() + d["br_o"]
    return torch.cat((hg @ d["wg"].t() + d["bg"], ho @ d["wo"].t() + d["bo"]), 1).t().contiguous()


def _gpu(t):
    return {k: v.cuda() for k, v in t.items()}


def _fold(hip, c, heads="go", x=None, r=None, out=None):
    return hip.heads_eps((c["c2g"], c["a2g"], c["b2g"]) if "g" in heads else None, (c["c2o"], c["a2o"], c["b2o"]) if "o" in heads else None,
                         c["x"] if x is None else x, c["r"] if r is None else r, c["wg"], c["wo"], c["wf"], c["bf"], out=out)


def _unfolded(hip, c, rows):
    """The sequence the fold replaces, on the GPU: res_conv of [x | r] with the SiLU(GN(c2)) `tr` epilogue per head, then head_out."""
    hs = []
    for h in "go":
        wkn = c["wr_" + h].t().contiguous().cpu()
        hs.append(hip.conv_gemm(c["x"], pack_kn(wkn).cuda(), c["c2" + h].shape[1], in1=c["r"], bias=c["br_" + h],
                                tr=(c["c2" + h], c["a2" + h], c["b2" + h]), w_bf3=pack_bf3(wkn).cuda(), F=1, Hi=rows, Wi=1))
    return hip.head_out(hs[0], hs[1], c["wg"], c["bg"], c["wo"], c["bo"])


def test_accuracy_against_fp64_next_to_the_two_kernel_path(hip):
    rows = 12800                 # (from 12,800 rows the res_conv GEMM is the split-bf16 row kernel of the full-size evaluation)
    t = _case(rows, 64, 64, 64)
    want, c = _want(t), _gpu(t)
    got = _fold(hip, c)
    old = _unfolded(hip, c, rows)
    scale = max(1.0, float(want.abs().max()))
    e_fold = float((got.double().cpu() - want).abs().max())
    e_old = float((old.double().cpu() - want).abs().max())
    print(f"heads_eps vs fp64: {e_fold:.3e}; res_conv + head_out vs fp64: {e_old:.3e}; bound {TOL * scale:.3e}")
    check("heads_eps/accuracy_12800", got, want, TOL)
    assert e_fold <= TOL * scale and e_old <= TOL * scale, \
        f"max|err| vs fp64: folded {e_fold:.3e}, two-kernel path {e_old:.3e}, bound {TOL * scale:.3e}"


@pytest.mark.parametrize("rows", [1, 15, 17, 50, 4099])
@pytest.mark.parametrize("Co,C0,C1,ld0", [(64, 64, 64, 64), (64, 64, 64, 96), (64, 64, 32, 64)])
def test_shapes(hip, rows, Co, C0, C1, ld0):
    """rows off the 16-row group and the 64-row workgroup (4099: 65 workgroups, the last one a single group of 3 rows); x as a column
    view of a wider tensor (ld0 = 96, ld1 = 64); C0 != C1."""
    t = _case(rows, Co, C0, C1, seed=1)
    want, c = _want(t), _gpu(t)
    x = c["x"]
    if ld0 != C0:
        wide = torch.full((rows, ld0), float("nan"), device="cuda")       # (a read outside the view's columns would poison the row)
        wide[:, 16:16 + C0] = c["x"]
        x = wide[:, 16:16 + C0]
        assert x.stride(0) == ld0 or rows == 1
    got = _fold(hip, c, x=x)
    assert got is not None and tuple(got.shape) == (3, rows)
    check(f"heads_eps/rows{rows}_Co{Co}_{C0}+{C1}_ld{ld0}", got, want, TOL)


def test_refused_shapes_return_none(hip):
    t = _case(20, 64, 64, 64, seed=2)
    c = _gpu(t)
    wide = torch.zeros(20, 67, device="cuda")
    assert _fold(hip, c, x=wide[:, :64]) is None                          # ld0 = 67
    assert _fold(hip, c, x=torch.zeros(20, 66, device="cuda")[:, 2:66]) is None      # base pointer off a 16-byte boundary
    # the library itself refuses with an error code (nothing launched)
    L = hip.L
    p = lambda v: v.data_ptr()      # noqa: E731
    rc = L.dawn_heads_eps(p(c["c2g"]), p(c["a2g"]), p(c["b2g"]), p(c["c2o"]), p(c["a2o"]), p(c["b2o"]), p(c["x"]), 66, 64, p(c["r"]), 64, 64,
                          p(c["wg"]), p(c["wo"]), p(c["wf"]), p(c["bf"]), 20, 64, p(torch.empty(3, 20, device="cuda")), None)
    assert rc != 0


@pytest.mark.parametrize("rows", [17, 4099])
def test_one_head_at_a_time_poison_and_guard_bands(hip, rows):
    t = _case(rows, 64, 64, 64, seed=3)
    want, c = _want(t), _gpu(t)
    pad = 256
    poison = torch.tensor(POISON)
    for heads, written, kept in (("g", slice(0, 2), slice(2, 3)), ("o", slice(2, 3), slice(0, 2))):
        buf = torch.full((pad + 3 * rows + pad,), POISON, device="cuda")
        eps = buf[pad:pad + 3 * rows].view(3, rows)
        assert _fold(hip, c, heads=heads, out=eps) is not None
        torch.cuda.synchronize()
        b = buf.cpu()
        e = b[pad:pad + 3 * rows].view(3, rows)
        assert torch.equal(b[:pad], poison.expand(pad)) and torch.equal(b[-pad:], poison.expand(pad)), "write outside 3 * rows"
        assert torch.equal(e[kept], poison.expand_as(e[kept])), f"head '{heads}' alone touched the other head's rows"
        check(f"heads_eps/only_{heads}_rows{rows}", e[written], want[written], TOL)
    # both halves into one buffer == both heads in one launch, bit for bit
    eps = torch.full((3, rows), POISON, device="cuda")
    _fold(hip, c, heads="g", out=eps)
    _fold(hip, c, heads="o", out=eps)
    assert torch.equal(eps, _fold(hip, c))


def test_deterministic(hip):
    c = _gpu(_case(4099, 64, 64, 64, seed=4))
    assert torch.equal(_fold(hip, c), _fold(hip, c))


def test_tiny_evaluation_folded_vs_unfolded_on_both_hosts():
    """dim 64, dim_mults (1, 2), 16 frames of 8 x 8: one evaluation with the heads folded and one without agree to the tolerance
    tests/test_hip_fullsize.py applies to an evaluation (1e-4 * max(1, max|y|)); the C evaluator is bit-identical to the Python host,
    with the fold on and with it off."""
    F, h = 16, 8
    unet = D.DynamicNfUnet3D(default_num_frames=F, num_frames=F, dim=64, cond_dim=40, cond_aud=32, cond_pose=6, cond_eye=2, channels=35,
                             dim_mults=(1, 2), use_hubert_audio_cond=True, win_width=8, init_seed=0).cuda()
    ops, P = unet._ops(), unet.packed()
    assert P.heads_wf is not None
    g = torch.Generator().manual_seed(5)
    fea272 = torch.randn(32, h, h, generator=g).cuda()
    cond, x3 = torch.randn(F, 40, generator=g).cuda(), torch.randn(3, F, h, h, generator=g).cuda()
    cs = unet.build_clip(fea272, cond)
    try:
        ops.fold_heads = True
        y_fold = unet_forward(ops, P, cs, x3, 500)
        ops.fold_heads = False
        y_old = unet_forward(ops, P, cs, x3, 500)
    finally:
        ops.fold_heads = True
    assert torch.isfinite(y_fold).all()
    err, bound = float((y_fold - y_old).abs().max()), 1e-4 * max(1.0, float(y_old.abs().max()))
    print(f"folded vs unfolded evaluation: max|diff| {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    ev = CtxEvaluator(P)
    clip = ev.prepare_clip(fea272, cond, cs.rcos, cs.rsin)
    ev.set_option(OPT_FOLD_HEADS, 1)
    got = ev.forward(clip, x3, 500.0)
    assert torch.equal(got, y_fold), float((got - y_fold).abs().max())
    ev.set_option(OPT_FOLD_HEADS, 0)
    got = ev.forward(clip, x3, 500.0)
    assert torch.equal(got, y_old), float((got - y_old).abs().max())
