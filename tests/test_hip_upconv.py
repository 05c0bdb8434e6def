"""-m gpu: the use_deconv=False upsampler (nearest x2 + 3x3 conv with a padding_mode, MT:169-172) on the mode-1 kernels -- folded
weights (pack.upconv_w_kn_phases) and dawn_conv_desc.border -- against the literal interpolate -> pad -> conv2d in fp64, on all
three kernels that gather mode-1 taps; then the whole net on both hosts against goldens generated from the reference
(tools/gen_goldens_upconv.py).

Gate (stated): this file's copy of test_hip_ops.check, |hip - want| <= 1e-4 * max(1, max|want|).  `want` is the fp64 literal of the
UNFOLDED fp32 weights: the folding adds one fp32 rounding per weight (2^-24 relative), far inside the gate."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from fullsize_cases import KW, build_inputs, checksum
from upconv_cases import BORDER_MODE, TINY_KW, literal_rows, tiny_upconv_sd
import dawn_pytorch_amd as D
from dawn_pytorch_amd import _lib
from dawn_pytorch_amd.policy import ConvPolicy
from dawn_pytorch_amd.pack import pack_bf3, pack_kn, upconv_w_kn_phases

pytestmark = pytest.mark.gpu
T = torch.from_numpy
SHIPPED_POLICY = ConvPolicy.DEFAULT
DAWN_SPLIT1X1_RESAMPLE = 4


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def check(name, got, want, tol=1e-4):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print(f"{name}: max|diff| {err:.3e} (gate {tol * scale:.3e})")
    assert not torch.isnan(got).any(), f"{name}: NaN"
    assert err <= tol * scale, f"{name}: max|diff| {err:.3e} > {tol * scale:.3e}"
    return err


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


class Case:
    """One up conv: seeded input rows, 3x3 weights, bias; the folded images on the GPU; the fp64 literals per border (computed once)."""

    def __init__(self, F, H, W, C, N):
        self.F, self.H, self.W, self.C, self.N = F, H, W, C, N
        self.x, self.b = rnd(F * H * W, C, seed=2), rnd(N, seed=3)
        self.w5 = rnd(N, C, 1, 3, 3, seed=5, scale=(C * 9) ** -0.5)
        ph = upconv_w_kn_phases(self.w5)
        self.wp = torch.stack([pack_kn(ph[i]) for i in range(4)], 0).cuda()
        self.ws = torch.stack([pack_bf3(ph[i]) for i in range(4)], 0).cuda() if (4 * C) % 256 == 0 else None
        self.xg, self.bg = self.x.cuda(), self.b.cuda()
        self.kw = dict(F=F, Hi=H, Wi=W, Ho=2 * H, Wo=2 * W, KH=2, KW=2, mode=1, bias=self.bg)
        self._want = {}

    def want(self, border):
        if border not in self._want:
            self._want[border] = literal_rows(self.x, self.F, self.H, self.W, self.w5, self.b, BORDER_MODE[border])
        return self._want[border]

    def run(self, hip, border, split=False, **extra):
        return hip.conv_gemm(self.xg, self.wp, self.N, w_bf3=self.ws if split else None, border=border, **self.kw, **extra)

    def ring(self):
        """(rows,) bool: output pixels on the outer ring of their frame -- exactly those with a tap outside the input."""
        m = torch.zeros(self.F, 2 * self.H, 2 * self.W, dtype=torch.bool)
        m[:, 0], m[:, -1], m[:, :, 0], m[:, :, -1] = True, True, True, True
        return m.reshape(-1)


_cases = {}


def case(*key):
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


FP32_SHAPES = [(3, 8, 8, 64, 64), (3, 4, 16, 64, 64), (2, 8, 8, 16, 16)]
SPLIT_SHAPES = [(50, 16, 16, 64), (25, 16, 32, 64), (50, 16, 16, 128), (200, 8, 8, 256)]


@pytest.mark.parametrize("glds", [True, False], ids=["shipped_policy", "no_direct_to_lds"])
@pytest.mark.parametrize("F,H,W,C,N", FP32_SHAPES)
def test_fp32_kernels_every_border(hip, F, H, W, C, N, glds):
    """Both fp32 kernels gather a border: conv_gemm_glds_kernel under the shipped policy, conv_gemm_kernel with ConvPolicy.GLDS cleared."""
    c = case(F, H, W, C, N)
    hip.conv_policy = 0 if glds else SHIPPED_POLICY & ~ConvPolicy.GLDS
    try:
        assert hip.conv_gemm(c.xg, c.wp, N, border=1, form_only=True, **c.kw)[1] == 0          # no split kernel here
        for border in (0, 1, 2):
            check(f"upconv_fp32/{'glds' if glds else 'reg'}_F{F}_{H}x{W}_C{C}_border{border}", c.run(hip, border), c.want(border))
    finally:
        hip.conv_policy = 0


@pytest.mark.parametrize("F,H,W,C", SPLIT_SHAPES)
def test_split_kernel_every_border(hip, F, H, W, C):
    c = case(F, H, W, C, C)
    assert c.ws is not None
    for border in (0, 1, 2):
        form = hip.conv_gemm(c.xg, c.wp, C, w_bf3=c.ws, border=border, form_only=True, **c.kw)
        assert form[1] == DAWN_SPLIT1X1_RESAMPLE, form
        want = c.want(border)
        e_split = check(f"upconv_split/F{F}_{H}x{W}_C{C}_border{border}", c.run(hip, border, split=True), want)
        e_f32 = check(f"upconv_split/fp32_kernel_F{F}_{H}x{W}_C{C}_border{border}", c.run(hip, border), want)
        # the project's relation between the split kernel and the fp32 kernel (test_conv_resample_on_split_pipeline)
        assert e_split <= 2.0 * e_f32 + 3e-6 * float(want.abs().max()), (border, e_split, e_f32)


@pytest.mark.parametrize("key,split", [((50, 16, 16, 64, 64), True), ((3, 4, 16, 64, 64), False)], ids=["split_50x16x16", "fp32_3x4x16"])
def test_border_is_confined_to_the_outer_ring(hip, key, split):
    c = case(*key)
    policies = [0] if split else [0, SHIPPED_POLICY & ~ConvPolicy.GLDS]
    try:
        for pol in policies:
            hip.conv_policy = pol
            outs = [c.run(hip, b, split=split).cpu() for b in (0, 1, 2)]
            ring = c.ring()
            for b in (1, 2):
                assert torch.equal(outs[b][~ring], outs[0][~ring]), (pol, b)                 # same instruction path inside: same bits
            for a, b in ((0, 1), (0, 2), (1, 2)):
                assert not torch.equal(outs[a][ring], outs[b][ring]), (pol, a, b)
            # a kernel that ignored the field would give the zero-border result for all three
            check(f"upconv_ring/border1_is_reflect_{key}_{pol:x}", outs[1], c.want(1))
            check(f"upconv_ring/border2_is_circular_{key}_{pol:x}", outs[2], c.want(2))
            for b, other in ((1, 0), (2, 0), (2, 1)):
                assert float((outs[b].double() - c.want(other)).abs().max()) > 1e-2, (pol, b, other)
    finally:
        hip.conv_policy = 0


def _tiny_net(tiny, mode):
    g0, sd0 = tiny
    g = load_golden(f"tiny_unet_upconv_{mode}.npz")
    unet = D.DynamicNfUnet3D(default_num_frames=12, **TINY_KW, padding_mode=mode)
    unet.load_state_dict({k[len("denoise_fn."):]: v for k, v in tiny_upconv_sd(sd0, g).items()}, strict=True)
    return g0, g, unet.cuda()


def _both_hosts(name, unet, x3, fea272, cond, t, want):
    """forward through the Python host (gated against the reference golden) and the C evaluator (bit-identical to it)."""
    x = torch.cat((x3, fea272[:, :, None].expand(-1, -1, x3.shape[2], -1, -1)), 1)
    y = unet.forward_with_cond_scale(x, torch.tensor([t], device="cuda"), cond=cond, cond_scale=1.0)
    check(name, y[0], want)
    from dawn_pytorch_amd.ctx import CtxEvaluator
    P = unet.packed()
    ev = CtxEvaluator(P)
    rcos, rsin = P.rotary_tables(x3.shape[2] + 2 * P.win)
    clip = ev.prepare_clip(fea272[0].contiguous(), cond[0].contiguous(), rcos, rsin)
    got = ev.forward(clip, x3[0].contiguous(), float(t))
    assert torch.equal(got, y[0]), float((got - y[0]).abs().max())
    return y


@pytest.mark.parametrize("mode", ["reflect", "zeros"])
def test_tiny_goldens_on_both_hosts(tiny, mode):
    g0, g, unet = _tiny_net(tiny, mode)
    assert unet.packed().up_border == (1 if mode == "reflect" else 0)
    x = T(g0["x"]).cuda()
    _both_hosts(f"upconv_tiny_{mode}", unet, x[:, :3].contiguous(), x[:, 3:, 0].contiguous(), T(g0["cond"]).cuda(),
                int(g0["time"][0]), T(g["y"])[0])


def test_full_architecture_runs_both_kernel_families(hip):
    g = load_golden("upconv_full_T50.npz")
    T_, h, t = int(g["T"]), int(g["h"]), int(g["time"][0])
    unet = D.DynamicNfUnet3D(default_num_frames=8, **{**KW, "use_deconv": False, "padding_mode": str(g["padding_mode"])}, init_seed=0)
    np.testing.assert_allclose(checksum(unet.state_dict().values()), g["weights_checksum"], rtol=1e-12)
    fea272, cond, x3 = build_inputs(T_, h, int(g["inputs_seed"]))
    np.testing.assert_allclose(checksum([fea272, cond, x3]), g["inputs_checksum"], rtol=1e-12)
    unet.update_num_frames(T_)
    unet = unet.cuda()
    P = unet.packed()
    assert P.up_border == 1
    # the 16x16 -> 32x32 up conv (12,800 rows) is on the split kernel, the 8x8 and 4x4 levels on the fp32 kernels
    forms = []
    for lvl, side in zip(P.ups[:-1], (h // 8, h // 4, h // 2)):
        wu, bu, wus = lvl["up"]
        C = bu.numel()
        forms.append(hip.conv_gemm(torch.empty(T_ * side * side, C, device="cuda"), wu, C, F=T_, Hi=side, Wi=side, Ho=2 * side,
                                   Wo=2 * side, KH=2, KW=2, mode=1, bias=bu, w_bf3=wus, border=1, form_only=True)[1])
    assert forms == [0, 0, DAWN_SPLIT1X1_RESAMPLE], forms
    _both_hosts("upconv_full_T50", unet, x3.cuda(), fea272.cuda(), cond.cuda(), t, T(g["y"]))


def test_sampler_entries_see_the_border(tiny):
    """3-step guided DDIM of the tiny reflect net, seeded noise: the Python orchestration and dawn_sampler_run_guided agree bit for bit
    (and the border is observable in the sample: the zeros net with the same weights gives another one)."""
    g0, g, unet = _tiny_net(tiny, "reflect")
    d = load_golden("ddim_tiny.npz")
    fea, bbox, cond, x_init = (T(d[k]).cuda() for k in ("fea", "bbox", "cond", "x_init"))

    def sample(net, use_ctx):
        diff = D.DynamicNfGaussianDiffusion(default_num_frames=12, denoise_fn=net, num_frames=12, image_size=8, sampling_timesteps=3,
                                            timesteps=1000, loss_type='l2', use_dynamic_thres=True, null_cond_prob=0.1,
                                            ddim_sampling_eta=1.0).cuda()
        diff.update_num_frames(12)
        diff.noise_seed = 5
        diff.use_ctx = use_ctx
        out = diff.sample(fea, bbox, cond=cond, cond_scale=2.5, x_init=x_init)
        assert diff.last_route == ("ctx" if use_ctx else "python")
        return out
    want = sample(unet, False)
    got = sample(unet, True)
    assert torch.isfinite(want).all()
    assert torch.equal(got, want), float((got - want).abs().max())
    _, _, zeros_net = _tiny_net(tiny, "zeros")
    assert float((sample(zeros_net, True) - want).abs().max()) > 1e-3


def test_border_errors_launch_nothing(hip):
    c = case(2, 8, 8, 16, 16)
    out = torch.full((2 * 8 * 8, 16), 7.0, device="cuda")
    w1 = pack_kn(rnd(16, 16, seed=9)).cuda()
    with pytest.raises(_lib.DawnHipError, match="border"):
        hip.conv_gemm(c.xg, w1, 16, F=2, Hi=8, Wi=8, border=1, out=out)                      # mode 0
    big = torch.full((2 * 16 * 16, 16), 7.0, device="cuda")
    for bad in (3, -1):
        with pytest.raises(_lib.DawnHipError, match="border"):
            c.run(hip, bad, out=big)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((big == 7.0).all())
    # ... and the C evaluator's option takes 0 / 1 / 2 only
    from dawn_pytorch_amd.ctx import OPT_UP_BORDER
    L = _lib.lib()
    assert L.dawn_ctx_set_option(None, OPT_UP_BORDER, 3) != 0
