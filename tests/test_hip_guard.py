"""-m gpu: the UNet evaluation's kernels between guard bands (tests/guarded.py; tests/test_guarded_cpu.py shows what the helper catches).
Every case asserts four things: the values against the reference and tolerance of the op's existing test (the case tables and `check` of
tests/test_hip_ops.py / tests/test_hip_upconv.py are imported, not copied); GuardedOps.verify() -- every output element written, nothing
written outside an output; GuardedOps.inputs_intact() -- no operand modified, and (through the NaN around every operand) nothing read outside
an operand reached the result; and, for conv_gemm, that the launch took the intended form (form_only on the very same descriptor).

Every tensor operand -- sources, weights, bias, epilogue operands -- is a guarded input.  conv_gemm runs three times per case: into its own
allocation, into a caller's contiguous `out`, and with every 2-D fp32 operand and `out` a column slice of a wider tensor (ld > C)."""
import pytest
import torch

import test_hip_ops as T
import test_hip_upconv as UP
from dawn_pytorch_amd.policy import ConvPolicy as CP, TemporalAttnFlags as TA_, TemporalFlags as TF
from guarded import GuardedOps
from oracle.ops_ref import RefOps
from test_hip_fp64_gates import TEMPORAL_FLAGS, temporal_fits
from test_hip_ops import check, packw, rnd

pytestmark = pytest.mark.gpu

PAD = 4                               # column neighbours of the strided runs, in elements: 16 bytes, the alignment every vector load needs
NONE, TILED, ROWREG, ROWACC, RESAMPLE = 0, 1, 2, 3, 4        # dawn_gemm1x1_form
_g = []
_cache = {}
ref = RefOps()


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
        o.conv_policy = o.temporal_flags = o.temporal_attn_flags = 0
        o.reset()


def params(test):
    """The argument list of an existing test's parametrize mark (the shapes are taken from there, not copied)."""
    return [m for m in test.pytestmark if m.name == "parametrize"][0].args[1]


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def gin(g, v, name, pad=0):
    """CPU tensor / tuple of tensors / None -> guarded inputs on the GPU; pad: column neighbours for the 2-D fp32 ones."""
    if v is None or not (torch.is_tensor(v) or isinstance(v, (tuple, list))):
        return v
    if isinstance(v, (tuple, list)):
        return tuple(gin(g, t, f"{name}[{i}]", pad) for i, t in enumerate(v))
    return g.guarded_in(v.cpu(), pad if (v.dim() == 2 and v.dtype == torch.float32) else 0, name=name)[0]


def finish(g, name, got, want, tol=1e-4, chk=check, overwritten=(), written=None):
    torch.cuda.synchronize()
    chk("guard/" + name, got, want, tol)
    g.verify(written=written)
    g.inputs_intact(overwritten)


# ---------------------------------------------------------------------------------------------- conv_gemm
class Conv:
    """One conv_gemm case on CPU tensors: in0, in1, w, N, kw (geometry + epilogue operands), split weight images, the reference."""

    def __init__(self, name, in0, in1, w, N, kw, want, images=None, gn=False, chk=check):
        self.name, self.in0, self.in1, self.w, self.N, self.kw, self.want = name, in0, in1, w, N, kw, want
        self.images, self.gn, self.chk = images or {}, gn, chk
        self.rows_out = kw["F"] * kw.get("Ho", kw["Hi"]) * kw.get("Wo", kw["Wi"])


def conv3_case(name, F, H, W, C0, C1, N, k, stride, pad, ex):
    """The inputs of test_hip_ops.test_conv_gemm / test_conv3x3_winograd for one row of their tables."""
    def make():
        from dawn_pytorch_amd.pack import pack_bf3, pack_wino4_bf3, pack_wino_bf3, unpack_kn
        rows = F * H * W
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        in0, in1 = rnd(rows, C0, seed=1), rnd(rows, C1, seed=2) if C1 else None
        w = packw(k * k * (C0 + C1), N, seed=3)
        kw = dict(F=F, Hi=H, Wi=W, Ho=Ho, Wo=Wo, KH=k, KW=k, stride=stride, pad=pad)
        if ex.get("bias"):
            kw["bias"] = rnd(N, seed=4)
        if ex.get("res"):
            kw["res"] = rnd(F * Ho * Wo, N, seed=8)
        want = ref.conv_gemm(in0, w, N, in1=in1, **kw)
        w5 = T._w5_from_packed(w, C0 + C1, N)
        images = dict(w_bf3=pack_bf3(unpack_kn(w)), w_wino=pack_wino_bf3(w5), w_wino4=pack_wino4_bf3(w5))
        return Conv(name, in0, in1, w, N, kw, want, images, gn=N % 64 == 0)        # gn_part.dawn_rows = the grid of the launch, see DIRECT
    return cached(("conv3", name), make)


def _row(table, name):
    return [c for c in table if c[0] == name][0]


def _wino_row(table, name):
    n, F, H, W, C0, C1, N, ex = _row(table, name)
    return (n, F, H, W, C0, C1, N, 3, 1, 1, ex)


CONV3 = {c[0]: c for c in (
    _row(T.CONV_CASES, "c3x3_ragged_M"),
    _row(T.CONV_CASES, "c3x3_halo_N192_ragged_ntile"),
    _wino_row(T.WINO_CASES, "H_not_square_32x64"),
    _wino_row(T.WINO_CASES, "L0_two_chunks"),
    _row(T.CONV_CASES, "c3x3_4x4_frames_cat_N128"),      # whole multi-frame tiles: 32 frames of 4 x 4, two sources ...
    _wino_row(T.WINO_CASES, "L3_8x8_four_frames"),       # ... and 12 frames of 8 x 8
    # what the tables lack: multi-frame tiles that are no exact multiple -- Winograd packs 4 frames of 8 x 8 per workgroup, the v2 direct
    # kernel 16 frames of 4 x 4 per 256-row tile
    ("F13_8x8", 13, 8, 8, 32, 0, 64, 3, 1, 1, {"bias": True, "gn": True}),
    ("F5_8x8_res", 5, 8, 8, 32, 0, 64, 3, 1, 1, {"res": True}),
    ("F17_4x4", 17, 4, 4, 32, 0, 128, 3, 1, 1, {"bias": True, "gn": True}),
    ("F33_4x4_cat", 33, 4, 4, 32, 32, 128, 3, 1, 1, {"bias": True}),
)}

# form name -> (policy, weight images handed over, (dawn_conv3x3_form, dawn_gemm1x1_form) of a 3x3 conv)
FORMS3 = {f"fp32_v{int(p)}": (p, (), (0, 0)) for p in T.FP32_POLICIES}          # the eight policies of test_conv_gemm
FORMS3.update({
    "split_v1": (CP.HALO_V1, ("w_bf3",), (0, 0)),
    "split_v2": (CP.DIRECT_V2, ("w_bf3",), (0, 0)),
    "split_v2_16x16x32": (CP.DIRECT_V2_K32, ("w_bf3",), (0, 0)),
    "wino2": (T.WINO, ("w_bf3", "w_wino"), (1, 0)),
    "wino4": (T.WINO4, ("w_bf3", "w_wino", "w_wino4"), (2, 0)),
})
# shapes a Winograd form does not take: dawn_conv3x3_form answers the next form down (F(4x4) -> F(2x2) -> the direct kernel), and that fallback
# is what is asserted (and guarded).  F(2x2) packs four 8 x 8 frames per workgroup and takes whole groups only: F = 13 and F = 5 are refused.
WINO_FALLBACK = {("c3x3_ragged_M", "wino2"): (0, 0), ("c3x3_ragged_M", "wino4"): (0, 0),
                 ("c3x3_halo_N192_ragged_ntile", "wino4"): (1, 0), ("F13_8x8", "wino2"): (0, 0), ("F5_8x8_res", "wino2"): (0, 0),
                 ("F13_8x8", "wino4"): (0, 0), ("F5_8x8_res", "wino4"): (0, 0),
                 ("c3x3_4x4_frames_cat_N128", "wino2"): (0, 0), ("c3x3_4x4_frames_cat_N128", "wino4"): (0, 0),
                 ("L3_8x8_four_frames", "wino4"): (1, 0),
                 ("F17_4x4", "wino2"): (0, 0), ("F17_4x4", "wino4"): (0, 0), ("F33_4x4_cat", "wino2"): (0, 0), ("F33_4x4_cat", "wino4"): (0, 0)}


# dawn_conv3x3_form / dawn_gemm1x1_form answer (0, 0) for the fp32 kernels, the direct split kernel v1 (conv3x3_halo_bf16_kernel) and v2
# (conv3x3_bf16_v2_kernel) alike, so form_only cannot tell these apart.  What does: the bits (the split kernels round differently from the fp32
# ones; a launch that fell through to the fp32 kernel is bit-identical to ConvPolicy.EXACT_FP32, whose fp32 bits the split policies share) and, where the
# grids differ, gn_part.dawn_rows (the launch's workgroup count).  Every multi-frame kernel of the 3x3 family -- both split kernels, the fp32 halo
# kernel, Winograd F(2x2) -- takes whole tiles only (M a multiple of its row tile AND F a multiple of the frames per tile): no kernel ever
# receives a ragged multi-frame tile, the ragged-F shapes run conv_gemm_glds_kernel / conv_gemm_kernel on 128-row tiles with a ragged last
# one.  (case, form) -> the kernel that serves it, where it is not the form's own:
RAGGED = ("c3x3_ragged_M", "F13_8x8", "F5_8x8_res", "F17_4x4", "F33_4x4_cat")
DIRECT = {(c, f): "fp32" for c in RAGGED for f in ("split_v1", "split_v2", "split_v2_16x16x32")}
DIRECT[("c3x3_4x4_frames_cat_N128", "split_v2")] = "v1"          # 16 frames = a 576-pixel patch: instantiated in the 16x16x32 form only


def direct_rows(kernel, M, N):
    """Workgroups (= gn_part rows) of a 3x3 launch: v2 256-row tiles x 64 columns (all cases here are `narrow`), v1 and the fp32 halo kernel
    256 x 64 (N <= 64) or 128 x 128, the generic fp32 kernels cdiv(M, 128) x cdiv(N, 64 or 128)."""
    bn = 64 if N <= 64 else 128
    if kernel == "v2":
        return M // 256 * (N // 64)
    if kernel == "v1":
        return M // (256 if N <= 64 else 128) * -(-N // bn)
    return -(-M // 128) * -(-N // bn)


def run_conv(g, c, tag, policy, want_form, images=(), **extra):
    """The three runs of one case in one launch form; see the module docstring.  -> (result of the first run on the CPU, its dawn_rows)."""
    first = None
    for mode in ("alloc", "out", "slice"):
        g.reset()
        g.conv_policy = policy
        pad = PAD if mode == "slice" else 0
        x0, x1, w = gin(g, c.in0, "in0", pad), gin(g, c.in1, "in1", pad), gin(g, c.w, "w")
        kw = {k: gin(g, v, k, pad) for k, v in c.kw.items()}
        kw.update({k: gin(g, c.images[k], k) for k in images})
        kw.update(extra)
        if c.gn:
            kw["gn_part"] = g.conv_gn_part(c.rows_out, c.N, x0)
        out = None if mode == "alloc" else g.guarded_out(c.rows_out, c.N, pad, name="out")
        n = len(g.outs)
        form = g.conv_gemm(x0, w, c.N, in1=x1, out=out, form_only=True, **kw)
        del g.outs[n:]                                   # (form_only allocated a result of its own when out is None: nothing wrote it)
        want = want_form[mode] if isinstance(want_form, dict) else want_form
        assert form == want, f"{c.name}/{tag}/{mode}: launch form {form}, intended {want}"
        got = g.conv_gemm(x0, w, c.N, in1=x1, out=out, **kw)
        assert out is None or got is out
        assert got.stride(0) == c.N + 2 * pad if out is not None else got.is_contiguous()
        finish(g, f"{c.name}/{tag}/{mode}", got, c.want, chk=c.chk)
        if c.gn:
            assert "conv_gn_part" in {r.name for r in g.outs} and kw["gn_part"].dawn_rows >= 1
        if first is None:
            first = (got.cpu(), kw["gn_part"].dawn_rows if c.gn else None)
    return first


@pytest.mark.parametrize("form", list(FORMS3))
@pytest.mark.parametrize("case", list(CONV3))
def test_conv3x3(g, case, form):
    policy, images, want_form = FORMS3[form]
    c = conv3_case(*CONV3[case])
    got, rows = run_conv(g, c, form, policy, WINO_FALLBACK.get((case, form), want_form), images)
    if not form.startswith("split"):
        return
    # which kernel ran (form_only cannot say: see DIRECT)
    kernel = DIRECT.get((case, form), "v1" if form == "split_v1" else "v2")
    f32, f32_rows = cached(("fp32_bits", case), lambda: run_conv(g, c, "fp32_exact", CP.EXACT_FP32, (0, 0)))
    M = c.rows_out
    if kernel == "fp32":
        assert torch.equal(got, f32), f"{case}/{form}: expected to fall through to the fp32 kernel, but the bits differ from ConvPolicy.EXACT_FP32"
        assert rows == f32_rows
    else:
        assert not torch.equal(got, f32), f"{case}/{form}: bit-identical to the fp32 kernel: the split kernel did not run"
        assert rows == direct_rows(kernel, M, c.N), (rows, kernel)


def gemm_case(M, C0, C1, N, extra):
    """The inputs of test_hip_ops.test_gemm1x1_split_variants."""
    def make():
        from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
        w = packw(C0 + C1, N, seed=2)
        kw = dict(F=M // 64, Hi=8, Wi=8) if M % 64 == 0 else dict(F=M, Hi=1, Wi=1)
        x0, x1 = rnd(M, C0, seed=1), rnd(M, C1, seed=5) if C1 else None
        if "tr" in extra:
            kw["tr"] = (rnd(M, N, seed=6), rnd(N, seed=7), rnd(N, seed=8))
            kw["bias"] = rnd(N, seed=4)
        if "res" in extra:
            kw["res"] = rnd(M, N, seed=3)
        if "bias" in extra:
            kw["bias"] = rnd(N, seed=4)
        if "rowstats" in extra:
            x0 = x0 * 1.7 + 0.4
            kw["row_stats"] = ref.ln_rowstats(x0, x1)
        want = ref.conv_gemm(x0, w, N, in1=x1, **kw)
        return Conv(f"M{M}_C{C0}+{C1}_N{N}_{extra}", x0, x1, w, N, kw, want, dict(w_bf3=pack_bf3(unpack_kn(w))))
    return cached(("gemm", M, C0, C1, N, extra), make)


# the stage-loop corner cases of test_gemm1x1_split_variants (its last five rows) at their M -- two of them are served by the fp32 kernel under
# the shipped policy (N = 64; 200 wide tiles at M = 25,600), which is asserted -- and two rows per row kernel at the smallest M
GEMM = [tuple(p) for p in params(T.test_gemm1x1_split_variants)[-5:]] + [(6400, 64, 64, 64, "tr"), (6400, 128, 0, 192, "rowstats"),
                                                                         (6400, 256, 0, 128, "res"), (6400, 256, 256, 192, "bias")]
GEMM_FORM = {(12800, 32, 0, 64, "bias"): NONE, (12800, 96, 0, 128, "rowstats"): TILED, (25600, 160, 128, 256, "res"): NONE,
             (12800, 32, 64, 128, "rowstats"): TILED, (6400, 96, 0, 256, "tr"): TILED, (6400, 64, 64, 64, "tr"): ROWREG,
             (6400, 128, 0, 192, "rowstats"): ROWREG, (6400, 256, 0, 128, "res"): ROWACC, (6400, 256, 256, 192, "bias"): ROWACC}


@pytest.mark.parametrize("p", GEMM, ids=["M%d_C%d+%d_N%d_%s" % p for p in GEMM])
def test_gemm1x1_split_forms(g, p):
    c = gemm_case(*p)
    run_conv(g, c, "shipped", 0, (0, GEMM_FORM[p]), ("w_bf3",))
    if GEMM_FORM[p] == TILED:
        run_conv(g, c, "tiles128x64", CP.DIRECT_V2_TILE128, (0, TILED), ("w_bf3",))
        run_conv(g, c, "nine_terms", CP.DIRECT_V2_NINE, (0, TILED), ("w_bf3",))
    elif GEMM_FORM[p] != NONE:
        run_conv(g, c, "tiled_for_every_shape", CP.TILED_ONLY, (0, TILED if p[3] != 64 else NONE), ("w_bf3",))       # (N = 64 tiles stay on the fp32 kernel)


@pytest.mark.parametrize("p,ln", [((6400, 64, 64, 64, ""), True), ((6400, 256, 0, 128, ""), True)], ids=["rowreg", "rowacc"])
def test_gemm1x1_layernorm_inside(g, p, ln):
    M, C0, C1, N, _ = p
    c = gemm_case(*p)
    want = cached(("gemm_ln", p), lambda: ref.conv_gemm(c.in0, c.w, N, in1=c.in1, row_stats=ref.ln_rowstats(c.in0, c.in1), **c.kw))
    c2 = Conv(c.name + "_ln", c.in0, c.in1, c.w, N, c.kw, want, c.images)
    run_conv(g, c2, "ln_inside", 0, (0, ROWREG if C0 + C1 <= 128 else ROWACC), ("w_bf3",), ln_eps=1e-5)


@pytest.mark.parametrize("p,form", [((6400, 96, 0, 256, "tr"), TILED), ((6400, 64, 64, 64, "tr"), ROWREG), ((6400, 256, 0, 128, "res"), ROWACC)],
                         ids=["tiled", "rowreg", "rowacc"])
def test_gemm1x1_split_forms_accept_no_ragged_M(g, p, form):
    """Every split 1x1 form takes whole 256-row panels only (the 128 x 64-tile configuration of the tiled kernel, ConvPolicy.TILE128_ALWAYS, too: its
    plan asks M % 256 == 0 although it steps in 128 rows): from the smallest M on, dawn_gemm1x1_form of the same descriptor answers NONE for
    every M that is no multiple of 256, under the shipped policy and under TILE128_ALWAYS -- nothing is there to find, which is what is asserted -- and
    the fp32 kernel that serves such an M instead is guarded."""
    import ctypes
    from dawn_pytorch_amd import _lib
    M, C0, C1, N, extra = p
    FAKE = 0x1000                                        # (nothing is launched: the pointers are never dereferenced)

    def form_of(m, policy):
        d = _lib.ConvDesc()
        d.in0, d.C0, d.ld0 = FAKE, C0, C0
        if C1:
            d.in1, d.C1, d.ld1 = FAKE, C1, C1
        d.F, d.Hi, d.Wi, d.Ho, d.Wo, d.KH, d.KW, d.stride = m, 1, 1, 1, 1, 1, 1, 1
        d.w, d.w_bf3, d.bias, d.N, d.out, d.ld_out, d.policy = FAKE, FAKE, FAKE, N, FAKE, N, policy
        if "res" in extra:
            d.res, d.ld_res = FAKE, N
        if "tr" in extra:
            d.tr, d.ld_tr, d.tr_a, d.tr_b = FAKE, N, FAKE, FAKE
        return g.L.dawn_gemm1x1_form(ctypes.byref(d))
    for policy in (0, CP.DIRECT_V2_TILE128):
        assert form_of(M, policy) == form, policy          # (the row kernels keep their shapes under TILE128_ALWAYS)
        for m in list(range(M - 255, M)) + list(range(M + 1, M + 256)) + [2 * M + 128, 8 * M - 1, 204800 + 128]:
            assert form_of(m, policy) == NONE, (m, policy)
    c = gemm_case(M + 128, C0, C1, N, extra)
    run_conv(g, c, "ragged_M_on_fp32", 0, (0, NONE), ("w_bf3",))
    run_conv(g, c, "ragged_M_on_fp32_tiles128x64", CP.DIRECT_V2_TILE128, (0, NONE), ("w_bf3",))


def resample_case(kind, F, H, W, Cc):
    """test_hip_ops.test_conv_resample_on_split_pipeline: Downsample 4x4 / s2 and the transposed Upsample, against torch's convolutions."""
    def make():
        from dawn_pytorch_amd.pack import conv_w_kn, deconv_w_kn_phases, pack_bf3, pack_kn
        x, b = rnd(F * H * W, Cc, seed=2), rnd(Cc, seed=3)
        img = x.reshape(F, H, W, Cc).permute(0, 3, 1, 2)
        if kind == "down":
            w5 = rnd(Cc, Cc, 1, 4, 4, seed=1, scale=(Cc * 16) ** -0.5)
            wkn = conv_w_kn(w5)
            want = torch.nn.functional.conv2d(img, w5[:, :, 0], b, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, Cc)
            kw = dict(F=F, Hi=H, Wi=W, Ho=H // 2, Wo=W // 2, KH=4, KW=4, stride=2, pad=1, bias=b)
            return Conv(f"down_F{F}_{H}x{W}_C{Cc}", x, None, pack_kn(wkn), Cc, kw, want, dict(w_bf3=pack_bf3(wkn)))
        w5t = rnd(Cc, Cc, 1, 4, 4, seed=4, scale=(Cc * 4) ** -0.5)
        ph = deconv_w_kn_phases(w5t)
        want = torch.nn.functional.conv_transpose2d(img, w5t[:, :, 0], b, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, Cc)
        kw = dict(F=F, Hi=H, Wi=W, Ho=2 * H, Wo=2 * W, KH=2, KW=2, mode=1, bias=b)
        return Conv(f"up_F{F}_{H}x{W}_C{Cc}", x, None, torch.stack([pack_kn(ph[i]) for i in range(4)], 0), Cc, kw, want,
                    dict(w_bf3=torch.stack([pack_bf3(ph[i]) for i in range(4)], 0)))
    return cached(("resample", kind, F, H, W, Cc), make)


@pytest.mark.parametrize("kind,F,H,W,Cc", [("up", 50, 16, 16, 64), ("down", 50, 32, 32, 64), ("up", 3, 8, 8, 64), ("down", 3, 16, 16, 64)],
                         ids=["up_rowacc", "down_rowacc", "up_small", "down_small"])
def test_resample(g, kind, F, H, W, Cc):
    """Row-accumulator kernel in modes 1 (transposed up) and 2 (4x4 / s2 down) at its smallest M (12,800 rows), and the fp32 kernels on the
    same operators (without the split image; and below that M, where the split image is refused)."""
    c = resample_case(kind, F, H, W, Cc)
    big = (F * H * W if kind == "up" else F * H * W // 4) >= 12800          # rows of the GEMM: input pixels (up), output pixels (down)
    run_conv(g, c, "split", 0, (0, RESAMPLE if big else NONE), ("w_bf3",))
    run_conv(g, c, "fp32", 0, (0, NONE))


UPCONV = [(k, b, f) for k, forms in (((2, 8, 8, 16, 16), ("glds", "reg")), ((3, 4, 16, 64, 64), ("glds", "reg")), ((50, 16, 16, 64, 64), ("split",)))
          for f in forms for b in (0, 1, 2)]


@pytest.mark.parametrize("key,border,form", UPCONV, ids=["F%d_%dx%d_C%d_N%d" % k + f"_{f}_border{b}" for k, b, f in UPCONV])
def test_upconv_phase_kernels(g, key, border, form):
    """use_deconv=False (nearest x2 + 3x3 as four 2x2 phases): the three kernels that gather mode-1 taps, every border mode; shapes, inputs,
    fp64 literal and gate of tests/test_hip_upconv.py."""
    u = UP.case(*key)
    kw = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in u.kw.items()}
    c = Conv("upconv_F%d_%dx%d_C%d_N%d" % key, u.x, None, u.wp.cpu(), u.N, kw, u.want(border),
             dict(w_bf3=None if u.ws is None else u.ws.cpu()), chk=UP.check)
    policy = CP.DEFAULT & ~CP.GLDS if form == "reg" else 0
    run_conv(g, c, f"{form}/border{border}", policy, (0, RESAMPLE if form == "split" else NONE), ("w_bf3",) if form == "split" else (),
             border=border)


EPILOGUE = ["c3x3_gn_prologue_add", "c1x1_tr_epilogue", "c1x1_res_epilogue", "c1x1_rowstats_cat_192", "c3x3_16_16_tinyN", "down4x4s2"]


@pytest.mark.parametrize("name", EPILOGUE)
def test_conv_epilogue_operands(g, name):
    """The small cases of test_conv_gemm that carry ch_ab / pro_add / tr / res / row_stats (and the 16-channel and 4x4 / s2 shapes), every
    operand guarded, on the shipped policy and on the register-staged fp32 kernel."""
    def make():
        _, F, H, W, C0, C1, N, k, stride, pad, ex = _row(T.CONV_CASES, name)
        rows = F * H * W
        Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        in0, in1 = rnd(rows, C0, seed=1), rnd(rows, C1, seed=2) if C1 else None
        w = packw(k * k * (C0 + C1), N, seed=3)
        kw = dict(F=F, Hi=H, Wi=W, Ho=Ho, Wo=Wo, KH=k, KW=k, stride=stride, pad=pad)
        if ex.get("bias"):
            kw["bias"] = rnd(N, seed=4)
        if ex.get("row_stats"):
            x = in0 if in1 is None else torch.cat((in0, in1), 1)
            kw["row_stats"] = (x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-5))
        if ex.get("ch_ab"):
            kw["ch_ab"] = (rnd(C0, seed=5) * 0.3 + 1.0, rnd(C0, seed=6) * 0.3)
        if ex.get("pro_act"):
            kw["pro_act"] = 1
        if ex.get("pro_add"):
            kw["pro_add"] = rnd(rows, C0, seed=7)
        if ex.get("res"):
            kw["res"] = rnd(F * Ho * Wo, N, seed=8)
        if ex.get("tr"):
            kw["tr"] = (rnd(F * Ho * Wo, N, seed=9), rnd(N, seed=10) * 0.3 + 1.0, rnd(N, seed=11) * 0.3)
        return Conv(name, in0, in1, w, N, kw, ref.conv_gemm(in0, w, N, in1=in1, **kw))
    c = cached(("epi", name), make)
    for policy in (0, CP.EXACT_FP32, CP.DEFAULT & ~CP.GLDS):
        run_conv(g, c, f"v{int(policy)}", policy, (0, 0))


# ---------------------------------------------------------------------------------------------- fused 64-channel layers, attention cores
def rotary(Fext):
    ang = torch.arange(Fext).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    return ang.cos().contiguous(), ang.sin().contiguous()


def temporal_case(Fext, HW, q0, Fq, win):
    def make():
        from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, unpack_kn
        x = rnd(Fext * HW, 64, seed=1) * 1.3 + 0.2
        wqkv, wout = packw(64, 768, seed=2), packw(256, 64, seed=3)
        rc, rs = rotary(Fext)
        band = rnd(2 * win + 1, 8, seed=4)
        want = ref.temporal_layer_c64(x, Fext, HW, q0, Fq, win, wqkv, wout, rc, rs, band)
        return x, wqkv, wout, rc, rs, band, pack_bf3(unpack_kn(wqkv)), pack_bf3_temporal_out(unpack_kn(wout)), want
    return cached(("temporal", Fext, HW, q0, Fq, win), make)


def temporal_args(g, c):
    x, wqkv, wout, rc, rs, band, bf3, bf3p, want = c
    return (gin(g, x, "x"), [gin(g, t, n) for t, n in ((wqkv, "wqkv"), (wout, "wout"), (rc, "rcos"), (rs, "rsin"), (band, "band"))],
            dict(wqkv_bf3=gin(g, bf3, "wqkv_bf3"), wout_bf3p=gin(g, bf3p, "wout_bf3p")), want)


# the shapes of test_temporal_layer_c64 that a CPU reference serves in well under a second: HW = 2 ... 5, q0 > 0, Fq < Fext, win up to 48.  Its
# HW = 64 case (and the HW >= 64 cases of test_temporal_attn below) is left to that test for run time; so that more than a few pixel columns, and a
# count that is no multiple of 4 (nor of the 16 / 32-column tiles), are guarded, one short clip at HW = 130 is added to both
TL_SHAPES = [tuple(s) for s in params(T.test_temporal_layer_c64) if s[0] * s[1] <= 600] + [(12, 130, 0, 12, 3), (20, 130, 3, 14, 5)]
TL = [(s, fl) for s in TL_SHAPES for fl in TEMPORAL_FLAGS + (TF.force_wmode(3) | TF.SCHED_HINTS, TF.force_wmode(3) | TF.OUT_FP32) if temporal_fits(fl, s[0], s[2], s[3], s[4])]


@pytest.mark.parametrize("shape,flags", TL, ids=["F%d_HW%d_q%d_%d_w%d" % s + f"_flags{fl}" for s, fl in TL])
def test_temporal_layer_c64(g, shape, flags):
    Fext, HW, q0, Fq, win = shape
    x, w, kw, want = temporal_args(g, temporal_case(*shape))
    g.temporal_flags = flags
    got = g.temporal_layer_c64(x, Fext, HW, q0, Fq, win, *w, **kw)
    finish(g, "temporal_layer_c64/F%d_HW%d_q%d_%d_w%d" % shape + f"/flags{flags}", got, want, 3e-5)
    if flags == 0:                                       # ... the fp32-MFMA form (no split images), and a caller's `out`
        g.reset()
        x, w, kw, want = temporal_args(g, temporal_case(*shape))
        got = g.temporal_layer_c64(x, Fext, HW, q0, Fq, win, *w, out=g.guarded_out(Fq * HW, 64))
        finish(g, "temporal_layer_c64/F%d_HW%d_q%d_%d_w%d" % shape + "/fp32_out", got, want, 3e-5)


@pytest.mark.parametrize("Fext,HW,q0,Fq", [tuple(s) for s in params(T.test_temporal_layer_c64_segmented) if s[1] <= 4])
def test_temporal_layer_c64_segmented(g, Fext, HW, q0, Fq):
    x, w, kw, want = temporal_args(g, temporal_case(Fext, HW, q0, Fq, 40))
    got = g.temporal_layer_c64_segmented(x, Fext, HW, q0, Fq, 40, *w, **kw)
    finish(g, f"temporal_layer_c64_segmented/F{Fext}_q{q0}_{Fq}", got, want, 3e-5)


TA_SHAPES = [tuple(s) for s in params(T.test_temporal_attn) if s[0] * s[1] <= 400] + [(12, 130, 0, 12, 3), (20, 130, 3, 14, 5)]


TA = [(s, fl) for s in TA_SHAPES for fl in (0, TA_.FP32, TA_.SPLIT_ALWAYS, TA_.WAVE13)
      if fl != TA_.WAVE13 or (s[4] <= 40 and s[0] <= 208 and (s[3] + (s[2] - s[4]) % 16 + 15) // 16 <= 13)]          # (the 13-wave kernel's instantiation)


@pytest.mark.parametrize("shape,flags", TA, ids=["F%d_HW%d_q%d_%d_w%d" % s + f"_flags{fl}" for s, fl in TA])
def test_temporal_attn(g, shape, flags):
    Fext, HW, q0, Fq, win = shape

    def make():
        qkv, (rc, rs), band = rnd(Fext * HW, 768, seed=1), rotary(Fext), rnd(2 * win + 1, 8, seed=2)
        return qkv, rc, rs, band, ref.temporal_attn(qkv, Fext, HW, q0, Fq, win, rc, rs, band)
    qkv, rc, rs, band, want = cached(("tattn", Fext, HW, q0, Fq, win), make)
    g.temporal_attn_flags = flags
    got = g.temporal_attn(gin(g, qkv, "qkv"), Fext, HW, q0, Fq, win, gin(g, rc, "rcos"), gin(g, rs, "rsin"), gin(g, band, "band"))
    finish(g, f"temporal_attn/F{Fext}_HW{HW}_q{q0}_{Fq}_w{win}/flags{flags}", got, want, 2e-5)


SLA_SHAPES = [tuple(s) for s in params(T.test_sla_layer_c64) if s[0] * s[1] <= 3000]


@pytest.mark.parametrize("split", [False, True], ids=["fp32", "wqkv_bf3"])
@pytest.mark.parametrize("F,HW", SLA_SHAPES)
def test_sla_layer_c64(g, F, HW, split):
    def make():
        from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
        x = rnd(F * HW, 64, seed=1) * 1.3 + 0.2
        wqkv, wout, bias = packw(64, 768, seed=2) * 2.0, packw(256, 64, seed=3), rnd(64, seed=4)
        return x, wqkv, wout, bias, pack_bf3(unpack_kn(wqkv)), ref.sla_layer_c64(x, F, HW, wqkv, wout, bias)
    x, wqkv, wout, bias, bf3, want = cached(("sla_layer", F, HW), make)
    for own_out in (False, True):
        g.reset()
        out = g.guarded_out(F * HW, 64) if own_out else None
        got = g.sla_layer_c64(gin(g, x, "x"), F, HW, gin(g, wqkv, "wqkv"), gin(g, wout, "wout"), gin(g, bias, "bias"),
                              wqkv_bf3=gin(g, bf3, "wqkv_bf3") if split else None, out=out)
        assert "sla_layer_c64.ws" in {r.name for r in g.outs}            # the exemption of guarded.PARTIAL is keyed by this name
        finish(g, f"sla_layer_c64/F{F}_HW{HW}/split{int(split)}/out{int(own_out)}", got, want, 3e-5)


@pytest.mark.parametrize("F,HW", params(T.test_sla))
def test_sla(g, F, HW):
    qkv, want = cached(("sla", F, HW), lambda: (lambda q: (q, ref.sla(q, F, HW)))(rnd(F * HW, 768, seed=1)))
    finish(g, f"sla/F{F}_HW{HW}", g.sla(gin(g, qkv, "qkv"), F, HW), want, 2e-5)


@pytest.mark.parametrize("F,N", params(T.test_frame_attn))
def test_frame_attn(g, F, N):
    qkv, want = cached(("fattn", F, N), lambda: (lambda q: (q, ref.frame_attn(q, F, N)))(rnd(F * N, 768, seed=1)))
    finish(g, f"frame_attn/F{F}_N{N}", g.frame_attn(gin(g, qkv, "qkv"), F, N), want, 2e-5)


def xattn_tabs(Fn):
    def make():
        kvtab, nulltab = torch.zeros(Fn, 3, 128), torch.zeros(3, 16)
        for b in range(3):
            ref.xattn_prep(rnd(Fn, 128, seed=20 + b), rnd(8, seed=30 + b) * 0.2 + 1, rnd(2, 8, seed=40 + b), kvtab, b, nulltab)
        return kvtab, nulltab
    return cached(("xtabs", Fn), make)


@pytest.mark.parametrize("C0,C1,Fn,HW", [tuple(s) for s in params(T.test_xattn_layer_c64) if s[2] * s[3] <= 400])
def test_xattn_layer_c64(g, C0, C1, Fn, HW):
    """Both Q projections (fp32, wq_bf3), the sources once contiguous and once as column slices (two-source: both), h_cond and the h1
    epilogue, the latter also written over c1."""
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    rows = Fn * HW
    kvtab, nulltab = xattn_tabs(Fn)

    def make():
        x, x2 = rnd(rows, C0, seed=1) * 1.5 + 0.3, rnd(rows, C1, seed=2) if C1 else None
        wq, wo = packw(C0 + C1, 192, seed=3), [packw(64, 64, seed=10 + b) for b in range(3)]
        g3, qs = rnd(3, 64, seed=4) * 0.2 + 1, rnd(3, 8, seed=5) * 0.2 + 1
        c1, ga, gb = rnd(rows, 64, seed=7) * 1.5, rnd(64, seed=8) * 0.3 + 1, rnd(64, seed=9) * 0.3
        return (x, x2, wq, wo, g3, qs, c1, ga, gb, ref.xattn_layer_c64(x, x2, HW, wq, wo, g3, qs, kvtab, nulltab),
                ref.xattn_layer_c64(x, x2, HW, wq, wo, g3, qs, kvtab, nulltab, gn=(c1, ga, gb)))
    x, x2, wq, wo, g3, qs, c1, ga, gb, want, want_h1 = cached(("xlayer", C0, C1, Fn, HW), make)
    for split in (False, True):
        for pad in (0, PAD):
            for h1 in (None, "out", "over_c1"):
                g.reset()
                a = (gin(g, x, "x", pad), gin(g, x2, "x2", pad), HW, gin(g, wq, "wq"), gin(g, wo, "wo"), gin(g, g3, "g3"), gin(g, qs, "q_scale"),
                     gin(g, kvtab, "kvtab"), gin(g, nulltab, "nulltab"))
                kw = dict(wq_bf3=gin(g, pack_bf3(unpack_kn(wq)), "wq_bf3") if split else None)
                if h1:
                    kw.update(gn=(gin(g, c1, "c1"), gin(g, ga, "gn_a"), gin(g, gb, "gn_b")), h1_over_c1=h1 == "over_c1")
                got = g.xattn_layer_c64(*a, **kw)
                assert (h1 is not None and got is kw["gn"][0]) == (h1 == "over_c1")
                finish(g, f"xattn_layer_c64/{C0}+{C1}_F{Fn}_HW{HW}/split{int(split)}/pad{pad}/{h1}", got, want_h1 if h1 else want, 3e-5,
                       overwritten=("c1",) if h1 == "over_c1" else ())


@pytest.mark.parametrize("Co,Fn,HW", [tuple(s) for s in params(T.test_xattn_sigma_out_equals_unfused_chain) if s[1] * s[2] <= 400])
def test_xattn_sigma_out(g, Co, Fn, HW):
    rows = Fn * HW
    kvtab, nulltab = xattn_tabs(Fn)

    def make():
        q = rnd(rows, 192, seed=1) * 1.3
        wo = [packw(64, Co, seed=10 + b) for b in range(3)]
        g3, qs = rnd(3, Co, seed=4) * 0.2 + 1, rnd(3, 8, seed=5) * 0.2 + 1
        c1, ga, gb = rnd(rows, Co, seed=7) * 1.5, rnd(Co, seed=8) * 0.3 + 1, rnd(Co, seed=9) * 0.3
        xtab = ref.xattn_tables(kvtab, nulltab, qs, wo, Co)
        o = ref.xattn_core(q.clone(), HW, kvtab, nulltab, qs)
        y3 = torch.cat([ref.conv_gemm(o[:, 64 * b:64 * b + 64], wo[b], Co, F=rows, Hi=1, Wi=1) for b in range(3)], 1)
        return q, g3, c1, ga, gb, xtab, ref.xattn_ln_sum(y3, g3, Co), ref.xattn_sigma_out(q, HW, xtab, g3, Co, gn=(c1, ga, gb))
    q, g3, c1, ga, gb, xtab, want, want_h1 = cached(("xsigma", Co, Fn, HW), make)
    for h1 in (None, "out", "over_c1"):
        g.reset()
        kw = dict(gn=(gin(g, c1, "c1"), gin(g, ga, "gn_a"), gin(g, gb, "gn_b")), h1_over_c1=h1 == "over_c1") if h1 else {}
        got = g.xattn_sigma_out(gin(g, q, "q"), HW, gin(g, xtab, "xtab"), gin(g, g3, "g3"), Co, **kw)
        finish(g, f"xattn_sigma_out/Co{Co}_F{Fn}_HW{HW}/{h1}", got, want_h1 if h1 else want, 3e-5, overwritten=("c1",) if h1 == "over_c1" else ())


def test_xattn_core_and_ln_sum(g):
    """test_hip_ops.test_xattn_pieces: the in-place 2-key attention on q, and the LayerNorm-sum of the three branches."""
    Fn, HW = 7, 12
    rows = Fn * HW
    kvtab, nulltab = xattn_tabs(Fn)
    q, qs = rnd(rows, 192, seed=3), rnd(3, 8, seed=4) * 0.2 + 1
    want = ref.xattn_core(q.clone(), HW, kvtab, nulltab, qs)
    qg = gin(g, q, "q")
    got = g.xattn_core(qg, HW, gin(g, kvtab, "kvtab"), gin(g, nulltab, "nulltab"), gin(g, qs, "q_scale"))
    assert got is qg
    finish(g, "xattn_core", got, want, 1e-5, overwritten=("q",))
    for Co in (16, 64, 96, 128, 512):
        g.reset()
        y3, g3 = rnd(rows, 3 * Co, seed=5), rnd(3, Co, seed=6) * 0.2 + 1
        finish(g, f"xattn_ln_sum/Co{Co}", g.xattn_ln_sum(gin(g, y3, "y3"), gin(g, g3, "g3"), Co), ref.xattn_ln_sum(y3, g3, Co), 2e-5)


@pytest.mark.parametrize("F,HW", params(T.test_c64_attention_layers_in_place)[-1:])
def test_c64_attention_layers_in_place(g, F, HW):
    """`out` is `x`: bands around the aliased buffer.  Values as in test_hip_ops.test_c64_attention_layers_in_place: in place == out of place,
    bit for bit, for the fp32-MFMA form, the window-tiled kernel and the 32 x 32 one, and for both SLA forms."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, unpack_kn
    win = 40
    x = rnd(F * HW, 64, seed=1) * 1.3 + 0.2
    wqkv, wout, bias = packw(64, 768, seed=2), packw(256, 64, seed=3), rnd(64, seed=4)
    rc, rs = rotary(F)
    band = rnd(2 * win + 1, 8, seed=5)
    wsplit, wosp = pack_bf3(unpack_kn(wqkv)), pack_bf3_temporal_out(unpack_kn(wout))

    def both(call):
        g.reset()
        want = call(gin(g, x, "x"), None).clone()
        torch.cuda.synchronize()
        g.verify()
        g.inputs_intact()
        g.reset()
        xin = gin(g, x, "x")
        got = call(xin, xin)
        torch.cuda.synchronize()
        assert got is xin and torch.equal(got, want)
        assert not torch.isnan(got).any()
        g.verify()
        g.inputs_intact(overwritten=("x",))

    for split, flags in ((False, 0), (True, 0), (True, TF.force_wmode(3))):
        g.temporal_flags = flags
        both(lambda xg, out: g.temporal_layer_c64(
            xg, F, HW, 0, F, win, *[gin(g, t, n) for t, n in ((wqkv, "wqkv"), (wout, "wout"), (rc, "rcos"), (rs, "rsin"), (band, "band"))],
            out=out, **(dict(wqkv_bf3=gin(g, wsplit, "wqkv_bf3"), wout_bf3p=gin(g, wosp, "wout_bf3p")) if split else {})))
    g.temporal_flags = 0
    for split in (False, True):
        both(lambda xg, out: g.sla_layer_c64(xg, F, HW, gin(g, wqkv, "wqkv"), gin(g, wout, "wout"), gin(g, bias, "bias"), out=out,
                                             wqkv_bf3=gin(g, wsplit, "wqkv_bf3") if split else None))


# ---------------------------------------------------------------------------------------------- norms, boundary kernels
@pytest.mark.parametrize("C,rows,film", params(T.test_gn_coeffs_and_apply))
def test_gn_coeffs_and_apply(g, C, rows, film):
    x = rnd(rows, C, seed=1) * 2 + 0.5
    gamma, beta = rnd(C, seed=2) * 0.2 + 1, rnd(C, seed=3) * 0.2
    fl = (rnd(C, seed=4) * 0.3, rnd(C, seed=5) * 0.3) if film else None
    wa, wb = ref.gn_coeffs(x, gamma, beta, fl, rows)
    for pad in (0, PAD):
        g.reset()
        ga, gb = g.gn_coeffs(gin(g, x, "x", pad), gin(g, gamma, "gamma"), gin(g, beta, "beta"), gin(g, fl, "film"), rows)
        finish(g, f"gn_coeffs/a_C{C}/pad{pad}", ga, wa, 2e-5)
        check(f"guard/gn_coeffs/b_C{C}/pad{pad}", gb, wb, 2e-5)
    res = rnd(rows, C, seed=6)
    want = torch.nn.functional.silu(x * wa + wb) + res
    for inplace in (False, True):
        g.reset()
        xg = gin(g, x, "x")
        got = g.gn_apply_res(xg, gin(g, wa, "a"), gin(g, wb, "b"), gin(g, res, "res"), inplace=inplace)
        assert (got is xg) == inplace
        finish(g, f"gn_apply_res/C{C}/inplace{int(inplace)}", got, want, 2e-5, overwritten=("x",) if inplace else ())


@pytest.mark.parametrize("C0,C1,rows", params(T.test_ln_rowstats))
def test_ln_rows_and_rowstats(g, C0, C1, rows):
    a = rnd(rows, C0, seed=1) * 1.5 + 0.3
    b = rnd(rows, C1, seed=2) if C1 else None
    wm, wr = ref.ln_rowstats(a, b)
    for pad in (0, PAD):
        g.reset()
        gm, gr = g.ln_rowstats(gin(g, a, "in0", pad), gin(g, b, "in1", pad))
        finish(g, f"ln_rowstats/mean_{C0}_{C1}/pad{pad}", gm, wm, 1e-5)
        check(f"guard/ln_rowstats/rstd_{C0}_{C1}/pad{pad}", gr, wr, 1e-5)
        g.reset()
        finish(g, f"ln_rows/{C0}_{C1}/pad{pad}", g.ln_rows(gin(g, a, "in0", pad), gin(g, b, "in1", pad)), ref.ln_rows(a, b), 1e-5)


@pytest.mark.parametrize("F,h,w", [(3, 8, 8), (2, 32, 32), (3, 16, 16), (2, 12, 64), (5, 5, 7)])
def test_init_conv_x(g, F, h, w):
    """The whole clip, and a frame sub-range (fa, fb): the frames before fa and after fb are then guarded input like everything else."""
    Co = 64
    x, w3, fp = rnd(3, F, h, w, seed=11), rnd(147, Co, seed=2) * 0.1, rnd(h * w, Co, seed=13)
    want = ref.init_conv_x(x, w3, fp, F, h, w, Co)
    for frames in (None, (1, F - 1) if F > 2 else (1, 2), (0, 1)):
        for own_out in (False, True):
            g.reset()
            fa, fb = frames or (0, F)
            out = g.guarded_out((fb - fa) * h * w, Co) if own_out else None
            got = g.init_conv_x(gin(g, x, "x"), gin(g, w3, "w3"), gin(g, fp, "fea_pre"), F, h, w, Co, frames=frames, out=out)
            finish(g, f"init_conv_x/{F}x{h}x{w}/{frames}/out{int(own_out)}", got, want[fa * h * w:fb * h * w], 2e-5)


@pytest.mark.parametrize("Co,rows", [(16, 500), (64, 500), (64, 1), (64, 257)])
def test_head_out(g, Co, rows):
    hg, ho = rnd(rows, Co, seed=4), rnd(rows, Co, seed=5)
    ws = [rnd(2, Co, seed=6), rnd(2, seed=7), rnd(1, Co, seed=8), rnd(1, seed=9)]
    want = ref.head_out(hg, ho, *ws)

    def run(a, b, out=None):
        return g.head_out(gin(g, a, "hg"), gin(g, b, "ho"), *[gin(g, t, n) for t, n in zip(ws, ("wg", "bg", "wo", "bo"))], out=out)
    got = run(hg, ho)
    assert "head_out.out" in {r.name for r in g.outs}
    finish(g, f"head_out/Co{Co}_rows{rows}", got, want, 2e-5)
    for a, b, sl in ((hg, None, slice(0, 2)), (None, ho, slice(2, 3))):       # one head at a time: only that head's rows of `out`
        g.reset()
        out = g.guarded_out(3, rows, name="head_out.out")
        got = run(a, b, out)
        torch.cuda.synchronize()
        check(f"guard/head_out/Co{Co}_rows{rows}/{sl}", got[sl], want[sl], 2e-5)
        g.verify(written={"head_out.out": sl})
        g.inputs_intact()


LINEAR = [tuple(p) for p in params(T.test_linear)] + [(1, 64, 67, 0, True), (3, 6, 130, 1, True)]          # ... and ragged N


@pytest.mark.parametrize("M,K,N,act,bias", LINEAR)
def test_linear(g, M, K, N, act, bias):
    x, W = rnd(M, K, seed=1), rnd(N, K, seed=2) * K ** -0.5
    b = rnd(N, seed=3) if bias else None
    want = ref.linear(x, W, b, act)
    for mode in ("alloc", "out", "slice"):
        g.reset()
        pad = PAD if mode == "slice" else 0
        out = None if mode == "alloc" else g.guarded_out(M, N, pad)
        got = g.linear(gin(g, x, "x", pad), gin(g, W, "W"), gin(g, b, "bias"), act, out=out)
        finish(g, f"linear/{M}x{K}x{N}_a{act}/{mode}", got, want, 2e-5)


def test_contiguous_only_operands_are_refused(g):
    """The fused layers, the attention cores and init_conv_x take contiguous x / qkv / out only: a column slice (ld > C) is refused before anything
    is launched -- the guarded `out` is still all poison, its neighbours untouched -- not computed with a wrong stride."""
    from dawn_pytorch_amd._lib import DawnHipError
    from guarded import _poisoned
    F, HW, win = 6, 4, 2
    x, qkv = rnd(F * HW, 64, seed=1), rnd(F * HW, 768, seed=2)
    wqkv, wout, bias = packw(64, 768, seed=2), packw(256, 64, seed=3), rnd(64, seed=4)
    rc, rs = rotary(F)
    band = rnd(2 * win + 1, 8, seed=4)
    lat, w3, fp = rnd(3, F, 2, 2, seed=11), rnd(147, 64, seed=2) * 0.1, rnd(HW, 64, seed=13)

    def tl(xg, out):
        return g.temporal_layer_c64(xg, F, HW, 0, F, win, *[gin(g, t, n) for t, n in ((wqkv, "wqkv"), (wout, "wout"), (rc, "rcos"), (rs, "rsin"), (band, "band"))], out=out)

    def sl(xg, out):
        return g.sla_layer_c64(xg, F, HW, gin(g, wqkv, "wqkv"), gin(g, wout, "wout"), gin(g, bias, "bias"), out=out)
    calls = {
        "temporal_layer_c64/out": lambda out: tl(gin(g, x, "x"), out),
        "temporal_layer_c64_segmented/out": lambda out: g.temporal_layer_c64_segmented(
            gin(g, x, "x"), F, HW, 0, F, win, *[gin(g, t, n) for t, n in ((wqkv, "wqkv"), (wout, "wout"), (rc, "rcos"), (rs, "rsin"), (band, "band"))], out=out),
        "sla_layer_c64/out": lambda out: sl(gin(g, x, "x"), out),
        "init_conv_x/out": lambda out: g.init_conv_x(gin(g, lat, "x"), gin(g, w3, "w3"), gin(g, fp, "fea_pre"), F, 2, 2, 64, out=out),
        "temporal_layer_c64/x": lambda out: tl(gin(g, x, "x", PAD), None),
        "temporal_layer_c64_segmented/x": lambda out: g.temporal_layer_c64_segmented(gin(g, x, "x", PAD), F, HW, 0, F, win, None, None, None, None, None),
        "sla_layer_c64/x": lambda out: sl(gin(g, x, "x", PAD), None),
        "temporal_attn/qkv": lambda out: g.temporal_attn(gin(g, qkv, "qkv", PAD), F, HW, 0, F, win, gin(g, rc, "rcos"), gin(g, rs, "rsin"), gin(g, band, "band")),
        "sla/qkv": lambda out: g.sla(gin(g, qkv, "qkv", PAD), F, HW),
        "frame_attn/qkv": lambda out: g.frame_attn(gin(g, qkv, "qkv", PAD), F, HW),
        "xattn_core/q": lambda out: g.xattn_core(gin(g, rnd(F * HW, 192, seed=3), "q", PAD), HW, None, None, None),
        "xattn_ln_sum/y3": lambda out: g.xattn_ln_sum(gin(g, rnd(F * HW, 192, seed=5), "y3", PAD), None, 64),
        "gn_apply_res/x": lambda out: g.gn_apply_res(gin(g, x, "x", PAD), None, None, None),
    }
    for name, call in calls.items():
        g.reset()
        out = g.guarded_out(F * HW, 64, PAD, name="out") if name.endswith("/out") else None
        with pytest.raises(DawnHipError, match="precondition"):
            call(out)
        torch.cuda.synchronize()
        for r in g.outs:
            r.check_surroundings(f"{name}: refused, yet written")
            assert bool(_poisoned(r.payload).all()), f"{name}: refused, yet {r.name} was written"
        g.inputs_intact()
