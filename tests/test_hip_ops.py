"""-m gpu: every HIP kernel (through the C ABI / HipOps) against the torch op reference of the same name
(oracle/ops_ref.py, evaluated on CPU in fp32) on the same seeded inputs.

Tolerance (stated): fp32 MFMA / VALU arithmetic vs CPU fp32 differ only in summation order, so
|hip - ref| <= 1e-4 * max(1, max|ref|) for GEMM-like ops (K up to ~9k), 1e-5-class for elementwise ops;
integer work (histograms, select state) is bit-exact."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from dawn_pytorch_amd.policy import ConvPolicy as CP, TemporalAttnFlags as TA, TemporalFlags as TF
from oracle.ops_ref import RefOps

pytestmark = pytest.mark.gpu

WMODE = TF.force_wmode             # temporal_flags that force WMODE m
# every fp32-MFMA tile configuration: automatic, 256 x 64 tiles, the direct-to-LDS path with BK = 32 / three stages / with and without its
# 256 x 64 tile, the shipped fp32 tiles, and those with the LDS-halo 3x3 kernel
FP32_POLICIES = (0, CP.BK32 | CP.TILE256 | CP.XCD_ORDER, CP.FP32_TILES | CP.GLDS_BK32, CP.FP32_TILES | CP.GLDS_STAGES3,
                 CP.FP32_TILES | CP.GLDS_TILE256, CP.FP32_TILES | CP.GLDS_NO_TILE256, CP.FP32_TILES, CP.EXACT_FP32)

LOG = os.path.join(ROOT, "gpurun_out", "op_errors.jsonl")


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


@pytest.fixture(scope="module")
def ref():
    return RefOps()


def gpu(*ts):
    return [None if t is None else (tuple(gpu(*t)) if isinstance(t, (tuple, list)) else t.cuda()) for t in ts]


def check(name, got, want, tol=1e-4):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(json.dumps({"op": name, "max_abs_err": err, "scale": scale, "tol": tol * scale,
                            "nan": bool(torch.isnan(got).any())}) + "\n")
    assert not torch.isnan(got).any(), f"{name}: NaN"
    assert err <= tol * scale, f"{name}: max|diff| {err:.3e} > {tol * scale:.3e}"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def packw(K, N, seed=0):
    from dawn_pytorch_amd.pack import pack_kn
    return pack_kn(rnd(K, N, seed=seed, scale=K ** -0.5))


# ---------------------------------------------------------------------------------------------- conv_gemm
CONV_CASES = [
    # name, F, H, W, C0, C1, N, KH, stride, pad, extras
    ("c3x3_64_64", 3, 16, 16, 64, 0, 64, 3, 1, 1, {}),
    ("c3x3_cat_128p128_256_bias", 2, 8, 8, 128, 128, 256, 3, 1, 1, {"bias": True}),
    ("c3x3_16_16_tinyN", 5, 8, 8, 16, 0, 16, 3, 1, 1, {"bias": True}),
    ("c1x1_rowstats_768", 2, 8, 8, 64, 0, 768, 1, 1, 0, {"row_stats": True}),
    ("c1x1_rowstats_cat_192", 3, 4, 4, 512, 512, 192, 1, 1, 0, {"row_stats": True}),
    ("c3x3_gn_prologue_add", 3, 8, 8, 128, 0, 128, 3, 1, 1, {"ch_ab": True, "pro_act": 1, "pro_add": True, "bias": True}),
    ("c1x1_tr_epilogue", 2, 8, 8, 256, 0, 128, 1, 1, 0, {"tr": True, "bias": True}),
    ("c1x1_res_epilogue", 2, 8, 8, 256, 0, 64, 1, 1, 0, {"res": True}),
    ("down4x4s2", 3, 16, 16, 64, 0, 64, 4, 2, 1, {"bias": True}),
    ("c7x7_fea", 1, 16, 16, 272, 0, 64, 7, 1, 3, {"bias": True}),
    ("c3x3_512_512_deepK", 7, 4, 4, 512, 0, 512, 3, 1, 1, {"bias": True}),
    ("c3x3_ragged_M", 1, 5, 7, 32, 0, 48, 3, 1, 1, {}),
    ("c3x3_bigM_N64_tile256", 2, 192, 190, 16, 0, 64, 3, 1, 1, {"bias": True}),
    ("c1x1_bigM_N64_rowstats_res", 3, 160, 150, 32, 32, 64, 1, 1, 0, {"row_stats": True, "res": True}),
    ("c3x3_k32_cat_N128", 2, 24, 24, 64, 32, 128, 3, 1, 1, {"bias": True}),
    ("c3x3_k32_cat_256p256_N128_deepK", 3, 8, 8, 256, 256, 128, 3, 1, 1, {"bias": True}),
    ("c3x3_halo_W64_rows4", 1, 64, 64, 32, 0, 64, 3, 1, 1, {"bias": True}),
    ("c3x3_halo_cat_W32_N128", 2, 32, 32, 64, 64, 128, 3, 1, 1, {"bias": True}),
    ("c3x3_halo_multiframe_tile", 8, 4, 4, 64, 0, 128, 3, 1, 1, {}),
    ("c3x3_halo_N192_ragged_ntile", 4, 8, 8, 32, 0, 192, 3, 1, 1, {"bias": True}),
    # 4 x 4-pixel frames (BASELINE configs[1]'s deepest level): 16 frames per 256-row tile = a 576-pixel halo patch, the 36-segment
    # instantiations of the v2 kernel (round 6): four-wave / 64-column tiles, and eight-wave / 128-column tiles (more than 128 tiles)
    ("c3x3_4x4_frames_cat_N128", 32, 4, 4, 64, 64, 128, 3, 1, 1, {"bias": True}),
    ("c3x3_4x4_frames_manytiles_N128", 2064, 4, 4, 16, 0, 128, 3, 1, 1, {"bias": True}),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_gemm(hip, ref, case):
    name, F, H, W, C0, C1, N, k, stride, pad, ex = case
    rows = F * H * W
    Ho = (H + 2 * pad - k) // stride + 1
    Wo = (W + 2 * pad - k) // stride + 1
    in0 = rnd(rows, C0, seed=1)
    in1 = rnd(rows, C1, seed=2) if C1 else None
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
    want = ref.conv_gemm(in0, w, N, in1=in1, **kw)
    for variant in FP32_POLICIES:
        hip.conv_policy = variant
        _conv_case(hip, name + f"/v{variant}", in0, in1, w, N, kw, want)
    if k == 3 and C0 % 16 == 0 and C1 % 16 == 0:
        from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
        kw["w_bf3"] = pack_bf3(unpack_kn(w)).cuda()
        for variant in (CP.HALO_V1_NINE, CP.DIRECT_V2_NINE, CP.HALO_V1, CP.DIRECT_V2, CP.DIRECT_V2_K32):   # split-operand bf16 MFMA: 9 / 6 terms, v1 / v2 kernels, v2 on 16x16x32
            hip.conv_policy = variant
            _conv_case(hip, name + f"/v{variant}", in0, in1, w, N, kw, want)
    hip.conv_policy = 0                            # shipped policy (left active)


def _conv_case(hip, name, in0, in1, w, N, kw, want):
    gkw = {k_: (tuple(t.cuda() for t in v) if isinstance(v, tuple) else (v.cuda() if torch.is_tensor(v) else v))
           for k_, v in kw.items()}
    got = hip.conv_gemm(in0.cuda(), w.cuda(), N, in1=None if in1 is None else in1.cuda(), **gkw)
    torch.cuda.synchronize()
    check("conv_gemm/" + name, got, want)


# ---------------------------------------------------------------------------------------------- Winograd F(2x2,3x3) split conv
WINO = CP.WINO                                     # shipped policy + the Winograd form where w_wino is supplied
WINO_CASES = [
    # name, F, H, W, C0, C1, N, extras
    ("L0_64x64_4rows", 3, 64, 64, 64, 0, 64, {"bias": True, "gn": True}),                  # tile = 4 rows: 2 x 32 Winograd tiles
    ("L0_cat_64p64_N64", 2, 64, 64, 64, 64, 64, {"bias": True, "gn": True}),               # two sources (skip concat), 8 chunks
    ("L0_two_chunks", 1, 64, 64, 32, 0, 64, {"bias": True}),                               # the shortest K the kernel takes
    ("odd_chunk_count_falls_back", 1, 64, 64, 48, 0, 64, {"bias": True, "fallback": True}),  # 3 chunks: the direct kernel runs
    ("L1_32x32_N128", 5, 32, 32, 64, 0, 128, {"bias": True, "gn": True}),                  # 8 rows: 4 x 16 tiles, two channel tiles
    ("L1_32x32_res", 3, 32, 32, 32, 0, 64, {"res": True}),
    ("L2_16x16_N256_gn", 7, 16, 16, 128, 0, 256, {"bias": True, "gn": True}),              # one frame per workgroup: 8 x 8 tiles
    ("L2_16x16_cat_N128", 4, 16, 16, 128, 128, 128, {"bias": True, "gn": True}),
    ("L3_8x8_four_frames", 12, 8, 8, 256, 0, 512, {"bias": True, "gn": True}),             # 4 whole frames per workgroup
    ("L3_8x8_cat_deepK", 8, 8, 8, 512, 512, 256, {"bias": True, "gn": True}),
    ("clip_edges_1frame", 1, 64, 64, 32, 0, 64, {"bias": True}),
    ("many_tiles_per_workgroup_L0", 50, 64, 64, 64, 0, 64, {"bias": True, "gn": True}),    # 800 tiles on 256 CUs: the flat (tile, chunk) loop crosses tiles
    ("many_tiles_per_workgroup_L2_N128", 300, 16, 16, 64, 0, 128, {"bias": True, "gn": True}),  # 600 tiles, two channel tiles per pixel tile
    ("many_tiles_per_workgroup_L3_two_chunks", 1200, 8, 8, 32, 0, 64, {"bias": True}),    # 300 x 1 tiles of 4 frames, the shortest K
    ("H_not_square_32x64", 2, 32, 64, 32, 0, 64, {"bias": True, "gn": True}),
]


def _w5_from_packed(w, Cin, N):
    """packed [K/4][N][4] (k = tap*Cin + c) -> Conv3d layout (N, Cin, 1, 3, 3)."""
    from dawn_pytorch_amd.pack import unpack_kn
    return unpack_kn(w).reshape(3, 3, Cin, N).permute(3, 2, 0, 1)[:, :, None].contiguous()


@pytest.mark.parametrize("case", WINO_CASES, ids=[c[0] for c in WINO_CASES])
def test_conv3x3_winograd(hip, ref, case):
    """conv3x3_wino_kernel (Winograd F(2x2,3x3) on the bf16 pipe with exactly split operands) == the torch conv, == the direct
    split kernel to fp32 rounding, bit-deterministic; GroupNorm sums from its epilogue == a statistics pass over its output."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_wino_bf3, unpack_kn
    name, F, H, W, C0, C1, N, ex = case
    rows = F * H * W
    in0 = rnd(rows, C0, seed=1)
    in1 = rnd(rows, C1, seed=2) if C1 else None
    w = packw(9 * (C0 + C1), N, seed=3)
    kw = dict(F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1)
    if ex.get("bias"):
        kw["bias"] = rnd(N, seed=4)
    if ex.get("res"):
        kw["res"] = rnd(rows, N, seed=8)
    want = ref.conv_gemm(in0, w, N, in1=in1, **kw)
    gkw = {k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in kw.items()}
    gkw["w_bf3"] = pack_bf3(unpack_kn(w)).cuda()
    gkw["w_wino"] = pack_wino_bf3(_w5_from_packed(w, C0 + C1, N)).cuda()
    x0g, x1g, wg = in0.cuda(), None if in1 is None else in1.cuda(), w.cuda()
    try:
        outs = []
        for variant in (WINO, CP.DIRECT_V2_K32):
            hip.conv_policy = variant
            part = hip.conv_gn_part(rows, N, x0g) if ex.get("gn") else None
            got = hip.conv_gemm(x0g, wg, N, in1=x1g, gn_part=part, **gkw)
            torch.cuda.synchronize()
            check(f"conv3x3_wino/{name}/v{variant:#x}", got, want)
            outs.append(got)
            if part is not None:
                gamma, beta = rnd(N, seed=14).cuda() * 0.2 + 1, rnd(N, seed=15).cuda() * 0.2
                a1, b1 = hip.gn_coeffs(got, gamma, beta, None, rows, part=part)
                a2, b2 = hip.gn_coeffs(got, gamma, beta, None, rows)
                check(f"conv3x3_wino/{name}/gn_a/v{variant:#x}", a1, a2, 1e-5)
                check(f"conv3x3_wino/{name}/gn_b/v{variant:#x}", b1, b2, 1e-5)
                if variant == WINO and not ex.get("fallback"):
                    # ... and the coefficients the launch finalises itself (gn_fin: last workgroup reduces + finalises, FiLM included),
                    # twice in a row: the ticket word is left zero for the next launch
                    film = (rnd(N, seed=16).cuda() * 0.1, rnd(N, seed=17).cuda() * 0.1)
                    a3, b3 = hip.gn_coeffs(got, gamma, beta, film, 3 * rows)
                    for rep in range(2):
                        part2 = hip.conv_gn_part(rows, N, x0g)
                        got2 = hip.conv_gemm(x0g, wg, N, in1=x1g, gn_part=part2, gn_fin=(gamma, beta, film, 3 * rows), **gkw)
                        assert part2.dawn_ab is not None and torch.equal(got2, got)
                        a4, b4 = hip.gn_coeffs(got2, gamma, beta, film, 3 * rows, part=part2)
                        assert a4 is part2.dawn_ab[0]
                        check(f"conv3x3_wino/{name}/gn_fused_a/{rep}", a4, a3, 1e-5)
                        check(f"conv3x3_wino/{name}/gn_fused_b/{rep}", b4, b3, 1e-5)
        hip.conv_policy = WINO
        again = hip.conv_gemm(x0g, wg, N, in1=x1g, **gkw)
        assert torch.equal(again, outs[0])                                    # fixed summation order
        scale = max(1.0, float(want.abs().max()))
        assert float((outs[0] - outs[1]).abs().max()) <= 2e-5 * scale         # vs the direct split kernel: fp32 rounding only
        assert torch.equal(outs[0], outs[1]) == bool(ex.get("fallback"))     # (the Winograd kernel really ran: different rounding)
    finally:
        hip.conv_policy = 0


def test_conv_wino_gn_handoff_stress(hip):
    """the last-workgroup GroupNorm finalisation relies on write-through atomics + `s_waitcnt vmcnt(0)` instead of a
    release / acquire pair (include/dawn_hip.h states the ISA-level assumption).  A stale partial row read by the last workgroup
    would show up as coefficients that differ from launch to launch (which workgroup is last -- and on which XCD -- varies): both
    reductions run in FIXED order, so on identical inputs the fused coefficients must be bit-identical on every one of many
    back-to-back launches, whatever the last workgroup was, and equal the separate reduce + finalize launch over the same rows
    to fp64-summation rounding.  Grids of 256 workgroups x 2 tiles, 256 x 1 and 16 x 1 (every XCD holds partial rows; short
    launches: many hand-offs per millisecond), 200 launches per shape without a host synchronisation in between."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_wino_bf3, unpack_kn
    try:
        hip.conv_policy = WINO
        for (F, H, W, Cc, N) in ((64, 32, 32, 32, 128), (32, 16, 16, 32, 512), (8, 8, 8, 64, 512)):
            rows = F * H * W
            x, w = rnd(rows, Cc, seed=21).cuda(), packw(9 * Cc, N, seed=22)
            kw = dict(F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1, w_bf3=pack_bf3(unpack_kn(w)).cuda(),
                      w_wino=pack_wino_bf3(_w5_from_packed(w, Cc, N)).cuda())
            wg = w.cuda()
            gamma, beta = rnd(N, seed=14).cuda() * 0.2 + 1, rnd(N, seed=15).cuda() * 0.2
            film = (rnd(N, seed=16).cuda() * 0.1, rnd(N, seed=17).cuda() * 0.1)
            hip.begin_evaluation(x)
            res = []
            for rep in range(200):
                part = hip.conv_gn_part(rows, N, x)
                out = hip.conv_gemm(x, wg, N, gn_part=part, gn_fin=(gamma, beta, film, rows), **kw)
                assert part.dawn_ab is not None, "the launch did not finalise the coefficients itself"
                res.append(part.dawn_ab)
            torch.cuda.synchronize()
            a0, b0 = res[0]
            for a, b in res[1:]:
                assert torch.equal(a, a0) and torch.equal(b, b0), (F, H, W, Cc, N)
            part = hip.conv_gn_part(rows, N, x)
            out = hip.conv_gemm(x, wg, N, gn_part=part, **kw)
            a1, b1 = hip.gn_coeffs(out, gamma, beta, film, rows, part=part)          # separate reduce + finalize over the same rows
            check(f"wino_gn_handoff/{F}x{H}x{W}x{Cc}->{N}/a", a0, a1, 1e-6)
            check(f"wino_gn_handoff/{F}x{H}x{W}x{Cc}->{N}/b", b0, b1, 1e-6)
    finally:
        hip.conv_policy = 0


def test_conv_wino_is_fp32_accurate(hip, ref):
    """Against an fp64 convolution the Winograd split kernel's error is that of an fp32 Winograd F(2x2,3x3): within 3x the direct
    split kernel's on N(0,1) data with entries spread over 10 decades (the transform adds values of different magnitude in fp32,
    which the direct form never does -- that, not the bf16 pipe, is what the factor pays for)."""
    import torch.nn.functional as F_
    from dawn_pytorch_amd.pack import pack_bf3, pack_wino_bf3, unpack_kn
    F, H, W, Cc, N = 4, 32, 32, 128, 128
    rows = F * H * W
    errs = {}
    for tag, spread in (("n01", False), ("spread", True)):
        x, w = rnd(rows, Cc, seed=1), packw(9 * Cc, N, seed=2)
        if spread:
            x[::7, ::5] *= 1.0e4
            x[::11, ::3] *= 1.0e-6
        wkn = unpack_kn(w).double()
        w4 = wkn.reshape(3, 3, Cc, N).permute(3, 2, 0, 1)
        want = F_.conv2d(x.double().reshape(F, H, W, Cc).permute(0, 3, 1, 2), w4, padding=1).permute(0, 2, 3, 1).reshape(rows, N)
        ws, ww = pack_bf3(unpack_kn(w)).cuda(), pack_wino_bf3(_w5_from_packed(w, Cc, N)).cuda()
        for variant in (CP.EXACT_FP32, CP.DIRECT_V2_K32, WINO):
            hip.conv_policy = variant
            got = hip.conv_gemm(x.cuda(), w.cuda(), N, F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1, w_bf3=ws, w_wino=ww)
            torch.cuda.synchronize()
            errs[(tag, variant)] = float((got.cpu().double() - want).abs().max() / want.abs().max())
    hip.conv_policy = 0
    with open(LOG, "a") as f:
        f.write(json.dumps({"op": "conv_wino/rel_err_vs_fp64", **{f"{t}/{v:#x}": e for (t, v), e in errs.items()}}) + "\n")
    for tag in ("n01", "spread"):
        assert errs[(tag, WINO)] <= 3.0 * errs[(tag, CP.DIRECT_V2_K32)] + 1e-7, errs



# ---------------------------------------------------------------------------------------------- Winograd F(4x4,3x3) split conv (opt-in)
WINO4 = CP.WINO4_EVERYWHERE                    # the F(4x4) form wherever its geometry fits (CP.WINO4 alone: only the shapes it wins on)
WINO4_CASES = [
    # name, F, H, W, C0, C1, N, extras
    ("L0_64x64", 3, 64, 64, 64, 0, 64, {"bias": True, "gn": True}),                         # tile = 4 rows x 64 columns: 1 x 16 Winograd tiles
    ("L0_cat_64p64", 2, 64, 64, 64, 64, 64, {"bias": True, "gn": True}),                    # two sources (skip concat), 8 chunks
    ("L0_two_chunks_res", 1, 64, 64, 32, 0, 64, {"res": True}),                             # the shortest K; residual epilogue
    ("L1_32x32_N128", 5, 32, 32, 64, 0, 128, {"bias": True, "gn": True}),                   # tile = 8 rows x 32 columns: 2 x 8 tiles, two channel tiles
    ("L1_32x32_K1152", 3, 32, 32, 128, 0, 128, {"bias": True, "gn": True}),
    ("many_tiles_L0", 50, 64, 64, 64, 0, 64, {"bias": True, "gn": True}),                   # 800 tiles on 256 CUs: the flat loop crosses tiles
    ("many_tiles_L1_N128", 80, 32, 32, 32, 0, 128, {"bias": True, "gn": True}),             # 640 tiles, n0 alternates between the workgroups
    ("H_not_square_32x64", 2, 32, 64, 32, 0, 64, {"bias": True, "gn": True}),
    ("H_128_W_32", 1, 128, 32, 32, 0, 64, {"bias": True}),
]


@pytest.mark.parametrize("case", WINO4_CASES, ids=[c[0] for c in WINO4_CASES])
def test_conv3x3_winograd4(hip, ref, case):
    """conv3x3_wino4_kernel (Winograd F(4x4,3x3) on the points 0, +-3/4, +-3/2, inf; bf16 pipe with exactly split operands) == the torch
    conv to fp32-Winograd rounding, bit-deterministic, GroupNorm sums / fused coefficients == a statistics pass over its output, and
    it really ran (its rounding differs from the F(2x2) kernel's)."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_wino_bf3, pack_wino4_bf3, unpack_kn
    name, F, H, W, C0, C1, N, ex = case
    rows = F * H * W
    assert hip.L.dawn_conv3x3_wino4_ok(F, H, W, C0, C1, N) == 1
    in0 = rnd(rows, C0, seed=1)
    in1 = rnd(rows, C1, seed=2) if C1 else None
    w = packw(9 * (C0 + C1), N, seed=3)
    kw = dict(F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1)
    if ex.get("bias"):
        kw["bias"] = rnd(N, seed=4)
    if ex.get("res"):
        kw["res"] = rnd(rows, N, seed=8)
    want = ref.conv_gemm(in0, w, N, in1=in1, **kw)
    gkw = {k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in kw.items()}
    w5 = _w5_from_packed(w, C0 + C1, N)
    gkw.update(w_bf3=pack_bf3(unpack_kn(w)).cuda(), w_wino=pack_wino_bf3(w5).cuda(), w_wino4=pack_wino4_bf3(w5).cuda())
    x0g, x1g, wg = in0.cuda(), None if in1 is None else in1.cuda(), w.cuda()
    try:
        hip.begin_evaluation(x0g)
        outs = {}
        for variant in (WINO4, WINO):
            hip.conv_policy = variant
            part = hip.conv_gn_part(rows, N, x0g) if ex.get("gn") else None
            got = hip.conv_gemm(x0g, wg, N, in1=x1g, gn_part=part, **gkw)
            torch.cuda.synchronize()
            check(f"conv3x3_wino4/{name}/v{variant:#x}", got, want)
            outs[variant] = got
            if part is not None and variant == WINO4:
                gamma, beta = rnd(N, seed=14).cuda() * 0.2 + 1, rnd(N, seed=15).cuda() * 0.2
                a1, b1 = hip.gn_coeffs(got, gamma, beta, None, rows, part=part)
                a2, b2 = hip.gn_coeffs(got, gamma, beta, None, rows)
                check(f"conv3x3_wino4/{name}/gn_a", a1, a2, 1e-5)
                check(f"conv3x3_wino4/{name}/gn_b", b1, b2, 1e-5)
                film = (rnd(N, seed=16).cuda() * 0.1, rnd(N, seed=17).cuda() * 0.1)
                a3, b3 = hip.gn_coeffs(got, gamma, beta, film, 3 * rows)
                for rep in range(2):
                    part2 = hip.conv_gn_part(rows, N, x0g)
                    got2 = hip.conv_gemm(x0g, wg, N, in1=x1g, gn_part=part2, gn_fin=(gamma, beta, film, 3 * rows), **gkw)
                    assert part2.dawn_ab is not None and torch.equal(got2, got)
                    check(f"conv3x3_wino4/{name}/gn_fused_a/{rep}", part2.dawn_ab[0], a3, 1e-5)
                    check(f"conv3x3_wino4/{name}/gn_fused_b/{rep}", part2.dawn_ab[1], b3, 1e-5)
        scale = max(1.0, float(want.abs().max()))
        assert float((outs[WINO4] - outs[WINO]).abs().max()) <= 5e-5 * scale
        assert not torch.equal(outs[WINO4], outs[WINO])                       # (the F(4x4) kernel really ran: different rounding)
    finally:
        hip.conv_policy = 0


REV_CASES = [WINO_CASES[i] for i in (0, 1, 4, 6, 8, 11, 12, 13)] + [("F4:" + c[0],) + c[1:] for c in (WINO4_CASES[0], WINO4_CASES[1], WINO4_CASES[3], WINO4_CASES[5], WINO4_CASES[6])]


@pytest.mark.parametrize("case", REV_CASES, ids=[c[0] for c in REV_CASES])
def test_conv_wino_reverse_tile_order(hip, case):
    """ConvPolicy.WINO_REVERSE: both Winograd kernels walk their tiles back to front (last frame first).  A tile's arithmetic does not depend
    on the order: the outputs must be BIT-identical to the front-to-back launch; the GroupNorm partial sums of a workgroup add the
    same tiles in the opposite order (fp64): fused coefficients equal to summation rounding."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_wino_bf3, pack_wino4_bf3, unpack_kn
    name, F, H, W, C0, C1, N, ex = case
    f4 = name.startswith("F4:")
    rows = F * H * W
    in0 = rnd(rows, C0, seed=1).cuda()
    in1 = rnd(rows, C1, seed=2).cuda() if C1 else None
    w = packw(9 * (C0 + C1), N, seed=3)
    w5 = _w5_from_packed(w, C0 + C1, N)
    kw = dict(F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1, bias=rnd(N, seed=4).cuda(), w_bf3=pack_bf3(unpack_kn(w)).cuda(), w_wino=pack_wino_bf3(w5).cuda())
    if f4:
        kw["w_wino4"] = pack_wino4_bf3(w5).cuda()
    gamma, beta = rnd(N, seed=14).cuda() * 0.2 + 1, rnd(N, seed=15).cuda() * 0.2
    base = WINO4 if f4 else WINO
    try:
        hip.begin_evaluation(in0)
        res = []
        for pol in (base, base | CP.WINO_REVERSE):
            hip.conv_policy = pol
            part = hip.conv_gn_part(rows, N, in0)
            got = hip.conv_gemm(in0, w.cuda(), N, in1=in1, gn_part=part, gn_fin=(gamma, beta, None, rows), **kw)
            torch.cuda.synchronize()
            assert part.dawn_ab is not None
            res.append((got, part.dawn_ab[0].clone(), part.dawn_ab[1].clone()))
        assert torch.equal(res[0][0], res[1][0])
        check(f"conv_wino_reverse/{name}/gn_a", res[1][1], res[0][1], 1e-6)
        check(f"conv_wino_reverse/{name}/gn_b", res[1][2], res[0][2], 1e-6)
    finally:
        hip.conv_policy = 0


def test_conv_wino4_is_fp32_accurate(hip, ref):
    """VERDICT r4 #1b's gate: against an fp64 convolution the F(4x4,3x3) kernel's error stays within 5x the exact-fp32-MFMA kernel's
    (ConvPolicy.EXACT_FP32) on N(0,1) data and on data spread over 10 decades (measured ~2x: the points 0, +-3/4, +-3/2 -- tools/wino4_points.py)."""
    import torch.nn.functional as F_
    from dawn_pytorch_amd.pack import pack_bf3, pack_wino_bf3, pack_wino4_bf3, unpack_kn
    F, H, W, Cc, N = 4, 32, 32, 128, 128
    rows = F * H * W
    errs = {}
    for tag, spread in (("n01", False), ("spread", True)):
        x, w = rnd(rows, Cc, seed=1), packw(9 * Cc, N, seed=2)
        if spread:
            x[::7, ::5] *= 1.0e4
            x[::11, ::3] *= 1.0e-6
        w4 = unpack_kn(w).double().reshape(3, 3, Cc, N).permute(3, 2, 0, 1)
        want = F_.conv2d(x.double().reshape(F, H, W, Cc).permute(0, 3, 1, 2), w4, padding=1).permute(0, 2, 3, 1).reshape(rows, N)
        w5 = _w5_from_packed(w, Cc, N)
        ws, ww, ww4 = pack_bf3(unpack_kn(w)).cuda(), pack_wino_bf3(w5).cuda(), pack_wino4_bf3(w5).cuda()
        for variant in (CP.EXACT_FP32, CP.DIRECT_V2_K32, WINO, WINO4):
            hip.conv_policy = variant
            got = hip.conv_gemm(x.cuda(), w.cuda(), N, F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1, w_bf3=ws, w_wino=ww, w_wino4=ww4)
            torch.cuda.synchronize()
            errs[(tag, variant)] = float((got.cpu().double() - want).abs().max() / want.abs().max())
    hip.conv_policy = 0
    with open(LOG, "a") as f:
        f.write(json.dumps({"op": "conv_wino4/rel_err_vs_fp64", **{f"{t}/{v:#x}": e for (t, v), e in errs.items()}}) + "\n")
    for tag in ("n01", "spread"):
        assert errs[(tag, WINO4)] <= 5.0 * errs[(tag, CP.EXACT_FP32)] + 1e-7, errs


@pytest.mark.parametrize("F,H,W,C0,N", [(3, 16, 16, 64, 64), (2, 8, 8, 128, 256), (5, 8, 8, 16, 16), (1, 40, 37, 32, 128),
                                       (12, 8, 8, 16, 32), (12, 4, 4, 64, 32), (12, 8, 8, 48, 16), (48, 4, 4, 32, 64)])
def test_conv_gemm_fused_gn_stats(hip, ref, F, H, W, C0, N):
    """GroupNorm partial sums emitted by the conv epilogue == statistics pass over the conv output."""
    rows = F * H * W
    x, w, b = rnd(rows, C0, seed=1), packw(9 * C0, N, seed=2), rnd(N, seed=3)
    gamma, beta = rnd(N, seed=4) * 0.2 + 1, rnd(N, seed=5) * 0.2
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    ws = pack_bf3(unpack_kn(w)).cuda() if C0 % 16 == 0 else None
    for variant in (CP.BK32 | CP.XCD_ORDER, CP.FP32_TILES | CP.GLDS_TILE256, CP.FP32_TILES, CP.EXACT_FP32, CP.HALO_V1, CP.DIRECT_V2,
                    CP.DIRECT_V2_K32):
        hip.conv_policy = variant
        xg = x.cuda()
        part = hip.conv_gn_part(rows, N, xg)
        c = hip.conv_gemm(xg, w.cuda(), N, F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1, bias=b.cuda(), gn_part=part, w_bf3=ws)
        a1, b1 = hip.gn_coeffs(c, gamma.cuda(), beta.cuda(), None, rows, part=part)
        a2, b2 = hip.gn_coeffs(c, gamma.cuda(), beta.cuda(), None, rows)
        check(f"conv_gn_stats/a_{C0}_{N}_v{variant}", a1, a2, 1e-5)
        check(f"conv_gn_stats/b_{C0}_{N}_v{variant}", b1, b2, 1e-5)


def test_conv_bf16_split_is_fp32_accurate(hip, ref):
    """The split-operand bf16-MFMA 3x3 path is an fp32 computation: against an fp64 reference its error is
    no larger than the fp32-MFMA path's (both are dominated by fp32 accumulation rounding)."""
    import torch.nn.functional as F_
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    F, H, W, Cc, N = 4, 32, 32, 128, 128
    rows = F * H * W
    x, w = rnd(rows, Cc, seed=1), packw(9 * Cc, N, seed=2)
    # a few large-magnitude and tiny entries: the split must stay exact across the exponent range
    x[::7, ::5] *= 1.0e4
    x[::11, ::3] *= 1.0e-6
    wkn = unpack_kn(w).double()                                              # (9*Cc, N), k = tap*Cc + c
    w4 = wkn.reshape(3, 3, Cc, N).permute(3, 2, 0, 1)
    want = F_.conv2d(x.double().reshape(F, H, W, Cc).permute(0, 3, 1, 2), w4, padding=1).permute(0, 2, 3, 1).reshape(rows, N)
    errs = {}
    FP32, V1, V1_NINE, V2, K32 = CP.EXACT_FP32, CP.HALO_V1, CP.HALO_V1_NINE, CP.DIRECT_V2, CP.DIRECT_V2_K32
    for variant, ws in ((FP32, None), (V1, pack_bf3(unpack_kn(w)).cuda()), (V1_NINE, pack_bf3(unpack_kn(w)).cuda()),
                        (V2, pack_bf3(unpack_kn(w)).cuda()), (K32, pack_bf3(unpack_kn(w)).cuda())):
        hip.conv_policy = variant
        got = hip.conv_gemm(x.cuda(), w.cuda(), N, F=F, Hi=H, Wi=W, KH=3, KW=3, pad=1, w_bf3=ws)
        torch.cuda.synchronize()
        errs[variant] = float((got.cpu().double() - want).abs().max() / want.abs().max())
    with open(LOG, "a") as f:
        f.write(json.dumps({"op": "conv_bf16_split/rel_err_vs_fp64", "fp32_mfma": errs[FP32], "bf16x6": errs[V1],
                            "bf16x9": errs[V1_NINE], "bf16x6_v2": errs[V2], "bf16x6_v2_16x16x32": errs[K32]}) + "\n")
    hip.conv_policy = 0
    assert errs[V1] <= 2.0 * errs[FP32] + 1e-7, errs
    assert errs[V2] <= 2.0 * errs[FP32] + 1e-7, errs
    assert errs[K32] <= 2.0 * errs[FP32] + 1e-7, errs
    assert errs[V1_NINE] <= 2.0 * errs[FP32] + 1e-7, errs


@pytest.mark.parametrize("M,K,N,res,bias", [(51200, 128, 768, False, False), (51200, 256, 128, True, True),
                                            (102400, 64, 256, True, False), (51200, 512, 384, False, True)])
def test_gemm1x1_split(hip, ref, M, K, N, res, bias):
    """Large prologue-free 1x1 GEMMs on the bf16 pipe with exactly split operands == fp32 GEMM."""
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    x, w = rnd(M, K, seed=1), packw(K, N, seed=2)
    kw = dict(F=M // 64, Hi=8, Wi=8)
    if res:
        kw["res"] = rnd(M, N, seed=3)
    if bias:
        kw["bias"] = rnd(N, seed=4)
    want = ref.conv_gemm(x, w, N, **kw)
    gkw = {k_: (v.cuda() if torch.is_tensor(v) else v) for k_, v in kw.items()}
    for variant in (CP.DIRECT_V2, CP.DIRECT_V2_NINE, CP.DIRECT_V2_TILE128):   # shipped policy, 9 cross terms, 128 x 64 tiles (2 WG / CU)
        hip.conv_policy = variant
        got = hip.conv_gemm(x.cuda(), w.cuda(), N, w_bf3=pack_bf3(unpack_kn(w)).cuda(), **gkw)
        torch.cuda.synchronize()
        check(f"gemm1x1_split/M{M}_K{K}_N{N}/v{variant}", got, want)
    hip.conv_policy = 0


@pytest.mark.parametrize("M,C0,C1,N", [(51200, 128, 0, 768), (25600, 64, 64, 192), (204800, 64, 0, 128), (12800, 32, 32, 64),
                                       (25600, 128, 128, 192), (12800, 512, 0, 128), (51200, 256, 0, 64), (12800, 512, 512, 192)])
def test_gemm1x1_layernorm_inside(hip, ref, M, C0, C1, N):
    """Row-stationary / row-accumulator split GEMMs with the LayerNorm of their input rows computed in the kernel (ln_eps) ==
    LayerNorm statistics pass + projection; shapes those kernels do not serve are refused, not silently computed otherwise."""
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    from dawn_pytorch_amd._lib import DawnHipError
    w = packw(C0 + C1, N, seed=2)
    x0 = rnd(M, C0, seed=1) * 1.7 + 0.4
    x1 = rnd(M, C1, seed=5) * 0.6 if C1 else None
    kw = dict(F=M // 64, Hi=8, Wi=8)
    want = ref.conv_gemm(x0, w, N, in1=x1, row_stats=ref.ln_rowstats(x0, x1), **kw)
    assert hip.ln_inline_ok(M, N, C0, C1)
    got = hip.conv_gemm(x0.cuda(), w.cuda(), N, in1=None if x1 is None else x1.cuda(), ln_eps=1e-5,
                        w_bf3=pack_bf3(unpack_kn(w)).cuda(), **kw)
    check(f"gemm1x1_ln_inside/M{M}_C{C0}+{C1}_N{N}", got, want)
    assert not hip.ln_inline_ok(M, N, 320, 0)            # neither <= 128 channels nor a multiple of 128
    with pytest.raises(DawnHipError):
        w2 = packw(320, N, seed=3)
        hip.conv_gemm(torch.zeros(M, 320, device="cuda"), w2.cuda(), N, ln_eps=1e-5, w_bf3=pack_bf3(unpack_kn(w2)).cuda(), **kw)


@pytest.mark.parametrize("M,C0,C1,N,extra", [(51200, 64, 64, 64, "tr"), (12800, 512, 512, 256, "tr"), (25600, 128, 0, 192, ""),
                                             (12800, 512, 0, 768, "res"), (51200, 64, 0, 128, "strided"),
                                             (12800, 64, 0, 512, "strided"), (204800, 32, 96, 64, "bias"),
                                             (51200, 128, 0, 768, "rowstats"), (25600, 128, 128, 192, "rowstats"),
                                             (12800, 512, 0, 768, "rowstats"), (25600, 256, 256, 128, "res"),
                                             (12800, 512, 512, 64, "tr"), (12800, 1024, 0, 192, "rowstats"), (51200, 192, 64, 192, "bias"),
                                             # the tile kernel's stage loop at its corners (round 6: stages in pairs, fetches clamped past the end of K):
                                             # one stage, three stages, nine stages with the source switch at an odd stage, a switch after stage 0
                                             (12800, 32, 0, 64, "bias"), (12800, 96, 0, 128, "rowstats"), (25600, 160, 128, 256, "res"),
                                             (12800, 32, 64, 128, "rowstats"), (6400, 96, 0, 256, "tr")])
def test_gemm1x1_split_variants(hip, ref, M, C0, C1, N, extra):
    """The same kernel family beyond the plain case: 64-column tiles (N = 64 / 192), two channel-concatenated sources
    (res_conv / to_q of cat[x, skip]), the res_conv epilogue out += SiLU(c2*a+b), M down to 12800 rows, and strided
    input / output views (to_out: a 64-column slice of q -> a Co-column slice of y3)."""
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    K = C0 + C1
    w = packw(K, N, seed=2)
    kw = dict(F=M // 64, Hi=8, Wi=8)
    x0 = rnd(M, C0, seed=1)
    x1 = rnd(M, C1, seed=5) if C1 else None
    if "tr" in extra:
        kw["tr"] = (rnd(M, N, seed=6), rnd(N, seed=7), rnd(N, seed=8))
        kw["bias"] = rnd(N, seed=4)
    if "res" in extra:
        kw["res"] = rnd(M, N, seed=3)
    if "bias" in extra:
        kw["bias"] = rnd(N, seed=4)
    if "rowstats" in extra:            # LayerNorm prologue: (x - mean[row]) * rstd[row] applied in the loader
        x0 = x0 * 1.7 + 0.4
        kw["row_stats"] = ref.ln_rowstats(x0, x1)
    want = ref.conv_gemm(x0, w, N, in1=x1, **kw)
    if "rowstats" in extra:            # == the GEMM on materialised normalised rows, bit for bit on the GPU path
        xn = hip.ln_rows(x0.cuda(), None if x1 is None else x1.cuda())
        via_rows = hip.conv_gemm(xn, w.cuda(), N, w_bf3=pack_bf3(unpack_kn(w)).cuda(), F=M // 64, Hi=8, Wi=8)
    gkw = {k_: (tuple(t.cuda() for t in v) if isinstance(v, tuple) else v.cuda() if torch.is_tensor(v) else v) for k_, v in kw.items()}
    x0g = x0.cuda()
    out = None
    if extra == "strided":
        wide = torch.zeros(M, C0 + 128, device="cuda")
        wide[:, 64:64 + C0] = x0g
        x0g = wide[:, 64:64 + C0]
        big = torch.full((M, 3 * N), 7.0, device="cuda")
        out = big[:, N:2 * N]
    got = hip.conv_gemm(x0g, w.cuda(), N, in1=None if x1 is None else x1.cuda(), w_bf3=pack_bf3(unpack_kn(w)).cuda(), out=out, **gkw)
    torch.cuda.synchronize()
    check(f"gemm1x1_split_variants/M{M}_C{C0}+{C1}_N{N}_{extra}", got, want)
    hip.conv_policy = CP.DIRECT_V2_TILE128                    # the 128 x 64-tile configuration of the same kernel
    got_small = hip.conv_gemm(x0g, w.cuda(), N, in1=None if x1 is None else x1.cuda(), w_bf3=pack_bf3(unpack_kn(w)).cuda(),
                              out=None if out is None else torch.empty_like(out), **gkw)
    hip.conv_policy = 0
    check(f"gemm1x1_split_variants_128x64/M{M}_C{C0}+{C1}_N{N}_{extra}", got_small, want)
    if "rowstats" in extra:            # with the statistics of the HIP LayerNorm kernel itself (the product's pairing)
        st = hip.ln_rowstats(x0.cuda(), None if x1 is None else x1.cuda())
        got_hs = hip.conv_gemm(x0.cuda(), w.cuda(), N, in1=None if x1 is None else x1.cuda(), row_stats=st,
                               w_bf3=pack_bf3(unpack_kn(w)).cuda(), F=M // 64, Hi=8, Wi=8)
        assert torch.equal(got_hs, via_rows)
    if out is not None:
        assert float(big[:, :N].min()) == 7.0 and float(big[:, 2 * N:].max()) == 7.0       # neighbours untouched
    # and it is the split kernel's accuracy class: no worse than the fp32 MFMA path against fp64
    hip.conv_policy = CP.EXACT_FP32
    got32 = hip.conv_gemm(x0.cuda(), w.cuda(), N, in1=None if x1 is None else x1.cuda(), **gkw)
    hip.conv_policy = 0
    e_split, e_f32 = float((got.cpu() - want).abs().max()), float((got32.cpu() - want).abs().max())
    assert e_split <= 2.0 * e_f32 + 1e-5 * max(1.0, float(want.abs().max())), (e_split, e_f32)


def test_conv_gemm_transposed(hip, ref):
    from dawn_pytorch_amd.pack import pack_kn, deconv_w_kn_phases
    F, H, W, Cc = 3, 8, 8, 64
    w5 = rnd(Cc, Cc, 1, 4, 4, seed=1, scale=(Cc * 4) ** -0.5)
    ph = deconv_w_kn_phases(w5)
    wp = torch.stack([pack_kn(ph[i]) for i in range(4)], 0)
    x = rnd(F * H * W, Cc, seed=2)
    b = rnd(Cc, seed=3)
    want = torch.nn.functional.conv_transpose2d(x.reshape(F, H, W, Cc).permute(0, 3, 1, 2), w5[:, :, 0], b, stride=2,
                                                padding=1).permute(0, 2, 3, 1).reshape(-1, Cc)
    r = ref.conv_gemm(x, wp, Cc, F=F, Hi=H, Wi=W, Ho=2 * H, Wo=2 * W, KH=2, KW=2, mode=1, bias=b)
    torch.testing.assert_close(r, want, atol=1e-5, rtol=1e-5)       # phase packing itself
    got = hip.conv_gemm(x.cuda(), wp.cuda(), Cc, F=F, Hi=H, Wi=W, Ho=2 * H, Wo=2 * W, KH=2, KW=2, mode=1, bias=b.cuda())
    check("conv_gemm/transposed_up", got, want)


@pytest.mark.parametrize("F,H,W,Cc", [(50, 32, 32, 64), (200, 16, 16, 128), (13, 64, 64, 64), (200, 16, 16, 256)])
def test_conv_resample_on_split_pipeline(hip, ref, F, H, W, Cc):
    """Downsample (4x4 / stride 2 / pad 1) and Upsample (transposed 4x4 / stride 2 / pad 1) with the exact bf16 split of their
    weights supplied run as implicit GEMMs on the row-accumulator split kernel == torch's own convolutions (and == the fp32
    implicit-GEMM kernel to its accuracy class)."""
    from dawn_pytorch_amd.pack import pack_kn, pack_bf3, conv_w_kn, deconv_w_kn_phases
    x, b = rnd(F * H * W, Cc, seed=2), rnd(Cc, seed=3)
    img = x.reshape(F, H, W, Cc).permute(0, 3, 1, 2)
    # down
    w5 = rnd(Cc, Cc, 1, 4, 4, seed=1, scale=(Cc * 16) ** -0.5)
    wkn = conv_w_kn(w5)
    want = torch.nn.functional.conv2d(img, w5[:, :, 0], b, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, Cc)
    kw = dict(F=F, Hi=H, Wi=W, Ho=H // 2, Wo=W // 2, KH=4, KW=4, stride=2, pad=1, bias=b.cuda())
    got = hip.conv_gemm(x.cuda(), pack_kn(wkn).cuda(), Cc, w_bf3=pack_bf3(wkn).cuda(), **kw)
    g32 = hip.conv_gemm(x.cuda(), pack_kn(wkn).cuda(), Cc, **kw)
    check(f"conv_resample_split/down_F{F}_{H}x{W}_C{Cc}", got, want)
    # (one accumulator chain over K = 16 Cin products: the rounding error grows with sqrt(K); allowance relative to the output scale)
    assert float((got.cpu() - want).abs().max()) <= 2.0 * float((g32.cpu() - want).abs().max()) + 3e-6 * float(want.abs().max())
    # up
    w5t = rnd(Cc, Cc, 1, 4, 4, seed=4, scale=(Cc * 4) ** -0.5)
    ph = deconv_w_kn_phases(w5t)
    wantu = torch.nn.functional.conv_transpose2d(img, w5t[:, :, 0], b, stride=2, padding=1).permute(0, 2, 3, 1).reshape(-1, Cc)
    kwu = dict(F=F, Hi=H, Wi=W, Ho=2 * H, Wo=2 * W, KH=2, KW=2, mode=1, bias=b.cuda())
    wp = torch.stack([pack_kn(ph[i]) for i in range(4)], 0).cuda()
    gotu = hip.conv_gemm(x.cuda(), wp, Cc, w_bf3=torch.stack([pack_bf3(ph[i]) for i in range(4)], 0).cuda(), **kwu)
    g32u = hip.conv_gemm(x.cuda(), wp, Cc, **kwu)
    check(f"conv_resample_split/up_F{F}_{H}x{W}_C{Cc}", gotu, wantu)
    assert float((gotu.cpu() - wantu).abs().max()) <= 2.0 * float((g32u.cpu() - wantu).abs().max()) + 3e-6 * float(wantu.abs().max())


def test_conv_gemm_strided_views(hip, ref):
    """channel slices as input (xattn to_out reads q[:, 64b:64b+64]) and output (y3[:, b*Co:(b+1)*Co])."""
    rows, Co = 200, 128
    q = rnd(rows, 192, seed=1)
    y3 = torch.zeros(rows, 3 * Co)
    y3g = torch.zeros(rows, 3 * Co).cuda()
    qg = q.cuda()
    for b in range(3):
        w = packw(64, Co, seed=10 + b)
        ref.conv_gemm(q[:, 64 * b:64 * b + 64], w, Co, F=rows, Hi=1, Wi=1, out=y3[:, b * Co:(b + 1) * Co])
        hip.conv_gemm(qg[:, 64 * b:64 * b + 64], w.cuda(), Co, F=rows, Hi=1, Wi=1, out=y3g[:, b * Co:(b + 1) * Co])
    check("conv_gemm/strided_views", y3g, y3)


# ---------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("C,rows,film", [(16, 12 * 64, True), (64, 3000, True), (128, 777, False), (512, 16 * 5, True)])
def test_gn_coeffs_and_apply(hip, ref, C, rows, film):
    x = rnd(rows, C, seed=1) * 2 + 0.5
    gamma, beta = rnd(C, seed=2) * 0.2 + 1, rnd(C, seed=3) * 0.2
    fl = (rnd(C, seed=4) * 0.3, rnd(C, seed=5) * 0.3) if film else None
    wa, wb = ref.gn_coeffs(x, gamma, beta, fl, rows)
    ga, gb = hip.gn_coeffs(x.cuda(), gamma.cuda(), beta.cuda(), None if fl is None else tuple(t.cuda() for t in fl), rows)
    check(f"gn_coeffs/a_C{C}", ga, wa, 2e-5)
    check(f"gn_coeffs/b_C{C}", gb, wb, 2e-5)
    # against torch's own GroupNorm on the 5-D view
    y = torch.nn.functional.group_norm(x.t().reshape(1, C, rows, 1, 1), 8, gamma, beta, eps=1e-5)[0, :, :, 0, 0].t()
    if fl is not None:
        y = y * (fl[0] + 1) + fl[1]
    res = rnd(rows, C, seed=6)
    want = torch.nn.functional.silu(y) + res
    got = hip.gn_apply_res(x.cuda(), ga, gb, res.cuda())
    check(f"gn_apply_res/C{C}", got, want, 2e-5)


@pytest.mark.parametrize("C0,C1,rows", [(16, 0, 700), (64, 0, 4097), (64, 64, 300), (512, 512, 130), (256, 0, 64)])
def test_ln_rowstats(hip, ref, C0, C1, rows):
    a = rnd(rows, C0, seed=1) * 1.5 + 0.3
    b = rnd(rows, C1, seed=2) if C1 else None
    wm, wr = ref.ln_rowstats(a, b)
    gm, gr = hip.ln_rowstats(a.cuda(), None if b is None else b.cuda())
    check(f"ln_rowstats/mean_{C0}_{C1}", gm, wm, 1e-5)
    check(f"ln_rowstats/rstd_{C0}_{C1}", gr, wr, 1e-5)
    check(f"ln_rows/{C0}_{C1}", hip.ln_rows(a.cuda(), None if b is None else b.cuda()), ref.ln_rows(a, b), 1e-5)


# ---------------------------------------------------------------------------------------------- cross attention
def test_xattn_pieces(hip, ref):
    Fn, HW, Co = 7, 12, 96
    rows = Fn * HW
    kvtab_w, nulltab_w = torch.zeros(Fn, 3, 128), torch.zeros(3, 16)
    kvtab_g, nulltab_g = torch.zeros(Fn, 3, 128).cuda(), torch.zeros(3, 16).cuda()
    for b in range(3):
        kv, ks, nk = rnd(Fn, 128, seed=b), rnd(8, seed=10 + b) * 0.2 + 1, rnd(2, 8, seed=20 + b)
        ref.xattn_prep(kv, ks, nk, kvtab_w, b, nulltab_w)
        hip.xattn_prep(kv.cuda(), ks.cuda(), nk.cuda(), kvtab_g, b, nulltab_g)
    check("xattn_prep/kvtab", kvtab_g, kvtab_w, 1e-5)
    check("xattn_prep/nulltab", nulltab_g, nulltab_w, 1e-5)
    q = rnd(rows, 192, seed=3)
    qs = rnd(3, 8, seed=4) * 0.2 + 1
    want = ref.xattn_core(q.clone(), HW, kvtab_w, nulltab_w, qs)
    got = hip.xattn_core(q.cuda(), HW, kvtab_g, nulltab_g, qs.cuda())
    check("xattn_core", got, want, 1e-5)
    for Co in (16, 64, 96, 128, 512):
        y3, g3 = rnd(rows, 3 * Co, seed=5), rnd(3, Co, seed=6) * 0.2 + 1
        check(f"xattn_ln_sum/Co{Co}", hip.xattn_ln_sum(y3.cuda(), g3.cuda(), Co), ref.xattn_ln_sum(y3, g3, Co), 2e-5)


@pytest.mark.parametrize("Co", [64, 128, 512])
def test_xattn_tables(hip, ref, Co):
    Fn = 7
    wo = [packw(64, Co, seed=10 + b) for b in range(3)]
    qs = rnd(3, 8, seed=5) * 0.2 + 1
    kvtab, nulltab = torch.zeros(Fn, 3, 128), torch.zeros(3, 16)
    for b in range(3):
        ref.xattn_prep(rnd(Fn, 128, seed=20 + b), rnd(8, seed=30 + b) * 0.2 + 1, rnd(2, 8, seed=40 + b), kvtab, b, nulltab)
    got = hip.xattn_tables(kvtab.cuda(), nulltab.cuda(), qs.cuda(), [w.cuda() for w in wo], Co)
    check(f"xattn_tables/Co{Co}", got, ref.xattn_tables(kvtab, nulltab, qs, wo, Co), 2e-6)


@pytest.mark.parametrize("C0,C1,Fn,HW", [(64, 0, 5, 64), (64, 64, 3, 96), (128, 0, 2, 32), (64, 0, 2, 4096), (64, 64, 2, 1024)])
def test_xattn_layer_c64(hip, ref, C0, C1, Fn, HW):
    """Fused branch kernel (per-clip table algebra: sigmoid of one dot product, to_out as a K = 9 product) ==
    LN stats + q GEMM + 2-key softmax attention + 3 out GEMMs + LN-sum in the ORIGINAL formulation."""
    rows = Fn * HW
    x = rnd(rows, C0, seed=1) * 1.5 + 0.3
    x2 = rnd(rows, C1, seed=2) if C1 else None
    wq = packw(C0 + C1, 192, seed=3)
    wo = [packw(64, 64, seed=10 + b) for b in range(3)]
    g3, qs = rnd(3, 64, seed=4) * 0.2 + 1, rnd(3, 8, seed=5) * 0.2 + 1
    kvtab, nulltab = torch.zeros(Fn, 3, 128), torch.zeros(3, 16)
    for b in range(3):
        ref.xattn_prep(rnd(Fn, 128, seed=20 + b), rnd(8, seed=30 + b) * 0.2 + 1, rnd(2, 8, seed=40 + b), kvtab, b, nulltab)
    want = ref.xattn_layer_c64(x, x2, HW, wq, wo, g3, qs, kvtab, nulltab)
    got = hip.xattn_layer_c64(x.cuda(), None if x2 is None else x2.cuda(), HW, wq.cuda(), [w.cuda() for w in wo],
                              g3.cuda(), qs.cuda(), kvtab.cuda(), nulltab.cuda())
    check(f"xattn_layer_c64/{C0}+{C1}_F{Fn}_HW{HW}", got, want, 3e-5)
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    got = hip.xattn_layer_c64(x.cuda(), None if x2 is None else x2.cuda(), HW, wq.cuda(), [w.cuda() for w in wo],
                              g3.cuda(), qs.cuda(), kvtab.cuda(), nulltab.cuda(), wq_bf3=pack_bf3(unpack_kn(wq)).cuda())
    check(f"xattn_layer_c64_split/{C0}+{C1}_F{Fn}_HW{HW}", got, want, 3e-5)


@pytest.mark.parametrize("Co", [64, 256])
def test_xattn_trained_weight_like_range(hip, ref, Co):
    """Cross-attention with trained-checkpoint-like scales: q_scale / k_scale of ~4 (logits up to 8*16*|cos| = +-128: the
    two-key softmax saturates to exactly 0 / 1 for many heads -- the closed form 1/(1+2^z) must neither overflow to NaN nor
    lose the small side), activations x30 with an offset (LayerNorm removes both) and a large null key."""
    Fn, HW = 3, 64
    rows = Fn * HW
    qs = rnd(3, 8, seed=5) * 0.5 + 4.0
    kvtab, nulltab = torch.zeros(Fn, 3, 128), torch.zeros(3, 16)
    for b in range(3):
        ref.xattn_prep(rnd(Fn, 128, seed=20 + b) * 5.0, rnd(8, seed=30 + b) * 0.5 + 4.0, rnd(2, 8, seed=40 + b) * 5.0, kvtab, b, nulltab)
    wo = [packw(64, Co, seed=10 + b) for b in range(3)]
    g3 = rnd(3, Co, seed=4) * 0.2 + 1
    if Co == 64:
        x = (rnd(rows, 64, seed=1) * 1.5 + 0.3) * 30.0
        wq = packw(64, 192, seed=3) * 4.0
        want = ref.xattn_layer_c64(x, None, HW, wq, wo, g3, qs, kvtab, nulltab)
        from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
        for bf3 in (None, pack_bf3(unpack_kn(wq)).cuda()):
            got = hip.xattn_layer_c64(x.cuda(), None, HW, wq.cuda(), [w.cuda() for w in wo], g3.cuda(), qs.cuda(), kvtab.cuda(),
                                      nulltab.cuda(), wq_bf3=bf3)
            check(f"xattn_layer_c64/wide_range_split{int(bf3 is not None)}", got, want, 1e-4)
    else:
        q = rnd(rows, 192, seed=1) * 40.0
        o = ref.xattn_core(q.clone(), HW, kvtab, nulltab, qs)
        y3 = torch.cat([ref.conv_gemm(o[:, 64 * b:64 * b + 64], wo[b], Co, F=rows, Hi=1, Wi=1) for b in range(3)], 1)
        want = ref.xattn_ln_sum(y3, g3, Co)
        xtab = hip.xattn_tables(kvtab.cuda(), nulltab.cuda(), qs.cuda(), [w.cuda() for w in wo], Co)
        check(f"xattn_sigma_out/Co{Co}_wide_range", hip.xattn_sigma_out(q.cuda(), HW, xtab, g3.cuda(), Co), want, 1e-4)


@pytest.mark.parametrize("Co,Fn,HW", [(128, 3, 1024), (256, 5, 64), (512, 7, 16), (32, 2, 4), (96, 3, 36), (64, 2, 64)])
def test_xattn_sigma_out_equals_unfused_chain(hip, ref, Co, Fn, HW):
    """One-pass kernel (tables + sigmoid + K = 9 affine form + LN + sum) == xattn_core + 3 to_out GEMMs + xattn_ln_sum in
    the original formulation, and == its own table-based reference."""
    rows = Fn * HW
    q = rnd(rows, 192, seed=1) * 1.3
    wo = [packw(64, Co, seed=10 + b) for b in range(3)]
    g3, qs = rnd(3, Co, seed=4) * 0.2 + 1, rnd(3, 8, seed=5) * 0.2 + 1
    kvtab, nulltab = torch.zeros(Fn, 3, 128), torch.zeros(3, 16)
    for b in range(3):
        ref.xattn_prep(rnd(Fn, 128, seed=20 + b), rnd(8, seed=30 + b) * 0.2 + 1, rnd(2, 8, seed=40 + b), kvtab, b, nulltab)
    o = ref.xattn_core(q.clone(), HW, kvtab, nulltab, qs)
    y3 = torch.cat([ref.conv_gemm(o[:, 64 * b:64 * b + 64], wo[b], Co, F=rows, Hi=1, Wi=1) for b in range(3)], 1)
    want = ref.xattn_ln_sum(y3, g3, Co)
    xtab = hip.xattn_tables(kvtab.cuda(), nulltab.cuda(), qs.cuda(), [w.cuda() for w in wo], Co)
    got = hip.xattn_sigma_out(q.cuda(), HW, xtab, g3.cuda(), Co)
    check(f"xattn_sigma_out/Co{Co}_F{Fn}_HW{HW}", got, want, 3e-5)
    check(f"xattn_sigma_out/Co{Co}_vs_table_ref", got, ref.xattn_sigma_out(q, HW, ref.xattn_tables(kvtab, nulltab, qs, wo, Co), g3, Co), 3e-5)


@pytest.mark.parametrize("Co,C0,Fn,HW", [(64, 64, 3, 64), (64, 128, 2, 96), (128, 128, 3, 1024), (512, 512, 5, 16)])
def test_xattn_h1_epilogue(hip, ref, Co, C0, Fn, HW):
    """The cross-attention kernels writing h1 = SiLU(c1*a + b) + h_cond from their epilogue == h_cond followed by the
    GroupNorm-apply pass (dawn_gn_apply_res), for the fused Co = 64 kernel and the one-pass kernel after to_q."""
    rows = Fn * HW
    g3, qs = rnd(3, Co, seed=4) * 0.2 + 1, rnd(3, 8, seed=5) * 0.2 + 1
    kvtab, nulltab = torch.zeros(Fn, 3, 128), torch.zeros(3, 16)
    for b in range(3):
        ref.xattn_prep(rnd(Fn, 128, seed=20 + b), rnd(8, seed=30 + b) * 0.2 + 1, rnd(2, 8, seed=40 + b), kvtab, b, nulltab)
    wo = [packw(64, Co, seed=10 + b) for b in range(3)]
    c1, ga, gb = rnd(rows, Co, seed=7) * 1.5, rnd(Co, seed=8) * 0.3 + 1, rnd(Co, seed=9) * 0.3
    xtab = hip.xattn_tables(kvtab.cuda(), nulltab.cuda(), qs.cuda(), [w.cuda() for w in wo], Co)
    gn = (c1.cuda(), ga.cuda(), gb.cuda())
    if Co == 64:
        from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
        x = rnd(rows, C0, seed=1) * 1.5 + 0.3
        wq = packw(C0, 192, seed=3)
        for bf3 in (None, pack_bf3(unpack_kn(wq)).cuda()):
            kw = dict(xtab=xtab, wq_bf3=bf3)
            hc = hip.xattn_layer_c64(x.cuda(), None, HW, wq.cuda(), None, g3.cuda(), None, None, None, **kw)
            h1 = hip.xattn_layer_c64(x.cuda(), None, HW, wq.cuda(), None, g3.cuda(), None, None, None, gn=gn, **kw)
            check(f"xattn_h1/c64_C{C0}_split{int(bf3 is not None)}", h1, hip.gn_apply_res(*gn, hc), 2e-6)
            c1g = gn[0].clone()                                      # ... and written OVER c1 (include/dawn_hip.h: out may be gn_x): the same bits
            over = hip.xattn_layer_c64(x.cuda(), None, HW, wq.cuda(), None, g3.cuda(), None, None, None, gn=(c1g, gn[1], gn[2]), h1_over_c1=True, **kw)
            assert over is c1g and torch.equal(over, h1)
        want = ref.xattn_layer_c64(x, None, HW, wq, wo, g3, qs, kvtab, nulltab, gn=(c1, ga, gb))
        check(f"xattn_h1/c64_C{C0}_vs_ref", h1, want, 3e-5)
    else:
        q = rnd(rows, 192, seed=1) * 1.3
        hc = hip.xattn_sigma_out(q.cuda(), HW, xtab, g3.cuda(), Co)
        h1 = hip.xattn_sigma_out(q.cuda(), HW, xtab, g3.cuda(), Co, gn=gn)
        check(f"xattn_h1/sigma_out_Co{Co}", h1, hip.gn_apply_res(*gn, hc), 2e-6)
        c1g = gn[0].clone()
        over = hip.xattn_sigma_out(q.cuda(), HW, xtab, g3.cuda(), Co, gn=(c1g, gn[1], gn[2]), h1_over_c1=True)
        assert over is c1g and torch.equal(over, h1)
        check(f"xattn_h1/sigma_out_Co{Co}_vs_ref", h1, ref.xattn_sigma_out(q, HW, ref.xattn_tables(kvtab, nulltab, qs, wo, Co), g3, Co, gn=(c1, ga, gb)), 3e-5)


def test_xattn_layer_c64_rejects_straddling_tiles(hip):
    """H*W not a multiple of 32 (a pixel tile would straddle two frames' tables): the op refuses, the orchestration
    (`can_fuse_xattn`) takes the unfused chain instead."""
    from dawn_pytorch_amd._lib import DawnHipError
    assert not hip.can_fuse_xattn(64, 64, 64, 100)
    with pytest.raises(DawnHipError):
        hip.xattn_layer_c64(torch.zeros(200, 64, device="cuda"), None, 100, torch.zeros(16, 192, 4, device="cuda"), None,
                            torch.ones(3, 64, device="cuda"), None, None, None, xtab=torch.zeros(2, 3, 640, device="cuda"))


# ---------------------------------------------------------------------------------------------- attention cores
@pytest.mark.parametrize("Fext,HW,q0,Fq,win", [(12, 5, 0, 12, 3), (100, 3, 0, 100, 40), (70, 2, 20, 33, 40),
                                                 (45, 4, 3, 40, 7), (33, 2, 0, 33, 40),
                                                 # the shapes the benchmark / long clips / T-shards run (several 128-query
                                                 # blocks, a full +-40 window on both sides, q0 != 0, >= 64 pixel columns)
                                                 (200, 64, 0, 200, 40), (280, 64, 40, 200, 40), (400, 64, 0, 400, 40),
                                                 (240, 70, 40, 200, 40), (327, 64, 40, 247, 40),
                                                 (64, 3, 0, 64, 16), (120, 2, 31, 70, 8), (150, 2, 0, 150, 48), (100, 2, 9, 80, 45)])
def test_temporal_attn(hip, ref, Fext, HW, q0, Fq, win):
    qkv = rnd(Fext * HW, 768, seed=1)
    ang = torch.arange(Fext).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    rc, rs = ang.cos().contiguous(), ang.sin().contiguous()
    band = rnd(2 * win + 1, 8, seed=2)
    want = ref.temporal_attn(qkv, Fext, HW, q0, Fq, win, rc, rs, band)
    got = hip.temporal_attn(qkv.cuda(), Fext, HW, q0, Fq, win, rc.cuda(), rs.cuda(), band.cuda())
    check(f"temporal_attn/F{Fext}_q{q0}_{Fq}_w{win}", got, want, 2e-5)
    try:                                                        # both kernels explicitly: fp32 MFMA / split operands on any grid
        hip.temporal_attn_flags = TA.FP32
        got32 = hip.temporal_attn(qkv.cuda(), Fext, HW, q0, Fq, win, rc.cuda(), rs.cuda(), band.cuda())
        hip.temporal_attn_flags = TA.SPLIT_ALWAYS
        got16 = hip.temporal_attn(qkv.cuda(), Fext, HW, q0, Fq, win, rc.cuda(), rs.cuda(), band.cuda())
    finally:
        hip.temporal_attn_flags = 0
    check(f"temporal_attn_fp32/F{Fext}_q{q0}_{Fq}_w{win}", got32, want, 2e-5)
    check(f"temporal_attn_split/F{Fext}_q{q0}_{Fq}_w{win}", got16, want, 2e-5)
    if win <= 40 and Fext <= 208 and (Fq + (q0 - win) % 16 + 15) // 16 <= 13:      # the window-tiled 13-wave kernel, on any grid
        try:
            hip.temporal_attn_flags = TA.WAVE13
            got13 = hip.temporal_attn(qkv.cuda(), Fext, HW, q0, Fq, win, rc.cuda(), rs.cuda(), band.cuda())
        finally:
            hip.temporal_attn_flags = 0
        check(f"temporal_attn_13wave/F{Fext}_q{q0}_{Fq}_w{win}", got13, want, 2e-5)


@pytest.mark.parametrize("Fext,HW,q0,Fq,win", [(200, 256, 0, 200, 40), (200, 130, 47, 120, 40), (184, 128, 0, 184, 40), (120, 128, 31, 70, 24),
                                                 (208, 128, 8, 200, 40), (200, 128, 40, 120, 40)])
def test_temporal_attn_13wave_at_chip_filling_grids(hip, ref, Fext, HW, q0, Fq, win):
    """temporal_attn13_kernel (opt-in, TemporalAttnFlags.WAVE13) at chip-filling grids (>= 128 pixel columns: the 128- / 256-channel levels of the benchmark,
    the 120-query segments of longer clips and T-shard ranks): against the oracle and the 32 x 32 kernel, and eight runs bit-identical (the kernel
    keeps the fused layer's load / compute regions: a load that lands in the registers of an MFMA still in flight shows up as a different tile
    every run)."""
    qkv = rnd(Fext * HW, 768, seed=11)
    ang = torch.arange(Fext).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    rc, rs = ang.cos().contiguous(), ang.sin().contiguous()
    band = rnd(2 * win + 1, 8, seed=12)
    want = ref.temporal_attn(qkv, Fext, HW, q0, Fq, win, rc, rs, band)
    args = (qkv.cuda(), Fext, HW, q0, Fq, win, rc.cuda(), rs.cuda(), band.cuda())
    old = hip.temporal_attn(*args)                                   # automatic: the 32 x 32 split kernel
    try:
        hip.temporal_attn_flags = TA.WAVE13
        got = hip.temporal_attn(*args)
        check(f"temporal_attn_13wave/F{Fext}_HW{HW}_q{q0}_{Fq}_w{win}", got, want, 2e-5)
        check(f"temporal_attn_13wave_vs_32x32/F{Fext}_HW{HW}", got, old, 2e-5)
        for _ in range(7):
            assert torch.equal(hip.temporal_attn(*args), got)
        # the layout experiment (TemporalAttnFlags.PIXEL_HEAD_MAJOR): the same rows in the (pixel, head)-major layout [pixel][head][q | k | v][buffer row][32]
        hip.temporal_attn_flags = TA.WAVE13 | TA.PIXEL_HEAD_MAJOR
        ph = qkv.view(Fext, HW, 3, 8, 32).permute(1, 3, 2, 0, 4).contiguous().view(Fext * HW, 768).cuda()
        assert torch.equal(hip.temporal_attn(ph, *args[1:]), got)
    finally:
        hip.temporal_attn_flags = 0


@pytest.mark.parametrize("Fext,HW,q0,Fq,win", [(12, 5, 0, 12, 3), (200, 3, 0, 200, 40), (280, 2, 40, 200, 40),
                                                 (45, 4, 3, 40, 7), (33, 2, 0, 33, 40), (240, 2, 40, 200, 40),
                                                 (200, 64, 0, 200, 40), (200, 3, 47, 120, 40), (190, 2, 5, 185, 33),
                                                 (96, 4, 0, 96, 40), (130, 2, 13, 100, 40), (150, 2, 0, 150, 48),
                                                 (100, 2, 9, 80, 45), (64, 3, 0, 64, 16), (120, 2, 31, 70, 24)])
def test_temporal_layer_c64(hip, ref, Fext, HW, q0, Fq, win):
    """Fused layer kernel == composition of LN stats + qkv GEMM + windowed attention + out GEMM + residual."""
    x = rnd(Fext * HW, 64, seed=1) * 1.3 + 0.2
    wqkv, wout = packw(64, 768, seed=2), packw(256, 64, seed=3)
    ang = torch.arange(Fext).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    rc, rs = ang.cos().contiguous(), ang.sin().contiguous()
    band = rnd(2 * win + 1, 8, seed=4)
    want = ref.temporal_layer_c64(x, Fext, HW, q0, Fq, win, wqkv, wout, rc, rs, band)
    got = hip.temporal_layer_c64(*gpu(x), Fext, HW, q0, Fq, win, *gpu(wqkv, wout, rc, rs, band))
    check(f"temporal_layer_c64/F{Fext}_q{q0}_{Fq}_w{win}", got, want, 3e-5)
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    from dawn_pytorch_amd.pack import pack_bf3_temporal_out
    wsplit = pack_bf3(unpack_kn(wqkv)).cuda()
    wosp = pack_bf3_temporal_out(unpack_kn(wout)).cuda()
    got = hip.temporal_layer_c64(*gpu(x), Fext, HW, q0, Fq, win, *gpu(wqkv, wout, rc, rs, band), wqkv_bf3=wsplit)
    check(f"temporal_layer_c64_split/F{Fext}_q{q0}_{Fq}_w{win}", got, want, 3e-5)
    # every kernel family explicitly
    try:
        for flags, name in ((WMODE(0), "wmode0"), (WMODE(1), "wmode1"), (WMODE(2), "wmode2"), (WMODE(3), "wmode3"),
                            (WMODE(3) | TF.SCHED_HINTS, "wmode3_hints"), (WMODE(3) | TF.OUT_FP32, "wmode3_out_fp32"), (WMODE(4), "wmode4_window_tiled"),
                            (WMODE(5), "wmode5_tile_per_wave"), (TF.KEEP_32X32, "auto_without_wmode4")):
            if flags in (WMODE(4), WMODE(5)) and (win > 40 or Fext > 208):
                continue                                         # outside the window-tiled kernels' instantiation
            if flags == WMODE(5) and (Fq + (q0 - win) % 16 + 15) // 16 > 13:
                continue                                         # more than 13 query tiles
            if flags & TF.FORCE_MASK == WMODE(3) and (Fext * 576 + ((Fext + 31) // 32) * 6144 + 8 * (32 * ((32 + 2 * win + 31) // 32) + 32) * 4 > 163840
                                   or Fq + (q0 - win) % 16 > 256):
                continue                                         # WMODE 3 does not fit this shape (LDS)
            if flags == WMODE(1) and Fext > 192:
                continue                                         # weight slices in LDS need the room
            hip.temporal_flags = flags
            got = hip.temporal_layer_c64(*gpu(x), Fext, HW, q0, Fq, win, *gpu(wqkv, wout, rc, rs, band), wqkv_bf3=wsplit,
                                         wout_bf3p=wosp)
            check(f"temporal_layer_c64_{name}/F{Fext}_q{q0}_{Fq}_w{win}", got, want, 3e-5)
    finally:
        hip.temporal_flags = 0


def test_temporal_attention_trained_weight_like_range(hip, ref):
    """Trained-checkpoint-like statistics (all parity is on random-init weights, where logits are O(1)): activations x30 with
    a trend along the frame axis, projection weights x6 -> logits of +-100s that grow towards late frames, so that every key
    tile raises the running softmax maximum and most probabilities underflow; the relative-position band spans +-20.  The
    fused layer (every kernel family) and the unfused attention core must still match the max-subtracted fp32 reference."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, unpack_kn
    Fext, HW, q0, Fq, win = 200, 4, 0, 200, 40
    ramp = torch.linspace(-1.0, 1.0, Fext).repeat_interleave(HW)[:, None]
    x = (rnd(Fext * HW, 64, seed=1) * 1.3 + ramp * rnd(1, 64, seed=7) * 3.0) * 30.0
    wqkv, wout = packw(64, 768, seed=2) * 6.0, packw(256, 64, seed=3)
    ang = torch.arange(Fext).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    rc, rs = ang.cos().contiguous(), ang.sin().contiguous()
    band = rnd(2 * win + 1, 8, seed=4) * 20.0
    want = ref.temporal_layer_c64(x, Fext, HW, q0, Fq, win, wqkv, wout, rc, rs, band)
    wsplit, wosp = pack_bf3(unpack_kn(wqkv)).cuda(), pack_bf3_temporal_out(unpack_kn(wout)).cuda()
    try:
        for flags, name in ((0, "default"), (WMODE(0), "wmode0"), (WMODE(2), "wmode2"), (WMODE(3), "wmode3"), (WMODE(4), "wmode4_window_tiled"),
                            (WMODE(5), "wmode5_tile_per_wave")):
            hip.temporal_flags = flags
            got = hip.temporal_layer_c64(*gpu(x), Fext, HW, q0, Fq, win, *gpu(wqkv, wout, rc, rs, band), wqkv_bf3=wsplit,
                                         wout_bf3p=wosp)
            check(f"temporal_layer_c64_{name}/wide_range", got, want, 1e-4)
    finally:
        hip.temporal_flags = 0
    qkv = rnd(Fext * HW, 768, seed=5) * 6.0
    qkv[:, 256:512] += ramp * 12.0                                    # keys trend along the frame axis
    want = ref.temporal_attn(qkv, Fext, HW, q0, Fq, win, rc, rs, band)
    check("temporal_attn/wide_range", hip.temporal_attn(qkv.cuda(), Fext, HW, q0, Fq, win, rc.cuda(), rs.cuda(), band.cuda()),
          want, 1e-4)


@pytest.mark.parametrize("F", [200, 184, 120])
def test_temporal_layer16_is_run_to_run_deterministic(hip, F):
    """The window-tiled layer (WMODE 4) on many workgroups, eight times on the same input: bit-identical, and equal to the 32 x 32
    kernel to round-off.  Guards the rule its regions implement (csrc/temporal_layer16.hip "REGIONS"): a load issued right behind an
    MFMA whose operand registers it overwrites corrupted one (pixel, head, tile) in ~300, a different one every run -- at 256 pixels
    x 8 heads x 13 tiles per run that is ~99.9 % per run to show up here."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, unpack_kn
    HW, win = 256, 40
    x = (rnd(F * HW, 64, seed=1) * 1.3 + 0.2).cuda()
    wqkv, wout = packw(64, 768, seed=2), packw(256, 64, seed=3)
    ang = torch.arange(F).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    rc, rs, band = ang.cos().contiguous().cuda(), ang.sin().contiguous().cuda(), rnd(2 * win + 1, 8, seed=5).cuda()
    kw = dict(wqkv_bf3=pack_bf3(unpack_kn(wqkv)).cuda(), wout_bf3p=pack_bf3_temporal_out(unpack_kn(wout)).cuda())
    try:
        hip.temporal_flags = WMODE(3)
        want = hip.temporal_layer_c64(x, F, HW, 0, F, win, *gpu(wqkv, wout), rc, rs, band, **kw)
        for flags in (WMODE(4), WMODE(5)):
            hip.temporal_flags = flags
            first = hip.temporal_layer_c64(x, F, HW, 0, F, win, *gpu(wqkv, wout), rc, rs, band, **kw)
            check(f"temporal_layer16_vs_wmode3/F{F}_flags{flags}", first, want.cpu(), 3e-5)
            for rep in range(7):
                again = hip.temporal_layer_c64(x, F, HW, 0, F, win, *gpu(wqkv, wout), rc, rs, band, **kw)
                assert torch.equal(again, first), f"flags {flags}: run {rep + 1} differs from run 0 in {int((again != first).sum())} elements"
    finally:
        hip.temporal_flags = 0


@pytest.mark.parametrize("Fext,HW,q0,Fq", [(400, 8, 0, 400), (280, 8, 40, 200), (330, 4, 17, 301), (240, 8, 0, 200)])
def test_temporal_layer_c64_segmented(hip, ref, Fext, HW, q0, Fq):
    """Long frame buffers (BASELINE configs[1]: 400 frames; T-shard windows of 280): one fused launch per 120-query segment
    on overlapping row windows == the unfused composition on the whole buffer."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, unpack_kn
    win = 40
    x = rnd(Fext * HW, 64, seed=1) * 1.3 + 0.2
    wqkv, wout = packw(64, 768, seed=2), packw(256, 64, seed=3)
    ang = torch.arange(Fext).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    rc, rs = ang.cos().contiguous(), ang.sin().contiguous()
    band = rnd(2 * win + 1, 8, seed=4)
    want = ref.temporal_layer_c64(x, Fext, HW, q0, Fq, win, wqkv, wout, rc, rs, band)
    got = hip.temporal_layer_c64_segmented(*gpu(x), Fext, HW, q0, Fq, win, *gpu(wqkv, wout, rc, rs, band),
                                           wqkv_bf3=pack_bf3(unpack_kn(wqkv)).cuda(), wout_bf3p=pack_bf3_temporal_out(unpack_kn(wout)).cuda())
    check(f"temporal_layer_c64_segmented/F{Fext}_q{q0}_{Fq}", got, want, 3e-5)
    # explicit segment order (interior first, as the T-shard path issues them)
    segs = [(q0 + 40, q0 + Fq - 40), (q0, q0 + 40), (q0 + Fq - 40, q0 + Fq)] if Fq - 80 <= 120 else None
    if segs:
        got = hip.temporal_layer_c64_segmented(*gpu(x), Fext, HW, q0, Fq, win, *gpu(wqkv, wout, rc, rs, band),
                                               wqkv_bf3=pack_bf3(unpack_kn(wqkv)).cuda(),
                                               wout_bf3p=pack_bf3_temporal_out(unpack_kn(wout)).cuda(), segments=segs)
        check(f"temporal_layer_c64_segmented_interior_first/F{Fext}_q{q0}_{Fq}", got, want, 3e-5)


@pytest.mark.parametrize("F,HW", [(3, 64), (2, 256), (5, 16), (2, 100)])
def test_sla(hip, ref, F, HW):
    qkv = rnd(F * HW, 768, seed=1)
    check(f"sla/F{F}_HW{HW}", hip.sla(qkv.cuda(), F, HW), ref.sla(qkv, F, HW), 2e-5)


@pytest.mark.parametrize("F,HW", [(3, 64), (2, 1024), (5, 256), (1, 4096), (2, 100), (3, 1000), (9, 2080)])
def test_sla_layer_c64(hip, ref, F, HW):
    """Fused layer == LN stats + qkv GEMM + linear attention + out GEMM (+bias) + residual."""
    x = rnd(F * HW, 64, seed=1) * 1.3 + 0.2
    wqkv, wout, bias = packw(64, 768, seed=2) * 2.0, packw(256, 64, seed=3), rnd(64, seed=4)
    want = ref.sla_layer_c64(x, F, HW, wqkv, wout, bias)
    got = hip.sla_layer_c64(*gpu(x), F, HW, *gpu(wqkv, wout, bias))
    check(f"sla_layer_c64/F{F}_HW{HW}", got, want, 3e-5)
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    got = hip.sla_layer_c64(*gpu(x), F, HW, *gpu(wqkv, wout, bias), wqkv_bf3=pack_bf3(unpack_kn(wqkv)).cuda())
    check(f"sla_layer_c64_split/F{F}_HW{HW}", got, want, 3e-5)


@pytest.mark.parametrize("F,HW", [(200, 256), (96, 1024), (200, 100)])
def test_c64_attention_layers_in_place(hip, F, HW):
    """include/dawn_hip.h: `out` may be `x` for dawn_sla_layer_c64 and, when the layer covers its whole frame buffer, for
    dawn_temporal_layer_c64_ex (the denoiser's unsharded 64-channel layers run in place).  In place == out of place, bit for bit, for
    every kernel family the benchmark's shapes take (fp32-MFMA and split-operand forms; many workgroups per CU slot at HW = 1024)."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, unpack_kn
    win = 40
    x = (rnd(F * HW, 64, seed=1) * 1.3 + 0.2).cuda()
    wqkv, wout, bias = packw(64, 768, seed=2), packw(256, 64, seed=3), rnd(64, seed=4)
    ang = torch.arange(F).float()[:, None] * (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32)))[None]
    rc, rs, band = ang.cos().contiguous().cuda(), ang.sin().contiguous().cuda(), rnd(2 * win + 1, 8, seed=5).cuda()
    wsplit, wosp = pack_bf3(unpack_kn(wqkv)).cuda(), pack_bf3_temporal_out(unpack_kn(wout)).cuda()
    try:
        for kw, flags in (({}, 0), ({"wqkv_bf3": wsplit, "wout_bf3p": wosp}, 0), ({"wqkv_bf3": wsplit, "wout_bf3p": wosp}, WMODE(3))):
            hip.temporal_flags = flags                                # 0 with both images: the window-tiled kernel; WMODE 3: the 32 x 32 one
            want = hip.temporal_layer_c64(x, F, HW, 0, F, win, *gpu(wqkv, wout), rc, rs, band, **kw)
            xin = x.clone()
            got = hip.temporal_layer_c64(xin, F, HW, 0, F, win, *gpu(wqkv, wout), rc, rs, band, out=xin, **kw)
            assert got is xin and torch.equal(got, want)
    finally:
        hip.temporal_flags = 0
    for kw in ({}, {"wqkv_bf3": wsplit}):
        want = hip.sla_layer_c64(x, F, HW, *gpu(wqkv, wout, bias), **kw)
        xin = x.clone()
        got = hip.sla_layer_c64(xin, F, HW, *gpu(wqkv, wout, bias), out=xin, **kw)
        assert got is xin and torch.equal(got, want)


def test_sla_softmax_reference_is_shift_safe(hip, ref):
    """The single-sweep linear-attention kernels keep a lazily raised softmax reference (raised only when a tile exceeds it by
    2^8) and merge slices by their references: logits with a large dynamic range and a strong trend along the pixel axis (every
    tile raises the maximum; late pixels dwarf early ones) must still match the two-pass reference."""
    from dawn_pytorch_amd.pack import pack_bf3, unpack_kn
    F, HW = 2, 2048
    ramp = torch.linspace(-1.0, 1.0, HW).repeat(F)[:, None]
    x = rnd(F * HW, 64, seed=1) * 2.0 + ramp * rnd(1, 64, seed=7) * 6.0
    wqkv, wout, bias = packw(64, 768, seed=2) * 6.0, packw(256, 64, seed=3), rnd(64, seed=4)
    want = ref.sla_layer_c64(x, F, HW, wqkv, wout, bias)
    got = hip.sla_layer_c64(*gpu(x), F, HW, *gpu(wqkv, wout, bias), wqkv_bf3=pack_bf3(unpack_kn(wqkv)).cuda())
    check("sla_layer_c64_split/wide_range", got, want, 1e-4)
    qkv = rnd(F * HW, 768, seed=5) * 4.0
    qkv[:, 256:512] += ramp * 25.0                                   # keys grow by ~50 over the frame
    check("sla/wide_range", hip.sla(qkv.cuda(), F, HW), ref.sla(qkv, F, HW), 1e-4)


@pytest.mark.parametrize("F,N", [(4, 16), (3, 64), (2, 100)])
def test_frame_attn(hip, ref, F, N):
    qkv = rnd(F * N, 768, seed=1)
    check(f"frame_attn/F{F}_N{N}", hip.frame_attn(qkv.cuda(), F, N), ref.frame_attn(qkv, F, N), 2e-5)


# ---------------------------------------------------------------------------------------------- boundary / small
def test_init_conv_x_and_head(hip, ref):
    F, h, w, Co = 3, 8, 8, 64
    x, w3, fp = rnd(3, F, h, w, seed=1), rnd(147, Co, seed=2) * 0.1, rnd(h * w, Co, seed=3)
    check("init_conv_x", hip.init_conv_x(x.cuda(), w3.cuda(), fp.cuda(), F, h, w, Co), ref.init_conv_x(x, w3, fp, F, h, w, Co), 2e-5)
    for (F, h, w) in ((2, 32, 32), (1, 64, 64), (3, 16, 16), (2, 12, 64)):   # MFMA kernel geometries (256 % w == 0, rows | h)
        x, fp = rnd(3, F, h, w, seed=11), rnd(h * w, Co, seed=13)
        check(f"init_conv_x_mfma/{F}x{h}x{w}", hip.init_conv_x(x.cuda(), w3.cuda(), fp.cuda(), F, h, w, Co),
              ref.init_conv_x(x, w3, fp, F, h, w, Co), 2e-5)
    for Co in (16, 64):
        hg, ho = rnd(500, Co, seed=4), rnd(500, Co, seed=5)
        wg, bg, wo, bo = rnd(2, Co, seed=6), rnd(2, seed=7), rnd(1, Co, seed=8), rnd(1, seed=9)
        check(f"head_out/Co{Co}", hip.head_out(*gpu(hg, ho, wg, bg, wo, bo)), ref.head_out(hg, ho, wg, bg, wo, bo), 2e-5)


@pytest.mark.parametrize("M,K,N,act,bias", [(1, 64, 256, 0, True), (1, 256, 256, 2, True), (1, 256, 4352, 1, True),
                                            (20, 1024, 128, 1, True), (20, 6, 128, 1, True), (20, 2, 32, 1, True),
                                            (20, 128, 128, 0, False)])
def test_linear(hip, ref, M, K, N, act, bias):
    x, W = rnd(M, K, seed=1), rnd(N, K, seed=2) * K ** -0.5
    b = rnd(N, seed=3) if bias else None
    check(f"linear/{M}x{K}x{N}_a{act}", hip.linear(x.cuda(), W.cuda(), None if b is None else b.cuda(), act), ref.linear(x, W, b, act), 2e-5)


def test_linear_strided_input(hip, ref):
    cond = rnd(9, 1032, seed=1)
    W, b = rnd(64, 6, seed=2), rnd(64, seed=3)
    check("linear/strided", hip.linear(cond.cuda()[:, 1024:1030], W.cuda(), b.cuda(), 1), ref.linear(cond[:, 1024:1030], W, b, 1), 2e-5)


def test_sinusoidal(hip, ref):
    import math
    fr = torch.exp(torch.arange(32, dtype=torch.float32) * -(math.log(10000) / 31))
    for t in (0, 19, 980):
        check(f"sinusoidal/t{t}", hip.sinusoidal(t, fr.cuda()), ref.sinusoidal(t, fr), 2e-6)


# ---------------------------------------------------------------------------------------------- sampler
def test_ddim_x0_and_histogram(hip, ref):
    x, e = rnd(3, 5, 8, 8, seed=1), rnd(3, 5, 8, 8, seed=2)
    wx0, wh = ref.ddim_x0(x, e, 1.25, 0.75)
    gx0, gh = hip.ddim_x0(x.cuda(), e.cuda(), 1.25, 0.75)
    check("ddim_x0", gx0, wx0, 1e-6)
    gbits = (gx0.abs().cpu().contiguous().view(torch.int32) >> 20).flatten().long()
    assert torch.equal(gh.cpu(), torch.bincount(gbits, minlength=2048).to(torch.int32)), "histogram not exact"


@pytest.mark.parametrize("n,scale", [(7, 2.0), (10, 0.3), (11, 2.0), (1000, 1.0), (36864, 3.0), (100001, 0.5),
                                     (2457600, 1.0)])
def test_quantile_matches_torch(hip, n, scale):
    v = rnd(n, seed=n % 97) * scale
    if n == 1000:
        v[::3] = 1.5                                   # heavy ties around the quantile
    want = torch.quantile(v.abs(), 0.9)
    x0 = v.cuda().contiguous()
    _, hist = hip.ddim_x0(x0, torch.zeros_like(x0), 1.0, 0.0)
    s = hip.quantile_threshold(x0, hist, n, 0.9).cpu()
    assert float(s[1]) == pytest.approx(float(want), rel=0, abs=1e-6 * max(1, float(want))), (float(s[1]), float(want))
    assert float(s[0]) == max(1.0, float(s[1]))


@pytest.mark.parametrize("n", [19660800, (1 << 24) + 2])
def test_quantile_exact_rank_above_2p24(hip, n):
    """n = 3*1600*64*64 (BASELINE configs[3], the T-sharded 1600-frame clip) is above torch.quantile's 2^24 cap: there the
    rank q*(n-1) must be exact (fp32 cannot represent n-1), checked against a sort-based fp64 evaluation."""
    g = torch.Generator(device="cuda").manual_seed(n % 1000)
    v = torch.randn(n, device="cuda", generator=g) * 1.7
    sv = torch.sort(v.abs()).values
    pos = 0.9 * (n - 1)                                  # python float = fp64
    lo = int(pos // 1)
    a, b = float(sv[lo]), float(sv[min(lo + 1, n - 1)])
    want = a + (b - a) * (pos - lo)
    assert hip.quantile_rank(n, 0.9)[0] == lo
    import numpy as np
    assert int(np.floor(np.float32(0.9) * np.float32(n - 1))) != lo, "fp32 rank would have been right: weak test size"
    _, hist = hip.ddim_x0(v, torch.zeros_like(v), 1.0, 0.0)
    s = hip.quantile_threshold(v, hist, n, 0.9).cpu()
    assert abs(float(s[1]) - want) <= 2e-7 * max(1.0, want), (float(s[1]), want)
    assert a <= float(s[1]) <= b


def test_quantile_golden(hip):
    from conftest import load_golden
    d = load_golden("quantile.npz")
    for k in d:
        if k.startswith("v"):
            for row, q in zip(torch.from_numpy(d[k]), d["q" + k[1:]]):
                x0 = row.cuda().contiguous()
                _, hist = hip.ddim_x0(x0, torch.zeros_like(x0), 1.0, 0.0)
                s = hip.quantile_threshold(x0, hist, x0.numel(), 0.9).cpu()
                assert abs(float(s[1]) - float(q)) <= 1e-6 * max(1.0, float(q)), (k, float(s[1]), float(q))


def test_ddim_update_and_cfg(hip, ref):
    x0, e, nz = rnd(3, 4, 8, 8, seed=1) * 2, rnd(3, 4, 8, 8, seed=2), rnd(3, 4, 8, 8, seed=3)
    s = torch.tensor([1.7, 1.7])
    check("ddim_update", hip.ddim_update(x0.cuda(), e.cuda(), s.cuda(), nz.cuda(), 0.9, 0.3, 0.2), ref.ddim_update(x0, e, s, nz, 0.9, 0.3, 0.2), 1e-6)
    check("ddim_update/nonoise", hip.ddim_update(x0.cuda(), e.cuda(), s.cuda(), None, 1.0, 0.0, 0.0), ref.ddim_update(x0, e, s, None, 1.0, 0.0, 0.0), 1e-6)
    check("cfg_combine", hip.cfg_combine(x0.cuda(), e.cuda(), 2.5), ref.cfg_combine(x0, e, 2.5), 1e-6)


def test_philox_normal(hip, ref):
    a = hip.philox_normal(3, 6, 0, 6, 64, 1234, 1, "cuda").cpu()
    w = ref.philox_normal(3, 6, 0, 6, 64, 1234, 1, "cpu")
    check("philox_normal", a, w, 2e-5)
    # shard invariance: frames [2,5) of a 6-frame clip equal the slice of the unsharded draw
    b = hip.philox_normal(3, 3, 2, 6, 64, 1234, 1, "cuda").cpu()
    assert torch.equal(b, a[:, 2:5])
    big = hip.philox_normal(3, 200, 0, 200, 4096, 7, 3, "cuda")
    assert abs(float(big.mean())) < 3e-3 and abs(float(big.std()) - 1) < 3e-3
