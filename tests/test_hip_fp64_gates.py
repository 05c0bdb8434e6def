"""-m gpu: every split-bf16 kernel against a float64 reference at fp32 accuracy (tests/split_gate.py), at the launch classes of the 256-px /
200-frame and the 128-px / 400-frame configurations (profiles/r6_insitu_shapes.txt, profiles/r6_config1_insitu_shapes.txt: H, W, channel counts
and N as they launch; the 1x1 and resample cases at their M, the 3x3 cases at the fewest frames that keep the kernel, its tile geometry and at
least two tiles), after asserting which kernel the launch takes (dawn_gemm1x1_form / dawn_conv3x3_form / dawn_conv3x3_direct_form of the very
descriptor); the fp32-MFMA kernels that take the same convs at an odd clip length; and repeated-run bit identity of the kernels whose loads are
placed by hand.

The gate (split_gate.fp32_gate): max|hip - fp64| / max|fp64| <= C_GATE x the same for the RefOps op in fp32 on CPU + FLOOR.
tests/test_split_gate_cpu.py shows that every case here rejects a kernel that lost its third weight plane or read a stale one.  C_GATE = 2
holds for the temporal, SLA and cross-attention kernels; the 1x1, resample and 3x3 kernels carry factors widened to their measured
ratios (split_gate.C_TILED ... C_DIRECT_DEEP, each with the MI355X measurement beside it).  The same gate holds the attention cores of the
unfused levels (HipOps.temporal_attn: the split-operand EXT core, the fp32 kernel, the 13-wave core) and the fp32 attention kernels (SLA,
frame attention, the unfused cross-attention chain).  Each gate appends its errors and its ratio to CPU fp32 to the op-error log of
test_hip_ops.check (split_gate.LOG)."""
import pytest
import torch

import split_gate as G
from dawn_pytorch_amd.policy import TemporalAttnFlags as TA, TemporalFlags as TF
from oracle.ops_ref import RefOps

pytestmark = pytest.mark.gpu

REPEATS = 8


@pytest.fixture(scope="module")
def hip():
    from dawn_pytorch_amd.ops import HipOps
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return HipOps()


def _w5(w_kn, Cin, N):
    """(9 Cin, N), k = tap * Cin + c -> Conv3d layout (N, Cin, 1, 3, 3)."""
    return w_kn.reshape(3, 3, Cin, N).permute(3, 2, 0, 1)[:, :, None].contiguous()


def cu(t):
    return None if t is None else t.cuda()


def conv_call(case, T, Wkn):
    """(HipOps.conv_gemm positional args, keyword args) of a gemm / down / up / conv3 case, on the GPU."""
    from dawn_pytorch_amd.pack import pack_bf3, pack_kn, pack_wino4_bf3, pack_wino_bf3
    p, k, w = case.p, case.kind, Wkn["w"]
    if k == "gemm":
        M, H = p["M"], p.get("H", 16)
        return ((cu(T["x0"]), pack_kn(w).cuda(), p["N"]),
                dict(in1=cu(T["x1"]), F=M // (H * H), Hi=H, Wi=H, res=cu(T["res"]), bias=cu(T["bias"]), ln_eps=1e-5 if p.get("ln") else 0.0,
                     w_bf3=pack_bf3(w).cuda()))
    H = p["H"]
    if k == "down":
        return ((cu(T["x"]), pack_kn(w).cuda(), p["N"]),
                dict(F=p["F"], Hi=H, Wi=H, Ho=H // 2, Wo=H // 2, KH=4, KW=4, stride=2, pad=1, bias=cu(T["bias"]), w_bf3=pack_bf3(w).cuda()))
    if k == "up":
        return ((cu(T["x"]), torch.stack([pack_kn(w[i]) for i in range(4)], 0).cuda(), p["N"]),
                dict(F=p["F"], Hi=H, Wi=H, Ho=2 * H, Wo=2 * H, KH=2, KW=2, mode=1, bias=cu(T["bias"]),
                     w_bf3=torch.stack([pack_bf3(w[i]) for i in range(4)], 0).cuda()))
    Cin, N = p["C0"] + p.get("C1", 0), p["N"]
    w5 = _w5(w, Cin, N)
    return ((cu(T["x0"]), pack_kn(w).cuda(), N),
            dict(in1=cu(T["x1"]), F=p["F"], Hi=H, Wi=H, KH=3, KW=3, pad=1, w_bf3=pack_bf3(w).cuda(), w_wino=pack_wino_bf3(w5).cuda(),
                 w_wino4=pack_wino4_bf3(w5).cuda()))


def references(case):
    T, Wkn = case.make()
    ops = RefOps()
    return T, Wkn, case.ref(ops, T, Wkn, torch.float64), case.base32(ops, T, Wkn)


# ---------------------------------------------------------------------------------------------- 1x1 / resample / 3x3 gates
CONV_CASES = [c for c in G.CASES if c.kind in ("gemm", "down", "up", "conv3")]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c.name for c in CONV_CASES])
def test_conv_split_fp64_gate(hip, case):
    T, Wkn, want64, base32 = references(case)
    args, kw = conv_call(case, T, Wkn)
    try:
        hip.conv_policy = case.p.get("policy", 0)
        f3, f1 = hip.conv_gemm(*args, **kw, form_only=True)
        if case.kind == "conv3":
            assert (f3, f1) == (case.form, 0), (case.name, f3, f1)
            if "direct" in case.p:           # which direct kernel, or none of them (the fp32 kernels): dawn_conv3x3_direct_form
                fd = hip.conv_gemm(*args, **kw, form_only="direct")
                assert fd in case.p["direct"], (case.name, fd)
        else:
            assert (f3, f1) == (0, case.form), (case.name, f3, f1)
        got = hip.conv_gemm(*args, **kw)
        torch.cuda.synchronize()
    finally:
        hip.conv_policy = 0
    G.fp32_gate(case.name, got, want64, base32, c=case.c)


# ---------------------------------------------------------------------------------------------- attention layers
# temporal_flags: automatic, every forced WMODE (4: the window-tiled kernel, 5: its tile-per-wave form), automatic without WMODE 4 / 5
WMODE = TF.force_wmode
TEMPORAL_FLAGS = (0, WMODE(0), WMODE(1), WMODE(2), WMODE(3), WMODE(4), WMODE(5), TF.KEEP_32X32)


def temporal_fits(flags, Fext, q0, Fq, win=40):
    """The shapes each forced WMODE instantiates (the same exclusions as test_hip_ops.test_temporal_layer_c64)."""
    if flags in (WMODE(4), WMODE(5)) and (win > 40 or Fext > 208):
        return False
    if flags == WMODE(5) and (Fq + (q0 - win) % 16 + 15) // 16 > 13:
        return False
    if flags & TF.FORCE_MASK == WMODE(3) and (Fext * 576 + ((Fext + 31) // 32) * 6144 + 8 * (32 * ((32 + 2 * win + 31) // 32) + 32) * 4 > 163840
                           or Fq + (q0 - win) % 16 > 256):
        return False
    return not (flags == WMODE(1) and Fext > 192)


def attention_call(hip, case, T, Wkn):
    from dawn_pytorch_amd.pack import pack_bf3, pack_bf3_temporal_out, pack_kn
    p, k = case.p, case.kind
    if k in ("temporal", "temporal_seg"):
        Fext, q0 = p["F"], p.get("q0", 0)
        a = (cu(T["x"]), Fext, p["HW"], q0, p.get("Fq", Fext), 40, pack_kn(Wkn["wqkv"]).cuda(), pack_kn(Wkn["wout"]).cuda(), cu(T["rc"]),
             cu(T["rs"]), cu(T["band"]))
        kw = dict(wqkv_bf3=pack_bf3(Wkn["wqkv"]).cuda(), wout_bf3p=pack_bf3_temporal_out(Wkn["wout"]).cuda())
        return (hip.temporal_layer_c64_segmented if k == "temporal_seg" else hip.temporal_layer_c64)(*a, **kw)
    if k == "sla":
        return hip.sla_layer_c64(cu(T["x"]), p["F"], p["HW"], pack_kn(Wkn["wqkv"]).cuda(), pack_kn(Wkn["wout"]).cuda(), cu(T["bias"]),
                                 wqkv_bf3=pack_bf3(Wkn["wqkv"]).cuda())
    return hip.xattn_layer_c64(cu(T["x"]), cu(T["x2"]), p["HW"], pack_kn(Wkn["wq"]).cuda(), [pack_kn(Wkn[f"wo{b}"]).cuda() for b in range(3)],
                               cu(T["g3"]), cu(T["qs"]), cu(T["kvtab"]), cu(T["nulltab"]), wq_bf3=pack_bf3(Wkn["wq"]).cuda())


TEMPORAL_CASES = [c for c in G.CASES if c.kind == "temporal"]


@pytest.mark.parametrize("case", TEMPORAL_CASES, ids=[c.name for c in TEMPORAL_CASES])
def test_temporal_layer_fp64_gate(hip, case):
    """Every kernel family of the fused temporal layer, with both split weight images."""
    T, Wkn, want64, base32 = references(case)
    p = case.p
    ran = []
    try:
        for flags in TEMPORAL_FLAGS:
            if not temporal_fits(flags, p["F"], p.get("q0", 0), p.get("Fq", p["F"])):
                continue
            hip.temporal_flags = flags
            got = attention_call(hip, case, T, Wkn)
            torch.cuda.synchronize()
            G.fp32_gate(f"{case.name}/flags{flags}", got, want64, base32, c=case.c)
            ran.append(flags)
    finally:
        hip.temporal_flags = 0
    assert 0 in ran and len(ran) >= 4, ran           # (at Fext 280 WMODE 1, 3, 4 and 5 do not fit: automatic, WMODE 0, 2 and KEEP_32X32 run)


OTHER_ATTN = [c for c in G.CASES if c.kind in ("temporal_seg", "sla", "xattn")]


@pytest.mark.parametrize("case", OTHER_ATTN, ids=[c.name for c in OTHER_ATTN])
def test_attention_layer_fp64_gate(hip, case):
    """The segmented temporal layer (400 frames), sla_layer_c64 with wqkv_bf3 (sla_c64_apply_bf16_kernel<OUTB = true>, whose third Wq plane
    is fetched a head ahead), and xattn_layer_c64 with wq_bf3."""
    T, Wkn, want64, base32 = references(case)
    got = attention_call(hip, case, T, Wkn)
    torch.cuda.synchronize()
    G.fp32_gate(case.name, got, want64, base32, c=case.c)


# ---------------------------------------------------------------------------------------------- attention cores of the unfused levels
# temporal_attn_flags (dawn_temporal_attn_ex): automatic, the fp32-MFMA kernel, the split-operand EXT core on any grid, the opt-in
# window-tiled 13-wave core
TATTN_FLAGS = (0, TA.FP32, TA.SPLIT_ALWAYS, TA.WAVE13)
TATTN_CASES = [c for c in G.CASES if c.kind == "tattn"]


def attn13_fits(Fext, q0, Fq, win=40):
    """The shapes the 13-wave core covers (the rule of test_hip_ops.test_temporal_attn)."""
    return win <= 40 and Fext <= 208 and (Fq + (q0 - win) % 16 + 15) // 16 <= 13


def core_call(hip, case, T):
    """The fp32-kernel case kinds and tattn on the GPU."""
    p, k = case.p, case.kind
    if k == "tattn":
        return hip.temporal_attn(cu(T["qkv"]), p["F"], p["HW"], p.get("q0", 0), p.get("Fq", p["F"]), 40, cu(T["rc"]), cu(T["rs"]),
                                 cu(T["band"]))
    if k == "sla_unfused":
        return hip.sla(cu(T["qkv"]), p["F"], p["HW"])
    if k == "frame":
        return hip.frame_attn(cu(T["qkv"]), p["F"], p["HW"])
    raise ValueError(k)


@pytest.mark.parametrize("case", TATTN_CASES, ids=[c.name for c in TATTN_CASES])
def test_temporal_attn_fp64_gate(hip, case):
    """HipOps.temporal_attn, every kernel that covers the shape: automatic, fp32 MFMA, the EXT split core, the 13-wave core."""
    T, Wkn, want64, base32 = references(case)
    p = case.p
    ran = []
    try:
        for flags in TATTN_FLAGS:
            if flags == TA.WAVE13 and not attn13_fits(p["F"], p.get("q0", 0), p.get("Fq", p["F"])):
                continue
            hip.temporal_attn_flags = flags
            got = core_call(hip, case, T)
            torch.cuda.synchronize()
            G.fp32_gate(f"{case.name}/flags{flags}", got, want64, base32, c=case.c)
            ran.append(flags)
    finally:
        hip.temporal_attn_flags = 0
    assert ran == ([0, 1, 2, 4] if attn13_fits(p["F"], p.get("q0", 0), p.get("Fq", p["F"])) else [0, 1, 2]), ran


FP32_CASES = [c for c in G.CASES if c.kind in ("sla_unfused", "frame", "xattn_unfused")]


@pytest.mark.parametrize("case", FP32_CASES, ids=[c.name for c in FP32_CASES])
def test_fp32_attention_fp64_gate(hip, case):
    """ops.sla (sla_context_kernel + sla_apply_kernel), ops.frame_attn, and the unfused cross-attention: xattn_tables + xattn_sigma_out
    against the original chain, xattn_core, xattn_ln_sum."""
    from dawn_pytorch_amd.pack import pack_kn
    T, Wkn, want64, base32 = references(case)
    if case.kind == "xattn_unfused":
        p = case.p
        if p["chain"] == "sigma":
            xtab = hip.xattn_tables(cu(T["kvtab"]), cu(T["nulltab"]), cu(T["qs"]), [pack_kn(Wkn[f"wo{b}"]).cuda() for b in range(3)], p["Co"])
            got = hip.xattn_sigma_out(cu(T["q"]), p["HW"], xtab, cu(T["g3"]), p["Co"])
        elif p["chain"] == "core":
            got = hip.xattn_core(cu(T["q"]).clone(), p["HW"], cu(T["kvtab"]), cu(T["nulltab"]), cu(T["qs"]))
        else:
            got = hip.xattn_ln_sum(cu(T["y3"]), cu(T["g3"]), p["Co"])
    else:
        got = core_call(hip, case, T)
    torch.cuda.synchronize()
    G.fp32_gate(case.name, got, want64, base32, c=case.c)


# ---------------------------------------------------------------------------------------------- repeated-run bit identity
def _repeat_equal(name, fn):
    first = fn()
    torch.cuda.synchronize()
    for rep in range(REPEATS - 1):
        again = fn()
        assert torch.equal(again, first), f"{name}: run {rep + 1} differs from run 0 in {int((again != first).sum())} elements"


DET_CONV = [
    G.Case("gemm1x1/tiled_M12800_N768_K512_res", "gemm", form=G.TILED, M=12800, C0=512, N=768, res=True),
    G.Case("gemm1x1/tiled_M51200_N768_K256", "gemm", form=G.TILED, M=51200, C0=256, N=768),
    # Winograd F(4x4): level 0 and level 1 (its deepest: the form needs 32- or 64-pixel rows); F(2x2): level 0 and level 3
    G.Case("wino4/L0_64x64_C64_N64", "conv3", form=G.WINO4, F=50, H=64, C0=64, N=64),
    G.Case("wino4/L1_32x32_C128_N128", "conv3", form=G.WINO4, F=50, H=32, C0=128, N=128),
    G.Case("wino/L0_64x64_C64+64_N64", "conv3", form=G.WINO, F=50, H=64, C0=64, C1=64, N=64),
    G.Case("wino/L3_8x8_C512_N512", "conv3", form=G.WINO, F=200, H=8, C0=512, N=512),
    # configs[1] (128 px): F(2x2) at its level 1 with the skip concatenated, F(4x4)'s 32-wide template at its level 0; the row kernels with the
    # LayerNorm inside on two sources
    G.Case("wino/L1_32x32_C128+128_N64", "conv3", form=G.WINO, F=50, H=32, C0=128, C1=128, N=64),
    G.Case("wino4/L0_32x32_C64_N64", "conv3", form=G.WINO4, F=100, H=32, C0=64, N=64),
    G.Case("gemm1x1/rowreg_M25600_N192_K64+64_ln", "gemm", form=G.ROWREG, M=25600, C0=64, C1=64, N=192, ln=True),
    G.Case("gemm1x1/rowacc_M6400_N192_K512+512_ln", "gemm", form=G.ROWACC, M=6400, C0=512, C1=512, N=192, ln=True),
]


@pytest.mark.parametrize("case", DET_CONV, ids=[c.name for c in DET_CONV])
def test_conv_split_run_to_run_identical(hip, case):
    """Eight launches on the same input in one process: bit-identical (the tiled 1x1 kernel's stage wait and the Winograd kernels' hand-placed
    loads would show a race as run-to-run differences)."""
    T, Wkn = case.make()
    args, kw = conv_call(case, T, Wkn)
    f3, f1 = hip.conv_gemm(*args, **kw, form_only=True)
    assert (f3 if case.kind == "conv3" else f1) == case.form, (case.name, f3, f1)
    _repeat_equal(case.name, lambda: hip.conv_gemm(*args, **kw))


def test_sla_apply_run_to_run_identical(hip):
    """sla_c64_apply_bf16_kernel<true> at production size (200 frames of 16 x 16), eight times: bit-identical."""
    case = G.Case("sla/F200_HW256", "sla", split=("wqkv",), F=200, HW=256)
    T, Wkn = case.make()
    _repeat_equal(case.name, lambda: attention_call(hip, case, T, Wkn))


def test_temporal_attn_ext_core_run_to_run_identical(hip):
    """The automatic attention core of the unfused levels (the EXT form of temporal_layer_c64_bf16_kernel: K / V / Q tiles requested one head
    ahead into pinned registers) at the 32 x 32 level of a 256-px clip, 200 frames: eight runs bit-identical."""
    case = G.Case("tattn/F200_HW1024", "tattn", split=(), F=200, HW=1024)
    T, _ = case.make()
    _repeat_equal(case.name, lambda: core_call(hip, case, T))
