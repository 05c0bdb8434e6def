"""Names of the kernel-selection bits: dawn_conv_desc.policy (HipOps.conv_policy, ctx.OPT_CONV_POLICY) and the flags of
dawn_temporal_layer_c64_ex (HipOps.temporal_flags, ctx.OPT_TEMPORAL_FLAGS) and dawn_temporal_attn_ex (HipOps.temporal_attn_flags).

The table -- what each bit selects, whether the shipped library honours it, what measured it -- is the DAWN_POLICY_* / DAWN_TL_* /
DAWN_TA_* block of include/dawn_hip.h; a member here is the header name minus its prefix, and tests/test_cabi_cpu.py holds the two
equal.  Members are ints: everything that takes a policy or flags word takes them, or any other integer, as before."""
from enum import IntFlag


class ConvPolicy(IntFlag):
    BK32 = 0x1
    TILE256 = 0x2
    XCD_ORDER = 0x4
    GLDS = 0x8
    ABL_NO_RESTAGE = 0x10
    ABL_NO_BARRIER = 0x20
    SK_PRIO_ALT = 0x40
    GLDS_BK32 = 0x80
    GLDS_STAGES3 = 0x100
    GLDS_TILE256 = 0x200
    SK_NO_PAIR_OFFSET = 0x200      # (same bit, in the stream-K build)
    GLDS_NO_TILE256 = 0x400
    STREAMK = 0x400                # (same bit, in the stream-K build)
    HALO = 0x800
    SPLIT = 0x1000
    NINE_TERMS = 0x2000
    SPLIT_V2 = 0x4000
    TILE128_ALWAYS = 0x8000
    TILE128_NEVER = 0x10000
    NO_ROW_KERNELS = 0x20000
    XCD_LAUNCH_ORDER = 0x80000
    VARIANT_MASK = 0xF0000
    STAGGER_MASK = 0xF00000
    MFMA_K32 = 0x1000000
    WINO2 = 0x2000000
    WINO2_DEEP_ONLY = 0x4000000
    WINO4 = 0x8000000
    WINO4_ALL_SHAPES = 0x10000000
    WINO_REVERSE = 0x20000000
    ABL_ROW_FETCH = 0x40000000

    # ---- compositions that tests and tools name again and again (not in the header, except DEFAULT = DAWN_CONV_POLICY_DEFAULT)
    FP32_TILES = BK32 | XCD_ORDER | GLDS                    # 0xD: the fp32 kernels' part of the shipped policy
    EXACT_FP32 = FP32_TILES | HALO                          # 0x80D: fp32 MFMA everywhere -- the exact family, the accuracy yardstick
    HALO_V1 = EXACT_FP32 | SPLIT                            # 0x180D: split-operand v1 halo kernel, six cross terms
    HALO_V1_NINE = HALO_V1 | NINE_TERMS                     # 0x380D: ... nine cross terms
    DIRECT_V2 = HALO_V1 | SPLIT_V2                          # 0x580D: direct split v2 kernel, six cross terms, 32x32x16 MFMA
    DIRECT_V2_NINE = DIRECT_V2 | NINE_TERMS                 # 0x780D: ... nine cross terms
    DIRECT_V2_K32 = DIRECT_V2 | MFMA_K32                    # 0x100580D: ... six terms on the 16x16x32 MFMA (the shipped direct kernel)
    DIRECT_V2_TILE128 = DIRECT_V2 | TILE128_ALWAYS          # 0xD80D: ... with 128 x 64 tiles for every eligible split 1x1 GEMM
    WINO = DIRECT_V2_K32 | WINO2                            # 0x300580D: + the Winograd F(2x2,3x3) form where w_wino is supplied
    WINO4_EVERYWHERE = WINO | WINO4 | WINO4_ALL_SHAPES      # 0x1B00580D: + the F(4x4,3x3) form wherever its geometry fits
    DEFAULT = WINO | WINO4 | WINO_REVERSE                   # 0x2B00580D: the shipped policy (what policy 0 means)
    TILED_ONLY = DEFAULT | NO_ROW_KERNELS                   # 0x2B02580D: shipped, but the tiled kernel for every split 1x1 shape

    @classmethod
    def variant(cls, n):
        """DAWN_POLICY_VARIANT(n): value n of the variant field (ablation / stream-K builds only)."""
        return cls(n << 16)

    @classmethod
    def stagger(cls, n):
        """DAWN_POLICY_STAGGER(n): value n of the stagger field."""
        return cls(n << 20)


class TemporalFlags(IntFlag):
    FORCE_MASK = 7
    SCHED_HINTS = 16
    OUT_FP32 = 32
    NO_FIXED200 = 64
    NO_KVI = 128
    KEEP_32X32 = 256

    @classmethod
    def force_wmode(cls, m):
        """DAWN_TL_FORCE_WMODE(m): the value of the force field that forces WMODE m (0 in the field = automatic)."""
        return cls(m + 1)


class TemporalAttnFlags(IntFlag):
    FP32 = 1
    SPLIT_ALWAYS = 2
    WAVE13 = 4
    PIXEL_HEAD_MAJOR = 16
