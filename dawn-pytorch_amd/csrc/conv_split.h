// Shared by the translation units of the conv / GEMM family, nothing else (not part of the C ABI: that is include/dawn_hip.h):
//   conv_gemm.hip      the fp32 kernels, the first split-bf16 3x3 kernel, ALL routing and every extern "C" entry point
//   conv3x3_split.hip  conv3x3_bf16_v2_kernel (the shipped direct 3x3 kernel)
//   gemm1x1_tiled.hip  gemm1x1_bf16_kernel (the tiled split 1x1 GEMM)
//   gemm1x1_rows.hip   gemm1x1_rowreg_kernel / gemm1x1_rowacc_kernel (the row-stationary split GEMMs)
// Only what two or more of them need lives here: the policy bits, the border rule and the host functions that cross the units.  The
// operand splits (dawn_split3_rne_quad for the activations of these kernels), the cross-term orders and the vector types are
// dawn_common.h's, shared with the attention kernels.  The library links without relocatable device code: no __device__ variable here.
#pragma once
#include "dawn_common.h"
#include "../../include/dawn_hip.h"

// dawn_conv_desc.policy: the bits are the DAWN_POLICY_* table of include/dawn_hip.h; the library reads them through the functions
// below and nowhere as a number.  A build honours the bits of its mask, policy_of() drops the rest.
constexpr int DAWN_CONV_POLICY_MASK_COMMON =
    DAWN_POLICY_BK32 | DAWN_POLICY_TILE256 | DAWN_POLICY_XCD_ORDER | DAWN_POLICY_GLDS | DAWN_POLICY_SK_PRIO_ALT | DAWN_POLICY_GLDS_BK32 |
    DAWN_POLICY_GLDS_STAGES3 | DAWN_POLICY_GLDS_TILE256 | DAWN_POLICY_GLDS_NO_TILE256 | DAWN_POLICY_HALO | DAWN_POLICY_SPLIT |
    DAWN_POLICY_NINE_TERMS | DAWN_POLICY_SPLIT_V2 | DAWN_POLICY_TILE128_ALWAYS | DAWN_POLICY_TILE128_NEVER | DAWN_POLICY_NO_ROW_KERNELS |
    DAWN_POLICY_MFMA_K32 | DAWN_POLICY_WINO2 | DAWN_POLICY_WINO2_DEEP_ONLY | DAWN_POLICY_WINO4 | DAWN_POLICY_WINO4_ALL_SHAPES |
    DAWN_POLICY_WINO_REVERSE;
constexpr int DAWN_CONV_POLICY_MASK_SHIPPED = DAWN_CONV_POLICY_MASK_COMMON | DAWN_POLICY_STAGGER_MASK;
// the whole variant field (TILE128_NEVER, TILED_ONLY and XCD_LAUNCH_ORDER lie inside it: the overlap the table states) and the
// fp32 ablations, without the stagger field
constexpr int DAWN_CONV_POLICY_MASK_ABLATION =
    DAWN_CONV_POLICY_MASK_COMMON | DAWN_POLICY_VARIANT_MASK | DAWN_POLICY_ABL_NO_RESTAGE | DAWN_POLICY_ABL_NO_BARRIER;
#ifdef DAWN_ABLATION
constexpr int DAWN_CONV_POLICY_MASK = DAWN_CONV_POLICY_MASK_ABLATION;
#else
constexpr int DAWN_CONV_POLICY_MASK = DAWN_CONV_POLICY_MASK_SHIPPED;
#endif
static_assert(DAWN_CONV_POLICY_DEFAULT == 0x2B00580D, "the shipped policy moved");
static_assert(DAWN_CONV_POLICY_MASK_SHIPPED == 0x3FF3FFCF && DAWN_CONV_POLICY_MASK_ABLATION == 0x3F0FFFFF, "a policy mask moved");
static_assert((DAWN_CONV_POLICY_DEFAULT & ~DAWN_CONV_POLICY_MASK_SHIPPED) == 0, "the shipped policy has a bit the shipped library drops");
static inline int policy_of(const dawn_conv_desc& d) { return (d.policy ? d.policy : DAWN_CONV_POLICY_DEFAULT) & DAWN_CONV_POLICY_MASK; }
static inline int policy_variant(const dawn_conv_desc& d) { return (policy_of(d) & DAWN_POLICY_VARIANT_MASK) / DAWN_POLICY_VARIANT(1); }
static inline int policy_stagger(int policy) { return (policy & DAWN_POLICY_STAGGER_MASK) / DAWN_POLICY_STAGGER(1); }
// DAWN_POLICY_XCD_LAUNCH_ORDER and DAWN_POLICY_ABL_ROW_FETCH lie outside both masks and are read from the descriptor as the caller
// wrote it: no default, no mask (a kernel may call this).  Moving them into policy_of() would change which builds honour them.
__host__ __device__ static inline bool policy_raw_bit(const dawn_conv_desc& d, int bit) { return (d.policy & bit) != 0; }

// dawn_conv_desc.border (mode 1): where a 2x2 phase tap that falls outside the H x W input reads.  0 leaves the coordinate alone
// (the callers' bounds test then reads zero), 1 clamps it to the edge pixel, 2 wraps it to the opposite edge.  A tap is at most one
// pixel outside, so one conditional step is enough; an in-range coordinate comes back unchanged for every border.
__device__ __forceinline__ int dawn_border_coord(int i, int n, int border) {
    if (border == 1) return i < 0 ? 0 : (i >= n ? n - 1 : i);
    if (border == 2) return i < 0 ? i + n : (i >= n ? i - n : i);
    return i;
}

// ---- host functions that cross the units.  The router (dawn_conv_gemm, conv_gemm.hip) decides; these launch what it chose.
// (hidden visibility: they add nothing to the library's exported symbols)
#pragma GCC visibility push(hidden)
int dawn_ncu();                                            // CUs of the current device (conv_gemm.hip)
int gemm1x1_split_plan(long M, int N, int C0, int C1);     // tile plan of the tiled split 1x1 GEMM (conv_gemm.hip)
// conv3x3_bf16_v2_kernel with 256 x 64 (narrow) or 256 x 128 tiles; false when the geometry does not fit (conv3x3_split.hip)
// dry: decide only -- the answer of the launch's own geometry checks, before any hipFuncSetAttribute, launch or write to *d.gn_rows
bool dawn_conv3x3_v2_try(const dawn_conv_desc& d, long M, hipStream_t s, bool nine, bool narrow, bool dry);
void dawn_gemm1x1_tiled_launch(const dawn_conv_desc& d, long M, hipStream_t s);              // gemm1x1_tiled.hip
void dawn_gemm1x1_rowreg_launch(const dawn_conv_desc& d, long M, hipStream_t s);             // gemm1x1_rows.hip
// mode 0: 1x1 projection, 1: 4x4 / stride-2 Downsample, 2: transposed 4x4 Upsample as four phases (gemm1x1_rows.hip)
void dawn_gemm1x1_rowacc_launch(const dawn_conv_desc& d, long M, int mode, hipStream_t s);
#pragma GCC visibility pop
