// Shared by the translation units of the conv / GEMM family, nothing else (not part of the C ABI: that is include/dawn_hip.h):
//   conv_gemm.hip      the fp32 kernels, the first split-bf16 3x3 kernel, ALL routing and every extern "C" entry point
//   conv3x3_split.hip  conv3x3_bf16_v2_kernel (the shipped direct 3x3 kernel)
//   gemm1x1_tiled.hip  gemm1x1_bf16_kernel (the tiled split 1x1 GEMM)
//   gemm1x1_rows.hip   gemm1x1_rowreg_kernel / gemm1x1_rowacc_kernel (the row-stationary split GEMMs)
// Only what two or more of them need lives here.  The library links without relocatable device code: no __device__ variable here.
#pragma once
#include "dawn_common.h"
#include "../../include/dawn_hip.h"

// the policy bits are described in conv_gemm.hip
constexpr int DAWN_CONV_POLICY_DEFAULT = 0x2B00580D;
#ifdef DAWN_ABLATION
constexpr int DAWN_CONV_POLICY_MASK = 0x3F0FFFFF;
#else
constexpr int DAWN_CONV_POLICY_MASK = 0x3FF3FFCF;
#endif
static inline int policy_of(const dawn_conv_desc& d) { return (d.policy ? d.policy : DAWN_CONV_POLICY_DEFAULT) & DAWN_CONV_POLICY_MASK; }

// dawn_conv_desc.border (mode 1): where a 2x2 phase tap that falls outside the H x W input reads.  0 leaves the coordinate alone
// (the callers' bounds test then reads zero), 1 clamps it to the edge pixel, 2 wraps it to the opposite edge.  A tap is at most one
// pixel outside, so one conditional step is enough; an in-range coordinate comes back unchanged for every border.
__device__ __forceinline__ int dawn_border_coord(int i, int n, int border) {
    if (border == 1) return i < 0 ? 0 : (i >= n ? n - 1 : i);
    if (border == 2) return i < 0 ? i + n : (i >= n ? i - n : i);
    return i;
}

typedef dawn_bf16x8 bf16x8;

// exact fp32 -> 3 x bf16 operand split (round to nearest even; see conv3x3_halo_bf16_kernel in conv_gemm.hip)
__device__ __forceinline__ void split3(const f32x4 v, uint2& p1, uint2& p2, uint2& p3) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    bf16x4 h1, h2, h3;
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { h1[i] = (__bf16)v[i]; r[i] = v[i] - (float)h1[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { h2[i] = (__bf16)r[i]; r[i] = r[i] - (float)h2[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) h3[i] = (__bf16)r[i];
    p1 = *reinterpret_cast<uint2*>(&h1);
    p2 = *reinterpret_cast<uint2*>(&h2);
    p3 = *reinterpret_cast<uint2*>(&h3);
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
