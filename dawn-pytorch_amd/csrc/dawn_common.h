// Common device helpers for the DAWN gfx950 kernels (wave64, CDNA4).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define DAWN_WAVE 64

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 dawn_bf16x8 __attribute__((ext_vector_type(8)));    // one bf16 MFMA operand fragment ...
typedef dawn_bf16x8 bf16x8;                                        // ... and its spelling inside the kernels

#define DAWN_LAUNCH_CHECK()                                   \
    do {                                                      \
        hipError_t e__ = hipGetLastError();                   \
        if (e__ != hipSuccess) return dawn_set_error(e__, __FILE__, __LINE__); \
    } while (0)

extern "C" int dawn_set_error(hipError_t e, const char* file, int line);
extern "C" int dawn_set_error_msg(int code, const char* msg);

__device__ __forceinline__ float dawn_silu(float x) { return x / (1.0f + __expf(-x)); }

// xor-shuffle reductions over the low `width` lanes groups (width power of two <= 64)
__device__ __forceinline__ float wave_sum(float v, int width = 64) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        if (o < width) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v, int width = 64) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        if (o < width) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum over the 16 lanes of a DPP row, result in every lane, as four v_add_f32_dpp (quad xor 1, quad xor 2, half-row mirror,
// row mirror): same pairing tree as the xor butterfly (bit-identical), without its ds_bpermute round trips.
__device__ __forceinline__ float row16_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

__device__ __forceinline__ f32x4 zero4() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}

// Buffer descriptor over `bytes` bytes at p: stride 0 (raw, offsets are bytes), reads past the end return 0 and writes are dropped.
// A macro: as an inlined function the builtin lands elsewhere in the caller's IR and the register allocation of some kernels moves.
constexpr int DAWN_BUFFER_FLAGS = 0x00020000;      // descriptor word 3: DATA_FORMAT (bits 15..18) = 4, a 32-bit element; every other field 0
#define DAWN_BUFFER(p, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(p), 0, (bytes), DAWN_BUFFER_FLAGS)

static inline int dawn_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- exact fp32 -> 3 x bf16 operand split shared by the split-operand (bf16 matrix pipe) kernels.  Two schemes, both with
// p1 + p2 + p3 == x bit for bit (tests/split_gate.py: trunc_planes3 and planes3); a kernel picks one by name and never spells it out.

// Truncation split of a PAIR of fp32 values into three words of two bf16 each ([hi16(a) | hi16(b) << 16]): p1 = the upper 16 bits
// of x (a valid bf16: truncation instead of round-to-nearest), r = x - p1 (exact), p2 = the upper 16 bits of r, p3 = r - p2 (exact,
// <= 8 significant bits left, so it IS a bf16).  The instruction mix is the cheap one on gfx950 (tools/ubench/valu_rate.hip: v_and /
// v_sub issue at ~2.4 cycles with two waves per SIMD, v_cvt_pk_bf16_f32 / v_lshlrev / v_perm at ~4.3): per pair of values
// 4 v_and + 4 v_sub + 3 v_perm.
__device__ __forceinline__ void dawn_split3_trunc_pair(const float a, const float b, unsigned& q1, unsigned& q2, unsigned& q3) {
    const unsigned a1 = __float_as_uint(a) & 0xffff0000u, b1 = __float_as_uint(b) & 0xffff0000u;
    const float ra = a - __uint_as_float(a1), rb = b - __uint_as_float(b1);
    const unsigned a2 = __float_as_uint(ra) & 0xffff0000u, b2 = __float_as_uint(rb) & 0xffff0000u;
    const float sa = ra - __uint_as_float(a2), sb = rb - __uint_as_float(b2);
    q1 = __builtin_amdgcn_perm(b1, a1, 0x07060302u);
    q2 = __builtin_amdgcn_perm(b2, a2, 0x07060302u);
    q3 = __builtin_amdgcn_perm(__float_as_uint(sb), __float_as_uint(sa), 0x07060302u);
}
// ... of four values into three bf16 quads (as a loop: two straight-line calls change the register allocation of the callers)
__device__ __forceinline__ void dawn_split3_trunc_quad(const f32x4 v, uint2& p1, uint2& p2, uint2& p3) {
    unsigned q1[2], q2[2], q3[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) dawn_split3_trunc_pair(v[2 * i], v[2 * i + 1], q1[i], q2[i], q3[i]);
    p1 = uint2{q1[0], q1[1]};
    p2 = uint2{q2[0], q2[1]};
    p3 = uint2{q3[0], q3[1]};
}
// ... of eight values into three bf16x8 MFMA fragments
__device__ __forceinline__ void dawn_split3_oct(const float (&v)[8], dawn_bf16x8& p1, dawn_bf16x8& p2, dawn_bf16x8& p3) {
    unsigned q1[4], q2[4], q3[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) dawn_split3_trunc_pair(v[2 * i], v[2 * i + 1], q1[i], q2[i], q3[i]);
    p1 = __builtin_bit_cast(dawn_bf16x8, u32x4{q1[0], q1[1], q1[2], q1[3]});
    p2 = __builtin_bit_cast(dawn_bf16x8, u32x4{q2[0], q2[1], q2[2], q2[3]});
    p3 = __builtin_bit_cast(dawn_bf16x8, u32x4{q3[0], q3[1], q3[2], q3[3]});
}

// Round-to-nearest-even split of four values into three bf16 quads (see conv3x3_halo_bf16_kernel in conv_gemm.hip).  The 16 x 16
// and the 32 x 32 temporal kernels (temporal_layer16.hip, temporal_layer.hip) must build identical X planes from the same
// LayerNorm rows: both call this.
__device__ __forceinline__ void dawn_split3_rne_quad(const f32x4 v, uint2& p1, uint2& p2, uint2& p3) {
    typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
    bf16x4 h1, h2, h3;
    f32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) { h1[i] = (__bf16)v[i]; r[i] = v[i] - (float)h1[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { h2[i] = (__bf16)r[i]; r[i] = r[i] - (float)h2[i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) h3[i] = (__bf16)r[i];
    p1 = __builtin_bit_cast(uint2, h1);
    p2 = __builtin_bit_cast(uint2, h2);
    p3 = __builtin_bit_cast(uint2, h3);
}

// The cross terms a_i . b_j of two split operands, smallest first, so that the fp32 accumulator takes the small products before
// the large one swamps them: term t multiplies plane DAWN_SPLIT6_A[t] of one operand by plane DAWN_SPLIT6_B[t] of the other.
// Six terms, (a3 b1) (a1 b3) (a2 b2) (a2 b1) (a1 b2) (a1 b1), drop everything below 2^-24 of the product; nine keep all.
// Index the tables directly at the use site: a local reference to them changes the register allocation of the callers.
constexpr int DAWN_SPLIT6_A[6] = {2, 0, 1, 1, 0, 0}, DAWN_SPLIT6_B[6] = {0, 2, 1, 0, 1, 0};
constexpr int DAWN_SPLIT9_A[9] = {2, 2, 1, 2, 0, 1, 1, 0, 0}, DAWN_SPLIT9_B[9] = {2, 1, 2, 0, 2, 1, 0, 1, 0};
