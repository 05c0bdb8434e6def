// Fused tri-modal cross-attention branch for 64-channel outputs: h_cond = sum_b LN(to_out_b(attn_b(LN(x))))
// in ONE kernel, reading x once and writing h_cond once.
//
// Reference: the three CrossAttention.forward calls of ResnetBlock_ca_mul (MT:454-468 -> MT:516-559):
// LayerNorm_img(x) (gain folded into to_q), to_q (Cin -> 3 x 64), per head (8 x 8) cosine-sim attention over
// the 2 keys [null, frame condition], to_out.0 (64 -> Co), to_out.1 LayerNorm_img, sum of the branches.
//
// Each wave owns 32 pixels; everything is chained in the transposed-GEMM form of temporal_layer.hip, so a lane
// owns ONE pixel and holds feature subsets {8c + 4*(lane>>5) + s}: a head's 8 features are the lane's 4 values
// plus the 4 of its xor-32 partner, an output row's 64 channels are 32 in-lane values plus the partner's 32.
// Hence q-normalisation, the two logits, the 2-way softmax and both LayerNorms are in-register arithmetic with
// single xor-32 exchanges; no LDS traffic for activations (LDS only holds the weights, staged once per block).
//
// Two exact rewrites keep the per-pixel work small (the keys / values depend on (frame, branch, head) only):
//  * softmax over [null, ctx] = sigmoid of ONE dot product: sigma_h = 1 / (1 + exp2(q_h . D_h / |q_h|)),
//    D_h = q_scale * (k_null - k_ctx,h) * 8 log2(e)                                (MT:540-552; table per frame);
//  * to_out of o_h = v_null + sigma_h (v_ctx,h - v_null) is affine in sigma: y = y0 + sum_h sigma_h u_h with
//    u_h = Wo[8h..8h+7]^T (v_ctx,h - v_null), y0 = Wo^T v_null  (MT:553-558) -- a K = 9 product against a per-frame
//    table instead of a K = 64 GEMM, and the 48 KB of to_out weights leave the LDS (2 workgroups per CU).
// dawn_xattn_tables builds [D | u_0..u_7 | y0] per (frame, branch) once per clip (the condition is step-invariant).
#include "dawn_common.h"
#include "../../include/dawn_hip.h"

#ifdef DAWN_XA_TIMING
__device__ unsigned long long* dawn_xa_dbg = nullptr;
extern "C" int dawn_xattn_set_debug(void* p) { return (int)hipMemcpyToSymbol(HIP_SYMBOL(dawn_xa_dbg), &p, sizeof(p)); }
#endif

namespace {

constexpr int CO = 64;

__device__ __forceinline__ float x32(float v) { return v + __shfl_xor(v, 32, 64); }

// SPLIT: to_q -- 87 % of the kernel's matrix work -- on the bf16 pipe with the exact 3-way operand split (6 cross terms, fp32
// accumulate, see conv3x3_halo_bf16_kernel in conv_gemm.hip): the pre-split weight planes (pack_bf3 image, [CIN/16][3][2][192][8]) take the place of the fp32
// weights in LDS (72 / 144 KB), the lane's LayerNorm'ed channels (8 consecutive ones per k-step: B operand, lane = pixel) are
// split once per tile in registers.  144 (288) bf16 MFMAs of 32 cycles instead of 192 (384) fp32 ones of 64 per tile.

template <int CIN, bool SPLIT>
__global__ __launch_bounds__(512, (CIN == 64 && !SPLIT) ? 4 : 2) void xattn_c64_kernel(const float* __restrict__ in0, int C0, int ld0,
                                                        const float* __restrict__ in1, int ld1, long rows, int HW,
                                                        const float* __restrict__ wq, const unsigned short* __restrict__ wq_s,
                                                        const float* __restrict__ g3,
                                                        const float* __restrict__ xtab, float eps,
                                                        float* out, long ntiles, const float* gn_x /* may alias `out` (h1 over c1) */,
                                                        const float* __restrict__ gn_a, const float* __restrict__ gn_b) {
    constexpr int NC = CIN / 8;
    constexpr int WQF = SPLIT ? CIN * 1152 / 4 : (CIN / 4) * 192 * 4;       // floats of LDS taken by the to_q weights
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Wq = smem;                         // fp32: [CIN/4][192][4]; SPLIT: planes [CIN/16][3][2][192] x 16 B
    float* Cs = smem + WQF;                   // g3 [3][64]
    float* Dw = Cs + 192;                     // per-wave copy of the current frame's D rows: [8 waves][3][64]
    const int tid = threadIdx.x;
    for (int i = tid; i < 192; i += 512) Cs[i] = g3[i];
    if (SPLIT) {
        for (int i = tid; i < WQF / 4; i += 512)
            *reinterpret_cast<f32x4*>(Wq + i * 4) = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(wq_s) + (size_t)i * 4);
    } else {
        for (int i = tid; i < (CIN / 4) * 192; i += 512)
            *reinterpret_cast<f32x4*>(Wq + i * 4) = *reinterpret_cast<const f32x4*>(wq + (size_t)i * 4);
    }
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int l31 = lane & 31, half = lane >> 5;
#ifdef DAWN_XA_TIMING
    unsigned long long* tsb = reinterpret_cast<unsigned long long*>(Dw + 8 * 192);  // after the per-wave tables
    int tix = 0, titer = 0;
#define TSTAMP() do { if (lane == 0 && titer == 1 && tix < 24) tsb[wave * 24 + tix++] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define TSTAMP() do { } while (0)
#endif
    // Each wave owns a contiguous range of 32-pixel tiles (same frame for ~all of them: the frame's D rows are copied to LDS
    // only when the frame changes, and the rows stream through HBM in order).  With room in the register file (SPLIT, Cin = 64:
    // two waves per SIMD) the next tile's rows are requested before this tile's work.
    constexpr bool PREF = SPLIT && CIN == 64;
    const long nwaves = (long)gridDim.x * 8;
    const long per = (ntiles + nwaves - 1) / nwaves;
    const long tbeg = ((long)blockIdx.x * 8 + wave) * per;
    const long tend = tbeg + per < ntiles ? tbeg + per : ntiles;
    f32x4 xq[PREF ? NC : 1];
    // rows of a tile through buffer descriptors rebuilt per tile from scalar bases (t is wave-uniform): the per-lane part of
    // an address is a small 32-bit offset, no 64-bit vector arithmetic (rows % 32 == 0: there are no partial tiles)
    auto request = [&](long t, f32x4* dst) {
        const __amdgpu_buffer_rsrc_t r0 = DAWN_BUFFER(in0 + t * 32 * ld0, 32 * ld0 * 4);
        const __amdgpu_buffer_rsrc_t r1 = DAWN_BUFFER(in1 ? in1 + t * 32 * ld1 : in0, 32 * ld1 * 4);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const int cb = SPLIT ? 16 * (c >> 1) + 4 * (c & 1) : 8 * c;          // wave-uniform part of the column
            const int col = cb + (SPLIT ? 8 : 4) * half;
            dst[c] = __builtin_bit_cast(f32x4, cb < C0 ? __builtin_amdgcn_raw_buffer_load_b128(r0, (l31 * ld0 + col) * 4, 0, 0)
                                                       : __builtin_amdgcn_raw_buffer_load_b128(r1, (l31 * ld1 + col - C0) * 4, 0, 0));
        }
    };
    if (PREF && tbeg < tend) request(tbeg, xq);
    long cur_frame = -1;
    for (long t = tbeg; t < tend; ++t) {
        TSTAMP();   // tile start
        // ---- x fragments + LayerNorm (biased variance, eps) in registers.  fp32: quads 8c + 4 half (k = 2s + half of the
        // 32x32x2 MFMA); SPLIT: the 8 consecutive channels 16 kc + 8 half + {0..7} of each 32x32x16 k-step = quads 2kc, 2kc+1
        f32x4 xn[NC];
        if (PREF) {
#pragma unroll
            for (int c = 0; c < NC; ++c) xn[c] = xq[c];
            if (t + 1 < tend) request(t + 1, xq);
        } else {
            request(t, xn);
        }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) s += xn[c].x + xn[c].y + xn[c].z + xn[c].w;
        s = x32(s);
        const float mu = s * (1.0f / CIN);
        float ss = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            xn[c] = xn[c] - mu;
            ss += xn[c].x * xn[c].x + xn[c].y * xn[c].y + xn[c].z * xn[c].z + xn[c].w * xn[c].w;
        }
        ss = x32(ss);
        const float rs = __builtin_amdgcn_rsqf(ss * (1.0f / CIN) + eps);
#pragma unroll
        for (int c = 0; c < NC; ++c) xn[c] = xn[c] * rs;
        bf16x8 xs[SPLIT ? CIN / 16 : 1][3];
        if (SPLIT) {
#pragma unroll
            for (int kc = 0; kc < CIN / 16; ++kc) {
                const float v8[8] = {xn[2 * kc].x, xn[2 * kc].y, xn[2 * kc].z, xn[2 * kc].w,
                                     xn[2 * kc + 1].x, xn[2 * kc + 1].y, xn[2 * kc + 1].z, xn[2 * kc + 1].w};
                dawn_split3_oct(v8, xs[kc][0], xs[kc][1], xs[kc][2]);
            }
        }
        TSTAMP();   // x loaded + LayerNorm

        // the tile's frame (HW % 32 == 0: a 32-pixel tile never straddles frames) and its table [3][D 64 | U 9 x 64]:
        // the D rows go to this wave's LDS copy (no global-load latency in the head loops)
        const long frame = (t * 32) / HW;
        const float* xt = xtab + frame * (3 * 640);
        float* dw = Dw + (tid >> 6) * 192;
        if (frame != cur_frame) {                                  // wave-uniform
            cur_frame = frame;
            if (lane < 48) {
                const int b = lane >> 4, j = (lane & 15) * 4;
                *reinterpret_cast<f32x4*>(dw + b * 64 + j) = *reinterpret_cast<const f32x4*>(xt + b * 640 + j);
            }
        }
        f32x16 hc[2];
        hc[0] = zero16();
        hc[1] = zero16();
#pragma unroll 1
        for (int b = 0; b < 3; ++b) {
            // rows u_0..u_7, y0 of this (frame, branch) as MFMA A operands (k = 2s + half; row 8 = y0 pairs with a constant
            // 1, the odd half of that step multiplies a finite value by 0): requested now, consumed after the heads
            float ua[2][5];
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int s2 = 0; s2 < 5; ++s2)
                    ua[ot][s2] = xt[b * 640 + 64 + (s2 < 4 ? 2 * s2 + half : 8) * CO + 32 * ot + l31];
            float bs[4];                              // B operand of step s: sigma of head 2s + half
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                // ---- Q^T tile: features 64b + 32tt + {0..31}
                f32x16 acc = zero16();
                if (SPLIT) {
                    const unsigned char* Wp = reinterpret_cast<const unsigned char*>(Wq);
#pragma unroll
                    for (int kc = 0; kc < CIN / 16; ++kc) {
                        bf16x8 wa[3];
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl)
                            wa[pl] = *reinterpret_cast<const bf16x8*>(Wp + ((size_t)(((kc * 3 + pl) * 2 + half) * 192 + 64 * b + 32 * tt + l31)) * 16);
#pragma unroll
                        for (int u = 0; u < 6; ++u)
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wa[DAWN_SPLIT6_A[u]], xs[kc][DAWN_SPLIT6_B[u]], acc, 0, 0, 0);
                    }
                } else {
                // weight fragments requested PF at a time ahead of their MFMAs (all 16 for CIN = 128 with its 256-register
                // budget; 4 for CIN = 64, which runs 4 waves per SIMD on 128 registers)
                constexpr int PF = CIN == 64 ? 4 : NC;
#pragma unroll
                for (int c0 = 0; c0 < NC; c0 += PF) {
                    f32x4 wq4[PF];
#pragma unroll
                    for (int c = 0; c < PF; ++c)
                        wq4[c] = *reinterpret_cast<const f32x4*>(Wq + ((2 * (c0 + c) + half) * 192 + 64 * b + 32 * tt + l31) * 4);
#pragma unroll
                    for (int c = 0; c < PF; ++c) {
#pragma unroll
                        for (int s2 = 0; s2 < 4; ++s2)
                            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wq4[c][s2], xn[c0 + c][s2], acc, 0, 0, 0);
                    }
                }
                }
                // ---- 2-key cosine-sim attention per head (head = 4tt + c4; lane holds features 4half..4half+3)
#pragma unroll
                for (int c4 = 0; c4 < 4; ++c4) {
                    const int hd = 4 * tt + c4;
                    const float q0 = acc[4 * c4], q1 = acc[4 * c4 + 1], q2 = acc[4 * c4 + 2], q3 = acc[4 * c4 + 3];
                    const f32x4 d4 = *reinterpret_cast<const f32x4*>(dw + b * 64 + hd * 8 + 4 * half);
                    const float n2 = x32(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
                    const float dd = x32(q0 * d4.x + q1 * d4.y + q2 * d4.z + q3 * d4.w);
                    const float inv = __builtin_amdgcn_rsqf(fmaxf(n2, 1e-24f));        // 1 / max(|q|, 1e-12)  (F.normalize)
                    // softmax over the 2 keys [null, condition] in closed form: weight of the condition key =
                    // sigmoid(8 (s_ctx - s_null)) = 1 / (1 + 2^(q.D/|q|)); one v_exp_f32 + one v_rcp_f32 (1 ulp each)
                    const float sg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(dd * inv));
                    if ((hd & 1) == 0) bs[hd >> 1] = sg;                  // (both halves hold every head's sigma)
                    else bs[hd >> 1] = half ? sg : bs[hd >> 1];
                }
                TSTAMP();   // Q tile tt + its 4 heads
            }
            // ---- y^T (64 co x 32 px) = [u_0 .. u_7 | y0]^T . [sigma_0 .. sigma_7 | 1]^T, then LayerNorm over co and
            // accumulate with gain g3[b]
            f32x16 yT[2];
#pragma unroll
            for (int ot = 0; ot < 2; ++ot) {
                f32x16 acc = zero16();
#pragma unroll
                for (int s2 = 0; s2 < 4; ++s2)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[ot][s2], bs[s2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ua[ot][4], half ? 0.0f : 1.0f, acc, 0, 0, 0);
                yT[ot] = acc;
            }
            TSTAMP();   // to_out MFMAs issued
            float ys = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) ys += yT[0][r] + yT[1][r];
            ys = x32(ys);
            const float ym = ys * (1.0f / CO);
            float yv = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float d0 = yT[0][r] - ym, d1 = yT[1][r] - ym;
                yv += d0 * d0 + d1 * d1;
            }
            yv = x32(yv);
            const float yr = __builtin_amdgcn_rsqf(yv * (1.0f / CO) + eps);
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const f32x4 g4 = *reinterpret_cast<const f32x4*>(Cs + b * CO + 32 * ot + 8 * g + 4 * half);
#pragma unroll
                    for (int j = 0; j < 4; ++j) hc[ot][4 * g + j] += (yT[ot][4 * g + j] - ym) * yr * g4[j];
                }
            TSTAMP();   // branch LayerNorm + accumulate
        }
        {
            const __amdgpu_buffer_rsrc_t ro = DAWN_BUFFER(out + t * 32 * CO, 32 * CO * 4);
            // optional: the block's h1 = SiLU(FiLM(GroupNorm(c1))) + h_cond (MT:473-476) straight from this epilogue -- gn_x = c1 rows,
            // (gn_a, gn_b) = the per-channel coefficients of dawn_gn_finalize: no h_cond tensor, no separate GroupNorm-apply pass
            const __amdgpu_buffer_rsrc_t rg = DAWN_BUFFER((gn_x ? gn_x : out) + t * 32 * CO, 32 * CO * 4);
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v = {hc[ot][4 * g], hc[ot][4 * g + 1], hc[ot][4 * g + 2], hc[ot][4 * g + 3]};
                    if (gn_x) {
                        const int cch = 32 * ot + 8 * g + 4 * half;
                        const f32x4 c4 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rg, (l31 * CO + cch) * 4, 0, 0));
                        const f32x4 a4 = *reinterpret_cast<const f32x4*>(gn_a + cch), b4 = *reinterpret_cast<const f32x4*>(gn_b + cch);
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = dawn_silu(c4[j] * a4[j] + b4[j]) + v[j];
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, v), ro,
                                                           (l31 * CO + 32 * ot + 8 * g + 4 * half) * 4, 0, 0);
                }
        }
        TSTAMP();   // stored
#ifdef DAWN_XA_TIMING
        ++titer;
#endif
    }
#ifdef DAWN_XA_TIMING
    if (lane == 0 && blockIdx.x < 256)
        for (int i = 0; i < 24; ++i) dawn_xa_dbg[((size_t)blockIdx.x * 8 + wave) * 24 + i] = i < tix ? tsb[wave * 24 + i] : 0ull;
#endif
}

// Per-clip tables of one conditioned block (see the header): xtab[f][b] = [D (8 heads x 8) | u_0 .. u_7 (Co each) | y0 (Co)].
// kvtab[f][b] = [k_ctx (l2-normalised * k_scale) 64 | v_ctx 64], nulltab[b] = [k_null 8 | v_null 8] (dawn_xattn_prep);
// wo_b packed [16][Co][4] (k = 8 h + i).  One block per (frame, branch); thread per table entry.
__global__ __launch_bounds__(256) void xattn_tables_kernel(const float* __restrict__ kvtab, const float* __restrict__ nulltab,
                                                           const float* __restrict__ q_scale, const float* __restrict__ wo0,
                                                           const float* __restrict__ wo1, const float* __restrict__ wo2,
                                                           int Co, float* __restrict__ xtab) {
    const int f = blockIdx.x / 3, b = blockIdx.x - 3 * f;
    const float* kv = kvtab + ((long)f * 3 + b) * 128;
    const float* nt = nulltab + b * 16;
    const float* wo = b == 0 ? wo0 : (b == 1 ? wo1 : wo2);
    const int W = 64 + 9 * Co;
    float* o = xtab + ((long)f * 3 + b) * W;
    for (int e = threadIdx.x; e < W; e += 256) {
        float v;
        if (e < 64) {
            const int i = e & 7;
            v = q_scale[b * 8 + i] * (nt[i] - kv[e]) * (8.0f * 1.4426950408889634f);
        } else {
            const int r = (e - 64) / Co, co = (e - 64) - r * Co;
            double a = 0.0;
            if (r < 8) {
                for (int i = 0; i < 8; ++i) {
                    const int k = 8 * r + i;
                    a += (double)wo[((k >> 2) * Co + co) * 4 + (k & 3)] * (double)(kv[64 + k] - nt[8 + i]);
                }
            } else {
                for (int k = 0; k < 64; ++k) a += (double)wo[((k >> 2) * Co + co) * 4 + (k & 3)] * (double)nt[8 + (k & 7)];
            }
            v = (float)a;
        }
        o[e] = v;
    }
}

}  // namespace

extern "C" int dawn_xattn_tables(const float* kvtab, const float* nulltab, const float* q_scale, const float* wo0,
                                 const float* wo1, const float* wo2, int F, int Co, float* xtab, void* stream) {
    if (F <= 0) return 0;
    hipLaunchKernelGGL(xattn_tables_kernel, dim3(3 * F), dim3(256), 0, (hipStream_t)stream, kvtab, nulltab, q_scale, wo0, wo1,
                       wo2, Co, xtab);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_xattn_layer_c64_h1(const float* in0, int C0, int ld0, const float* in1, int C1, int ld1, long rows,
                                       int HW, const float* wq, const void* wq_bf3, const float* g3, const float* xtab, float eps,
                                       const float* gn_x, const float* gn_a, const float* gn_b, float* out, void* stream) {
    const int Cin = C0 + C1;
    if (gn_x && (!gn_a || !gn_b)) return dawn_set_error_msg(-54, "dawn_xattn_layer_c64_h1: gn_x needs gn_a and gn_b");
    if ((Cin != 64 && Cin != 128) || C0 % 8 != 0 || (ld0 % 4) || (in1 && (ld1 % 4)))
        return dawn_set_error_msg(-51, "dawn_xattn_layer_c64: Cin must be 64 or 128 (two sources allowed), Co = 64");
    if (HW % 32 != 0 || rows % 32 != 0)
        return dawn_set_error_msg(-52, "dawn_xattn_layer_c64: H*W must be a multiple of 32 (a 32-pixel tile lies in one frame)");
    if (rows <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const long ntiles = rows / 32;
    long grid = (ntiles + 7) / 8;
    const bool split = wq_bf3 != nullptr && C0 % 16 == 0;
    // resident blocks: fp32 weights 2 per CU at 56 KB of LDS (Cin = 64), 1 at 105 KB; split planes 2 per CU at 79 KB, 1 at 151 KB
    // the split kernels run two 256-register waves per SIMD: a CU holding one of their persistent workgroups has no registers
    // left for anybody else, and the one-block GroupNorm reduction of the OTHER stream (on the critical path of every ResBlock)
    // waited for a whole cross-attention launch to drain (23 us average instead of 5).  Eight CUs stay out of the persistent grid.
    const long cap = (Cin == 64 && !split) ? 512 : 248;
    if (grid > cap) grid = cap;
    int lds = ((split ? Cin * 1152 / 4 : (Cin / 4) * 192 * 4) + 192 + 8 * 192) * 4;
#ifdef DAWN_XA_TIMING
    lds += 8 * 24 * 8;
#endif
#define LAUNCH_XA(CINV, SPV)                                                                                                 \
    do {                                                                                                                     \
        (void)hipFuncSetAttribute((const void*)xattn_c64_kernel<CINV, SPV>, hipFuncAttributeMaxDynamicSharedMemorySize, lds); \
        hipLaunchKernelGGL((xattn_c64_kernel<CINV, SPV>), dim3((unsigned)grid), dim3(512), lds, s, in0, C0, ld0, in1, ld1, rows, \
                           HW, wq, (const unsigned short*)wq_bf3, g3, xtab, eps, out, ntiles, gn_x, gn_a, gn_b);            \
    } while (0)
    if (Cin == 64) { if (split) LAUNCH_XA(64, true); else LAUNCH_XA(64, false); }
    else { if (split) LAUNCH_XA(128, true); else LAUNCH_XA(128, false); }
#undef LAUNCH_XA
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_xattn_layer_c64(const float* in0, int C0, int ld0, const float* in1, int C1, int ld1, long rows,
                                    int HW, const float* wq, const void* wq_bf3, const float* g3, const float* xtab, float eps,
                                    float* out, void* stream) {
    return dawn_xattn_layer_c64_h1(in0, C0, ld0, in1, C1, ld1, rows, HW, wq, wq_bf3, g3, xtab, eps, nullptr, nullptr, nullptr, out, stream);
}
