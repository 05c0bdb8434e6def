// The router of every convolution / linear projection (dawn_conv_gemm and the other extern "C" entry points of the family), the
// implicit-GEMM kernels on the fp32 MFMA (v_mfma_f32_32x32x2_f32) and the first split-bf16 3x3 kernel, gfx950.
//
//   out[row][n] = bias[n] + sum_{tap,c} P(in[pixel(row)+tap][c]) * W[tap][c][n] (+ epilogue terms)
//
// Replaces (reference file:line, MT = ...ca_multi_test.py): Block.proj Conv3d(1,3,3) MT:229, res_conv
// MT:417, Downsample MT:176, Upsample ConvTranspose3d MT:167, init_conv (fea part) MT:776, and all
// Linear / 1x1 projections MT:505,512,608,609,662,663 -- with the LayerNorm (row statistics) that precedes
// them fused into the A-operand loader and bias / residual / "silu(gn(.))" terms fused into the epilogue.
//
// This file: conv_gemm_kernel, conv_gemm_glds_kernel, conv3x3_halo_kernel (fp32), conv3x3_halo_bf16_kernel, their launchers, then
// ALL routing: the predicates that say which kernel serves a descriptor and dawn_conv_gemm, which launches what they answer.  The
// split-operand kernels the shipped policy routes to live in translation units of their own, reached through the plain host functions
// of conv_split.h (as the Winograd forms are through dawn_conv3x3_wino_try): conv3x3_split.hip (conv3x3_bf16_v2_kernel),
// gemm1x1_tiled.hip (gemm1x1_bf16_kernel), gemm1x1_rows.hip (gemm1x1_rowreg_kernel, gemm1x1_rowacc_kernel).
//
// Tiling of the fp32 kernel: BM x BN block tile, 4 waves (WM x WN), each wave TM x TN tiles of 32x32, K-chunks of BK.
// Activations are channels-last so a K-chunk (one tap, BK channels of one pixel) is BK*4 contiguous bytes.
// LDS A image [row][BK+4] (pad -> conflict-free ds_read_b128), B image [k/4][n][4] (weights are pre-packed
// in exactly that order, so the B stage is a linear copy).  The MFMA k index is a free permutation:
// lanes 0-31 feed k = {0..3}, lanes 32-63 feed k = {4..7} of each 8-wide k group, so every lane reads ONE
// float4 per operand tile for four MFMAs.  Workgroups are remapped so that each XCD (private L2) walks a
// contiguous range of M tiles: the +-1 row halos of a 3x3 conv then hit in that XCD's L2.
#include <algorithm>

#include "conv_split.h"

namespace {

// Which kernel runs is decided per call by dawn_conv_desc.policy (0 = the shipped default; no process-global tuning state): the DAWN_POLICY_*
// table of include/dawn_hip.h, read through policy_of() and its companions in conv_split.h (measurements beyond the table's line: DESIGN.md).

struct RowInfo {
    long rowoff;  // (f*Hi + yb)*Wi + xb : input pixel index of tap (0,0) (may point outside; bounds via yb/xb)
    int yb, xb;
    bool valid;
};

// PRO: 0 = no prologue, 1 = per-pixel (mean, rstd) only, 2 = generic (row stats / channel affine / SiLU / add).
// The prologue is applied when the chunk is written to LDS (after the MFMA burst), never right after the
// global load: the loads of chunk c+1 stay in flight behind the MFMAs of chunk c.
template <int BM, int BN, int BK, int WM, int WN, int PRO, int ABL = 0>
__global__ __launch_bounds__(256) void conv_gemm_kernel(const dawn_conv_desc d, const int xcd_remap) {
    constexpr int LDA = BK + 4;
    constexpr int WTM = BM / WM, WTN = BN / WN;   // wave tile
    constexpr int TM = WTM / 32, TN = WTN / 32;
    constexpr int TPR = BK / 4;                   // threads (float4) per A row
    constexpr int RPT = BM * TPR / 256;           // A rows per thread
    constexpr int RSTEP = 256 / TPR;
    constexpr int NB4 = BN * (BK / 4) / 256;      // B float4 per thread per chunk
    constexpr int KQ = BK / 4;
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1 && RPT >= 1 && NB4 >= 1, "bad tile config");

    __shared__ __attribute__((aligned(16))) float smem[2 * BM * LDA + 2 * KQ * BN * 4];
    float* As = smem;
    float* Bs = smem + 2 * BM * LDA;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, half = lane >> 5;

    const int Cin = d.C0 + d.C1;
    const int nC = Cin / BK;
    const int nChunks = d.KH * d.KW * nC;
    const int phase = blockIdx.z;  // mode 1 only
    const int py = phase >> 1, px = phase & 1;
    const long M = (d.mode == 0) ? (long)d.F * d.Ho * d.Wo : (long)d.F * d.Hi * d.Wi;
    const int nNt = (d.N + BN - 1) / BN;
    const int nMt = (int)((M + BM - 1) / BM);
    // ---- tile assignment: n fastest; optionally give each XCD a contiguous range of M tiles
    int bid = blockIdx.x;
    if (xcd_remap) {
        const int nwg = gridDim.x;
        const int xcd = bid & 7, idx = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;   // bijective for any nwg
    }
    const int mt = bid / nNt, nt = bid - mt * nNt;
    if (mt >= nMt) return;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;
    const float* wbase = d.w + (d.mode == 1 ? (size_t)phase * (size_t)nChunks * BK * d.N : 0);

    // ---- per-thread A rows
    const int kqA = tid % TPR;
    const int r0 = tid / TPR;
    RowInfo ri[RPT];
#pragma unroll
    for (int i = 0; i < RPT; ++i) {
        const long m = m0 + r0 + RSTEP * i;
        ri[i].valid = m < M;
        const long mm = ri[i].valid ? m : 0;
        if (d.mode == 0) {
            const int hw = d.Ho * d.Wo;
            const int f = (int)(mm / hw);
            const int rem = (int)(mm - (long)f * hw);
            const int yo = rem / d.Wo, xo = rem - yo * d.Wo;
            ri[i].yb = yo * d.stride - d.pad;
            ri[i].xb = xo * d.stride - d.pad;
            ri[i].rowoff = ((long)f * d.Hi + ri[i].yb) * d.Wi + ri[i].xb;
        } else {
            const int hw = d.Hi * d.Wi;
            const int f = (int)(mm / hw);
            const int rem = (int)(mm - (long)f * hw);
            ri[i].yb = rem / d.Wi;
            ri[i].xb = rem - ri[i].yb * d.Wi;
            ri[i].rowoff = (long)f * hw + rem;
        }
    }

    f32x4 ga[RPT];
    f32x4 gadd[PRO == 2 ? RPT : 1];
    float gmu[PRO >= 1 ? RPT : 1], grs[PRO >= 1 ? RPT : 1];
    bool ginb[RPT];
    int gc = 0;                       // channel offset of the chunk held in ga (for the channel-affine prologue)
    f32x4 gb[NB4];
    // incremental chunk state (uniform): channel chunk, tap coordinates
    int cc = 0, ky = 0, kx = 0;

    auto load_chunk = [&](int chunk) {
        int dy, dx;
        if (d.mode == 0) { dy = ky; dx = kx; }
        else { dy = ky ? (py ? 1 : -1) : 0; dx = kx ? (px ? 1 : -1) : 0; }
        const int tapoff = dy * d.Wi + dx;
        const int c = cc * BK + kqA * 4;
        const bool src1 = c >= d.C0;
        const float* src = src1 ? d.in1 : d.in0;
        const int ld = src1 ? d.ld1 : d.ld0;
        const int cs = src1 ? c - d.C0 : c;
        gc = c;
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            int yi = ri[i].yb + dy, xi = ri[i].xb + dx;
            long poff = tapoff;
            if (d.border) {            // (uniform; mode 1 only) a remapped tap's pixel: rowoff + tapoff holds for in-range taps only
                yi = dawn_border_coord(yi, d.Hi, d.border);
                xi = dawn_border_coord(xi, d.Wi, d.border);
                poff = (long)(yi - ri[i].yb) * d.Wi + (xi - ri[i].xb);
            }
            const bool inb = ri[i].valid && yi >= 0 && yi < d.Hi && xi >= 0 && xi < d.Wi;
            const long pix = inb ? ri[i].rowoff + poff : 0;
            ginb[i] = inb;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (inb) v = *reinterpret_cast<const f32x4*>(src + pix * ld + cs);
            ga[i] = v;
            if (PRO >= 1 && d.row_mean) {
                gmu[i] = d.row_mean[pix];
                grs[i] = d.row_rstd[pix];
            }
            if (PRO == 2 && d.pro_add) {
                f32x4 av = {0.f, 0.f, 0.f, 0.f};
                if (inb) av = *reinterpret_cast<const f32x4*>(d.pro_add + pix * d.ld_add + c);
                gadd[i] = av;
            }
        }
#pragma unroll
        for (int i = 0; i < NB4; ++i) {
            const int idx = tid + 256 * i;
            const int kq = idx / BN, n = idx % BN;   // BN is a power of two
            const int gn = n0 + n;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (gn < d.N) v = *reinterpret_cast<const f32x4*>(wbase + ((size_t)(chunk * KQ + kq) * d.N + gn) * 4);
            gb[i] = v;
        }
        // advance the uniform chunk state
        if (++cc == nC) {
            cc = 0;
            if (++kx == d.KW) { kx = 0; ++ky; }
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int i = 0; i < RPT; ++i) {
            f32x4 v = ga[i];
            if (PRO >= 1 && d.row_mean) v = (v - gmu[i]) * grs[i];
            if (PRO == 2) {
                if (d.ch_a) {
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(d.ch_a + gc);
                    const f32x4 b4 = *reinterpret_cast<const f32x4*>(d.ch_b + gc);
                    v = v * a4 + b4;
                }
                if (d.pro_act) {
                    v.x = dawn_silu(v.x); v.y = dawn_silu(v.y); v.z = dawn_silu(v.z); v.w = dawn_silu(v.w);
                }
                if (d.pro_add) v += gadd[i];
            }
            if (PRO >= 1 && !ginb[i]) v = f32x4{0.f, 0.f, 0.f, 0.f};     // zero padding applies AFTER the prologue
            *reinterpret_cast<f32x4*>(As + buf * BM * LDA + (r0 + RSTEP * i) * LDA + kqA * 4) = v;
        }
#pragma unroll
        for (int i = 0; i < NB4; ++i)
            *reinterpret_cast<f32x4*>(Bs + buf * KQ * BN * 4 + (tid + 256 * i) * 4) = gb[i];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_chunk(0);
    store_chunk(0);
    __syncthreads();

    for (int chunk = 0; chunk < nChunks; ++chunk) {
        const int buf = ABL ? 0 : (chunk & 1);
        if (ABL == 0 && chunk + 1 < nChunks) load_chunk(chunk + 1);
        const float* Ab = As + buf * BM * LDA;
        const float* Bb = Bs + buf * KQ * BN * 4;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            const int kq = kk * 2 + half;
            f32x4 a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                a[i] = *reinterpret_cast<const f32x4*>(Ab + (wm * WTM + i * 32 + l31) * LDA + kq * 4);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                b[j] = *reinterpret_cast<const f32x4*>(Bb + (kq * BN + wn * WTN + j * 32 + l31) * 4);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][s], b[j][s], acc[i][j], 0, 0, 0);
        }
        if (ABL == 0 && chunk + 1 < nChunks) store_chunk(buf ^ 1);
        if (ABL < 2) __syncthreads();
    }

    // ---- epilogue: C layout col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    float gs[TN], gss[TN];            // per-column sums of the stored values (GroupNorm statistics fused here)
#pragma unroll
    for (int j = 0; j < TN; ++j) { gs[j] = 0.f; gss[j] = 0.f; }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long m = m0 + wm * WTM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m >= M) continue;
            long orow = m;
            if (d.mode == 1) {
                const int hw = d.Hi * d.Wi;
                const int f = (int)(m / hw);
                const int rem = (int)(m - (long)f * hw);
                const int a = rem / d.Wi, b = rem - a * d.Wi;
                orow = ((long)f * d.Ho + 2 * a + py) * d.Wo + 2 * b + px;
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 32 + l31;
                if (n >= d.N) continue;
                float v = acc[i][j][r];
                if (d.bias) v += d.bias[n];
                if (d.res) v += d.res[orow * d.ld_res + n];
                if (d.tr) v += dawn_silu(d.tr[orow * d.ld_tr + n] * d.tr_a[n] + d.tr_b[n]);
                d.out[orow * d.ld_out + n] = v;
                gs[j] += v;
                gss[j] += v * v;
            }
        }
    }
    if (d.gn_part) {
        // fp64 (sum, sumsq) per GroupNorm group of this block's columns -> gn_part[block][16] (MT:230,235)
        double* red = reinterpret_cast<double*>(smem);       // every LDS read of the main loop has retired
        if (tid < 16) red[tid] = 0.0;
        __syncthreads();
        const int cpg = d.N >> 3;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WTN + j * 32 + l31;
            if (n < d.N) {
                const int g = n / cpg;
                atomicAdd(&red[2 * g], (double)gs[j]);
                atomicAdd(&red[2 * g + 1], (double)gss[j]);
            }
        }
        __syncthreads();
        if (tid < 16) d.gn_part[((long)blockIdx.z * gridDim.x + blockIdx.x) * 16 + tid] = red[tid];
    }
}

// ---------------------------------------------------------------------------------------------------------
// Direct-to-LDS variant for prologue-free convs / GEMMs (the bulk of the FLOPs): both operand tiles are
// staged with global_load_lds_dwordx4 (no VGPR round trip, no ds_write, almost no address VALU).  An LDS-DMA
// write is lane-linear (wave-uniform base + lane*16 B), so the A image is unpadded [row][16 floats] and the
// bank-conflict fix is an XOR swizzle of the 16-B slot, applied on the SOURCE address (lane L loads the
// global bytes that belong at physical slot L&3 of row L>>2) and again on the ds_read_b128 address.
// Out-of-frame taps / tail rows / tail columns read from a zero block instead of being predicated.
// Measured ablation (profiles/r1_j_conv_ablation.txt): the register-staged kernel loses ~20 % to staging.
__device__ __attribute__((aligned(64))) float dawn_zero_block[16];

// NST = 3: three LDS stages, loads issued TWO chunks ahead and retired with a COUNTED s_waitcnt vmcnt(IPC) + raw
// s_barrier (a __syncthreads() would drain the whole DMA queue), so one chunk of loads is always in flight
// across the barrier (cdna_hip_programming.md "Pipelining across barriers").
// FOLD (K >= GLDS_FOLD_MIN_K, the 1-D convs and Linears of the HuBERT stage, the 7x7 fea conv): every GLDS_FOLD_K products the MFMA
// accumulators are added to a second set and cleared.  One fp32 chain over all of K (K / 2 MFMA additions per output) measured 6.4x (K =
// 1536), 9.3x (K = 4096) and 12x (K = 8192) the error of a blocked CPU fp32 GEMM against float64, half of what a 16-bit-mantissa operand
// costs; two-level chains of GLDS_FOLD_K / 2 + K / GLDS_FOLD_K additions stay at CPU fp32's level (tests/stage_gate.py).
constexpr int GLDS_FOLD_K = 512, GLDS_FOLD_MIN_K = 1024;
template <int BN, int NST, int BK, int WN = 2, bool FOLD = false>
__global__ __launch_bounds__(256) void conv_gemm_glds_kernel(const dawn_conv_desc d, const int xcd_remap) {
    constexpr int BM = 64 * (4 / WN), KQ = BK / 4; // 4 waves as (4/WN) x WN, 64 rows each; KQ 16-B slots per A row
    constexpr int WTN = BN / WN;
    constexpr int TM = 2, TN = WTN / 32;
    constexpr int NAI = BM * KQ / 64 / 4;          // A wave-instructions per wave per chunk (2 or 4)
    constexpr int RPI = 64 / KQ;                   // A rows per wave-instruction (16 or 8)
    constexpr int NBI = BN * KQ / 64 / 4;          // B wave-instructions per wave per chunk
    constexpr int IPC = NAI + NBI;                 // LDS-DMA instructions per wave per chunk
    constexpr int SW = (BK == 16) ? 2 : 1;         // swizzle: slot ^= (row >> SW) & (KQ-1)
    __shared__ __attribute__((aligned(16))) float smem[NST * BM * BK + NST * KQ * BN * 4];
    float* As = smem;
    float* Bs = smem + NST * BM * BK;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, half = lane >> 5;

    const int Cin = d.C0 + d.C1;
    const int nC = Cin / BK;
    const int nChunks = d.KH * d.KW * nC;
    const int phase = blockIdx.z;
    const int py = phase >> 1, px = phase & 1;
    const long M = (d.mode == 0) ? (long)d.F * d.Ho * d.Wo : (long)d.F * d.Hi * d.Wi;
    const int nNt = (d.N + BN - 1) / BN;
    int bid = blockIdx.x;
    if (xcd_remap) {
        const int nwg = gridDim.x;
        const int xcd = bid & 7, idx = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int mt = bid / nNt, nt = bid - mt * nNt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;
    const float* wbase = d.w + (d.mode == 1 ? (size_t)phase * (size_t)nChunks * BK * d.N : 0);

    // ---- this lane's A rows (one per wave-instruction) and its logical k-slot
    RowInfo ri[NAI];
    int kql[NAI];
#pragma unroll
    for (int j = 0; j < NAI; ++j) {
        const int row = (wave * NAI + j) * RPI + lane / KQ;
        kql[j] = (lane % KQ) ^ ((row >> SW) & (KQ - 1));
        const long m = m0 + row;
        ri[j].valid = m < M;
        const long mm = ri[j].valid ? m : 0;
        if (d.mode == 0) {
            const int hw = d.Ho * d.Wo;
            const int f = (int)(mm / hw);
            const int rem = (int)(mm - (long)f * hw);
            const int yo = rem / d.Wo, xo = rem - yo * d.Wo;
            ri[j].yb = yo * d.stride - d.pad;
            ri[j].xb = xo * d.stride - d.pad;
            ri[j].rowoff = ((long)f * d.Hi + ri[j].yb) * d.Wi + ri[j].xb;
        } else {
            const int hw = d.Hi * d.Wi;
            const int f = (int)(mm / hw);
            const int rem = (int)(mm - (long)f * hw);
            ri[j].yb = rem / d.Wi;
            ri[j].xb = rem - ri[j].yb * d.Wi;
            ri[j].rowoff = (long)f * hw + rem;
        }
    }
    int cc = 0, ky = 0, kx = 0;
    auto issue = [&](int chunk, int buf) {
        int dy, dx;
        if (d.mode == 0) { dy = ky; dx = kx; }
        else { dy = ky ? (py ? 1 : -1) : 0; dx = kx ? (px ? 1 : -1) : 0; }
        const int tapoff = dy * d.Wi + dx;
        const int cbase = cc * BK;
        const bool src1 = cbase >= d.C0;
        const float* src = src1 ? d.in1 : d.in0;
        const int ld = src1 ? d.ld1 : d.ld0;
        const int cs0 = src1 ? cbase - d.C0 : cbase;
#pragma unroll
        for (int j = 0; j < NAI; ++j) {
            int yi = ri[j].yb + dy, xi = ri[j].xb + dx;
            long poff = tapoff;
            if (d.border) {            // (uniform; mode 1 only) as conv_gemm_kernel
                yi = dawn_border_coord(yi, d.Hi, d.border);
                xi = dawn_border_coord(xi, d.Wi, d.border);
                poff = (long)(yi - ri[j].yb) * d.Wi + (xi - ri[j].xb);
            }
            const bool inb = ri[j].valid && yi >= 0 && yi < d.Hi && xi >= 0 && xi < d.Wi;
            const float* g = inb ? src + (ri[j].rowoff + poff) * ld + cs0 + kql[j] * 4 : dawn_zero_block;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(As + buf * BM * BK + (wave * NAI + j) * 256),
                                             16, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NBI; ++j) {
            const int q = wave * NBI + j;
            const int idx = q * 64 + lane;
            const int kq = idx / BN, n = idx % BN;
            const int gn = n0 + n;
            const float* g = gn < d.N ? wbase + ((size_t)(chunk * KQ + kq) * d.N + gn) * 4 : dawn_zero_block;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(Bs + buf * KQ * BN * 4 + q * 256),
                                             16, 0, 0);
        }
        if (++cc == nC) {
            cc = 0;
            if (++kx == d.KW) { kx = 0; ++ky; }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    constexpr int FOLD_CHUNKS = GLDS_FOLD_K / BK;
    f32x16 tot[FOLD ? TM : 1][FOLD ? TN : 1];
    if (FOLD) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) tot[FOLD ? i : 0][FOLD ? j : 0][r] = 0.f;
    }

    issue(0, 0);
    if (NST == 3) {
        if (nChunks > 1) {
            issue(1, 1);
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"(IPC) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_s_barrier();
    } else {
        __syncthreads();
    }
    int buf = 0;
    for (int chunk = 0; chunk < nChunks; ++chunk) {
        if (NST == 3) {
            if (chunk + 2 < nChunks) issue(chunk + 2, buf >= 1 ? buf - 1 : 2);     // (buf + 2) % 3
        } else {
            if (chunk + 1 < nChunks) issue(chunk + 1, buf ^ 1);
        }
        const float* Ab = As + buf * BM * BK;
        const float* Bb = Bs + buf * KQ * BN * 4;
#pragma unroll
        for (int kk = 0; kk < BK / 8; ++kk) {
            const int kq = kk * 2 + half;
            f32x4 a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * 64 + i * 32 + l31;
                a[i] = *reinterpret_cast<const f32x4*>(Ab + row * BK + ((kq ^ ((row >> SW) & (KQ - 1))) << 2));
            }
#pragma unroll
            for (int j = 0; j < TN; ++j)
                b[j] = *reinterpret_cast<const f32x4*>(Bb + (kq * BN + wn * WTN + j * 32 + l31) * 4);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(b[j][s], a[i][s], acc[i][j], 0, 0, 0);   // D^T: lane = row
        }
        if (FOLD && ((chunk + 1) & (FOLD_CHUNKS - 1)) == 0) {   // (uniform) close this chain of GLDS_FOLD_K products
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        tot[FOLD ? i : 0][FOLD ? j : 0][r] += acc[i][j][r];
                        acc[i][j][r] = 0.f;
                    }
        }
        if (NST == 3) {
            // chunk+1 must have landed, chunk+2 (just issued) may stay in flight; all reads of `buf` retired
            if (chunk + 2 < nChunks) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(IPC) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            buf = buf == 2 ? 0 : buf + 1;
        } else {
            __syncthreads();   // drains the LDS-DMA of chunk+1 (vmcnt) and retires every read of `buf`
            buf ^= 1;
        }
    }

    if (FOLD) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += tot[FOLD ? i : 0][FOLD ? j : 0][r];
    }

    // ---- epilogue.  The tiles are accumulated TRANSPOSED (A = weights, B = rows): lane = output row, registers
    // 4g..4g+3 = columns 8g + 4*half + {0..3} of the 32-column tile, so the stores are 16-byte row segments (16
    // dwordx4 per wave instead of 64 scalar stores -- the store epilogue dominated the small-K GEMMs) and the
    // GroupNorm partial sums stay in registers per 4-channel piece until one block reduction.
    const int cpg = d.N >> 3;
    const bool quad_groups = (cpg & 3) == 0;                 // a 4-channel piece never straddles two groups
    double* red = reinterpret_cast<double*>(smem);           // slow path (tiny N): LDS atomics per element
    if (d.gn_part && !quad_groups) {
        if (tid < 16) red[tid] = 0.0;
        __syncthreads();
    }
    float gs[TN][4], gss[TN][4];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) { gs[j][g] = 0.f; gss[j][g] = 0.f; }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const long m = m0 + wm * 64 + i * 32 + l31;
        if (m >= M) continue;
        long orow = m;
        if (d.mode == 1) {
            const int hw = d.Hi * d.Wi;
            const int f = (int)(m / hw);
            const int rem = (int)(m - (long)f * hw);
            const int ya = rem / d.Wi, xb = rem - ya * d.Wi;
            orow = ((long)f * d.Ho + 2 * ya + py) * d.Wo + 2 * xb + px;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * WTN + j * 32 + 8 * g + 4 * half;
                if (n >= d.N) continue;
                f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                if (n + 3 < d.N && !(d.ld_out & 3) && !(d.res && (d.ld_res & 3)) && !(d.tr && (d.ld_tr & 3))) {
                    if (d.bias) v = v + *reinterpret_cast<const f32x4*>(d.bias + n);
                    if (d.res) v = v + *reinterpret_cast<const f32x4*>(d.res + orow * d.ld_res + n);
                    if (d.tr) {
                        const f32x4 t4 = *reinterpret_cast<const f32x4*>(d.tr + orow * d.ld_tr + n);
                        const f32x4 ta = *reinterpret_cast<const f32x4*>(d.tr_a + n), tb = *reinterpret_cast<const f32x4*>(d.tr_b + n);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += dawn_silu(t4[e] * ta[e] + tb[e]);
                    }
                    *reinterpret_cast<f32x4*>(d.out + orow * d.ld_out + n) = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if (n + e >= d.N) { v[e] = 0.f; continue; }
                        if (d.bias) v[e] += d.bias[n + e];
                        if (d.res) v[e] += d.res[orow * d.ld_res + n + e];
                        if (d.tr) v[e] += dawn_silu(d.tr[orow * d.ld_tr + n + e] * d.tr_a[n + e] + d.tr_b[n + e]);
                        d.out[orow * d.ld_out + n + e] = v[e];
                    }
                }
                if (d.gn_part) {
                    if (quad_groups) {
                        gs[j][g] += (v.x + v.y) + (v.z + v.w);
                        gss[j][g] += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (n + e < d.N) {
                                atomicAdd(&red[2 * ((n + e) / cpg)], (double)v[e]);
                                atomicAdd(&red[2 * ((n + e) / cpg) + 1], (double)v[e] * (double)v[e]);
                            }
                    }
                }
            }
        }
    }
    if (d.gn_part) {
        // fp64 (sum, sumsq) per GroupNorm group of this block's columns -> gn_part[block][16] (MT:230,235)
        const long prow = ((long)blockIdx.z * gridDim.x + blockIdx.x) * 16;
        __syncthreads();                                     // every LDS read of the main loop has retired
        if (!quad_groups) {
            if (tid < 16) d.gn_part[prow + tid] = red[tid];
            return;
        }
        constexpr int NCOL = TN * 8;                         // (j, g, which) columns per thread
        float* pf = smem;                                    // [NCOL][256]
        double* pd = reinterpret_cast<double*>(smem + NCOL * 256);   // [NCOL][8]
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                pf[((j * 4 + g) * 2) * 256 + tid] = gs[j][g];
                pf[((j * 4 + g) * 2 + 1) * 256 + tid] = gss[j][g];
            }
        __syncthreads();
        if (tid < NCOL * 8) {
            const int c = tid >> 3, p = tid & 7;
            double acc2 = 0.0;
#pragma unroll 8
            for (int e = 0; e < 32; ++e) acc2 += (double)pf[c * 256 + p * 32 + e];
            pd[c * 8 + p] = acc2;
        }
        __syncthreads();
        if (tid < 16) {
            const int grp = tid >> 1, which = tid & 1;
            double acc2 = 0.0;
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int jg = 0; jg < TN * 4; ++jg) {
                    const int n = n0 + (w % WN) * WTN + (jg >> 2) * 32 + 8 * (jg & 3);   // half 0's piece; half 1: n + 4
                    if (n < d.N && n / cpg == grp) acc2 += pd[(jg * 2 + which) * 8 + w * 2];
                    if (n + 4 < d.N && (n + 4) / cpg == grp) acc2 += pd[(jg * 2 + which) * 8 + w * 2 + 1];
                }
            d.gn_part[prow + tid] = acc2;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// 3x3 / stride 1 / pad 1 convolution with an LDS HALO tile: the loop is channel-chunk-major -- for each 16-channel
// chunk the block stages its input patch (TR+2 rows x (W+2) pixels per frame part, zero-padded) ONCE and runs
// all nine taps out of it; only the 16 x BN weight chunk changes per tap.  The implicit-GEMM kernels above
// re-fetch the A tile for every tap (9x; they are bound by the per-CU fetch rate, profiles/r1_j_conv_glds.txt);
// here the A fetch drops to (TR+2)(W+2)/(TR W) ~ 1.1-2x.  Staging is direct-to-LDS (global_load_lds) with the
// same source-side XOR swizzle as conv_gemm_glds_kernel; the A fragment of tap (ky,kx) is read at position
// pos(pixel) + (ky-1)(W+2) + (kx-1).
// Tile = BM consecutive output pixels = TR full rows of one frame (or nf whole frames when a frame is < BM).
template <int BN, int WN>
__global__ __launch_bounds__(256) void conv3x3_halo_kernel(const dawn_conv_desc d, const int xcd_remap, const int TR,
                                                           const int nf, const int P16) {
    constexpr int BM = 64 * (4 / WN), BK = 16, KQ = 4;
    constexpr int WTN = BN / WN;
    constexpr int TM = 2, TN = WTN / 32;
    constexpr int NBI = BN * KQ / 64 / 4;
    constexpr int MAXS = 7;                         // A wave-instructions per wave per channel chunk (P16/16/4 <= 7)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                               // [2][P16][16]
    float* Bs = smem + 2 * P16 * BK;                // [2][4][BN][4]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, half = lane >> 5;
    const int H = d.Hi, W = d.Wi, PW = W + 2, PP = (TR + 2) * PW;
    const int Cin = d.C0 + d.C1;
    const int nC = Cin / BK;
    const long M = (long)d.F * H * W;
    const int nNt = (d.N + BN - 1) / BN;
    int bid = blockIdx.x;
    if (xcd_remap) {
        const int nwg = gridDim.x;
        const int xcd = bid & 7, idx = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int mt = bid / nNt, nt = bid - mt * nNt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;
    // tile origin: frame f0, first row y0
    const int f0 = (int)(m0 / ((long)H * W));
    const int y0 = (int)((m0 - (long)f0 * H * W) / W);

    // ---- staging slots of this lane: position -> source pixel (or -1 = zero padding), logical k-slot
    const int nInstr = P16 >> 4;
    long spix[MAXS];
    int skq[MAXS];
#pragma unroll
    for (int sidx = 0; sidx < MAXS; ++sidx) {
        const int ii = sidx * 4 + wave;
        const int pos = ii * 16 + (lane >> 2);
        skq[sidx] = (lane & 3) ^ ((pos >> 2) & 3);
        long pix = -1;
        if (ii < nInstr && pos < nf * PP) {
            const int fi = pos / PP;
            const int rem = pos - fi * PP;
            const int pyy = rem / PW, pxx = rem - pyy * PW;
            const int y = y0 + pyy - 1, x = pxx - 1;
            if (y >= 0 && y < H && x >= 0 && x < W) pix = ((long)(f0 + fi) * H + y) * W + x;
        }
        spix[sidx] = pix;
    }
    // ---- A fragment base positions of this lane's output pixels (centre tap)
    int pc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = wm * 64 + i * 32 + l31;
        const int fi = r / (TR * W);
        const int rem = r - fi * TR * W;
        const int ty = rem / W, x = rem - ty * W;
        pc[i] = fi * PP + (ty + 1) * PW + (x + 1);
    }

    // one staging slot (<= 1 wave-instruction per wave) of channel chunk cc; the 7 slots of the next chunk are
    // spread over taps 0..6 of the current one so the fetch stream is even
    auto issueA = [&](int cc, int buf, int sidx) {
        const int cbase = cc * BK;
        const bool src1 = cbase >= d.C0;
        const float* src = src1 ? d.in1 : d.in0;
        const int ld = src1 ? d.ld1 : d.ld0;
        const int cs0 = src1 ? cbase - d.C0 : cbase;
        const int ii = sidx * 4 + wave;
        if (ii < nInstr) {
            const float* g = spix[sidx] >= 0 ? src + spix[sidx] * ld + cs0 + skq[sidx] * 4 : dawn_zero_block;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(As + buf * P16 * BK + ii * 256),
                                             16, 0, 0);
        }
    };
    auto issueB = [&](int chunk, int buf) {
#pragma unroll
        for (int j = 0; j < NBI; ++j) {
            const int q = wave * NBI + j;
            const int idx = q * 64 + lane;
            const int kq = idx / BN, n = idx % BN;
            const int gn = n0 + n;
            const float* g = gn < d.N ? d.w + ((size_t)(chunk * KQ + kq) * d.N + gn) * 4 : dawn_zero_block;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(Bs + buf * KQ * BN * 4 + q * 256),
                                             16, 0, 0);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
    for (int sidx = 0; sidx < MAXS; ++sidx) issueA(0, 0, sidx);
    issueB(0, 0);           // step (cc=0, tap=0): weight chunk tap*nC + cc = 0
    __syncthreads();
    int bufA = 0, bufB = 0;
    for (int cc = 0; cc < nC; ++cc) {
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            if (tap < MAXS && cc + 1 < nC) issueA(cc + 1, bufA ^ 1, tap);
            {   // next step's weight chunk
                int ntap = tap + 1, ncc = cc;
                if (ntap == 9) { ntap = 0; ncc = cc + 1; }
                if (ncc < nC) issueB(ntap * nC + ncc, bufB ^ 1);
            }
            const int ky = tap / 3, kx = tap - ky * 3;
            const int toff = (ky - 1) * PW + (kx - 1);
            const float* Ab = As + bufA * P16 * BK;
            const float* Bb = Bs + bufB * KQ * BN * 4;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                const int kq = kk * 2 + half;
                f32x4 a[TM], b[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int pos = pc[i] + toff;
                    a[i] = *reinterpret_cast<const f32x4*>(Ab + pos * BK + ((kq ^ ((pos >> 2) & 3)) << 2));
                }
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    b[j] = *reinterpret_cast<const f32x4*>(Bb + (kq * BN + wn * WTN + j * 32 + l31) * 4);
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i][s], b[j][s], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
            bufB ^= 1;
        }
        bufA ^= 1;
    }

    float gs[TN], gss[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) { gs[j] = 0.f; gss[j] = 0.f; }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 32 + l31;
                if (n >= d.N) continue;
                float v = acc[i][j][r];
                if (d.bias) v += d.bias[n];
                if (d.res) v += d.res[m * d.ld_res + n];
                if (d.tr) v += dawn_silu(d.tr[m * d.ld_tr + n] * d.tr_a[n] + d.tr_b[n]);
                d.out[m * d.ld_out + n] = v;
                gs[j] += v;
                gss[j] += v * v;
            }
        }
    }
    if (d.gn_part) {
        double* red = reinterpret_cast<double*>(smem);
        if (tid < 16) red[tid] = 0.0;
        __syncthreads();
        const int cpg = d.N >> 3;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WTN + j * 32 + l31;
            if (n < d.N) {
                const int g = n / cpg;
                atomicAdd(&red[2 * g], (double)gs[j]);
                atomicAdd(&red[2 * g + 1], (double)gss[j]);
            }
        }
        __syncthreads();
        if (tid < 16) d.gn_part[(long)blockIdx.x * 16 + tid] = red[tid];
    }
}

// host-side geometry test + launch; returns false when the shape does not fit the halo tiling
template <int BN, int WN>
bool try_launch_halo(const dawn_conv_desc& d, long M, hipStream_t s) {
    constexpr int BM = 64 * (4 / WN);
    const int H = d.Hi, W = d.Wi;
    if (M % BM != 0 || W > BM || BM % W != 0) return false;
    int TR = BM / W, nf = 1;
    if (TR <= H) { if (H % TR != 0) return false; }
    else { if (TR % H != 0) return false; nf = TR / H; TR = H; if (d.F % nf != 0) return false; }
    const int P = nf * (TR + 2) * (W + 2);
    const int P16 = (P + 15) / 16 * 16;
    if (P16 / 16 > 7 * 4) return false;
    const size_t lds = ((size_t)2 * P16 * 16 + (size_t)2 * 4 * BN * 4) * sizeof(float);
    if (lds > 160 * 1024) return false;
    const int nwg = (int)(M / BM) * dawn_cdiv(d.N, BN);
    const int remap = ((policy_of(d) & DAWN_POLICY_XCD_ORDER) && nwg >= 64 && H * W >= 1024) ? 1 : 0;
    if (lds > 65536)
        (void)hipFuncSetAttribute((const void*)conv3x3_halo_kernel<BN, WN>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
    hipLaunchKernelGGL((conv3x3_halo_kernel<BN, WN>), dim3(nwg), dim3(256), lds, s, d, remap, TR, nf, P16);
    return true;
}

// ---------------------------------------------------------------------------------------------------------
// fp32 3x3 convolution on the bf16 matrix pipe by exact operand splitting ("bf16x3" emulation of fp32):
// every fp32 operand is written as x = x1 + x2 + x3 with x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2)
// (round-to-nearest-even; the residuals are exact in fp32, and 3 x 8 significand bits cover the fp32
// significand), every bf16 x bf16 product is exact in the fp32 accumulator, and the NT largest cross terms are
// accumulated (NT = 6: all terms down to 2^-16 relative, i.e. x1w1, x1w2, x2w1, x2w2, x1w3, x3w1; the dropped terms
// are <= 2^-24 relative -- the size of one fp32 rounding; NT = 9: every term).  v_mfma_f32_32x32x16_bf16 runs at
// 16x the fp32 MFMA rate, so 6 terms cost 3/8 of the fp32 instruction time.
// Structure = conv3x3_halo_kernel; the staged fp32 patch is split ONCE per channel chunk into three bf16 planes
// in LDS ([plane][k-half][pos][8 ch], conflict-free ds_read_b128), the weights arrive pre-split from the host
// ([chunk][plane][k-half][N][8]).

template <int BN, int WN, int NT>
__global__ __launch_bounds__(256) void conv3x3_halo_bf16_kernel(const dawn_conv_desc d, const int xcd_remap,
                                                                const int TR, const int nf, const int P16) {
    constexpr int BM = 64 * (4 / WN);
    constexpr int WTN = BN / WN;
    constexpr int TM = 2, TN = WTN / 32;
    constexpr int NBI = 6 * BN / 64;                // weight wave-instructions per stage (3 planes x BN x 32 B)
    constexpr int MAXS = 7;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    float* raw = reinterpret_cast<float*>(smem_b);                               // [P16][16] fp32
    const int HPS = P16 * 16 + 128;                                              // half-plane stride (+32 banks)
    unsigned char* planes = smem_b + (size_t)P16 * 64;                           // [3 planes][2 k-halves][HPS]: pos x 16 B
    unsigned char* Bs = planes + (size_t)6 * HPS;                                // [2][3][2][BN][16 B]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, half = lane >> 5;
    const int H = d.Hi, W = d.Wi, PW = W + 2, PP = (TR + 2) * PW;
    const int Cin = d.C0 + d.C1;
    const int nC = Cin / 16;
    const long M = (long)d.F * H * W;
    const int nNt = (d.N + BN - 1) / BN;
    int bid = blockIdx.x;
    if (xcd_remap) {
        const int nwg = gridDim.x;
        const int xcd = bid & 7, idx = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int mt = bid / nNt, nt = bid - mt * nNt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;
    const int f0 = (int)(m0 / ((long)H * W));
    const int y0 = (int)((m0 - (long)f0 * H * W) / W);

    const int nInstr = P16 >> 4;
    long spix[MAXS];
#pragma unroll
    for (int sidx = 0; sidx < MAXS; ++sidx) {
        const int ii = sidx * 4 + wave;
        const int pos = ii * 16 + (lane >> 2);
        long pix = -1;
        if (ii < nInstr && pos < nf * PP) {
            const int fi = pos / PP;
            const int rem = pos - fi * PP;
            const int pyy = rem / PW, pxx = rem - pyy * PW;
            const int y = y0 + pyy - 1, x = pxx - 1;
            if (y >= 0 && y < H && x >= 0 && x < W) pix = ((long)(f0 + fi) * H + y) * W + x;
        }
        spix[sidx] = pix;
    }
    int pc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = wm * 64 + i * 32 + l31;
        const int fi = r / (TR * W);
        const int rem = r - fi * TR * W;
        const int ty = rem / W, x = rem - ty * W;
        pc[i] = fi * PP + (ty + 1) * PW + (x + 1);
    }

    const float* zb = dawn_zero_block;
    asm volatile("" : "+s"(zb));                    // keep the address in SGPRs (no GOT reload per tap)
    auto issueA = [&](int cc, int sidx) -> bool {
        const int cbase = cc * 16;
        const bool src1 = cbase >= d.C0;
        const float* src = src1 ? d.in1 : d.in0;
        const int ld = src1 ? d.ld1 : d.ld0;
        const int cs0 = src1 ? cbase - d.C0 : cbase;
        const int ii = sidx * 4 + wave;
        if (ii < nInstr) {
            const float* g = spix[sidx] >= 0 ? src + spix[sidx] * ld + cs0 + (lane & 3) * 4 : zb;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(raw + ii * 256), 16, 0, 0);
        }
        return ii < nInstr;
    };
    const unsigned short* wsp = reinterpret_cast<const unsigned short*>(d.w_bf3);
    auto issueB = [&](int chunk, int buf) {
#pragma unroll
        for (int j = 0; j < (NBI + 3) / 4; ++j) {
            const int q = j * 4 + wave;
            if (q < NBI) {
                const int idx = q * 64 + lane;
                const int ph = idx / BN, n = idx - ph * BN;       // ph = plane*2 + k-half
                const int gn = n0 + n;
                const void* g = gn < d.N ? (const void*)(wsp + (((size_t)chunk * 6 + ph) * d.N + gn) * 8)
                                         : (const void*)zb;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                                 (__attribute__((address_space(3))) void*)(Bs + (size_t)buf * 3 * BN * 32 + q * 1024),
                                                 16, 0, 0);
            }
        }
    };
    auto split_pass = [&]() {
        const int nq = P16 * 4;
        for (int q = tid; q < nq; q += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(raw + q * 4);
            uint2 p1, p2, p3;
            dawn_split3_rne_quad(v, p1, p2, p3);
            const int pos = q >> 2, slot = q & 3;
            unsigned char* dst = planes + (size_t)(slot >> 1) * HPS + pos * 16 + (slot & 1) * 8;
            *reinterpret_cast<uint2*>(dst) = p1;
            *reinterpret_cast<uint2*>(dst + 2 * HPS) = p2;
            *reinterpret_cast<uint2*>(dst + 4 * HPS) = p3;
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

#pragma unroll
    for (int sidx = 0; sidx < MAXS; ++sidx) issueA(0, sidx);
    issueB(0, 0);
    int bufB = 0;
    for (int cc = 0; cc < nC; ++cc) {
        __syncthreads();            // raw(cc) and the first weight chunk have landed; planes are free
        split_pass();
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            // weights of the next tap first, then one slot of the next chunk's patch: the vmcnt wait at the end of
            // this tap then leaves the patch load in flight (it gets two taps of latency budget)
            {
                int ntap = tap + 1, ncc = cc;
                if (ntap == 9) { ntap = 0; ncc = cc + 1; }
                if (ncc < nC) issueB(ntap * nC + ncc, bufB ^ 1);
            }
            bool issuedA = false;
            if (tap < MAXS && cc + 1 < nC) issuedA = issueA(cc + 1, tap);
            const int ky = tap / 3, kx = tap - ky * 3;
            const int toff = (ky - 1) * PW + (kx - 1);
            const unsigned char* Bb = Bs + (size_t)bufB * 3 * BN * 32;
            bf16x8 a[TM][3], b[TN][3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    a[i][pl] = *reinterpret_cast<const bf16x8*>(planes + (size_t)(pl * 2 + half) * HPS + (pc[i] + toff) * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    b[j][pl] = *reinterpret_cast<const bf16x8*>(Bb + ((size_t)((pl * 2 + half) * BN + wn * WTN + j * 32 + l31)) * 16);
            }
#pragma unroll
            for (int t = 9 - NT; t < 9; ++t)                   // (six terms: the last six of the nine)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][DAWN_SPLIT9_A[t]], b[j][DAWN_SPLIT9_B[t]], acc[i][j], 0, 0, 0);
            if (tap < 8) {
                if (issuedA) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
            bufB ^= 1;
        }
    }

    float gs[TN], gss[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) { gs[j] = 0.f; gss[j] = 0.f; }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const long m = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m >= M) continue;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + wn * WTN + j * 32 + l31;
                if (n >= d.N) continue;
                float v = acc[i][j][r];
                if (d.bias) v += d.bias[n];
                if (d.res) v += d.res[m * d.ld_res + n];
                if (d.tr) v += dawn_silu(d.tr[m * d.ld_tr + n] * d.tr_a[n] + d.tr_b[n]);
                d.out[m * d.ld_out + n] = v;
                gs[j] += v;
                gss[j] += v * v;
            }
        }
    }
    if (d.gn_part) {
        __syncthreads();
        double* red = reinterpret_cast<double*>(smem_b);
        if (tid < 16) red[tid] = 0.0;
        __syncthreads();
        const int cpg = d.N >> 3;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WTN + j * 32 + l31;
            if (n < d.N) {
                const int g = n / cpg;
                atomicAdd(&red[2 * g], (double)gs[j]);
                atomicAdd(&red[2 * g + 1], (double)gss[j]);
            }
        }
        __syncthreads();
        if (tid < 16) d.gn_part[(long)blockIdx.x * 16 + tid] = red[tid];
    }
}

template <int BN, int WN>
bool try_launch_halo_bf16(const dawn_conv_desc& d, long M, hipStream_t s, bool nine, bool dry /* decide only, launch nothing */) {
    constexpr int BM = 64 * (4 / WN);
    const int H = d.Hi, W = d.Wi;
    if (M % BM != 0 || W > BM || BM % W != 0 || d.C0 % 16 != 0 || d.C1 % 16 != 0) return false;
    int TR = BM / W, nf = 1;
    if (TR <= H) { if (H % TR != 0) return false; }
    else { if (TR % H != 0) return false; nf = TR / H; TR = H; if (d.F % nf != 0) return false; }
    const int P = nf * (TR + 2) * (W + 2);
    const int P16 = (P + 15) / 16 * 16;
    if (P16 / 16 > 7 * 4) return false;
    const size_t lds = (size_t)P16 * 64 + (size_t)6 * (P16 * 16 + 128) + (size_t)2 * 3 * BN * 32;
    if (lds > 160 * 1024) return false;
    if (dry) return true;
    const int nwg = (int)(M / BM) * dawn_cdiv(d.N, BN);
    const int remap = ((policy_of(d) & DAWN_POLICY_XCD_ORDER) && nwg >= 64 && H * W >= 1024) ? 1 : 0;
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
    if (nine) {
        (void)hipFuncSetAttribute((const void*)conv3x3_halo_bf16_kernel<BN, WN, 9>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        hipLaunchKernelGGL((conv3x3_halo_bf16_kernel<BN, WN, 9>), dim3(nwg), dim3(256), lds, s, d, remap, TR, nf, P16);
    } else {
        (void)hipFuncSetAttribute((const void*)conv3x3_halo_bf16_kernel<BN, WN, 6>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)lds);
        hipLaunchKernelGGL((conv3x3_halo_bf16_kernel<BN, WN, 6>), dim3(nwg), dim3(256), lds, s, d, remap, TR, nf, P16);
    }
    return true;
}

template <int BM, int BN, int BK, int WM, int WN, int PRO>
void launch_pro(const dawn_conv_desc& d, long M, hipStream_t s) {
    const int nMt = dawn_cdiv(M, BM), nNt = dawn_cdiv(d.N, BN);
    const int z = d.mode == 1 ? 4 : 1;
    const int nwg = nMt * nNt;
    const int remap = ((policy_of(d) & DAWN_POLICY_XCD_ORDER) && nwg >= 64 && d.KH * d.KW > 1 && d.Hi * d.Wi >= 1024) ? 1 : 0;
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
    hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, BK, WM, WN, PRO>), dim3(nwg, 1, z), dim3(256), 0, s, d, remap);
}

template <int BM, int BN, int BK, int WM, int WN>
void launch(const dawn_conv_desc& d, long M, hipStream_t s) {
#ifdef DAWN_ABLATION
    if (policy_of(d) & (DAWN_POLICY_ABL_NO_RESTAGE | DAWN_POLICY_ABL_NO_BARRIER)) {   // perf ablations only (wrong results)
        const int nMt = dawn_cdiv(M, BM), nNt = dawn_cdiv(d.N, BN);
        const int nwg = nMt * nNt;
        if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
        if (policy_of(d) & DAWN_POLICY_ABL_NO_BARRIER)
            hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, BK, WM, WN, 0, 2>), dim3(nwg, 1, 1), dim3(256), 0, s, d, 0);
        else
            hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, BK, WM, WN, 0, 1>), dim3(nwg, 1, 1), dim3(256), 0, s, d, 0);
        return;
    }
#endif
    if ((policy_of(d) & DAWN_POLICY_GLDS) && BM == 128 && !d.ch_a && !d.pro_act && !d.pro_add && !d.row_mean) {
        const int nMt = dawn_cdiv(M, BM), nNt = dawn_cdiv(d.N, BN);
        const int nwg = nMt * nNt;
        const int remap = ((policy_of(d) & DAWN_POLICY_XCD_ORDER) && nwg >= 64 && d.KH * d.KW > 1 && d.Hi * d.Wi >= 1024) ? 1 : 0;
        const dim3 grid(nwg, 1, d.mode == 1 ? 4 : 1);
        const bool deep = d.KH * d.KW * (d.C0 + d.C1) >= 2304 && d.N >= 256;
        if (BN == 64 && M >= 65536 && ((policy_of(d) & DAWN_POLICY_GLDS_TILE256) ||
                                       (d.KH * d.KW > 1 && d.C0 + d.C1 <= 64 && !(policy_of(d) & DAWN_POLICY_GLDS_NO_TILE256)))) {
            // 256 x 64 tile (weights amortised over 2x the rows): +7 % on the K=576 3x3 convs, not on 1x1 / K>=1152
            const int nwg2 = dawn_cdiv(M, 256);
            if (d.gn_rows) *d.gn_rows = nwg2;   // rows of gn_part this launch writes
            hipLaunchKernelGGL((conv_gemm_glds_kernel<64, 2, 16, 1>), dim3(nwg2, 1, d.mode == 1 ? 4 : 1), dim3(256), 0, s, d,
                               remap);
            return;
        }
        if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
        const bool fold = d.KH * d.KW * (d.C0 + d.C1) >= GLDS_FOLD_MIN_K;     // two-level K accumulation (see the kernel)
        if (((policy_of(d) & DAWN_POLICY_GLDS_BK32) || deep) && d.C0 % 32 == 0 && d.C1 % 32 == 0) {
            if (fold) hipLaunchKernelGGL((conv_gemm_glds_kernel<BN, 2, 32, 2, true>), grid, dim3(256), 0, s, d, remap);
            else hipLaunchKernelGGL((conv_gemm_glds_kernel<BN, 2, 32>), grid, dim3(256), 0, s, d, remap);
        } else if (policy_of(d) & DAWN_POLICY_GLDS_STAGES3) {
            hipLaunchKernelGGL((conv_gemm_glds_kernel<BN, 3, 16>), grid, dim3(256), 0, s, d, remap);
        } else if (fold) {
            hipLaunchKernelGGL((conv_gemm_glds_kernel<BN, 2, 16, 2, true>), grid, dim3(256), 0, s, d, remap);
        } else {
            hipLaunchKernelGGL((conv_gemm_glds_kernel<BN, 2, 16>), grid, dim3(256), 0, s, d, remap);
        }
        return;
    }
    if (d.ch_a || d.pro_act || d.pro_add) launch_pro<BM, BN, BK, WM, WN, 2>(d, M, s);
    else if (d.row_mean) launch_pro<BM, BN, BK, WM, WN, 1>(d, M, s);
    else launch_pro<BM, BN, BK, WM, WN, 0>(d, M, s);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// Routing (host code from here on): which kernel serves a descriptor, and the entry points that launch what that answers.
int dawn_ncu() {
    static int ncu = 0;
    if (!ncu) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        ncu = n;
    }
    return ncu;
}

// smallest M the split-operand 1x1 kernels take.  12,800 (the deepest level of the 256 x 256 / 200-frame clip) until round 6: at BASELINE
// configs[1] the deepest level has 6,400 rows and every projection there ran on the fp32-MFMA kernel at 42..62 TF/s
// (profiles/r6_config1_insitu_shapes.txt)
constexpr long GEMM1X1_SPLIT_MIN_M = 6400;

static bool gemm1x1_rowreg_ok(long M, int N, int C0, int C1) {
    const int K = C0 + C1;
    return (K == 64 || K == 128) && C0 % 16 == 0 && C1 % 16 == 0 && N % 64 == 0 && M % 256 == 0 && M >= GEMM1X1_SPLIT_MIN_M;
}

static bool gemm1x1_rowacc_ok(long M, int N, int C0, int C1) {
    const int K = C0 + C1;
    return K >= 256 && K % 128 == 0 && C0 % 16 == 0 && C1 % 16 == 0 && N % 64 == 0 && N <= 192 && M % 256 == 0 && M >= GEMM1X1_SPLIT_MIN_M;
}

static bool gemm1x1_rowacc_fits(const dawn_conv_desc& d, long M) {
    return gemm1x1_rowacc_ok(M, d.N, d.C0, d.C1) && (long)d.ld0 * 32 * 4 < (1L << 31) && (long)d.ld1 * 32 * 4 < (1L << 31) &&
           (long)(d.C0 + d.C1) / 16 * 6 * d.N * 16 < (1L << 31);
}

// Downsample (4x4 / stride 2 / pad 1) and Upsample (transposed 4x4 / stride 2 / pad 1 as 4 phases of 2x2 taps) on the split
// pipeline: single source of 64-channel multiples, N = 64 / 128 / 256 (256: two column groups per row panel), bias-only epilogue,
// 32-pixel tiles inside one frame.
static bool conv_resample_rowacc_ok(const dawn_conv_desc& d, long M) {
    const bool down = d.mode == 0 && d.KH == 4 && d.KW == 4 && d.stride == 2 && d.pad == 1 && d.Hi == 2 * d.Ho && d.Wi == 2 * d.Wo;
    const bool up = d.mode == 1;
    if (!(down || up) || d.C1 != 0 || d.in1 || d.C0 % 64 != 0 || (d.N != 64 && d.N != 128 && d.N != 256) || M % 256 != 0 || M < 12800) return false;
    if (d.row_mean || d.ch_a || d.pro_act || d.pro_add || d.res || d.tr || d.gn_part || d.ln_eps > 0.f) return false;
    const long hw = down ? (long)d.Ho * d.Wo : (long)d.Hi * d.Wi;
    if (hw % 32 != 0 || (long)d.Hi * d.Wi * d.ld0 * 4 >= (1L << 31) || (d.ld0 & 3) || (d.ld_out & 3)) return false;
    return (long)(down ? 16 : 4) * d.C0 / 16 * 6 * d.N * 16 * (up ? 4 : 1) < (1L << 31);
}

static bool gemm1x1_rowreg_fits(const dawn_conv_desc& d, long M) {
    return gemm1x1_rowreg_ok(M, d.N, d.C0, d.C1) && (long)d.ld0 * 32 * 4 < (1L << 31) && (long)d.ld1 * 32 * 4 < (1L << 31);
}

// Which split-operand 1x1 GEMM tile (0 = none: fp32 kernel, 1 = 256 x 64, 2 = 256 x 128) serves an (M x N) projection of
// C0 (+ C1) channels.  Tile policy from the per-shape table of the benchmark (profiles/r1_final_gemm1x1_policy.txt):
// 256 x 128 tiles when they fill the chip; 256 x 64 tiles for N = 192 and for the small GEMMs that would leave more than
// half of the CUs idle with 128-wide tiles; the thin N = 64 GEMMs and the short (M < 51200) 128..255-tile cases stay on
// the fp32 kernel (many small workgroups hide HBM latency better than one 126 KB-LDS workgroup per CU).
int gemm1x1_split_plan(long M, int N, int C0, int C1) {
    if (C0 % 32 != 0 || C1 % 32 != 0 || N % 64 != 0 || M % 256 != 0 || M < GEMM1X1_SPLIT_MIN_M) return 0;
    int plan;
    if (N % 128 == 0) {
        const long t2 = (M / 256) * (N / 128);
        if (t2 >= 256 || (t2 >= 128 && M >= 51200)) plan = 2;
        else plan = (t2 < 128 || M <= 12800) ? 1 : 0;    // (M = 12,800 with 128..255 wide tiles fell through to the fp32 kernel: 128 x 64 tiles below)
    } else {
        plan = N == 64 ? 0 : 1;
    }
    // plan 3 = 128 x 64 tiles, two workgroups per CU (fetch / store of one under the MFMAs of the other): measured per shape
    // at the benchmark (profiles/r2_gemm1x1_tiles_*.txt) it wins 12..30 % on the N = 192 to_q projections, on the M = 12800
    // GEMMs and on the long thin N = 128 ones; the N = 768 qkv GEMMs stay on the 256-row tiles (7..13 % better there)
    if (plan != 0 && (N % 128 != 0 || M <= 12800 || (N == 128 && M >= 204800))) plan = 3;
    return plan;
}

// operand layout every split 1x1 kernel (tiled, row-stationary, row-accumulator) relies on: 16-byte aligned row strides of the
// sources, the output and the epilogue tensors (f32x4 loads / stores), offsets inside 31 bits
static bool gemm1x1_split_layout_ok(const dawn_conv_desc& d) {
    if ((d.C1 != 0) != (d.in1 != nullptr) || d.gn_part) return false;
    if ((d.ld0 & 3) || (d.in1 && (d.ld1 & 3)) || (d.ld_out & 3) || (d.res && (d.ld_res & 3)) || (d.tr && (d.ld_tr & 3)) ||
        (long)d.ld0 * 256 * 4 >= (1L << 31) || (long)d.ld1 * 256 * 4 >= (1L << 31))
        return false;
    return true;
}

// Which split-operand kernel serves a 1x1 projection or a 4x4 / stride-2 resample (DAWN_SPLIT1X1_* of include/dawn_hip.h; 0 = none
// of them: the 3x3 paths or the fp32 kernels).  THE routing of dawn_conv_gemm -- it launches what this answers -- and of
// dawn_gemm1x1_form.  With ln_eps > 0 only the row-stationary / row-accumulator kernels qualify (they hold whole rows).
static int split1x1_form(const dawn_conv_desc& d, long M) {
    const int p = policy_of(d);
    if (!(p & DAWN_POLICY_SPLIT) || !d.w_bf3) return DAWN_SPLIT1X1_NONE;
    const bool rows_ok = !(p & DAWN_POLICY_NO_ROW_KERNELS);   // (A/B only: the tiled kernel for every 1x1 shape)
    const bool proj = d.mode == 0 && d.KH == 1 && d.KW == 1 && d.stride == 1 && d.pad == 0 && !d.ch_a && !d.pro_act && !d.pro_add;
    if (d.ln_eps > 0.f) {
        if (!proj || d.row_mean || d.row_rstd || !gemm1x1_split_layout_ok(d) || !rows_ok) return DAWN_SPLIT1X1_NONE;
        return gemm1x1_rowreg_fits(d, M) ? DAWN_SPLIT1X1_ROWREG : gemm1x1_rowacc_fits(d, M) ? DAWN_SPLIT1X1_ROWACC : DAWN_SPLIT1X1_NONE;
    }
    if (rows_ok && conv_resample_rowacc_ok(d, M)) return DAWN_SPLIT1X1_RESAMPLE;
    if (!proj || (d.row_mean == nullptr) != (d.row_rstd == nullptr) || !gemm1x1_split_layout_ok(d)) return DAWN_SPLIT1X1_NONE;
    if (rows_ok && gemm1x1_rowreg_fits(d, M)) return DAWN_SPLIT1X1_ROWREG;      // short K: rows stationary in registers
    if (rows_ok && gemm1x1_rowacc_fits(d, M)) return DAWN_SPLIT1X1_ROWACC;
    return gemm1x1_split_plan(M, d.N, d.C0, d.C1) != 0 ? DAWN_SPLIT1X1_TILED : DAWN_SPLIT1X1_NONE;
}

#ifdef DAWN_WITH_STREAMK
int dawn_conv3x3_sk_try(const dawn_conv_desc& d, long M, int policy, hipStream_t s, int* nrows);   // tools/ubench/conv3x3_sk.hip (experimental build)
#endif
int dawn_conv3x3_wino_try(const dawn_conv_desc& d, long M, int policy, hipStream_t s, int* nrows, int dry); // conv3x3_wino.hip
int dawn_conv3x3_wino4_try(const dawn_conv_desc& d, long M, int policy, hipStream_t s, int* nrows, int dry); // conv3x3_wino4.hip

/* 1 when a 1x1 projection (M rows, N columns, C0 + C1 input channels, w_bf3 supplied, shipped policy, 16-byte aligned row strides)
 * runs on a row-stationary / row-accumulator split GEMM, which can compute the LayerNorm of its input rows itself
 * (dawn_conv_desc.ln_eps): the host then launches no statistics pass (see unet_forward._ln_gemm / dawn_ctx.hip).  dawn_conv_gemm
 * re-checks the layout and policy conditions per call and answers -14 when they fail. */
extern "C" int dawn_gemm1x1_ln_inline_ok(long M, int N, int C0, int C1) {
    return gemm1x1_rowreg_ok(M, N, C0, C1) || gemm1x1_rowacc_ok(M, N, C0, C1);
}
extern "C" int dawn_gemm1x1_split_ok(long M, int N, int C0, int C1) {
    return gemm1x1_split_plan(M, N, C0, C1) != 0 || gemm1x1_rowreg_ok(M, N, C0, C1) || gemm1x1_rowacc_ok(M, N, C0, C1);
}

extern "C" int dawn_conv_gemm_nblocks(long M, int N) {
    const int sk = 2 * dawn_ncu();             // the persistent 3x3 kernel writes one row per resident workgroup
    if (N <= 64) return std::max(sk, dawn_cdiv(M, 128));   // upper bound (the 256-row tile variants launch fewer blocks; the
                                             // caller zero-fills the buffer)
    return std::max(sk, dawn_cdiv(M, 128) * dawn_cdiv(N, 128));
}

// the split-operand 3x3 family serves this descriptor (the condition dawn_conv_gemm dispatches on)
static bool conv3x3_split_path(const dawn_conv_desc& d) {
    return (policy_of(d) & DAWN_POLICY_SPLIT) && d.w_bf3 && d.mode == 0 && d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.Ho == d.Hi &&
           d.Wo == d.Wi && !d.ch_a && !d.pro_act && !d.pro_add && !d.row_mean;
}

/* The transformed forms of the split 3x3 conv, in dawn_conv_gemm's order: Winograd F(4x4,3x3), Winograd F(2x2,3x3) and -- in the
 * experimental stream-K build only -- the persistent kernel.  Launches the first that takes the descriptor (dry: launches nothing) and
 * answers which: 2 = F(4x4), 1 = F(2x2), 3 = stream-K, 0 = none of them (nine cross terms exist in the direct kernels only).
 * *nrows receives the gn_part rows of the launch.  THE routing of dawn_conv_gemm, dawn_conv3x3_form and dawn_conv3x3_direct_form. */
static int conv3x3_transformed(const dawn_conv_desc& d, long M, hipStream_t s, int* nrows, bool dry) {
    const int p = policy_of(d);
    if (p & DAWN_POLICY_NINE_TERMS) return 0;
    if ((p & DAWN_POLICY_WINO4) && d.w_wino4 && dawn_conv3x3_wino4_try(d, M, p, s, nrows, dry)) return 2;
    if ((p & DAWN_POLICY_WINO2) && d.w_wino && dawn_conv3x3_wino_try(d, M, p, s, nrows, dry)) return 1;
#ifdef DAWN_WITH_STREAMK
    // (the stream-K kernel has no dry form: asked dry, 3 says that it MAY take the descriptor)
    if ((p & DAWN_POLICY_STREAMK) && d.sk_ws && (dry || dawn_conv3x3_sk_try(d, M, p, s, nrows))) return 3;
#endif
    return 0;
}

/* Which form of the 3x3 conv dawn_conv_gemm would run for this descriptor (host code, launches nothing): 2 = Winograd F(4x4,3x3),
 * 1 = Winograd F(2x2,3x3), 0 = anything else (direct split kernel, fp32 kernels, not a 3x3 conv).  The launch's own decision code
 * (conv3x3_transformed) -- for profiling labels and tests, instead of mirroring the policy bits and per-shape gates in the caller. */
extern "C" int dawn_conv3x3_form(const dawn_conv_desc* dp) {
    if (!dp || !conv3x3_split_path(*dp)) return 0;
    const int form = conv3x3_transformed(*dp, (long)dp->F * dp->Ho * dp->Wo, nullptr, nullptr, true);
    return form <= 2 ? form : 0;
}

/* The direct split-operand 3x3 kernels, in dawn_conv_gemm's order: conv3x3_bf16_v2_kernel with 256 x 64 or 256 x 128 tiles, then the v1 halo
 * kernel.  Launches the first that takes the descriptor (dry: launches nothing) and answers which (DAWN_DIRECT3X3_* of include/dawn_hip.h;
 * NONE: the fp32 kernels are next).  THE routing of dawn_conv_gemm and of dawn_conv3x3_direct_form. */
static int conv3x3_direct(const dawn_conv_desc& d, long M, hipStream_t s, bool nine, bool dry) {
    if (policy_of(d) & DAWN_POLICY_SPLIT_V2) {   // v2 structure (row-of-taps weight stages, register-prefetched patch)
        // 256 x 128 tiles run one 8-wave workgroup per CU: when they occupy at most half of the 256 CUs (M = 12,800 rows,
        // N = 256: 100 tiles), 256 x 64 tiles put one 4-wave workgroup on twice as many CUs and the launch takes
        // 0.67x the time (measured 520 -> 349 us at K = 9216, 142 -> 97 us at K = 2304; with 129..256 tiles the same
        // CUs stay busy either way and nothing is gained)
        // ... and at N = 128 with many tiles (level 1: 1600 narrow tiles): two 4-wave workgroups per CU (76 KB of LDS each)
        // overlap each other's prologue / epilogue, the 8-wave 128-column workgroup (108 KB) holds its CU alone:
        // 356 -> 314 us at M = 204,800, K = 1152 (no difference at N = 256 / 512 with 800 / 400 narrow tiles)
        const bool narrow = d.N <= 64 || (d.N % 64 == 0 && M % 256 == 0 && ((M / 256) * ((d.N + 127) / 128) <= 128 ||
                                                                          (d.N == 128 && (M / 256) * 2 >= 1536)));
        if (dawn_conv3x3_v2_try(d, M, s, nine, narrow, dry)) return narrow ? DAWN_DIRECT3X3_V2_WN1 : DAWN_DIRECT3X3_V2_WN2;
        if (narrow && d.N > 64 && dawn_conv3x3_v2_try(d, M, s, nine, false, dry)) return DAWN_DIRECT3X3_V2_WN2;
    }
    const bool ok = d.N <= 64 ? try_launch_halo_bf16<64, 1>(d, M, s, nine, dry) : try_launch_halo_bf16<128, 2>(d, M, s, nine, dry);
    return ok ? DAWN_DIRECT3X3_HALO : DAWN_DIRECT3X3_NONE;
}

/* Which direct split-operand 3x3 kernel dawn_conv_gemm would run for this descriptor (host code, launches nothing): DAWN_DIRECT3X3_HALO =
 * conv3x3_halo_bf16_kernel, _V2_WN1 / _V2_WN2 = conv3x3_bf16_v2_kernel with 256 x 64 (four waves) / 256 x 128 (eight waves) tiles, NONE when
 * the descriptor does not reach them: a split 1x1 / resample kernel or a Winograd form takes it, or it falls to the fp32 kernels.  The
 * launch's own decision code (conv3x3_direct), as dawn_conv3x3_form. */
extern "C" int dawn_conv3x3_direct_form(const dawn_conv_desc* dp) {
    if (!dp) return DAWN_DIRECT3X3_NONE;
    const dawn_conv_desc& d = *dp;
    if (d.C0 % 16 != 0 || d.C1 % 16 != 0 || d.C0 + d.C1 == 0 || (d.ld0 % 4) || (d.in1 && (d.ld1 % 4)) || d.border)
        return DAWN_DIRECT3X3_NONE;   // dawn_conv_gemm rejects these
    const long M = (long)d.F * d.Ho * d.Wo;
    if (M <= 0 || d.N <= 0 || !conv3x3_split_path(d) || split1x1_form(d, M) != DAWN_SPLIT1X1_NONE ||
        conv3x3_transformed(d, M, nullptr, nullptr, true) != 0)
        return DAWN_DIRECT3X3_NONE;
    return conv3x3_direct(d, M, nullptr, (policy_of(d) & DAWN_POLICY_NINE_TERMS) != 0, true);
}

/* Which split-operand kernel dawn_conv_gemm runs a 1x1 projection / 4x4 resample descriptor on (host code, launches nothing): the
 * launch's own decision code, as dawn_conv3x3_form for the 3x3 convs. */
extern "C" int dawn_gemm1x1_form(const dawn_conv_desc* dp) {
    if (!dp) return DAWN_SPLIT1X1_NONE;
    const dawn_conv_desc& d = *dp;
    return split1x1_form(d, d.mode == 0 ? (long)d.F * d.Ho * d.Wo : (long)d.F * d.Hi * d.Wi);
}

extern "C" int dawn_conv_gemm(const dawn_conv_desc* dp, void* stream) {
    const dawn_conv_desc d = *dp;
    const int Cin = d.C0 + d.C1;
    if (d.C0 % 16 != 0 || d.C1 % 16 != 0 || Cin == 0)
        return dawn_set_error_msg(-10, "dawn_conv_gemm: channel counts must be multiples of 16");
    if ((d.ld0 % 4) || (d.in1 && (d.ld1 % 4)) || (d.pro_add && (d.ld_add % 4)))
        return dawn_set_error_msg(-11, "dawn_conv_gemm: pixel strides must be multiples of 4 floats");
    if (d.mode == 1 && (d.KH != 2 || d.KW != 2 || d.Ho != 2 * d.Hi || d.Wo != 2 * d.Wi))
        return dawn_set_error_msg(-12, "dawn_conv_gemm: mode 1 expects 2x2 phase taps and 2x upsampling");
    if (d.border < 0 || d.border > 2 || (d.border && d.mode != 1))
        return dawn_set_error_msg(-15, "dawn_conv_gemm: border is 0 (zero), 1 (edge) or 2 (wrap), and non-zero only in mode 1");
    if ((d.ch_a || d.pro_add) && d.C1 != 0)
        return dawn_set_error_msg(-13, "dawn_conv_gemm: channel-affine / add prologue needs a single source");
    const long M = (d.mode == 0) ? (long)d.F * d.Ho * d.Wo : (long)d.F * d.Hi * d.Wi;
    if (M <= 0 || d.N <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int form1 = split1x1_form(d, M);
    if (d.ln_eps > 0.f && form1 == DAWN_SPLIT1X1_NONE)    // LayerNorm inside the GEMM: only the row-stationary kernels hold whole rows
        return dawn_set_error_msg(-14, "dawn_conv_gemm: ln_eps needs a split 1x1 projection with dawn_gemm1x1_ln_inline_ok, 16-byte aligned "
                                       "row strides and the split-kernel policy bits (DAWN_POLICY_SPLIT (0x1000) set, DAWN_POLICY_NO_ROW_KERNELS (0x20000) clear)");
    if (form1 != DAWN_SPLIT1X1_NONE) {
        if (form1 == DAWN_SPLIT1X1_ROWREG) dawn_gemm1x1_rowreg_launch(d, M, s);
        else if (form1 == DAWN_SPLIT1X1_ROWACC) dawn_gemm1x1_rowacc_launch(d, M, 0, s);
        else if (form1 == DAWN_SPLIT1X1_RESAMPLE) dawn_gemm1x1_rowacc_launch(d, M, d.mode == 0 ? 1 : 2, s);
        else dawn_gemm1x1_tiled_launch(d, M, s);
        DAWN_LAUNCH_CHECK();
        return 0;
    }
    if (conv3x3_split_path(d)) {
        int rows = 0;
        const bool transformed = conv3x3_transformed(d, M, s, &rows, false) != 0;
        if (transformed && d.gn_rows) *d.gn_rows = rows;      // (the direct kernels write it themselves)
        if (transformed || conv3x3_direct(d, M, s, (policy_of(d) & DAWN_POLICY_NINE_TERMS) != 0, false) != DAWN_DIRECT3X3_NONE) {
            DAWN_LAUNCH_CHECK();
            return 0;
        }
    }
    if ((policy_of(d) & DAWN_POLICY_HALO) && d.mode == 0 && d.KH == 3 && d.KW == 3 && d.stride == 1 && d.pad == 1 && d.Ho == d.Hi &&
        d.Wo == d.Wi && !d.ch_a && !d.pro_act && !d.pro_add && !d.row_mean) {
        const bool ok = d.N <= 64 ? try_launch_halo<64, 1>(d, M, s) : try_launch_halo<128, 2>(d, M, s);
        if (ok) {
            DAWN_LAUNCH_CHECK();
            return 0;
        }
    }
    const bool k32 = (policy_of(d) & DAWN_POLICY_BK32) && (d.C0 % 32 == 0) && (d.C1 % 32 == 0) && (d.KH * d.KW * Cin >= 4096);
    if (d.N <= 64) {
        if ((policy_of(d) & DAWN_POLICY_TILE256) && M >= 256 * 256) launch<256, 64, 16, 4, 1>(d, M, s);
        else launch<128, 64, 16, 2, 2>(d, M, s);
    } else {
        if (k32) launch<128, 128, 32, 2, 2>(d, M, s);
        else launch<128, 128, 16, 2, 2>(d, M, s);
    }
    DAWN_LAUNCH_CHECK();
    return 0;
}
