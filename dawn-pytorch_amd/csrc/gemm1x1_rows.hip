// The row-stationary split-operand GEMMs: gemm1x1_rowreg_kernel (short K, rows held in registers) and gemm1x1_rowacc_kernel (deep K /
// narrow N, and the 4x4 stride-2 resampling convs as implicit GEMMs).  Reached from dawn_conv_gemm's router (conv_gemm.hip) through
// dawn_gemm1x1_rowreg_launch / dawn_gemm1x1_rowacc_launch; which shapes they serve is decided there (gemm1x1_row*_fits,
// conv_resample_rowacc_ok).  The fetch-pattern ablation (DAWN_POLICY_ABL_ROW_FETCH) exists only in -DDAWN_ABLATION builds.
#include "conv_split.h"

namespace {

// Row-stationary split-operand GEMM for the short-K projections (K = 64 / 128: to_qkv and to_q of the 64 / 128-channel
// levels).  What bounds gemm1x1_bf16_kernel (gemm1x1_tiled.hip) there is not the matrix pipe: with 4..8 MFMA stages per tile its phases (fetch +
// split + LDS round trip of the A rows | MFMA | stores) run back to back and ADD (ablation at M = 204800, N = 768, K = 128:
// 465 us = 251 us with neither MFMAs nor stores + 86 us of MFMAs + 113 us of stores), and every one of the N / 128 column
// tiles of a row panel re-fetches and re-splits the same rows.  Here a lane owns ONE row (B operand of the transposed MFMA,
// 8 consecutive channels per k-step -- the layout of sla_c64_apply / xattn_c64): the wave reads its 32 rows once, normalises
// and splits them once into K/16 x 3 register fragments (96 VGPRs at K = 128) and keeps them while the workgroup walks the N
// dimension in 64-column chunks whose pre-split weights arrive by LDS-DMA (double-buffered, one barrier per chunk).  The
// activations never touch LDS, the split work per row drops by N / 128, waves only meet at the weight-chunk barrier, and a
// workgroup's (panel, chunk) range is balanced over the CUs to +-1 unit.
template <int KS>
__global__ __launch_bounds__(512) void gemm1x1_rowreg_kernel(const dawn_conv_desc d, const long M, const int units_per_wg) {
#if __HIP_DEVICE_COMPILE__
    constexpr int BM = 256, BNC = 64;                     // rows per panel (8 waves x 32), columns per chunk
    constexpr int CHB = KS * 6 * BNC * 16;                // bytes of one weight chunk: [KS][3 planes][2 k-halves][64 cols][16 B]
    constexpr int NDMA = KS * 6 / 8;                      // 1 KB DMA instructions per wave per chunk (KS = 4: 3, KS = 8: 6)
    static_assert(KS * 6 % 8 == 0, "weight DMA split");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int nCh = d.N / BNC;
    const long nunits = (M / BM) * nCh;
    const long u0 = (long)blockIdx.x * units_per_wg;
    const long u1 = u0 + units_per_wg < nunits ? u0 + units_per_wg : nunits;
    if (u0 >= u1) return;
    const int ld1 = d.in1 ? d.ld1 : d.ld0;
    const __amdgpu_buffer_rsrc_t rsw = DAWN_BUFFER(d.w_bf3, KS * 6 * d.N * 16);
    auto issueB = [&](long u, int buf) __attribute__((always_inline)) {
        const int n0 = (int)(u % nCh) * BNC;
#pragma unroll
        for (int j = 0; j < NDMA; ++j) {
            const int piece = j * 8 + wave;                // (kc, plane, k-half) row of the packed weights: 64 cols x 16 B
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (__attribute__((address_space(3))) void*)(smem_b + (size_t)buf * CHB + piece * 1024),
                                                     16, (unsigned)(lane * 16), (piece * d.N + n0) * 16, 0, 0);
        }
    };
    bf16x8 xs[KS][3];
    auto load_panel = [&](long panel) __attribute__((always_inline)) {
        const long r0 = panel * BM + wave * 32;            // wave-uniform first row
        const __amdgpu_buffer_rsrc_t ra = DAWN_BUFFER(d.in0 + r0 * d.ld0, 32 * d.ld0 * 4);
        const __amdgpu_buffer_rsrc_t rb = DAWN_BUFFER((d.in1 ? d.in1 : d.in0) + r0 * ld1, 32 * ld1 * 4);
        f32x4 raw[KS][2];
        // one per-lane byte offset per source (row l31, k-half); the channel chunk goes into the scalar / immediate offset (16 separate
        // offset registers otherwise, hoisted out of the unit loop)
        const unsigned vo0 = (unsigned)((l31 * d.ld0 + 8 * half) * 4), vo1 = (unsigned)((l31 * ld1 + 8 * half) * 4);
#ifdef DAWN_ABLATION
        // perf ablation (wrong results: the right bytes in the wrong lanes): 8 rows x 128 contiguous bytes per instruction instead of 32 rows x 32 bytes
        if (policy_raw_bit(d, DAWN_POLICY_ABL_ROW_FETCH)) {
#pragma unroll
            for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const int j = kc * 2 + h2, row = (lane >> 3) + 8 * (j & 3), ch = 4 * ((lane & 7) + 8 * (j >> 2));
                    raw[kc][h2] = __builtin_bit_cast(f32x4, ch < d.C0 ? __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)((row * d.ld0 + ch) * 4), 0, 0)
                                                                       : __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)((row * ld1 + ch - d.C0) * 4), 0, 0));
                }
        } else
#endif
#pragma unroll
        for (int kc = 0; kc < KS; ++kc) {
            const int cb = 16 * kc;                        // wave-uniform: C0 % 16 == 0
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
                raw[kc][h2] = __builtin_bit_cast(
                    f32x4, cb < d.C0 ? __builtin_amdgcn_raw_buffer_load_b128(ra, vo0, (cb + 4 * h2) * 4, 0)
                                     : __builtin_amdgcn_raw_buffer_load_b128(rb, vo1, (cb - d.C0 + 4 * h2) * 4, 0));
        }
        float mu = 0.f, rs = 1.f;
        if (d.row_mean) { mu = d.row_mean[r0 + l31]; rs = d.row_rstd[r0 + l31]; }
        if (d.ln_eps > 0.f) {
            // LayerNorm statistics of the lane's row from the registers: this lane holds one half of the K channels, its
            // xor-32 partner the other half (two-pass: mean, then biased variance of the centred values)
            float sm = 0.f;
#pragma unroll
            for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) sm += (raw[kc][h2].x + raw[kc][h2].y) + (raw[kc][h2].z + raw[kc][h2].w);
            sm += __shfl_xor(sm, 32, 64);
            mu = sm * (1.0f / (16 * KS));
            float sq = 0.f;
#pragma unroll
            for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const f32x4 dl = raw[kc][h2] - mu;
                    sq += (dl.x * dl.x + dl.y * dl.y) + (dl.z * dl.z + dl.w * dl.w);
                }
            sq += __shfl_xor(sq, 32, 64);
            rs = 1.0f / sqrtf(sq * (1.0f / (16 * KS)) + d.ln_eps);
        }
        const bool nrm = d.row_mean != nullptr || d.ln_eps > 0.f;
#pragma unroll
        for (int kc = 0; kc < KS; ++kc) {
            float v8[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v8[e] = raw[kc][0][e]; v8[4 + e] = raw[kc][1][e]; }
            if (nrm) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v8[e] = (v8[e] - mu) * rs;      // == dawn_ln_rows
            }
            dawn_split3_oct(v8, xs[kc][0], xs[kc][1], xs[kc][2]);
        }
    };

    // N = 64: one chunk for every unit -- the weights are fetched once and the waves never meet again
    const bool single = nCh == 1;
    long panel = u0 / nCh;
    issueB(u0, 0);
    load_panel(panel);
    for (long u = u0; u < u1; ++u) {
        const int cur = single ? 0 : (int)((u - u0) & 1);
        const long pn = u / nCh;
        bool full_wait = u == u0;
        if (pn != panel) { panel = pn; load_panel(panel); full_wait = true; }   // wave-uniform; rows of the new panel (no LDS involved)
        if (!single || u == u0) {
            // this chunk's weights (this wave's pieces) have landed.  VMEM operations complete in issue order: the 8 row-segment
            // stores of the previous chunk, issued after the weight request, may stay in flight
            if (full_wait) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
            __builtin_amdgcn_s_barrier();                               // ... everyone's; the other buffer is no longer read
            if (!single && u + 1 < u1) issueB(u + 1, cur ^ 1);
        }
        const unsigned char* Bb = smem_b + (size_t)cur * CHB;
        f32x16 acc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
        // weight fragments of k-step kc+1 are requested before the MFMAs of k-step kc (register double buffer): the LDS
        // latency hides under 12 MFMAs instead of stalling both waves of the SIMD at every step
        bf16x8 fb[2][2][3];
        auto read_frags = [&](int kc, int slot) __attribute__((always_inline)) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    fb[slot][j][pl] = *reinterpret_cast<const bf16x8*>(Bb + ((size_t)((kc * 3 + pl) * 2 + half) * BNC + j * 32 + l31) * 16);
        };
        read_frags(0, 0);
#pragma unroll
        for (int kc = 0; kc < KS; ++kc) {
            if (kc + 1 < KS) read_frags(kc + 1, (kc + 1) & 1);
            __builtin_amdgcn_sched_barrier(0);            // keep the requests above this step's MFMAs
            // (the cross-term tables with their roles swapped, here and in the row-accumulating kernel: _B picks the weight plane)
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[kc & 1][j][DAWN_SPLIT6_B[t]], xs[kc][DAWN_SPLIT6_A[t]], acc[j], 0, 0, 0);
                }
        }
        // ---- epilogue.  The accumulators hold lane = row, registers 4g..4g+3 = columns 8g + 4*half + {0..3}: stored directly,
        // one instruction touches 32 rows x 32 B = 32 cache lines, and the CU's address unit -- one line per cycle or so --
        // becomes the bottleneck (8 waves x 8 such stores = 4.4 k cycles per chunk, measured as 83 us of 309 that did not
        // overlap with anything).  Each 32 x 32 tile goes through a wave-private LDS staging tile instead and leaves as
        // 4 stores of 8 rows x 128 B: whole lines, a quarter of the line touches.
        const long m = panel * BM + wave * 32 + l31;
        const int n0 = (int)(u % nCh) * BNC;
        float* stg = reinterpret_cast<float*>(smem_b + 2 * CHB) + wave * (32 * 36);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + j * 32 + 8 * g + 4 * half;
                f32x4 v = {acc[j][4 * g], acc[j][4 * g + 1], acc[j][4 * g + 2], acc[j][4 * g + 3]};
                if (d.bias) v = v + *reinterpret_cast<const f32x4*>(d.bias + n);
                if (d.res) v = v + *reinterpret_cast<const f32x4*>(d.res + m * d.ld_res + n);
                if (d.tr) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(d.tr + m * d.ld_tr + n);
                    const f32x4 ta = *reinterpret_cast<const f32x4*>(d.tr_a + n), tb = *reinterpret_cast<const f32x4*>(d.tr_b + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += dawn_silu(t4[e] * ta[e] + tb[e]);
                }
                *reinterpret_cast<f32x4*>(stg + l31 * 36 + 8 * g + 4 * half) = v;
            }
            // (LDS operations of one wave execute in order: no barrier between the writes above and these reads)
            float* orow = d.out + (panel * BM + wave * 32 + (lane >> 3)) * d.ld_out + n0 + j * 32 + 4 * (lane & 7);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(stg + ((lane >> 3) + 8 * i) * 36 + 4 * (lane & 7));
                *reinterpret_cast<f32x4*>(orow + (long)(8 * i) * d.ld_out) = v;
            }
        }
    }
#endif
}

// Deep-K sibling of gemm1x1_rowreg_kernel for narrow outputs (N = 64 / 128 / 192: the cross-attention to_q projections of the
// 256..1024-channel blocks, K a multiple of 128): the wave keeps the accumulators of ALL its N / 64 column chunks (96 VGPRs at
// N = 192) and walks K in 128-channel blocks -- rows of the block fetched, normalised (row statistics supplied) and split once
// into registers, then one weight chunk per (K block, column chunk) step through the same double-buffered LDS-DMA pipeline.
// The tiled kernel re-split every row for each of its N / 64 column tiles and ran fetch | MFMA | store phases back to back.
// MODE 0: plain rows (1x1 projection).  MODE 1 / 2: the same pipeline as an implicit GEMM -- the strided 4x4 / stride-2 / pad-1
// convolution of Downsample (MT:176; a row = an output pixel, K block = 64 channels of one of the 16 taps) and the transposed 4x4
// convolution of Upsample as four output phases of 2x2 taps (MT:167; a row = an input pixel of one phase): the lane gathers
// its pixel's channels per tap through a per-frame buffer descriptor (padding = out-of-range offset = 0), everything else
// is unchanged.  These launches were the last convolutions on the fp32 matrix pipe.
template <int NCH, int KS, int MODE>
__global__ __launch_bounds__(512) void gemm1x1_rowacc_kernel(const dawn_conv_desc d, const long M, const int panels_per_wg) {
#if __HIP_DEVICE_COMPILE__
    // KS k-steps (16 channels each) per K block: 8 with one column chunk, 4 with two or three (up to 96 accumulator registers)
    constexpr int BM = 256, BNC = 64, KBC = 16 * KS;
    constexpr int CHB = KS * 6 * BNC * 16;
    constexpr int NDMA = KS * 6 / 8;
    static_assert(KS * 6 % 8 == 0, "weight DMA split");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int Ktot = (MODE == 0 ? 1 : (MODE == 1 ? 16 : 4)) * (d.C0 + d.C1);      // GEMM depth: taps x channels
    const int nKB = Ktot / KBC;
    const int cpb = d.C0 / KBC;                        // K blocks per tap (conv modes: single source)
    const long ppp = M / BM;                           // panels per phase (MODE 2: 4 phases, each over the M input pixels)
    // a unit = (row panel [x phase], group of NCH column chunks): N = ngrp * NCH * 64 (ngrp > 1 only for the resampling convs at
    // N = 256: the rows of a panel are then fetched and split once per group)
    const int ngrp = d.N / (NCH * BNC);
    const long npanels = (MODE == 2 ? 4 : 1) * ppp * ngrp;
    const long p0 = (long)blockIdx.x * panels_per_wg;
    const long p1 = p0 + panels_per_wg < npanels ? p0 + panels_per_wg : npanels;
    if (p0 >= p1) return;
    const int ld1 = d.in1 ? d.ld1 : d.ld0;
    const __amdgpu_buffer_rsrc_t rsw = DAWN_BUFFER(d.w_bf3, (MODE == 2 ? 4 : 1) * (Ktot / 16) * 6 * d.N * 16);
    auto issueB = [&](long unit, int kb, int c, int buf) __attribute__((always_inline)) {
        const long panel = unit / ngrp;
        const int cg = (int)(unit - panel * ngrp) * NCH;       // first column chunk of the unit's group
        const int phase = MODE == 2 ? (int)(panel / ppp) : 0;
#pragma unroll
        for (int j = 0; j < NDMA; ++j) {
            const int piece = phase * (Ktot / 16 * 6) + kb * (KS * 6) + j * 8 + wave;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsw, (__attribute__((address_space(3))) void*)(smem_b + (size_t)buf * CHB + (j * 8 + wave) * 1024),
                                                     16, (unsigned)(lane * 16), (piece * d.N + (cg + c) * BNC) * 16, 0, 0);
        }
    };
    bf16x8 xs[KS][3];
    float mu = 0.f, rs = 1.f;
    // conv modes: the lane's pixel of the current panel (set by locate())
    int pf = 0, py_ = 0, px_ = 0;                          // frame; MODE 1: top-left input coordinate (2 oy - 1, 2 ox - 1); MODE 2: (a, b)
    auto locate = [&](long panel) __attribute__((always_inline)) {
        if (MODE == 0) return;
        const long m = (MODE == 2 ? panel % ppp : panel) * BM + wave * 32 + l31;
        const int hw = MODE == 1 ? d.Ho * d.Wo : d.Hi * d.Wi;
        pf = (int)(m / hw);
        const int rem = (int)(m - (long)pf * hw);
        if (MODE == 1) { const int oy = rem / d.Wo; py_ = 2 * oy - 1; px_ = 2 * (rem - oy * d.Wo) - 1; }
        else { py_ = rem / d.Wi; px_ = rem - py_ * d.Wi; }
    };
    // the rows of K block kb of the wave's 32 rows -> `raw` (2 KS loads per lane; split_rows() turns them into the operand planes).  In the
    // implicit-GEMM modes the fetch of block kb + 1 is issued BEFORE the multiplies of block kb (round 5: fetch -> wait -> split -> multiply ran back to back
    // per block, every wave of the workgroup at the same point -- the barrier per step keeps them in lockstep --, so each block sat out
    // one full memory round trip: 10.7 k cycles per block against 3 k of matrix work at the level-0 resampling convs)
    f32x4 raw[KS][2];
    auto fetch_rows = [&](long panel, int kb) __attribute__((always_inline)) {
        if (MODE == 0) {
            const long r0 = panel * BM + wave * 32;
            const __amdgpu_buffer_rsrc_t ra = DAWN_BUFFER(d.in0 + r0 * d.ld0, 32 * d.ld0 * 4);
            const __amdgpu_buffer_rsrc_t rb = DAWN_BUFFER((d.in1 ? d.in1 : d.in0) + r0 * ld1, 32 * ld1 * 4);
            if (kb == 0 && d.row_mean) { mu = d.row_mean[r0 + l31]; rs = d.row_rstd[r0 + l31]; }
            const int lrow = l31;
#ifdef DAWN_ABLATION
            // perf ablation (wrong results: the right bytes in the wrong lanes): the same 32 rows x 64 channels, fetched as 8 rows x 128 contiguous
            // bytes per instruction (8 line touches instead of 32) -- what would a coalesced fetch + a free transpose buy?
            if (policy_raw_bit(d, DAWN_POLICY_ABL_ROW_FETCH)) {
#pragma unroll
                for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int j = kc * 2 + h2, row = (lane >> 3) + 8 * (j & 3), piece = (lane & 7) + 8 * (j >> 2);
                        const int cb = kb * KBC + 4 * piece;
                        raw[kc][h2] = __builtin_bit_cast(
                            f32x4, kb * KBC < d.C0 ? __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)((row * d.ld0 + cb) * 4), 0, 0)
                                                   : __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)((row * ld1 + cb - d.C0) * 4), 0, 0));
                    }
            } else
#endif
#pragma unroll
            for (int kc = 0; kc < KS; ++kc) {
                const int cb = kb * KBC + 16 * kc;             // wave-uniform: C0 % 16 == 0
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
                    raw[kc][h2] = __builtin_bit_cast(
                        f32x4, cb < d.C0 ? __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)((lrow * d.ld0 + cb + 8 * half + 4 * h2) * 4), 0, 0)
                                         : __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)((lrow * ld1 + cb - d.C0 + 8 * half + 4 * h2) * 4), 0, 0));
            }
        } else {
            // a 32-pixel tile lies in one frame (host check): frame-sized descriptor, the lane's offset = its tap pixel
            const int fr = __builtin_amdgcn_readfirstlane(pf);
            const __amdgpu_buffer_rsrc_t ra = DAWN_BUFFER(d.in0 + (long)fr * d.Hi * d.Wi * d.ld0, d.Hi * d.Wi * d.ld0 * 4);
            const int tap = kb / cpb, c0 = (kb - tap * cpb) * KBC;
            int iy, ix;
            if (MODE == 1) { iy = py_ + (tap >> 2); ix = px_ + (tap & 3); }
            else {
                const int phase = (int)(panel / ppp), ppy = phase >> 1, ppx = phase & 1;
                iy = py_ + ((tap >> 1) ? (ppy ? 1 : -1) : 0);
                ix = px_ + ((tap & 1) ? (ppx ? 1 : -1) : 0);
                if (d.border) {        // (uniform) outside taps read the edge / the opposite edge instead of zero: always in range below
                    iy = dawn_border_coord(iy, d.Hi, d.border);
                    ix = dawn_border_coord(ix, d.Wi, d.border);
                }
            }
            const bool inb = iy >= 0 && iy < d.Hi && ix >= 0 && ix < d.Wi;
            unsigned off = inb ? (unsigned)(((iy * d.Wi + ix) * d.ld0 + c0 + 8 * half) * 4) : 0xffffff00u;   // padding reads 0
#ifdef DAWN_ABLATION
            // perf ablation (wrong results by design): every lane gathers the pixel of lane 0 -- one cache line per instruction instead of 32:
            // what do the scattered line touches of the gather cost?
            if (policy_raw_bit(d, DAWN_POLICY_ABL_ROW_FETCH)) {
                // ... as MODE 0: 8 pixels x 128 contiguous bytes per instruction; the pixel's offset comes from the lane that owns it
                const unsigned pbase = inb ? off - (unsigned)(8 * half * 4) : 0xffffff00u;
#pragma unroll
                for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                    for (int h2 = 0; h2 < 2; ++h2) {
                        const int j = kc * 2 + h2, row = (lane >> 3) + 8 * (j & 3), piece = (lane & 7) + 8 * (j >> 2);
                        const unsigned pb = (unsigned)__shfl((int)pbase, row, 64);
                        raw[kc][h2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, pb >= 0xffffff00u ? pb : pb + (unsigned)(16 * piece), 0, 0));
                    }
            } else
#endif
#pragma unroll
            for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
                    raw[kc][h2] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, inb ? off + (unsigned)((16 * kc + 4 * h2) * 4) : off, 0, 0));
        }
    };
    auto split_rows = [&]() __attribute__((always_inline)) {
        // (nothing of the split moves above this point: the scheduler otherwise hoists it -- and the wait for the rows in flight -- in front
        //  of the previous block's multiplies once both sit in one basic block, which is exactly the overlap the prefetch is for)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kc = 0; kc < KS; ++kc) {
            float v8[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { v8[e] = raw[kc][0][e]; v8[4 + e] = raw[kc][1][e]; }
            if (MODE == 0 && (d.row_mean || d.ln_eps > 0.f)) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v8[e] = (v8[e] - mu) * rs;      // == dawn_ln_rows
            }
            dawn_split3_oct(v8, xs[kc][0], xs[kc][1], xs[kc][2]);
        }
    };
    // LayerNorm inside the GEMM (dawn_conv_desc.ln_eps, MODE 0): one statistics sweep over the panel's rows before its K loop
    // (the rows come back from L2 for the GEMM sweep: 32 KB per wave) -- shifted one-pass sums, both halves of a row combined by one
    // xor-32 exchange.  Shift = the mean of the row's first 16 channels (C0 >= 16; each half sums its 8, the same sum in both lanes), so
    // that E[d^2] - E[d]^2 does not cancel: with the first channel alone as the shift, a row whose first channel lies 3..4 sigma off its
    // mean has E[d]^2 = 10..16 Var, and 1 / sigma came out wrong by 3.2e-6 (K = 512) and 5.0e-6 (K = 1024) of its value, 9.3x the error
    // of an fp32 GEMM in the result (tests/split_gate.py, C_ROWACC_LN); 16 channels put the shift within sigma / 4 of the mean
    auto ln_stats = [&](long panel) __attribute__((always_inline)) {
        const long r0 = panel * BM + wave * 32;
        const __amdgpu_buffer_rsrc_t ra = DAWN_BUFFER(d.in0 + r0 * d.ld0, 32 * d.ld0 * 4);
        const __amdgpu_buffer_rsrc_t rb = DAWN_BUFFER((d.in1 ? d.in1 : d.in0) + r0 * ld1, 32 * ld1 * 4);
        float shift;
        {
            const f32x4 a = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)((l31 * d.ld0 + 8 * half) * 4), 0, 0));
            const f32x4 b = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)((l31 * d.ld0 + 8 * half + 4) * 4), 0, 0));
            const float h8 = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w));
            shift = (h8 + __shfl_xor(h8, 32, 64)) * (1.0f / 16);
        }
        float s1 = 0.f, s2 = 0.f;
        for (int kb = 0; kb < nKB; ++kb) {
            f32x4 raw[KS][2];
#pragma unroll
            for (int kc = 0; kc < KS; ++kc) {
                const int cb = kb * KBC + 16 * kc;
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2)
                    raw[kc][h2] = __builtin_bit_cast(
                        f32x4, cb < d.C0 ? __builtin_amdgcn_raw_buffer_load_b128(ra, (unsigned)((l31 * d.ld0 + cb + 8 * half + 4 * h2) * 4), 0, 0)
                                         : __builtin_amdgcn_raw_buffer_load_b128(rb, (unsigned)((l31 * ld1 + cb - d.C0 + 8 * half + 4 * h2) * 4), 0, 0));
            }
#pragma unroll
            for (int kc = 0; kc < KS; ++kc)
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const f32x4 dl = raw[kc][h2] - shift;
                    s1 += (dl.x + dl.y) + (dl.z + dl.w);
                    s2 += (dl.x * dl.x + dl.y * dl.y) + (dl.z * dl.z + dl.w * dl.w);
                }
        }
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        const float invk = 1.0f / (float)(d.C0 + d.C1);
        const float md = s1 * invk;
        mu = shift + md;
        rs = 1.0f / sqrtf(fmaxf(s2 * invk - md * md, 0.f) + d.ln_eps);
    };
    f32x16 acc[NCH][2];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[c][j][r] = 0.f;
    float* stg = reinterpret_cast<float*>(smem_b + 2 * CHB) + wave * (32 * 36);
    int buf = 0;
    // (row prefetch: the resampling convs only -- the 1x1 variants hold 228..256 registers without the 32 / 64 of a block in flight)
    // (tried for the N = 128 projections as well: 10 spilled registers, -2 %: not worth the scratch)
    constexpr bool PRE = MODE != 0;
    // ... across units too for the transposed conv (K = 4 taps x C: 4..16 blocks per unit, the first one a quarter of them); the strided conv
    // (16 taps) measured faster with its first block fetched at the top of the unit (profiles/r5_resample_row_prefetch.txt)
    constexpr bool CROSS = MODE == 2;
    issueB(p0, 0, 0, 0);
    if (CROSS) { locate(p0 / ngrp); fetch_rows(p0 / ngrp, 0); }     // the workgroup's very first block: nothing to hide it behind
    for (long unit = p0; unit < p1; ++unit) {
        const long panel = unit / ngrp;
        const int cg = (int)(unit - panel * ngrp) * NCH;
        if (!CROSS) locate(panel);
        if (MODE == 0 && d.ln_eps > 0.f) ln_stats(panel);
        for (int kb = 0; kb < nKB; ++kb) {
            if (!PRE || (!CROSS && kb == 0)) fetch_rows(panel, kb);
            split_rows();
            const bool last_kb = kb == nKB - 1;
            // the NEXT block's rows -- of this unit, or the first block of the next one (under this unit's last multiplies and epilogue) --
            // go out here, in flight under this block's multiplies.  ONE fetch site in the loop: with two, the compiler copies the
            // loaded registers into the loop-carried ones right away and waits for every load in front of the multiplies
            bool pre_issued = false;
            if (PRE) {
                long npanel = panel;
                int nkb = kb + 1;
                pre_issued = true;
                if (last_kb) {
                    nkb = 0;
                    pre_issued = CROSS && unit + 1 < p1;
                    npanel = (unit + 1) / ngrp;
                    if (pre_issued) locate(npanel);         // (locate() state is only read by fetch_rows: nothing of this unit needs it any more)
                }
                if (pre_issued) fetch_rows(npanel, nkb);
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                // weights of this step have landed (requested one step ago; VMEM completes in issue order: after an epilogue
                // with no row fetch since, its 8 stores may stay in flight; behind the row prefetch just issued, its 2 KS loads may)
                if (c > 0 && last_kb && !(d.bias || d.res || d.tr)) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                else if (c == 0 && pre_issued) { if (KS == 4) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); }
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                {   // request the next step's chunk into the other buffer
                    int nkb = kb, nc = c + 1;
                    long npan = unit;
                    if (nc == NCH) { nc = 0; nkb = kb + 1; if (nkb == nKB) { nkb = 0; npan = unit + 1; } }
                    if (c + 1 < NCH || kb + 1 < nKB || unit + 1 < p1) issueB(npan, nkb, nc, buf ^ 1);
                }
                const unsigned char* Bb = smem_b + (size_t)buf * CHB;
                // weight fragments: double-buffered over the k-steps where the register budget allows (one column chunk)
                constexpr int NFB = NCH == 1 ? 2 : 1;
                bf16x8 fb[NFB][2][3];
                auto read_frags = [&](int kc, int slot) __attribute__((always_inline)) {
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            fb[slot][j][pl] = *reinterpret_cast<const bf16x8*>(Bb + ((size_t)((kc * 3 + pl) * 2 + half) * BNC + j * 32 + l31) * 16);
                };
                if (NFB == 2) read_frags(0, 0);
#pragma unroll
                for (int kc = 0; kc < KS; ++kc) {
                    if (NFB == 2) {
                        if (kc + 1 < KS) read_frags(kc + 1, (kc + 1) & 1);
                        __builtin_amdgcn_sched_barrier(0);
                    } else {
                        read_frags(kc, 0);
                    }
#pragma unroll
                    for (int t = 0; t < 6; ++t)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc[c][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[NFB == 2 ? (kc & 1) : 0][j][DAWN_SPLIT6_B[t]], xs[kc][DAWN_SPLIT6_A[t]], acc[c][j], 0, 0, 0);
                }
                buf ^= 1;
                if (last_kb) {
                    const long m = (MODE == 2 ? panel % ppp : panel) * BM + wave * 32 + l31;      // GEMM row of the lane (residual / tr index)
                    const int n0 = (cg + c) * BNC;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const int n = n0 + j * 32 + 8 * g + 4 * half;
                            f32x4 v = {acc[c][j][4 * g], acc[c][j][4 * g + 1], acc[c][j][4 * g + 2], acc[c][j][4 * g + 3]};
                            if (d.bias) v = v + *reinterpret_cast<const f32x4*>(d.bias + n);
                            if (d.res) v = v + *reinterpret_cast<const f32x4*>(d.res + m * d.ld_res + n);
                            if (d.tr) {
                                const f32x4 t4 = *reinterpret_cast<const f32x4*>(d.tr + m * d.ld_tr + n);
                                const f32x4 ta = *reinterpret_cast<const f32x4*>(d.tr_a + n), tb = *reinterpret_cast<const f32x4*>(d.tr_b + n);
#pragma unroll
                                for (int e = 0; e < 4; ++e) v[e] += dawn_silu(t4[e] * ta[e] + tb[e]);
                            }
                            *reinterpret_cast<f32x4*>(stg + l31 * 36 + 8 * g + 4 * half) = v;
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[c][j][4 * g + e] = 0.f;
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            long orow_i = (MODE == 2 ? panel % ppp : panel) * BM + wave * 32 + (lane >> 3) + 8 * i;
                            if (MODE == 2) {           // input pixel (a, b) of phase (ppy, ppx) -> output pixel (2a + ppy, 2b + ppx)
                                const int phase = (int)(panel / ppp), hw = d.Hi * d.Wi;
                                const int f = (int)(orow_i / hw), rem = (int)(orow_i - (long)f * hw);
                                const int a_ = rem / d.Wi, b_ = rem - a_ * d.Wi;
                                orow_i = ((long)f * d.Ho + 2 * a_ + (phase >> 1)) * d.Wo + 2 * b_ + (phase & 1);
                            }
                            *reinterpret_cast<f32x4*>(d.out + orow_i * d.ld_out + n0 + j * 32 + 4 * (lane & 7)) =
                                *reinterpret_cast<const f32x4*>(stg + ((lane >> 3) + 8 * i) * 36 + 4 * (lane & 7));
                        }
                    }
                }
            }
        }
    }
#endif
}

template <int MODE>
static void launch_rowacc(const dawn_conv_desc& d, long M, hipStream_t s) {
    int nch = d.N == 64 ? 1 : ((d.N == 128 || d.N == 256) ? 2 : 3);
    const int ncu = dawn_ncu();
    const int Ktot = (MODE == 0 ? 1 : (MODE == 1 ? 16 : 4)) * (d.C0 + d.C1);
    // the deepest level (M = 12,800: 50 row panels) leaves most CUs without a workgroup: one 64-column chunk per unit there -- the
    // rows of a panel are fetched and split once per chunk instead of once per 2..3, on 2..3x as many CUs
    if (nch > 1 && (MODE == 2 ? 4 : 1) * (M / 256) * (d.N / (nch * 64)) * 2 <= ncu && (MODE != 0 || Ktot % 128 == 0)) nch = 1;
    const long npanels = (MODE == 2 ? 4 : 1) * (M / 256) * (d.N / (nch * 64));
    const int per = (int)((npanels + ncu - 1) / ncu);
    const int nwg = (int)((npanels + per - 1) / per);
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
#define LAUNCH_RA(NCHV, KSV)                                                                                              \
    do {                                                                                                                  \
        const size_t lds = (size_t)2 * KSV * 6 * 64 * 16 + 8 * 32 * 36 * 4;                                               \
        (void)hipFuncSetAttribute((const void*)gemm1x1_rowacc_kernel<NCHV, KSV, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
        hipLaunchKernelGGL((gemm1x1_rowacc_kernel<NCHV, KSV, MODE>), dim3(nwg), dim3(512), lds, s, d, M, per);             \
    } while (0)
    if (nch == 1) { if constexpr (MODE == 0) LAUNCH_RA(1, 8); else LAUNCH_RA(1, 4); }
    else if (nch == 2) LAUNCH_RA(2, 4);
    else { if constexpr (MODE == 0) LAUNCH_RA(3, 4); }
#undef LAUNCH_RA
}

}  // namespace

void dawn_gemm1x1_rowreg_launch(const dawn_conv_desc& d, long M, hipStream_t s) {
    const int K = d.C0 + d.C1;
    const long nunits = (M / 256) * (d.N / 64);
    const int ncu = dawn_ncu();
    const int per = (int)((nunits + ncu - 1) / ncu);
    const int nwg = (int)((nunits + per - 1) / per);
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
    const size_t lds = (size_t)2 * (K / 16) * 6 * 64 * 16 + 8 * 32 * 36 * 4;      // two weight chunks + the waves' staging tiles
    if (K == 128) {
        (void)hipFuncSetAttribute((const void*)gemm1x1_rowreg_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((gemm1x1_rowreg_kernel<8>), dim3(nwg), dim3(512), lds, s, d, M, per);
    } else {
        (void)hipFuncSetAttribute((const void*)gemm1x1_rowreg_kernel<4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((gemm1x1_rowreg_kernel<4>), dim3(nwg), dim3(512), lds, s, d, M, per);
    }
}

void dawn_gemm1x1_rowacc_launch(const dawn_conv_desc& d, long M, int mode, hipStream_t s) {
    if (mode == 0) launch_rowacc<0>(d, M, s);
    else if (mode == 1) launch_rowacc<1>(d, M, s);
    else launch_rowacc<2>(d, M, s);
}
