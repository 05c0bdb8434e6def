// The tiled split-operand 1x1 GEMM (gemm1x1_bf16_kernel) and its launchers.  Reached from dawn_conv_gemm's router (conv_gemm.hip)
// through dawn_gemm1x1_tiled_launch when split1x1_form answers DAWN_SPLIT1X1_TILED.
#include <type_traits>

#include "conv_split.h"

namespace {

// Split-operand GEMM for the large prologue-free 1x1 projections (to_qkv after dawn_ln_rows, to_out + residual):
// out (M x N) = A (M x K, fp32 rows) . W, on the bf16 matrix pipe with the exact 3-way operand split and 6 cross
// terms (see conv3x3_halo_bf16_kernel, conv_gemm.hip).  256 x 128 tile, 8 waves (64 x 64 each), K consumed 32 channels per stage:
// the A rows of stage s+2 are in flight as register loads, those of stage s+1 are split between the MFMAs of
// stage s and written to the idle plane buffer, the pre-split weights arrive by LDS-DMA one stage ahead -- one
// barrier per 48 MFMAs per wave.  Accumulated transposed (lane = row) -> 16-byte row-segment stores.
template <int NT, int WN, int CFG = 0>
__global__ __launch_bounds__(256 * (CFG ? 1 : WN)) void gemm1x1_bf16_kernel(const dawn_conv_desc d, const long M) {
#if __HIP_DEVICE_COMPILE__
    // BN = 64*WN output columns, 4*WN waves (64 x 64 each).  WN = 1 serves N % 64 == 0 (to_q: 192 columns, the 64-channel
    // res_conv) and small tile counts; the A rows may come from two channel-concatenated sources (stage s reads in0 while
    // 32 s < C0, in1 afterwards) -- the up-path res_conv / to_q of cat[x, skip] without materialising the cat.
    // CFG 1: 128 x 64 tile, 4 waves as 2 (M) x 2 (N) of 64 x 32 each -- 77 KB of LDS, so TWO workgroups share a CU and one's
    // A-row fetch / epilogue stores overlap the other's MFMAs.  The 256-row tiles hold a CU alone (126..150 KB): with the
    // short K of the projections (4..16 stages) a tile is fetch -> MFMA -> store in sequence, each ~5 us, and the per-CU
    // share of HBM bandwidth (25 GB/s) is idle two thirds of the time.
    constexpr int BM = CFG ? 128 : 256, BN = CFG ? 64 : 64 * WN, NTHR = CFG ? 256 : 256 * WN, NW = CFG ? 4 : 4 * WN;
    constexpr int WNN = CFG ? 2 : WN;                          // waves along N
    constexpr int TM = 2, TN = CFG ? 1 : 2;
    constexpr int NQ = BM * 8 / NTHR;                          // A quads per thread per stage (4 or 8)
    static_assert(NQ == 4 || NQ == 8, "the stage wait below names NQ as an immediate");
    constexpr int HPS = BM * 16 + 128;                         // half-plane stride (bytes)
    // a sub-chunk's six half planes + 64 bytes: a wave's plane write covers 8 rows x (2 sub-chunks x 2 k-halves x 8 + 8 bytes); with the k-halves
    // 128 B apart modulo the 256 B of the banks (HPS) and the sub-chunks 64 B apart (SPS) the 32 lanes of a write pass hit 64 different banks
    constexpr int SPS = 6 * HPS + 64;
    constexpr int PSZ = 2 * SPS;                               // planes of one stage (2 sub-chunks of 16 channels)
    constexpr int BSZ = 2 * 6 * BN * 16;                       // weights of one stage
    constexpr int NBI = BSZ / 1024;                            // DMA wave-instructions per stage: 3 per wave
    static_assert(NBI == 3 * NW, "weight DMA split");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    unsigned char* planes = smem_b;                            // [2 stages][2 sub][3 planes][2 halves][HPS]
    unsigned char* Bs = smem_b + 2 * PSZ;                      // [2 stages][2 sub][3][2][BN][16 B]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WNN, wn = wave % WNN;
    const int l31 = lane & 31, half = lane >> 5;
    const int K = d.C0 + d.C1;
    const int nS = K / 32, nS0 = d.C0 / 32;
    const int nNt = d.N / BN;
    // workgroups are dealt round-robin to the 8 XCDs, each with its own L2: the tiles of one row panel (all nNt column tiles read
    // the same A rows) go to ONE XCD -- XCD x walks the contiguous tile range [x q + min(x, r), ...) of the row-major tile order
    // (q = tiles / 8, r = tiles % 8), so a row panel comes over the fabric once instead of once per XCD that holds a column tile
    int tile = blockIdx.x;
    if (!policy_raw_bit(d, DAWN_POLICY_XCD_LAUNCH_ORDER)) {
        const int nT = gridDim.x, q = nT >> 3, r = nT & 7, x = tile & 7, j = tile >> 3;
        tile = x * q + (x < r ? x : r) + j;
    }
    const int mt = tile / nNt, nt = tile - mt * nNt;
    const long m0 = (long)mt * BM;
    const int n0 = nt * BN;
    const int ld1 = d.in1 ? d.ld1 : d.ld0;
    const __amdgpu_buffer_rsrc_t rsa = DAWN_BUFFER(d.in0 + m0 * d.ld0, BM * d.ld0 * 4);
    const __amdgpu_buffer_rsrc_t rsa1 = DAWN_BUFFER((d.in1 ? d.in1 : d.in0) + m0 * ld1, BM * ld1 * 4);
    const __amdgpu_buffer_rsrc_t rsw = DAWN_BUFFER(d.w_bf3, (K / 16) * 6 * d.N * 16);
    // A quads of a stage: BM rows x 8 quads -> NQ per thread: q = tid + NTHR i -> row = q >> 3, quad = q & 7
    const int row0 = tid >> 3, qoff = (tid & 7) * 16;
    unsigned voffB[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int idx = (j * NW + wave) * 64 + lane;           // 16-byte piece within the stage
        const int sub = idx / (6 * BN), rem = idx - sub * (6 * BN);
        const int ph = rem / BN, n = rem - ph * BN;
        voffB[j] = (unsigned)((((sub * 6 + ph) * d.N) + n0 + n) * 16);
    }
    f32x4 araw[2][NQ];
    uint2 ap[NQ][3];
    // optional LayerNorm prologue (PreNorm / LayerNorm_img with the gain folded into the weights): A = (x - mean[row]) *
    // rstd[row], applied to the row quads right before the operand split -- the same arithmetic as dawn_ln_rows, so the
    // result is bit-identical to the GEMM on materialised normalised rows, without writing and re-reading them
    const bool norm = d.row_mean != nullptr;
    float rmu[NQ], rrs[NQ];
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const long row = m0 + row0 + (NTHR >> 3) * i;
        rmu[i] = norm ? d.row_mean[row] : 0.f;
        rrs[i] = norm ? d.row_rstd[row] : 1.f;
    }
    auto splitq = [&](int slot, int qi) {
#pragma clang fp contract(off)          // the normalised value is ROUNDED before its split (as dawn_ln_rows stores it)
        f32x4 v = slot ? araw[1][qi] : araw[0][qi];
        v = (v - rmu[qi]) * rrs[qi];                           // (without a prologue: mean 0, rstd 1 -- exact)
        asm volatile("" : "+v"(v));                         // (the split's first residual must not fuse with the product either)
        dawn_split3_rne_quad(v, ap[qi][0], ap[qi][1], ap[qi][2]);
    };
    auto loadA = [&](int s, int slot) {
        const bool src1 = s >= nS0;                            // wave-uniform
        const int ldb = (src1 ? ld1 : d.ld0) * 4;
        const int soff = (src1 ? s - nS0 : s) * 128;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const unsigned voff = (unsigned)((row0 + (NTHR >> 3) * i) * ldb + qoff);
            araw[slot][i] = __builtin_bit_cast(f32x4, src1 ? __builtin_amdgcn_raw_buffer_load_b128(rsa1, voff, soff, 0)
                                                           : __builtin_amdgcn_raw_buffer_load_b128(rsa, voff, soff, 0));
        }
    };
    auto writeA = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int q = tid + NTHR * i;
            const int row = q >> 3, quad = q & 7;               // quad: sub-chunk = quad >> 2, k-half = (quad >> 1) & 1
            unsigned char* dst = planes + (size_t)buf * PSZ + (size_t)(quad >> 2) * SPS + (size_t)((quad >> 1) & 1) * HPS +
                                 row * 16 + (quad & 1) * 8;
            *reinterpret_cast<uint2*>(dst) = ap[i][0];
            *reinterpret_cast<uint2*>(dst + 2 * HPS) = ap[i][1];
            *reinterpret_cast<uint2*>(dst + 4 * HPS) = ap[i][2];
        }
    };
    auto issueB = [&](int s, int buf) {
        const int soff = s * 2 * 6 * d.N * 16;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                rsw, (__attribute__((address_space(3))) void*)(Bs + (size_t)buf * BSZ + (j * NW + wave) * 1024), 16, voffB[j], soff, 0, 0);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // every stage wait below (vmcnt(NQ)) counts the A-row loads as the YOUNGEST NQ memory operations: the weight DMA of a stage
    // is issued before its A rows, and the sched_barrier keeps the scheduler from moving either across the other
    issueB(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    loadA(0, 0);
    loadA(nS > 1 ? 1 : 0, 1);
#pragma unroll
    for (int i = 0; i < NQ; ++i) splitq(0, i);
    writeA(0);
    // One stage = ONE basic block (round 6): every fetch / split / plane write of a stage is unconditional -- past the end of K the
    // stage index is clamped, so the last stages re-fetch valid bytes into buffers nobody reads again -- and the register slot of
    // the A rows is a compile-time constant of the stage's parity.  Before, `if (s + 1 < nS)` around the splits put them into a
    // basic block of their own BEHIND the stage's MFMAs: a wave issued 12 MFMAs (its issue port blocked for 12 x 32 cycles), then
    // ~70 vector instructions with the matrix pipe idle (SQ counters of the M = 12,800 launches: matrix pipe 21 % busy, vector ALU
    // 26 %, LDS 28 %, 1.4 waves per SIMD -- the three in sequence, profiles/r6_gemm1x1_deep_pmc.md).  Now the scheduling groups
    // below put the split arithmetic BETWEEN the MFMAs of the same wave.
    auto stage = [&](auto PARC, const int s) {
        constexpr int PAR = decltype(PARC)::value;           // s & 1: plane / weight buffer of this stage, register slot of stage s + 2
        // the weights of stage s (LDS-DMA) must have landed; the A rows of stage s+1 -- the NQ youngest loads, issued after that DMA --
        // may stay in flight (vmcnt retires in order): they are first read by the splits between this stage's MFMAs
        if constexpr (NQ == 4) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();       // planes(s) + weights(s) complete; buffers of stage s-1 are free
        issueB(s + 1 < nS ? s + 1 : nS - 1, PAR ^ 1);
        __builtin_amdgcn_sched_barrier(0);  // (the weight DMA before the A rows: the vmcnt(NQ) above relies on that order)
        // stage s+2's rows go into the register slot stage s used (split during stage s-1): a stage and a half ahead of their split
        loadA(s + 2 < nS ? s + 2 : nS - 1, PAR);
        __builtin_amdgcn_sched_barrier(0);  // (the fetches stay at the top of the stage)
        const unsigned char* Pb = planes + (size_t)PAR * PSZ;
        const unsigned char* Bb = Bs + (size_t)PAR * BSZ;
        bf16x8 fa[2][TM][3], fb[2][TN][3];
        auto read_frags = [&](const int sub) {
            constexpr int RA[3] = {2, 0, 1}, RB[3] = {0, 2, 1};
#pragma unroll
            for (int g = 0; g < 3; ++g) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    fa[sub][i][RA[g]] = *reinterpret_cast<const bf16x8*>(Pb + (size_t)sub * SPS + (size_t)(RA[g] * 2 + half) * HPS +
                                                                          (wm * 64 + i * 32 + l31) * 16);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    fb[sub][j][RB[g]] = *reinterpret_cast<const bf16x8*>(
                        Bb + ((size_t)((sub * 6 + RB[g] * 2 + half) * BN + wn * (32 * TN) + j * 32 + l31)) * 16);
            }
        };
        // the split of one PAIR of A values in three steps of 5 / 5 / 3 vector instructions (the arithmetic of
        // dawn_split3_rne_quad, dawn_common.h, in its order; staged by hand because a call cannot be cut into steps):
        // one step goes behind each MFMA, so the vector ALU works while the matrix pipe runs that MFMA (8 issue slots)
        constexpr int NMF = NT * TM * TN, NSTEP = 3 * NQ;       // per half stage: MFMAs; split steps (NQ pairs: NQ / 2 quads)
        f32x2 px[NQ], pe[NQ];
        auto split_step = [&](const int sub, const int k) {
#pragma clang fp contract(off)      // the normalised value is ROUNDED before its split (as dawn_ln_rows stores it): no fma of the product into the residual
            typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
            const int pr = k / 3, st = k - 3 * pr;
            const int qi = sub * (NQ / 2) + (pr >> 1), e = pr & 1;
            bf16x2 h;
            if (st == 0) {
                const f32x4 q4 = (PAR ^ 1) ? araw[1][qi] : araw[0][qi];
                f32x2 x = {q4[2 * e], q4[2 * e + 1]};
                x = (x - rmu[qi]) * rrs[qi];                      // (without a prologue: mean 0, rstd 1 -- exact)
                h[0] = (__bf16)x[0]; h[1] = (__bf16)x[1];
                px[pr] = x;
                pe[pr][0] = (float)h[0]; pe[pr][1] = (float)h[1];
            } else if (st == 1) {
                const f32x2 x = px[pr] - pe[pr];
                h[0] = (__bf16)x[0]; h[1] = (__bf16)x[1];
                px[pr] = x;
                pe[pr][0] = (float)h[0]; pe[pr][1] = (float)h[1];
            } else {
                const f32x2 x = px[pr] - pe[pr];
                h[0] = (__bf16)x[0]; h[1] = (__bf16)x[1];
            }
            const unsigned hb = __builtin_bit_cast(unsigned, h);
            if (e == 0) ap[qi][st].x = hb; else ap[qi][st].y = hb;
        };
        // fences: MFMA and vector ALU instructions keep the order written here; LDS / global / scalar instructions may cross
        constexpr int FENCE = 0x4 | 0x10 | 0x20 | 0x40 | 0x80 | 0x100 | 0x200;
        read_frags(0);
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int m = 0; m < NMF; ++m) {
                const int t = 9 - NT + m / (TM * TN), i = (m / TN) % TM, j = m % TN;
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[sub][j][DAWN_SPLIT9_B[t]], fa[sub][i][DAWN_SPLIT9_A[t]], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int k = 0; k < NSTEP; ++k)
                    if (k * NMF / NSTEP == m) split_step(sub, k);
                if (sub == 0 && m == NMF / 2) read_frags(1);
                __builtin_amdgcn_sched_barrier(FENCE);
            }
        }
        writeA(PAR ^ 1);                    // readers of that buffer (stage s-1) passed the barrier above
    };
    for (int s = 0; s < nS; s += 2) {
        stage(std::integral_constant<int, 0>{}, s);
        if (s + 1 < nS) stage(std::integral_constant<int, 1>{}, s + 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // (the clamped weight DMA of the last stage still targets this workgroup's LDS)

    // ---- epilogue (lane = row, registers 4g..4g+3 = columns 8g + 4*half + {0..3})
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const long m = m0 + wm * 64 + i * 32 + l31;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * (32 * TN) + j * 32 + 8 * g + 4 * half;
                f32x4 v = {acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                if (d.bias) v = v + *reinterpret_cast<const f32x4*>(d.bias + n);
                if (d.res) v = v + *reinterpret_cast<const f32x4*>(d.res + m * d.ld_res + n);
                if (d.tr) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(d.tr + m * d.ld_tr + n);
                    const f32x4 ta = *reinterpret_cast<const f32x4*>(d.tr_a + n), tb = *reinterpret_cast<const f32x4*>(d.tr_b + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += dawn_silu(t4[e] * ta[e] + tb[e]);
                }
                *reinterpret_cast<f32x4*>(d.out + m * d.ld_out + n) = v;
            }
    }
#endif
}

template <int WN>
void launch_gemm1x1_bf16(const dawn_conv_desc& d, long M, hipStream_t s) {
    constexpr int BN = 64 * WN;
    const size_t lds = (size_t)2 * 2 * (6 * (256 * 16 + 128) + 64) + (size_t)2 * 2 * 6 * BN * 16;
    const int nwg = (int)(M / 256) * (d.N / BN);
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
    if (policy_of(d) & DAWN_POLICY_NINE_TERMS) {
        (void)hipFuncSetAttribute((const void*)gemm1x1_bf16_kernel<9, WN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((gemm1x1_bf16_kernel<9, WN>), dim3(nwg), dim3(256 * WN), lds, s, d, M);
    } else {
        (void)hipFuncSetAttribute((const void*)gemm1x1_bf16_kernel<6, WN>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((gemm1x1_bf16_kernel<6, WN>), dim3(nwg), dim3(256 * WN), lds, s, d, M);
    }
}

void launch_gemm1x1_bf16_small(const dawn_conv_desc& d, long M, hipStream_t s) {
    const size_t lds = (size_t)2 * 2 * (6 * (128 * 16 + 128) + 64) + (size_t)2 * 2 * 6 * 64 * 16;      // 77 KB: two per CU
    const int nwg = (int)(M / 128) * (d.N / 64);
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
    (void)hipFuncSetAttribute((const void*)gemm1x1_bf16_kernel<6, 1, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((gemm1x1_bf16_kernel<6, 1, 1>), dim3(nwg), dim3(256), lds, s, d, M);
}

}  // namespace

// the tiled split kernel (gemm1x1_bf16_kernel) for a descriptor split1x1_form() routed to it
void dawn_gemm1x1_tiled_launch(const dawn_conv_desc& d, long M, hipStream_t s) {
    const int plan = gemm1x1_split_plan(M, d.N, d.C0, d.C1);
    if (plan != 0 && ((policy_of(d) & DAWN_POLICY_TILE128_ALWAYS) || (plan == 3 && !(policy_of(d) & DAWN_POLICY_TILE128_NEVER)))) launch_gemm1x1_bf16_small(d, M, s);
    else if (plan == 3) {                            // TILE128_NEVER: the round-1 choice for these shapes
        if (d.N % 128 == 0 && (M / 256) * (d.N / 128) >= 128) launch_gemm1x1_bf16<2>(d, M, s);
        else launch_gemm1x1_bf16<1>(d, M, s);
    }
    else if (plan == 2) launch_gemm1x1_bf16<2>(d, M, s);
    else launch_gemm1x1_bf16<1>(d, M, s);
}
