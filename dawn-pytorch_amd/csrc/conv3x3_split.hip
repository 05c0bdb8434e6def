// The shipped direct 3x3 / stride 1 / pad 1 convolution: fp32 on the bf16 matrix pipe by exact operand splitting (dawn_split3_rne_quad, dawn_common.h),
// second generation of conv3x3_halo_bf16_kernel (conv_gemm.hip).  Reached from dawn_conv_gemm's router through dawn_conv3x3_v2_try;
// the s_memtime stamps (TSTAMP, ABL bit 3) and the other ABL instantiations exist only in -DDAWN_ABLATION builds (hipbuild.py ablation).
#include "conv_split.h"

namespace {

__device__ unsigned long long* g_dbg = nullptr;   // s_memtime stamps of the instrumented build (ABL bit 3)

// sums over lanes 0..31 and over lanes 32..63 of a wave, valid in lanes 16..31 / 48..63: the sum inside each row of 16
// (row16_sum), then row_bcast15 into rows 1 and 3 -- no LDS round trips
__device__ __forceinline__ float half_wave_sum_dpp(float v) {
    v = row16_sum(v);
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false));
    return v;
}

// Second-generation split-operand kernel for the large-M levels: BM = 256 output pixels x BN = 64*WN channels,
// 64*4*WN threads (every wave owns a 64 x 64 tile).  Differences from conv3x3_halo_bf16_kernel (conv_gemm.hip):
//  * the fp32 patch of the NEXT channel chunk is prefetched into registers during stages 0-1 of the current chunk,
//    split into its three bf16 pieces BETWEEN the MFMAs of stages 1-2 (VALU work hidden in the matrix pipe's
//    shadow) and only written to the LDS planes at the chunk boundary -- no raw LDS buffer, no split pass;
//  * the weights are staged one KERNEL ROW (3 taps) at a time, double-buffered: one barrier per 72 MFMAs per wave
//    instead of one per 24, and every load has a whole stage (>= 2300 MFMA cycles) to land;
//  * all loads are buffer instructions (SGPR descriptor + precomputed 32-bit lane offsets + scalar chunk offset):
//    padding and out-of-tile lanes are out-of-range offsets that return 0, so issuing a stage's loads is ~20
//    instructions with no branches and no 64-bit address arithmetic.
// (measured with the s_memtime build, tools/conv_phase_timing.py: per chunk the first version spent 3 x 1650 cycles
//  issuing loads and 2400 in the split pass next to 3 x 2300 cycles of MFMA.)
//
// K32 (round 3): the same kernel on v_mfma_f32_16x16x32_bf16.  The split kernels are POWER-limited (profiles/r3_mfma_power_ubench.txt),
// and the 16x16x32 shape spends ~11 % less energy per flop than 32x32x16 on the same operand data (half the accumulator traffic
// per flop).  Its K = 32 is filled from ONE 16-channel chunk by giving the two k-halves of an instruction two different cross
// terms: lanes 0..31 (k-groups 0, 1) and lanes 32..63 (k-groups 2, 3) read different split planes, so with
//   X1 = [x1 | x2], X2 = [x3 | x1] (pixels)   W1 = [w1 | w2], W2 = [w3 | w1] (weights)
// the three products X2.W1 = x3 w1 + x1 w2, X1.W2 = x1 w3 + x2 w1, X1.W1 = x1 w1 + x2 w2 are exactly the 6 cross terms: 3 half-size
// MFMAs per 16 x 16 block instead of 6 full-size ones per 32 x 32, 16 fragment reads per tap instead of 12, same LDS layout.
// PSEG (round 6) = 16-pixel segments of the halo patch the instantiation holds: 28 (P16 <= 448) everywhere but at 4 x 4-pixel frames
// (BASELINE configs[1]'s deepest level: 16 frames x 6 x 6 = 576 patch pixels per 256-pixel tile), which ran on the round-1 kernel with
// 128-row tiles -- 200 four-wave workgroups two per CU, i.e. 100 of 256 CUs busy, 58..123 TF/s (profiles/r6_config1_insitu_shapes.txt)
template <int WN, int NT, int ABL, bool K32 = false, int PSEG = 28>
__global__ __launch_bounds__(256 * WN, (K32 && PSEG == 28) ? 2 / WN : 1) void conv3x3_bf16_v2_kernel(const dawn_conv_desc d, const int xcd_remap,
                                                                    const int TR, const int nf, const int P16,
                                                                    const int WT, const int stagger) {
#if __HIP_DEVICE_COMPILE__   // (the host pass only needs the launch stub; buffer-resource builtins are device-only)
    // Two workgroups share a CU (LDS-limited).  Launched together they stay phase-locked for the whole grid -- both in their
    // prologue / epilogue (no MFMA) at the same time, then both in the main loop (sharing the matrix pipe).  Delaying the
    // second resident set (blocks 256..511 with one workgroup per CU and round) by about half a tile puts one workgroup's
    // prologue + epilogue under the other's main loop; later workgroups inherit the offset of the slot they replace.
    if (stagger > 0 && blockIdx.x >= 256 && blockIdx.x < 512)
        for (int i = 0; i < stagger; ++i) __builtin_amdgcn_s_sleep(127);
    constexpr int NTHR = 256 * WN, BM = 256, BN = 64 * WN;
    constexpr int TM = 2, TN = 2;
    constexpr int MAXQ = (PSEG * 16 * 4 + NTHR - 1) / NTHR;    // patch quads per thread (P16 <= 16 PSEG)
    constexpr int L0 = (MAXQ + 1) / 2;                         // quads loaded in stage 0 (the rest in stage 1)
    constexpr int SB = 18 * BN * 16;                           // bytes of one weight stage (3 taps x 3 planes x 2 halves)
    constexpr int NBI = SB / 1024;                             // DMA wave-instructions per stage
    constexpr int NW = 4 * WN;
    constexpr int NBJ = (NBI + NW - 1) / NW;
    constexpr unsigned OOB = 0x80000000u;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_b[];
    const int HPS = P16 * 16 + 128;
    const size_t DBG_OFF = (size_t)6 * HPS + 2 * SB;           // instrumented build only: 64 stamps
    unsigned char* planes = smem_b;                            // [3][2][HPS]
    unsigned char* Bs = smem_b + (size_t)6 * HPS;              // [2][3 taps][3 planes][2 halves][BN][16 B]

    int tix = 0;
    bool tstamp_on = true;                                     // (stamps of chunks >= 2 are skipped: 64 slots)
#define TSTAMP()                                                                                       \
    do {                                                                                               \
        if ((ABL & 8) && threadIdx.x == 0 && tix < 64 && tstamp_on)                                    \
            reinterpret_cast<unsigned long long*>(smem_b + DBG_OFF)[tix++] = __builtin_amdgcn_s_memtime(); \
    } while (0)
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, half = lane >> 5;
    // tile = TR rows x WT columns of one frame (WT == W: whole rows, possibly nf whole small frames; WT < W: the wide
    // images of the flow decoder are cut into column tiles so that the halo patch stays (TR+2) x (WT+2))
    const int H = d.Hi, W = d.Wi, PW = WT + 2, PP = (TR + 2) * PW;
    const int Cin = d.C0 + d.C1;
    const int nC = Cin / 16;
    const int nNt = d.N / BN;
    int bid = blockIdx.x;
    if (xcd_remap) {
        const int nwg = gridDim.x;
        const int xcd = bid & 7, idx = bid >> 3;
        const int q = nwg >> 3, r = nwg & 7;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int mt = bid / nNt, nt = bid - mt * nNt;
    const int n0 = nt * BN;
    const int ncx = W / WT;
    const int band = mt / ncx;
    const int x0 = (mt - band * ncx) * WT;
    const int grow0 = band * (BM / WT);                 // first image row of the tile, counted over all frames
    const int f0 = grow0 / H;
    const int y0 = grow0 - f0 * H;
    TSTAMP();   // 0: start

    // ---- buffer descriptors: the patch window of each source (first pixel = row y0-1 of frame f0), the weights
    const long pb = ((long)f0 * H + y0 - 1) * W;
    const int ext = nf * H * W + (nf > 1 ? 2 * W : (TR + 2) * W - H * W);    // pixels spanned by the window
    const __amdgpu_buffer_rsrc_t rs0 = DAWN_BUFFER(d.in0 + pb * d.ld0, ext * d.ld0 * 4);
    const __amdgpu_buffer_rsrc_t rs1 = DAWN_BUFFER((d.in1 ? d.in1 : d.in0) + pb * (d.in1 ? d.ld1 : d.ld0), ext * (d.in1 ? d.ld1 : d.ld0) * 4);
    const __amdgpu_buffer_rsrc_t rsw = DAWN_BUFFER(d.w_bf3, 9 * nC * 6 * d.N * 16);

    // ---- this thread's patch quads: q = tid + NTHR*i -> (pos = q>>2, 4-channel slot = q&3); rel = window pixel
    const int nq = P16 * 4;
    const float rPP = 1.0f / (float)PP, rPW = 1.0f / (float)PW, rTW = 1.0f / (float)(TR * WT), rW = 1.0f / (float)WT;
    int rel[MAXQ];
#pragma unroll
    for (int i = 0; i < MAXQ; ++i) {
        const int q = tid + NTHR * i;
        const int pos = q >> 2;
        int r = -1;
        if (q < nq && pos < nf * PP) {
            const int fi = (int)(((float)pos + 0.5f) * rPP);
            const int rem = pos - fi * PP;
            const int pyy = (int)(((float)rem + 0.5f) * rPW), pxx = rem - pyy * PW;
            const int y = y0 + pyy - 1, x = x0 + pxx - 1;
            if (y >= 0 && y < H && x >= 0 && x < W) r = fi * H * W + pyy * W + x;
        }
        rel[i] = r;
    }
    int pc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = wm * 64 + i * 32 + l31;
        const int fi = (int)(((float)r + 0.5f) * rTW);
        const int rem = r - fi * TR * WT;
        const int ty = (int)(((float)rem + 0.5f) * rW), x = rem - ty * WT;
        pc[i] = fi * PP + (ty + 1) * PW + (x + 1);
    }
    // K32: lane = (pixel | channel l15 of a 16-block, k-group kg); k-groups 0,1 = the two k-halves of the FIRST term of an MFMA,
    // 2,3 = of the second.  Byte offsets of this lane's fragments: pixels X1 = [x1|x2], X2 = [x3|x1]; weights W1 = [w1|w2], W2 = [w3|w1]
    const int l15 = lane & 15, kg = lane >> 4, kh = kg & 1, ks = kg >> 1;
    int px1[4], dpx = 0, wo1 = 0, wo2 = 0;                // X2 fragment = X1 fragment + dpx bytes (another plane)
    if constexpr (K32) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int r = wm * 64 + b * 16 + l15;
            const int fi = (int)(((float)r + 0.5f) * rTW);
            const int rem = r - fi * TR * WT;
            const int ty = (int)(((float)rem + 0.5f) * rW), x = rem - ty * WT;
            const int pcb = (fi * PP + (ty + 1) * PW + (x + 1)) * 16;
            px1[b] = ((ks ? 1 : 0) * 2 + kh) * HPS + pcb;
        }
        dpx = (ks ? -2 : 4) * HPS;
        wo1 = (((ks ? 1 : 0) * 2 + kh) * BN + wn * 64 + l15) * 16;
        wo2 = (((ks ? 0 : 2) * 2 + kh) * BN + wn * 64 + l15) * 16;
    }
    // weight DMA lane offsets (bytes) within a (chunk cc, kernel row ky) stage
    unsigned voffB[NBJ];
#pragma unroll
    for (int j = 0; j < NBJ; ++j) {
        const int q = j * NW + wave;
        const int idx = q * 64 + lane;
        const int tp = idx / (6 * BN);
        const int rem = idx - tp * (6 * BN);
        const int ph = rem / BN, n = rem - ph * BN;
        voffB[j] = q < NBI ? (unsigned)(((tp * nC * 6 + ph) * d.N + n0 + n) * 16) : OOB;
    }

    f32x4 araw[MAXQ];
    uint2 ap[MAXQ][3];
    auto loadA = [&](int cc, int i) {
        const int cbase = cc * 16;
        const bool src1 = cbase >= d.C0;
        const int ldb = (src1 ? d.ld1 : d.ld0) * 4;
        const int soff = (src1 ? cbase - d.C0 : cbase) * 4;
        const unsigned voff = rel[i] < 0 ? OOB : (unsigned)(rel[i] * ldb + (tid & 3) * 16);
        const i32x4 v = src1 ? __builtin_amdgcn_raw_buffer_load_b128(rs1, voff, soff, 0)
                             : __builtin_amdgcn_raw_buffer_load_b128(rs0, voff, soff, 0);
        araw[i] = __builtin_bit_cast(f32x4, v);
    };
    auto convA = [&](int i) { dawn_split3_rne_quad(araw[i], ap[i][0], ap[i][1], ap[i][2]); };
    auto writeA = [&]() {
#pragma unroll
        for (int i = 0; i < MAXQ; ++i) {
            const int q = tid + NTHR * i;
            if (q < nq) {
                const int pos = q >> 2, slot = q & 3;
                unsigned char* dst = planes + (size_t)(slot >> 1) * HPS + pos * 16 + (slot & 1) * 8;
                *reinterpret_cast<uint2*>(dst) = ap[i][0];
                *reinterpret_cast<uint2*>(dst + 2 * HPS) = ap[i][1];
                *reinterpret_cast<uint2*>(dst + 4 * HPS) = ap[i][2];
            }
        }
    };
    auto issueB = [&](int cc, int ky, int buf) {
        const int soff = (ky * 3 * nC + cc) * 6 * d.N * 16;
#pragma unroll
        for (int j = 0; j < NBJ; ++j) {
            const int q = j * NW + wave;
            if (q < NBI)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsw, (__attribute__((address_space(3))) void*)(Bs + (size_t)buf * SB + q * 1024), 16, voffB[j], soff, 0, 0);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    f32x4 acq[4][4];                                    // K32: [pixel block][channel block], lane = pixel l15, channels 4 kg + 0..3
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acq[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    TSTAMP();   // 1: index math done
    issueB(0, 0, 0);
#pragma unroll
    for (int i = 0; i < MAXQ; ++i) loadA(0, i);
#pragma unroll
    for (int i = 0; i < MAXQ; ++i) convA(i);
    writeA();
    TSTAMP();   // 2: first patch landed + split
    int bufB = 0;
    for (int cc = 0; cc < nC; ++cc) {
        tstamp_on = cc < 2;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                   // planes(cc) written, weight stage (cc, 0) landed
        TSTAMP();   // chunk top
        const bool more = cc + 1 < nC;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            // prefetch: the next weight stage, then (stages 0, 1) the next chunk's patch quads
            {
                int nky = ky + 1, ncc = cc;
                if (nky == 3) { nky = 0; ncc = cc + 1; }
                if (ncc < nC) issueB(ncc, nky, bufB ^ 1);
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < MAXQ; ++i)
                    if ((ky == 0 && i < L0) || (ky == 1 && i >= L0)) loadA(cc + 1, i);
            }
            TSTAMP();   // stage: loads issued
            const unsigned char* Bb = Bs + (size_t)bufB * SB;
            if constexpr (K32) {
                const int yoff = (ky - 1) * PW * 16 - 16;           // taps kx = 0..2 are +0 / +16 / +32 bytes from here
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    // pixel fragments of the 4 pixel blocks for the whole tap (32 VGPRs), weight fragments one 16-channel block ahead
                    // (16 VGPRs); per channel block the three products in the order smallest first, each weight fragment held as the A
                    // operand of four consecutive MFMAs
                    bf16x8 fx1[4], fx2[4], fw1[2], fw2[2];
#pragma unroll
                    for (int b = 0; b < 4; ++b) fx2[b] = *reinterpret_cast<const bf16x8*>(planes + px1[b] + (dpx + yoff) + kx * 16);
                    fw1[0] = *reinterpret_cast<const bf16x8*>(Bb + wo1 + (kx * 6 * BN) * 16);
#pragma unroll
                    for (int b = 0; b < 4; ++b) fx1[b] = *reinterpret_cast<const bf16x8*>(planes + px1[b] + yoff + kx * 16);
                    fw2[0] = *reinterpret_cast<const bf16x8*>(Bb + wo2 + (kx * 6 * BN) * 16);
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        const int c = cb & 1, n = c ^ 1;
                        if (cb < 3) {
                            fw1[n] = *reinterpret_cast<const bf16x8*>(Bb + wo1 + (kx * 6 * BN + (cb + 1) * 16) * 16);
                            fw2[n] = *reinterpret_cast<const bf16x8*>(Bb + wo2 + (kx * 6 * BN + (cb + 1) * 16) * 16);
                        }
#pragma unroll
                        for (int b = 0; b < 4; ++b) acq[b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw1[c], fx2[b], acq[b][cb], 0, 0, 0);
#pragma unroll
                        for (int b = 0; b < 4; ++b) acq[b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw2[c], fx1[b], acq[b][cb], 0, 0, 0);
#pragma unroll
                        for (int b = 0; b < 4; ++b) acq[b][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw1[c], fx1[b], acq[b][cb], 0, 0, 0);
                    }
                    if (more && ky > 0) {
#pragma unroll
                        for (int i = 0; i < MAXQ; ++i) {
                            const bool mine = ky == 1 ? i < L0 : i >= L0;
                            const int ord = ky == 1 ? i : i - L0;
                            if (mine && ord % 3 == kx) convA(i);
                        }
                    }
                    __builtin_amdgcn_sched_group_barrier(0x100, 10, 0);           // X2, W1[0], X1, W2[0] first
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) {
                        if (cb < 3) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);    // the next channel block's weight fragments
                            __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
                        }
#pragma unroll
                        for (int t = cb < 3 ? 1 : 0; t < 12; ++t) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // MFMA, 1 VALU (split), MFMA, ...
                            __builtin_amdgcn_sched_group_barrier(0x002, 1, 0);
                        }
                    }
                }
            } else {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int toff = (ky - 1) * PW + (kx - 1);
                bf16x8 fa[TM][3], fb[TN][3];
                // fragment reads in the order the terms consume them (a3,b1 | a1,b3 | a2,b2): the LDS returns in
                // order, so the first MFMAs start after 4 of the 12 reads (counted lgkmcnt) while the rest stream in
                constexpr int RA[3] = {2, 0, 1}, RB[3] = {0, 2, 1};
#pragma unroll
                for (int g = 0; g < 3; ++g) {
#pragma unroll
                    for (int i = 0; i < TM; ++i)
                        fa[i][RA[g]] = *reinterpret_cast<const bf16x8*>(planes + (size_t)(RA[g] * 2 + half) * HPS + (pc[i] + toff) * 16);
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        fb[j][RB[g]] = *reinterpret_cast<const bf16x8*>(
                            Bb + ((size_t)((kx * 6 + RB[g] * 2 + half) * BN + wn * 64 + j * 32 + l31)) * 16);
                }
#pragma unroll
                for (int t = 9 - NT; t < 9; ++t)
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[j][DAWN_SPLIT9_B[t]], fa[i][DAWN_SPLIT9_A[t]], acc[i][j], 0, 0, 0);
                // split the quads that landed during the previous stage, in the shadow of the MFMAs above
                if (more && ky > 0) {
#pragma unroll
                    for (int i = 0; i < MAXQ; ++i) {
                        const bool mine = ky == 1 ? i < L0 : i >= L0;
                        const int ord = ky == 1 ? i : i - L0;
                        if (mine && ord % 3 == kx) convA(i);
                    }
                }
                if (NT == 6) {
                    __builtin_amdgcn_sched_group_barrier(0x100, 12, 0);       // the 12 fragment reads first
#pragma unroll
                    for (int t = 0; t < 24; ++t) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);    // then MFMA, 2 VALU (split), MFMA, ...
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    }
                }
            }
            }
            TSTAMP();   // stage: MFMAs issued
            if (ky < 2) {
                // (the register operands pin the split of these quads behind the wait)
                if (MAXQ == 9)
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
                                 : "+v"(araw[0]), "+v"(araw[1]), "+v"(araw[2]), "+v"(araw[3]), "+v"(araw[4]), "+v"(araw[5]),
                                   "+v"(araw[6]), "+v"(araw[MAXQ > 7 ? 7 : 0]), "+v"(araw[MAXQ > 8 ? 8 : 0])
                                 :: "memory");
                else if (MAXQ == 7)
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
                                 : "+v"(araw[0]), "+v"(araw[1]), "+v"(araw[2]), "+v"(araw[3]), "+v"(araw[4]), "+v"(araw[5]),
                                   "+v"(araw[6])
                                 :: "memory");
                else if (MAXQ == 5)
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
                                 : "+v"(araw[0]), "+v"(araw[1]), "+v"(araw[2]), "+v"(araw[3]), "+v"(araw[MAXQ - 1])
                                 :: "memory");
                else
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)"
                                 : "+v"(araw[0]), "+v"(araw[1]), "+v"(araw[2]), "+v"(araw[MAXQ - 1])
                                 :: "memory");
                __builtin_amdgcn_s_barrier();           // next weight stage landed; this one may be overwritten
            }
            TSTAMP();   // stage: barrier passed
            bufB ^= 1;
        }
        if (more) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();               // every wave is done reading planes(cc)
            TSTAMP();   // planes-free barrier passed
            writeA();
            TSTAMP();   // planes written
        }
    }
    tstamp_on = true;
    TSTAMP();   // main loop done

    // ---- epilogue.  The products are accumulated TRANSPOSED (A = weights, B = pixels): lane = output pixel, registers
    // 4g..4g+3 = channels 8g + 4*half + {0..3} of the 32-channel tile, so every store is a 16-byte row segment
    // (16 dwordx4 stores per wave instead of 64 scalar ones) and the GroupNorm partial sums are in-register per
    // 8-channel group until one cross-lane reduction at the end.
    float gs[TN][4], gss[TN][4];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) { gs[j][g] = 0.f; gss[j][g] = 0.f; }
    if constexpr (K32) {
        // lane = output pixel l15 of a 16-pixel block, registers = channels 16 cb + 4 kg + {0..3}: 16-byte row segments, 4 lanes
        // cover the 64 contiguous bytes of a pixel's 16-channel block.  The lane's GroupNorm partials belong to the 8-channel
        // subgroup 2 cb + (kg >> 1) of the wave's 64 channels; the other subgroup of the pair gets a zero from this lane
        // (columns of the block reduction below: j = cb >> 1, g = 2 (cb & 1) + {0, 1}).
        long mrq[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int r = wm * 64 + b * 16 + l15;
            const int fi = (int)(((float)r + 0.5f) * rTW);
            const int rem = r - fi * TR * WT;
            const int ty = (int)(((float)rem + 0.5f) * rW), x = rem - ty * WT;
            mrq[b] = ((long)(f0 + fi) * H + y0 + ty) * W + x0 + x;
        }
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
            const int n = n0 + wn * 64 + cb * 16 + 4 * kg;
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (d.bias) bv = *reinterpret_cast<const f32x4*>(d.bias + n);
            float sv = 0.f, sq = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long m = mrq[b];
                f32x4 v = acq[b][cb] + bv;
                if (d.res) v = v + *reinterpret_cast<const f32x4*>(d.res + m * d.ld_res + n);
                if (d.tr) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(d.tr + m * d.ld_tr + n);
                    const f32x4 ta = *reinterpret_cast<const f32x4*>(d.tr_a + n), tb = *reinterpret_cast<const f32x4*>(d.tr_b + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += dawn_silu(t4[e] * ta[e] + tb[e]);
                }
                *reinterpret_cast<f32x4*>(d.out + m * d.ld_out + n) = v;
                sv += (v.x + v.y) + (v.z + v.w);
                sq += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            }
            gs[cb >> 1][2 * (cb & 1)] = sv;             // (K32: slot [cb] = this lane's 4 channels of channel block cb; reduced below)
            gss[cb >> 1][2 * (cb & 1)] = sq;
        }
        if (d.gn_part) {
            // lanes 0..31 (k-groups 0, 1) own the lower 8 channels of every 16-channel block, lanes 32..63 the upper 8: two DPP
            // half-wave sums per block, one 128-byte exchange, one barrier; fp64 from the per-wave sums on
            float* wsum = reinterpret_cast<float*>(smem_b + DBG_OFF);          // [waves][8 subgroups][sum, sumsq]
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const float s1 = half_wave_sum_dpp(gs[cb >> 1][2 * (cb & 1)]), s2 = half_wave_sum_dpp(gss[cb >> 1][2 * (cb & 1)]);
                if (l31 == 31) {
                    wsum[wave * 16 + (2 * cb + half) * 2] = s1;
                    wsum[wave * 16 + (2 * cb + half) * 2 + 1] = s2;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            if (tid < 16) {
                const int which = tid & 1;
                const int cpg = d.N >> 3;
                const int lo = (tid >> 1) * cpg - n0, hi = lo + cpg;           // this group's channel range relative to the tile
                // (branch-free: NW x 8 unconditional LDS reads issued back to back and a select each -- as `if (in range) a += ...` the
                //  compiler emitted one exec-masked block with its own LDS wait per term, a chain of up to 64 dependent round trips
                //  at the very end of the workgroup)
                double a = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w)
#pragma unroll
                    for (int jg = 0; jg < 8; ++jg) {
                        const int c = (w % WN) * 64 + 8 * jg;
                        const unsigned keep = (c >= lo && c < hi) ? 0xffffffffu : 0u;       // (a bit mask, not a select: the load cannot sink under it)
                        a += (double)__uint_as_float(__float_as_uint(wsum[w * 16 + jg * 2 + which]) & keep);
                    }
                d.gn_part[(long)blockIdx.x * 16 + tid] = a;
            }
        }
    } else {
    long mrow[TM];                                      // output pixel (row of the (M, N) result) of this lane
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int r = wm * 64 + i * 32 + l31;
        const int fi = (int)(((float)r + 0.5f) * rTW);
        const int rem = r - fi * TR * WT;
        const int ty = (int)(((float)rem + 0.5f) * rW), x = rem - ty * WT;
        mrow[i] = ((long)(f0 + fi) * H + y0 + ty) * W + x0 + x;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = n0 + wn * 64 + j * 32 + 8 * g + 4 * half;
            f32x4 bv = {0.f, 0.f, 0.f, 0.f};
            if (d.bias) bv = *reinterpret_cast<const f32x4*>(d.bias + n);
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const long m = mrow[i];
                f32x4 v = f32x4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]} + bv;
                if (d.res) v = v + *reinterpret_cast<const f32x4*>(d.res + m * d.ld_res + n);
                if (d.tr) {
                    const f32x4 t4 = *reinterpret_cast<const f32x4*>(d.tr + m * d.ld_tr + n);
                    const f32x4 ta = *reinterpret_cast<const f32x4*>(d.tr_a + n), tb = *reinterpret_cast<const f32x4*>(d.tr_b + n);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] += dawn_silu(t4[e] * ta[e] + tb[e]);
                }
                *reinterpret_cast<f32x4*>(d.out + m * d.ld_out + n) = v;
                gs[j][g] += (v.x + v.y) + (v.z + v.w);
                gss[j][g] += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            }
        }
    }
    }
    TSTAMP();   // stores issued
    if (!K32 && d.gn_part) {
        // block reduction through LDS: fp32 per-lane partials (8 values each) -> fp64 from there on
        __syncthreads();
        float* pf = reinterpret_cast<float*>(smem_b);                        // [16 columns][NTHR]
        double* pd = reinterpret_cast<double*>(smem_b + 16 * NTHR * 4);       // [16 columns][NTHR / 32]
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                pf[((j * 4 + g) * 2) * NTHR + tid] = gs[j][g];
                pf[((j * 4 + g) * 2 + 1) * NTHR + tid] = gss[j][g];
            }
        __syncthreads();
        constexpr int NP = NTHR / 32;
        if (tid < 16 * NP) {
            const int c = tid / NP, p = tid - c * NP;
            // (start offset rotated per thread: consecutive threads read rows 128 B apart -- unrotated, all 64 lanes of a wave
            //  hit one LDS bank in every one of the 32 steps)
            double a = 0.0;
#pragma unroll 8
            for (int e = 0; e < 32; ++e) a += (double)pf[c * NTHR + p * 32 + ((e + tid) & 31)];
            pd[c * NP + p] = a;
        }
        __syncthreads();
        if (tid < 16) {
            const int grp = tid >> 1, which = tid & 1;
            const int cpg = d.N >> 3;
            double a = 0.0;
            for (int w = 0; w < NW; ++w)
#pragma unroll
                for (int jg = 0; jg < 8; ++jg)
                    if ((n0 + (w % WN) * 64 + (jg >> 2) * 32 + 8 * (jg & 3)) / cpg == grp)
                        a += pd[(jg * 2 + which) * NP + w * 2] + pd[(jg * 2 + which) * NP + w * 2 + 1];
            d.gn_part[(long)blockIdx.x * 16 + tid] = a;
        }
    }
    TSTAMP();   // end
#undef TSTAMP
    if ((ABL & 8) && threadIdx.x == 0 && blockIdx.x < 4096)
        for (int i = 0; i < 64; ++i)
            g_dbg[(size_t)blockIdx.x * 64 + i] = i < tix ? reinterpret_cast<unsigned long long*>(smem_b + DBG_OFF)[i] : 0ull;
#endif
}

template <int WN>
bool try_launch_bf16_v2(const dawn_conv_desc& d, long M, hipStream_t s, bool nine, bool dry /* decide only, launch nothing */) {
    constexpr int BM = 256, BN = 64 * WN;
    const int H = d.Hi, W = d.Wi;
    // tile width: whole image rows up to W = 64 (every level of the denoiser); wider images (the flow decoder's
    // 128 / 256-pixel levels) are cut into 32-column tiles of 8 rows -> a 10 x 34 halo patch (1.33x the tile)
    const int WT = W > 64 ? 32 : W;
    if (M % BM != 0 || W % WT != 0 || BM % WT != 0 || d.C0 % 16 != 0 || d.C1 % 16 != 0 || d.N % BN != 0) return false;
    if ((d.ld0 & 3) || (d.in1 && (d.ld1 & 3)) || (d.ld_out & 3) || (d.res && (d.ld_res & 3)) || (d.tr && (d.ld_tr & 3)) ||
        (long)9 * (d.C0 + d.C1) * d.N * 6 >= (1L << 31) || (long)d.F * H >= (1L << 31))
        return false;
    int TR = BM / WT, nf = 1;
    if (TR <= H) { if (H % TR != 0) return false; }
    else { if (WT != W || TR % H != 0) return false; nf = TR / H; TR = H; if (d.F % nf != 0) return false; }
    const int P = nf * (TR + 2) * (WT + 2);
    const int P16 = (P + 15) / 16 * 16;
    const bool timing = policy_variant(d) == 8;
    const bool k32 = !nine && (policy_of(d) & DAWN_POLICY_MFMA_K32);
    // (the 36-segment instantiation exists for the shipped form only: 16 x 16 x 32, six cross terms)
    const bool big_patch = P16 > 448;
    if (P16 > 576 || (big_patch && !k32)) return false;
    const size_t lds = (size_t)6 * (P16 * 16 + 128) + (size_t)2 * 18 * BN * 16 + (timing || k32 ? 512 : 0);   // (+ the GroupNorm exchange)
    if (lds > 160 * 1024) return false;
    if (dry) return true;
    const int nwg = (int)(M / BM) * (d.N / BN);
    const int remap = ((policy_of(d) & DAWN_POLICY_XCD_ORDER) && nwg >= 64 && H * W >= 1024) ? 1 : 0;
    // start delay of the second resident workgroup set in units of ~8k cycles (DAWN_POLICY_STAGGER; default 0 = none): in
    // isolation it takes 8..11 % off the 64-input-channel launches (354 -> 316..328 us, profiles/r2_conv_stagger.txt) and nothing
    // off deeper K; inside an evaluation, next to the side stream's kernels, it changes nothing (385.4 vs 384.5 us): off
    const int stagger = nwg >= 1024 ? policy_stagger(policy_of(d)) : 0;
#define LAUNCH_V2K(NTV, ABLV, K32V)                                                                                   \
    do {                                                                                                              \
        (void)hipFuncSetAttribute((const void*)conv3x3_bf16_v2_kernel<WN, NTV, ABLV, K32V>,                           \
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                              \
        hipLaunchKernelGGL((conv3x3_bf16_v2_kernel<WN, NTV, ABLV, K32V>), dim3(nwg), dim3(256 * WN), lds, s, d, remap, TR, nf, \
                           P16, WT, stagger);                                                                         \
    } while (0)
#define LAUNCH_V2(NTV, ABLV) LAUNCH_V2K(NTV, ABLV, false)
    if (d.gn_rows) *d.gn_rows = nwg;   // rows of gn_part this launch writes
    if (nine) LAUNCH_V2(9, 0);
    // 16x16x32 form: less energy per flop, more instructions -- inside an evaluation -2.4..-5.6 % per launch wherever the grid keeps
    // the chip busy (power-limited), +4..6 % on the four under-filled launches of the deepest level (100 workgroups;
    // profiles/r3_k32_shapes.txt).  Chosen by the policy alone, never by the grid size: a frame computes the same bits whatever
    // the batch it is launched in
    else if (big_patch) {
        (void)hipFuncSetAttribute((const void*)conv3x3_bf16_v2_kernel<WN, 6, 0, true, 36>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL((conv3x3_bf16_v2_kernel<WN, 6, 0, true, 36>), dim3(nwg), dim3(256 * WN), lds, s, d, remap, TR, nf, P16, WT, stagger);
    }
    else if (policy_of(d) & DAWN_POLICY_MFMA_K32) LAUNCH_V2K(6, 0, true);
#ifdef DAWN_ABLATION
    else if (timing) LAUNCH_V2(6, 8);
    else if (policy_variant(d) == 1) LAUNCH_V2(6, 1);
    else if (policy_variant(d) == 2) LAUNCH_V2(6, 2);
    else if (policy_variant(d) == 4) LAUNCH_V2(6, 4);
    else if (policy_variant(d) == 7) LAUNCH_V2(6, 7);
#endif
    else LAUNCH_V2(6, 0);
#undef LAUNCH_V2
#undef LAUNCH_V2K
    return true;
}

}  // namespace

bool dawn_conv3x3_v2_try(const dawn_conv_desc& d, long M, hipStream_t s, bool nine, bool narrow, bool dry) {
    return narrow ? try_launch_bf16_v2<1>(d, M, s, nine, dry) : try_launch_bf16_v2<2>(d, M, s, nine, dry);
}

#ifdef DAWN_ABLATION
extern "C" int dawn_conv_set_debug(void* p) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), &p, sizeof(p));
}
#endif
