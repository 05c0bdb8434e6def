// HuBERT audio features (unified_video_generator.py:433-501 `_get_hubert_from_16k_speech` ->
// transformers.HubertModel, hubert-large-ls960-ft: `feat_extract_norm = "layer"`, `do_stable_layer_norm = True`) and the
// 25 fps linear interpolation that follows it (UVG:229-247, scipy.interpolate.interp1d).
//
// The encoder's GEMM-shaped work -- conv layers 1..6 of the waveform feature extractor, the grouped positional conv,
// every Linear -- goes through dawn_conv_gemm (fp32 MFMA implicit GEMM on (time, channel) channels-last rows).  This
// file holds what is left: the Cin = 1 first conv, LayerNorm (+ exact GELU) over channels, the elementwise GELU / add
// passes, the 16-head x 64 self-attention over <= ~1000 frames per chunk, and the fp64 interpolation.
#include "dawn_common.h"
#include "../../include/dawn_hip.h"

namespace {

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }

// ---- utterance normalisation of Wav2Vec2FeatureExtractor (do_normalize): (x - mean) / sqrt(var + 1e-7), numpy float32
// statistics (np.mean / np.var of a float32 array use pairwise float32 sums; fp64 partial sums here, rounded once --
// within 1 ulp of numpy's value, the test tolerance covers it)
__global__ __launch_bounds__(1024) void wave_stats_kernel(const float* __restrict__ x, long n, double* __restrict__ out2) {
    __shared__ double sh[2][16];
    double s = 0.0, ss = 0.0;
    for (long i = threadIdx.x; i < n; i += 1024) { const double v = x[i]; s += v; ss += v * v; }
    s = wave_sum_d(s); ss = wave_sum_d(ss);
    if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = s; sh[1][threadIdx.x >> 6] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < 16; ++i) { a += sh[0][i]; b += sh[1][i]; }
        const double mean = a / (double)n;
        out2[0] = mean;
        out2[1] = b / (double)n - mean * mean;
    }
}
__global__ __launch_bounds__(256) void wave_normalize_kernel(const float* __restrict__ x, long n, const double* __restrict__ st,
                                                             float* __restrict__ out) {
    const float mean = (float)st[0];
    const float inv = 1.0f / sqrtf((float)st[1] + 1e-7f);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (x[i] - mean) * inv;
}

// ---- feature_extractor.conv_layers[0]: Conv1d(1, C, k, stride) on the waveform -> (T0, C) channels-last (+ bias)
// w (C, k) row-major (the Conv1d weight with its singleton input-channel dimension dropped)
__global__ __launch_bounds__(256) void conv0_kernel(const float* __restrict__ x, long n, const float* __restrict__ w,
                                                    const float* __restrict__ bias, int C, int k, int stride, long T0,
                                                    float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int cq = C / 4;
    if (idx >= T0 * cq) return;
    const long t = idx / cq;
    const int c = (int)(idx - t * cq) * 4;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (bias) acc = *reinterpret_cast<const f32x4*>(bias + c);
    const float* xp = x + t * stride;
    for (int j = 0; j < k; ++j) {
        const float xv = xp[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = fmaf(w[(c + e) * k + j], xv, acc[e]);
    }
    *reinterpret_cast<f32x4*>(out + t * C + c) = acc;
}

// ---- LayerNorm over the C channels of every row, affine, optional exact GELU: one wave per row (C <= 4096, C % 4 == 0)
__global__ __launch_bounds__(256) void ln_affine_act_kernel(const float* __restrict__ x, long rows, int C, const float* __restrict__ g,
                                                            const float* __restrict__ b, float eps, int act, float* __restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + row * C;
    float s = 0.f;
    for (int c = lane * 4; c < C; c += 256) { const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c); s += (v.x + v.y) + (v.z + v.w); }
    s = wave_sum(s);
    const float mu = s / (float)C;
    float ss = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c) - mu;
        ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
    ss = wave_sum(ss);
    const float rs = 1.0f / sqrtf(ss / (float)C + eps);
    for (int c = lane * 4; c < C; c += 256) {
        f32x4 v = (*reinterpret_cast<const f32x4*>(xr + c) - mu) * rs;
        v = v * *reinterpret_cast<const f32x4*>(g + c) + *reinterpret_cast<const f32x4*>(b + c);
        if (act == 2) { v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w); }
        *reinterpret_cast<f32x4*>(out + row * C + c) = v;
    }
}

// out = (a ? a : 0) + act(b): act 0 none, 2 exact GELU (FFN activation; `hidden + gelu(pos_conv)`), n % 4 == 0
__global__ __launch_bounds__(256) void add_act_kernel(const float* __restrict__ a, const float* __restrict__ b, int act, long n4,
                                                      float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        f32x4 v = reinterpret_cast<const f32x4*>(b)[i];
        if (act == 2) { v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w); }
        if (a) v = v + reinterpret_cast<const f32x4*>(a)[i];
        reinterpret_cast<f32x4*>(out)[i] = v;
    }
}

// ---- self-attention, heads of 64 features, full softmax over the T frames of a chunk (HubertAttention, no mask):
// qkv (T, 3*E) = [q | k | v] rows (q unscaled: * 64^-1/2 here), out (T, E), E = heads * 64.
// One wave per (head, 32-query tile); K / V tiles of 32 frames staged in LDS; S^T = K . Q^T so that a lane owns one query
// column (softmax in registers + one xor-32 exchange), O^T += V^T . P^T with P fed from the S^T accumulators (the scheme of
// temporal_attn.hip), fp32 MFMA throughout.
__global__ __launch_bounds__(64) void attn64_kernel(const float* __restrict__ qkv, int T, int heads, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float Ks[32 * 68];
    __shared__ __attribute__((aligned(16))) float Vs[32 * 64];
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int h = blockIdx.y, q0 = blockIdx.x * 32;
    const int E = heads * 64, ld = 3 * E;
    const int iq = min(q0 + l31, T - 1);
    // Q^T fragments: B operand of S^T = K . Q^T: lane (query l31, k-half) holds q[d = 2m + half] for MFMA m
    float qf[32];
    {
        const float* qr = qkv + (long)iq * ld + h * 64;
#pragma unroll
        for (int m = 0; m < 32; ++m) qf[m] = qr[2 * m + half] * 0.125f;
    }
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float mrun = -3.0e38f, lrun = 0.f;
    const int nkt = (T + 31) / 32;
    for (int kt = 0; kt < nkt; ++kt) {
        __syncthreads();
        // stage K / V rows kt*32 .. +31 (zero rows past T): 32 rows x 64 floats each = 512 float4 per matrix / 64 lanes
        for (int i = lane; i < 512; i += 64) {
            const int r = i >> 4, c4 = (i & 15) * 4;
            const int j = kt * 32 + r;
            f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
            if (j < T) {
                kv = *reinterpret_cast<const f32x4*>(qkv + (long)j * ld + E + h * 64 + c4);
                vv = *reinterpret_cast<const f32x4*>(qkv + (long)j * ld + 2 * E + h * 64 + c4);
            }
            *reinterpret_cast<f32x4*>(Ks + r * 68 + c4) = kv;
            *reinterpret_cast<f32x4*>(Vs + r * 64 + c4) = vv;
        }
        __syncthreads();
        // S^T (32 keys x 32 queries): A = K rows (lane = key l31, k = d), B = Q^T
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int m = 0; m < 32; ++m) st = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[l31 * 68 + 2 * m + half], qf[m], st, 0, 0, 0);
        // online softmax over keys: registers = keys (r&3) + 8 (r>>2) + 4 half of this tile, lane = query
        float mt = -3.0e38f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            st[r] = j < T ? st[r] : -3.0e38f;
            mt = fmaxf(mt, st[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mnew = fmaxf(mrun, mt);
        const float alpha = __expf(mrun - mnew);
        float lt = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = __expf(st[r] - mnew); lt += st[r]; }
        lt += __shfl_xor(lt, 32, 64);
        lrun = lrun * alpha + lt;
        mrun = mnew;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
        // O^T (64 d x 32 queries) += V^T . P^T: MFMA r consumes keys k0(r) (lanes 0-31) and k0(r) + 4 (lanes 32-63)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = (r & 3) + 8 * (r >> 2) + 4 * half;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * 64 + l31], st[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * 64 + 32 + l31], st[r], o1, 0, 0, 0);
        }
    }
    // O^T accumulators: lane = query l31, registers = d (r&3) + 8 (r>>2) + 4 half (+ 32 for o1)
    if (q0 + l31 < T) {
        const float inv = 1.0f / lrun;
        float* orow = out + (long)(q0 + l31) * E + h * 64;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d = 8 * g + 4 * half;
            *reinterpret_cast<f32x4*>(orow + d) = f32x4{o0[4 * g], o0[4 * g + 1], o0[4 * g + 2], o0[4 * g + 3]} * inv;
            *reinterpret_cast<f32x4*>(orow + 32 + d) = f32x4{o1[4 * g], o1[4 * g + 1], o1[4 * g + 2], o1[4 * g + 3]} * inv;
        }
    }
}

// ---- scipy.interpolate.interp1d(kind="linear", axis=0) on x = arange(n) at the positions xi (fp64, from np.linspace):
// slope = (y_hi - y_lo) / (x_hi - x_lo); out = float32(slope * (xi - x_lo) + y_lo) with scipy's mixed precision (bit-exact
// against scipy 1.15: the float32 difference, then float64) (UVG:236-243)
__global__ __launch_bounds__(256) void interp_linear_kernel(const float* __restrict__ y, long n, int C, const double* __restrict__ xi,
                                                            long m, float* __restrict__ out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * C) return;
    const long i = idx / C;
    const int c = (int)(idx - i * C);
    const double x = xi[i];
    // interp1d: x_new_indices = searchsorted(x, x_new), clipped to [1, n-1]; lo = idx - 1, hi = idx
    long hi = (long)ceil(x);
    if ((double)hi < x) ++hi;
    if (hi < 1) hi = 1;
    if (hi > n - 1) hi = n - 1;
    const long lo = hi - 1;
    const float ylo = y[lo * C + c], yhi = y[hi * C + c];
    const float df = __fsub_rn(yhi, ylo);                 // the float32 feature array is differenced in float32 by numpy ...
    const double slope = (double)df / ((double)hi - (double)lo);   // ... and promoted to float64 by the division with x_hi - x_lo
    out[idx] = (float)(slope * (x - (double)lo) + (double)ylo);
}


// ---- HubertPositionalConvEmbedding + the residual that follows it, one launch (hubert.py encode; transformers: Conv1d(E, E, k,
// padding = k / 2, groups) -> SamePad drop for even k -> GELU; hidden + that):
//   out[t][g gw + n] = hid[t][g gw + n] + gelu(bias[g gw + n] + sum_{j < k} sum_{c < gw} w[g][j][c][n] hid[t + j - k/2][g gw + c])
// One workgroup = one group x 64 output columns x 64 rows; grid (groups * column chunks, row tiles): the linear id puts a group's row
// tiles on one XCD (id % 8 = group % 8 for 16 groups), so its weights cross that L2 once.  The 64 + k - 1 input rows every tap of the
// tile reads are staged once in LDS (row pitch gw + 2 floats: the 32 rows of a ds_read_b64 fall on 32 different bank pairs); the K
// loop then streams nothing but the pack_kn weight image.  Four waves = 2 column halves x 2 halves of K (16-k units, in order); each
// holds two 32 x 32 accumulators (rows 0-31 / 32-63) that share its B operand.  A 4-k quad q of the image feeds two MFMAs: lane half
// h supplies k = 4q + 2h, then 4q + 2h + 1 (one 8-byte load per operand).  Sum order = fixed: each half of K in fp32 MFMA chains of
// 256 products added in order, lower half + upper half (through LDS), + bias; no atomics, bit-identical run to run.
#define POS_BM 64

__global__ __launch_bounds__(256) void pos_conv_kernel(const float* __restrict__ hid, int T, int E, int gw, int k,
                                                       const float* __restrict__ w, const float* __restrict__ bias,
                                                       float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int nch = (gw + 63) / 64;
    const int g = blockIdx.x / nch, chunk = blockIdx.x - g * nch;
    const int t0 = blockIdx.y * POS_BM;
    const int ldw = gw + 2, wrows = POS_BM + k - 1, c4n = gw / 4;
    // window row r = hid row t0 - k/2 + r, zero outside [0, T)
    for (int i = threadIdx.x; i < wrows * c4n; i += 256) {
        const int r = i / c4n, c = (i - r * c4n) * 4;
        const int t = t0 - k / 2 + r;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (t >= 0 && t < T) v = *reinterpret_cast<const f32x4*>(hid + (long)t * E + g * gw + c);
        *reinterpret_cast<f32x2*>(sm + r * ldw + c) = f32x2{v.x, v.y};
        *reinterpret_cast<f32x2*>(sm + r * ldw + c + 2) = f32x2{v.z, v.w};
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l31 = lane & 31, half = lane >> 5;
    const int ch = wave & 1, kh = wave >> 1;
    const int n0 = chunk * 64 + ch * 32;                   // first of this wave's 32 columns, within the group
    const bool live = n0 < gw;                             // wave-uniform (gw = 16 / 32 leave the second column half empty)
    const int n = min(n0 + l31, gw - 1);                   // columns past gw (gw % 32 == 16) load the last one and store nothing
    const int upt = gw / 16, nu = k * upt;                 // 16-k units: per tap, in all
    const int ua = kh ? (nu + 1) / 2 : 0, ub = kh ? nu : (nu + 1) / 2;
    // two levels of sums: the MFMA chains run over 16 units (256 products), then join the wave's totals -- a single chain of K / 2 =
    // 4096 fp32 additions measured 7.5x the rounding error of CPU fp32 GEMM at T = 1000
    f32x16 acc0, acc1, tot0, tot1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; tot0[r] = 0.f; tot1[r] = 0.f; }
    if (live && ua < ub) {
        // image of group g: [k gw / 4][gw][4]; unit u = quads 4u .. 4u + 3, 16 gw floats apart
        const float* wp = w + (long)g * k * gw * gw + (long)n * 4 + 2 * half;
        const long us = 16L * gw;
        f32x2 b0[4], b1[4], b2[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            b0[q] = *reinterpret_cast<const f32x2*>(wp + ua * us + q * 4 * gw);
            b1[q] = b2[q] = f32x2{0.f, 0.f};
            if (ua + 1 < ub) b1[q] = *reinterpret_cast<const f32x2*>(wp + (ua + 1) * us + q * 4 * gw);
            if (ua + 2 < ub) b2[q] = *reinterpret_cast<const f32x2*>(wp + (ua + 2) * us + q * 4 * gw);
        }
        int j = ua / upt, cu = ua - j * upt;
        for (int u = ua; u < ub; ++u) {
            const float* ap = sm + (l31 + j) * ldw + 16 * cu + 2 * half;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x2 a0 = *reinterpret_cast<const f32x2*>(ap + 4 * q);
                const f32x2 a1 = *reinterpret_cast<const f32x2*>(ap + 32 * ldw + 4 * q);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0[q].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b0[q].x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b0[q].y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b0[q].y, acc1, 0, 0, 0);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {                  // three units of weights in flight
                b0[q] = b1[q];
                b1[q] = b2[q];
                if (u + 3 < ub) b2[q] = *reinterpret_cast<const f32x2*>(wp + (u + 3) * us + q * 4 * gw);
            }
            if (++cu == upt) { cu = 0; ++j; }
            if (((u - ua) & 15) == 15 || u + 1 == ub) {
                tot0 += acc0;
                tot1 += acc1;
#pragma unroll
                for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
            }
        }
    }
    __syncthreads();                                       // the window is dead: its memory takes the upper half's partial sums
    float* red = sm + ch * 2048 + lane;                    // [column half][accumulator][register][lane]
    if (kh == 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { red[r * 64] = tot0[r]; red[1024 + r * 64] = tot1[r]; }
    }
    __syncthreads();
    if (kh == 0 && n0 + l31 < gw) {
        // accumulators: lane = column l31, registers = rows (r&3) + 8 (r>>2) + 4 half
        const int col = g * gw + n0 + l31;
        const float bv = bias[col];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (t < T) out[(long)t * E + col] = hid[(long)t * E + col] + gelu_erf((tot0[r] + red[r * 64]) + bv);
            if (t + 32 < T)
                out[(long)(t + 32) * E + col] = hid[(long)(t + 32) * E + col] + gelu_erf((tot1[r] + red[1024 + r * 64]) + bv);
        }
    }
}

}  // namespace

extern "C" int dawn_wave_normalize(const float* x, long n, double* stats2, float* out, void* stream) {
    if (n <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wave_stats_kernel, dim3(1), dim3(1024), 0, s, x, n, stats2);
    hipLaunchKernelGGL(wave_normalize_kernel, dim3(dawn_cdiv(n, 256 * 8)), dim3(256), 0, s, x, n, stats2, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_hubert_conv0(const float* x, long n, const float* w, const float* bias, int C, int k, int stride,
                                 float* out, void* stream) {
    if (C % 4 != 0 || n < k) return dawn_set_error_msg(-80, "dawn_hubert_conv0: C % 4 == 0 and n >= kernel size");
    const long T0 = (n - k) / stride + 1;
    hipLaunchKernelGGL(conv0_kernel, dim3(dawn_cdiv(T0 * (C / 4), 256)), dim3(256), 0, (hipStream_t)stream, x, n, w, bias, C, k,
                       stride, T0, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_ln_affine_act(const float* x, long rows, int C, const float* gamma, const float* beta, float eps, int act,
                                  float* out, void* stream) {
    if (C % 4 != 0 || C > 4096) return dawn_set_error_msg(-81, "dawn_ln_affine_act: C % 4 == 0, C <= 4096");
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(ln_affine_act_kernel, dim3(dawn_cdiv(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, rows, C, gamma, beta,
                       eps, act, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_add_act(const float* a, const float* b, int act, long n, float* out, void* stream) {
    if (n % 4 != 0) return dawn_set_error_msg(-82, "dawn_add_act: n % 4 == 0");
    if (n <= 0) return 0;
    long grid = dawn_cdiv(n / 4, 256);
    if (grid > 8192) grid = 8192;
    hipLaunchKernelGGL(add_act_kernel, dim3((int)grid), dim3(256), 0, (hipStream_t)stream, a, b, act, n / 4, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_attn64(const float* qkv, int T, int heads, float* out, void* stream) {
    if (T <= 0) return 0;
    hipLaunchKernelGGL(attn64_kernel, dim3(dawn_cdiv(T, 32), heads), dim3(64), 0, (hipStream_t)stream, qkv, T, heads, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_interp_linear(const float* y, long n, int C, const double* xi, long m, float* out, void* stream) {
    if (n < 2) return dawn_set_error_msg(-83, "dawn_interp_linear: needs at least two samples");
    if (m <= 0) return 0;
    hipLaunchKernelGGL(interp_linear_kernel, dim3(dawn_cdiv(m * C, 256)), dim3(256), 0, (hipStream_t)stream, y, n, C, xi, m, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_hubert_pos_conv(const float* hid, int T, int E, int groups, int k, const float* w, const float* bias, float* out,
                                    void* stream) {
    if (groups <= 0 || k <= 0 || E <= 0 || E % groups != 0 || (E / groups) % 16 != 0)
        return dawn_set_error_msg(-84, "dawn_hubert_pos_conv: E = groups * gw with gw % 16 == 0, k >= 1");
    if (T <= 0) return 0;
    const int gw = E / groups;
    const size_t lds = (size_t)(POS_BM + k - 1) * (gw + 2) * 4;
    if (lds > 65536) return dawn_set_error_msg(-84, "dawn_hubert_pos_conv: (63 + k) * (gw + 2) floats must fit 64 KB of LDS");
    if (!hid || !w || !bias || !out || (((uintptr_t)hid | (uintptr_t)w | (uintptr_t)out) & 15) != 0)
        return dawn_set_error_msg(-84, "dawn_hubert_pos_conv: NULL or not 16-byte aligned pointer");
    const float *he = hid + (long)T * E, *oe = out + (long)T * E;
    if (out < he && hid < oe) return dawn_set_error_msg(-85, "dawn_hubert_pos_conv: out overlaps hid (neighbouring rows are read)");
    hipLaunchKernelGGL(pos_conv_kernel, dim3(groups * ((gw + 63) / 64), dawn_cdiv(T, POS_BM)), dim3(256), lds < 16384 ? 16384 : lds,
                       (hipStream_t)stream, hid, T, E, gw, k, w, bias, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
