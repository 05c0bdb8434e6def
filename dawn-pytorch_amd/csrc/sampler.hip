// DDIM and ancestral sampler step pieces, all on device, no host synchronisation inside the loop.
// Reference: GaussianDiffusion.ddim_sample MT:1169-1205 (predict_start_from_noise MT:1072-1076, dynamic
// thresholding by torch.quantile(|x0|, q) MT:1183-1196, DDIM update MT:1198-1205).  The clipping modes without a quantile (static
// s = 1, and no clipping) have ONE fused step-tail kernel per sampler instead: step_fixed_kernel below.
//
// The quantile is EXACT: a 3-pass radix select (11+10+10 bits) over the bit patterns of |x0| (non-negative
// floats order like unsigned ints) finds the order statistic v[lo]; v[lo+1] is either the same value
// (duplicates) or the smallest element above it (one more min pass); the result is torch's
// lerp(v[lo], v[hi], w).  Histograms are plain unsigned counters so that T-shards can all-reduce them.
#include "dawn_common.h"
#include "../../include/dawn_hip.h"
#include <stdio.h>

namespace {

__global__ __launch_bounds__(256) void ddim_x0_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                      float recip, float recipm1, long n, float* __restrict__ x0,
                                                      unsigned* __restrict__ hist) {
    __shared__ unsigned hs[2048];
    for (int i = threadIdx.x; i < 2048; i += 256) hs[i] = 0;
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float v = __fsub_rn(__fmul_rn(recip, x[i]), __fmul_rn(recipm1, eps[i]));
        x0[i] = v;
        const unsigned u = __float_as_uint(v) & 0x7fffffffu;
        atomicAdd(&hs[u >> 20], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += 256)
        if (hs[i]) atomicAdd(&hist[i], hs[i]);
}

// pass 2: keep (u>>20)==prefix, bin (u>>10)&1023 ; pass 3: keep (u>>10)==prefix, bin u&1023
// pass 4: hist[0] = min(u : u > prefix)   (hist[0] preset to 0x7fffffff, a NaN pattern no finite |x0| reaches; signed-MIN reducible)
__global__ __launch_bounds__(256) void select_hist_kernel(const float* __restrict__ x0, long n,
                                                          const unsigned* __restrict__ state, int pass,
                                                          unsigned* __restrict__ hist) {
    __shared__ unsigned hs[1024];
    const unsigned prefix = state[0];
    if (pass < 4) {
        for (int i = threadIdx.x; i < 1024; i += 256) hs[i] = 0;
    } else if (threadIdx.x == 0) {
        hs[0] = 0x7fffffffu;
    }
    __syncthreads();
    const int sh = pass == 2 ? 20 : 10;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const unsigned u = __float_as_uint(x0[i]) & 0x7fffffffu;
        if (pass == 4) {
            if (u > prefix) atomicMin(&hs[0], u);
        } else if ((u >> sh) == prefix) {
            atomicAdd(&hs[(pass == 2 ? (u >> 10) : u) & 1023u], 1u);
        }
    }
    __syncthreads();
    if (pass == 4) {
        if (threadIdx.x == 0) atomicMin(&hist[0], hs[0]);
    } else {
        for (int i = threadIdx.x; i < 1024; i += 256)
            if (hs[i]) atomicAdd(&hist[i], hs[i]);
    }
}

// single block: locate the bin holding 0-based rank r; state = {prefix, rank within bin, count in bin, dup flag}
__global__ __launch_bounds__(256) void select_scan_kernel(const unsigned* __restrict__ hist, int nbins,
                                                          unsigned long long rank0, unsigned* __restrict__ state,
                                                          int pass) {
    __shared__ unsigned long long part[256];
    const int per = nbins / 256;
    const int t = threadIdx.x;
    unsigned long long s = 0;
    for (int i = 0; i < per; ++i) s += hist[t * per + i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        const unsigned long long r = pass == 1 ? rank0 : (unsigned long long)state[1];
        unsigned long long cum = 0;
        int ch = -1;
        for (int i = 0; i < 256; ++i) {
            if (r < cum + part[i]) { ch = i; break; }
            cum += part[i];
        }
        if (ch < 0) { ch = 255; cum -= part[255]; }  // rank beyond the total count: clamp (inconsistent input)
        int b = ch * per + per - 1;
        unsigned long long before = cum;
        for (int i = 0; i < per; ++i) {
            const unsigned long long c = hist[ch * per + i];
            if (r < before + c) { b = ch * per + i; break; }
            if (i < per - 1) before += c;
        }
        const unsigned long long rin = r >= before ? r - before : 0;
        const unsigned prefix = pass == 1 ? 0u : state[0];
        state[0] = pass == 1 ? (unsigned)b : ((prefix << 10) | (unsigned)b);
        state[1] = (unsigned)rin;
        state[2] = hist[b];
        state[3] = (rin + 1 < (unsigned long long)hist[b]) ? 1u : 0u;
    }
}

__global__ void select_finalize_kernel(const unsigned* __restrict__ state, const unsigned* __restrict__ hmin,
                                       float weight, float* __restrict__ s_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const float lo = __uint_as_float(state[0]);
        float hi = lo;
        if (!state[3] && hmin[0] != 0x7fffffffu) hi = __uint_as_float(hmin[0]);
        // torch.lerp: w < 0.5 ? a + w (b-a) : b - (b-a)(1-w)
        const float df = __fsub_rn(hi, lo);
        float q = weight < 0.5f ? __fadd_rn(lo, __fmul_rn(weight, df)) : __fsub_rn(hi, __fmul_rn(df, __fsub_rn(1.0f, weight)));
        s_out[0] = fmaxf(q, 1.0f);
        s_out[1] = q;
    }
}

__global__ __launch_bounds__(256) void ddim_update_kernel(const float* __restrict__ x0, const float* __restrict__ eps,
                                                          const float* __restrict__ sp, const float* __restrict__ noise,
                                                          float san, float c, float sigma, long n,
                                                          float* __restrict__ x) {
    const float s = sp[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = fminf(fmaxf(x0[i], -s), s) / s;
        float r = __fadd_rn(__fmul_rn(v, san), __fmul_rn(c, eps[i]));
        if (noise) r = __fadd_rn(r, __fmul_rn(sigma, noise[i]));
        x[i] = r;
    }
}

// ancestral (DDPM) posterior step (GaussianDiffusion.p_sample MT:1113-1121 with q_posterior MT:1078-1085): the form of
// ddim_update_kernel with eps := x_t, san := c1, c := c2, sigma := std, so the two are bit-identical.  out may alias x_t
// (element-wise read-then-write): no __restrict__ on that pair.
__global__ __launch_bounds__(256) void ancestral_update_kernel(const float* __restrict__ x0, const float* x_t,
                                                               const float* __restrict__ sp, const float* __restrict__ noise,
                                                               float c1, float c2, float std, long n, float* out) {
    const float s = sp[0];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float v = fminf(fmaxf(x0[i], -s), s) / s;
        float r = __fadd_rn(__fmul_rn(v, c1), __fmul_rn(c2, x_t[i]));
        if (noise) r = __fadd_rn(r, __fmul_rn(std, noise[i]));
        out[i] = r;
    }
}

__device__ __forceinline__ void philox_round(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0,
                                             unsigned k1) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
}

// the four N(0,1) values of quad gq (= global element index / 4) of stream stream_id: Philox4x32-10 keyed by the seed, then Box-Muller.
// ONE definition for every kernel that draws (philox_normal_kernel, known_replace_kernel): their bits agree by construction.
__device__ __forceinline__ f32x4 philox_normal4(unsigned long long gq, unsigned long long seed, unsigned stream_id) {
    unsigned c0 = (unsigned)gq, c1 = (unsigned)(gq >> 32), c2 = stream_id, c3 = 0x44415757u;
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const float u0 = ((float)c0 + 0.5f) * 2.3283064365386963e-10f;
    const float u1 = ((float)c1 + 0.5f) * 2.3283064365386963e-10f;
    const float u2 = ((float)c2 + 0.5f) * 2.3283064365386963e-10f;
    const float u3 = ((float)c3 + 0.5f) * 2.3283064365386963e-10f;
    const float r0 = sqrtf(-2.0f * logf(fminf(fmaxf(u0, 1e-10f), 1.0f)));
    const float r1 = sqrtf(-2.0f * logf(fminf(fmaxf(u2, 1e-10f), 1.0f)));
    float s0, c0f, s1, c1f;
    sincosf(6.283185307179586f * u1, &s0, &c0f);
    sincosf(6.283185307179586f * u3, &s1, &c1f);
    f32x4 v = {r0 * c0f, r0 * s0, r1 * c1f, r1 * s1};
    return v;
}

// out (C, F, hw) local shard of a (C, Ftotal, hw) tensor; frames [f0, f0+F).  One Philox call per 4
// consecutive elements of the GLOBAL tensor => values do not depend on how T is sharded.
__global__ __launch_bounds__(256) void philox_normal_kernel(float* __restrict__ out, int C, int F, int f0, int Ftotal,
                                                            int hw, unsigned long long seed, unsigned stream_id) {
    const int qpf = hw >> 2;
    const long total = (long)C * F * qpf;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long)gridDim.x * 256) {
        const int qd = (int)(t % qpf);
        const long cf = t / qpf;
        const int f = (int)(cf % F), c = (int)(cf / F);
        const unsigned long long gq = ((unsigned long long)c * Ftotal + (f0 + f)) * qpf + qd;
        *reinterpret_cast<f32x4*>(out + ((long)c * F + f) * hw + qd * 4) = philox_normal4(gq, seed, stream_id);
    }
}

// ---- known-frame replacement (include/dawn_hip.h has the definition): x[:, f] = (a * known[:, f]) + (b * z[:, f]) for the frames with
// mask[f] != 0, two products and one sum, each rounded on its own (contraction off: a fused a*k + b*z would differ from the definition
// in the last bit); MODE 0 (b == 0): x = a * known, no noise read or drawn.  Grid (blocks per plane, frames, 3 channels): a block reads
// its frame's mask byte ONCE -- a uniform branch -- and leaves when it is zero, so a frame outside the known set costs no traffic.
// MODE 1, injected noise, any hw and any 4-byte alignment: when the plane's x / known / noise pointers are congruent modulo 16 bytes
// the block peels up to three scalar elements, runs a 128-bit body and a scalar tail; otherwise the whole plane goes scalar.
// MODE 2, the generator (hw % 4 == 0): one philox_normal4 per quad of the plane, keyed by the GLOBAL quad index exactly as
// philox_normal_kernel keys it, so the values are those dawn_philox_normal(seed, stream_id) writes at these elements, whatever the
// shard; 128-bit accesses when x and known are 16-byte aligned, four scalar ones otherwise.
__device__ __forceinline__ float known_one(float a, float k, float b, float z, bool has_z) {
#pragma clang fp contract(off)
    const float ak = a * k;
    if (!has_z) return ak;
    const float bz = b * z;
    return ak + bz;
}

template <int MODE>
__global__ __launch_bounds__(256) void known_replace_kernel(float* x, const float* __restrict__ known,
                                                            const unsigned char* __restrict__ mask, int F, int f0, int Ftotal, int hw,
                                                            float a, float b, const float* __restrict__ noise,
                                                            unsigned long long seed, unsigned stream_id) {
    const int c = blockIdx.z;
    const int start = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int f = blockIdx.y; f < F; f += gridDim.y) {
        if (mask[f] == 0) continue;                                     // uniform over the block
        const long plane = ((long)c * F + f) * hw;
        float* xp = x + plane;
        const float* kp = known + plane;
        if (MODE == 2) {
            const int qpf = hw >> 2;
            const bool vec = (((uintptr_t)xp | (uintptr_t)kp) & 15) == 0;
            const unsigned long long gq0 = ((unsigned long long)c * Ftotal + (f0 + f)) * qpf;
            for (int qd = start; qd < qpf; qd += stride) {
                const f32x4 z = philox_normal4(gq0 + qd, seed, stream_id);
                f32x4 kv, r;
                if (vec) kv = reinterpret_cast<const f32x4*>(kp)[qd];
                else { kv[0] = kp[4 * qd]; kv[1] = kp[4 * qd + 1]; kv[2] = kp[4 * qd + 2]; kv[3] = kp[4 * qd + 3]; }
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = known_one(a, kv[k], b, z[k], true);
                if (vec) reinterpret_cast<f32x4*>(xp)[qd] = r;
                else { xp[4 * qd] = r[0]; xp[4 * qd + 1] = r[1]; xp[4 * qd + 2] = r[2]; xp[4 * qd + 3] = r[3]; }
            }
            continue;
        }
        const float* np = MODE == 1 ? noise + plane : nullptr;
        const unsigned ax = (unsigned)((uintptr_t)xp >> 2) & 3u;
        const bool cong = ((unsigned)((uintptr_t)kp >> 2) & 3u) == ax && (MODE != 1 || ((unsigned)((uintptr_t)np >> 2) & 3u) == ax);
        int head = cong ? (int)((4u - ax) & 3u) : hw;                   // scalar elements before the 128-bit body
        if (head > hw) head = hw;
        const int n4 = (hw - head) >> 2;
        for (int i = start; i < n4; i += stride) {
            const f32x4 kv = reinterpret_cast<const f32x4*>(kp + head)[i];
            f32x4 zv = {0.f, 0.f, 0.f, 0.f};
            if (MODE == 1) zv = reinterpret_cast<const f32x4*>(np + head)[i];
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = known_one(a, kv[k], b, zv[k], MODE == 1);
            reinterpret_cast<f32x4*>(xp + head)[i] = r;
        }
        const int ns = hw - 4 * n4;                                     // scalar elements: [0, head) and [head + 4 n4, hw)
        for (int j = start; j < ns; j += stride) {
            const int i = j < head ? j : j + 4 * n4;
            xp[i] = known_one(a, kp[i], b, MODE == 1 ? np[i] : 0.f, MODE == 1);
        }
    }
}

// classifier-free guidance combine (MT:889-890): out = null + (cond - null) * scale
__global__ __launch_bounds__(256) void cfg_combine_kernel(const float* __restrict__ e_null, const float* __restrict__ e_cond,
                                                          float scale, long n, float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = __fadd_rn(e_null[i], __fmul_rn(__fsub_rn(e_cond[i], e_null[i]), scale));
}

// classifier-free guidance combine followed by the x0 prediction and the first radix-select histogram, in ONE pass: the same
// fp32 expressions as cfg_combine_kernel then ddim_x0_kernel, so eps, x0 and the histogram are bit-identical to the two-launch
// sequence.  (gfx950 ISA, -O3: the compiler contracts these expressions, identically in all three kernels -- eps = v_fmac(null,
// cond - null, scale), x0 = v_fma(recip, x, -(recipm1 * eps)).)  eps_out may alias e_null or e_cond (element-wise read-then-write).
__global__ __launch_bounds__(256) void cfg_x0_kernel(const float* e_null, const float* e_cond, float scale,
                                                     const float* __restrict__ x, float recip, float recipm1, long n,
                                                     float* eps_out, float* __restrict__ x0, unsigned* __restrict__ hist) {
    __shared__ unsigned hs[2048];
    for (int i = threadIdx.x; i < 2048; i += 256) hs[i] = 0;
    __syncthreads();
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float en = e_null[i];
        const float e = __fadd_rn(en, __fmul_rn(__fsub_rn(e_cond[i], en), scale));
        eps_out[i] = e;
        const float v = __fsub_rn(__fmul_rn(recip, x[i]), __fmul_rn(recipm1, e));
        x0[i] = v;
        const unsigned u = __float_as_uint(v) & 0x7fffffffu;
        atomicAdd(&hs[u >> 20], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2048; i += 256)
        if (hs[i]) atomicAdd(&hist[i], hs[i]);
}

// ---- step tails of the clipping modes that need no quantile (static: s == 1, MT:1095 / MT:1184; none: clip_denoised=False, DDIM only).
// ONE element-wise pass: x0 as ddim_x0_kernel forms it, v = clamp(x0, -1, 1) (clamp != 0) or x0, then the update of
// ddim_update_kernel (ANC = false: second operand eps) or ancestral_update_kernel (ANC = true: second operand x_t = x), so static
// equals the two-launch sequence with s = 1 bit for bit (clamp(x0,-1,1)/1 is exact).
// The roundings are PINNED here, to the ones the kernels above compile to (gfx950 ISA, -O3; the __f*_rn spellings do not stop the
// compiler's contraction): x0 = fma(recip, x, -(recipm1 * eps)) as in ddim_x0_kernel / cfg_x0_kernel; r = (v * a) + (b * m) with three
// roundings and r = fma(sigma, noise, r) as in ddim_update_kernel / ancestral_update_kernel.  Left to the compiler, the 128-bit body and
// the scalar tail of this very kernel came out contracted differently from each other; the GPU test holds the identity.
// x0 never goes through memory unless x0_out is given.  out may alias x (every thread reads its elements before it writes them): no
// __restrict__ on that pair.  vec != 0: every pointer is 16-byte aligned, 128-bit accesses over the first n/4*4 elements, scalar tail.
__device__ __forceinline__ float step_fixed_one(float xv, float ev, float recip, float recipm1, float a, float b, int clamp,
                                                bool anc, bool has_noise, float sg, float nz, float& x0v) {
#pragma clang fp contract(off)
    x0v = __builtin_fmaf(recip, xv, -(recipm1 * ev));
    const float v = clamp ? fminf(fmaxf(x0v, -1.0f), 1.0f) : x0v;
    float r = (v * a) + (b * (anc ? xv : ev));
    if (has_noise) r = __builtin_fmaf(sg, nz, r);
    return r;
}

template <bool ANC>
__global__ __launch_bounds__(256) void step_fixed_kernel(const float* x, const float* __restrict__ eps,
                                                         const float* __restrict__ noise, float recip, float recipm1, float a,
                                                         float b, float sg, int clamp, long n, int vec,
                                                         float* __restrict__ x0_out, float* out) {
    const long stride = (long)gridDim.x * 256;
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 ev = reinterpret_cast<const f32x4*>(eps)[i];
        f32x4 nv = {0.f, 0.f, 0.f, 0.f};
        if (noise) nv = reinterpret_cast<const f32x4*>(noise)[i];
        f32x4 r, x0v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t0;
            r[k] = step_fixed_one(xv[k], ev[k], recip, recipm1, a, b, clamp, ANC, noise != nullptr, sg, nv[k], t0);
            x0v[k] = t0;
        }
        if (x0_out) reinterpret_cast<f32x4*>(x0_out)[i] = x0v;
        reinterpret_cast<f32x4*>(out)[i] = r;
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float t0;
        const float t = step_fixed_one(x[i], eps[i], recip, recipm1, a, b, clamp, ANC, noise != nullptr, sg, noise ? noise[i] : 0.f, t0);
        if (x0_out) x0_out[i] = t0;
        out[i] = t;
    }
}

// ---- DPM-Solver++(2M) step tails (include/dawn_hip.h has the definition): out = A*x + b*v + c*v_prev with v the clipped x0, which is also
// stored (v_out) as the next step's history.  ONE expression for both kernels, roundings pinned: r = (A*x) + (b*v), three roundings, then
// r = fma(c, v_prev, r) when the history term exists -- so the fused kernel equals dawn_ddim_x0 followed by dawn_dpmpp_update bit for bit
// (static: clamp(x0,-1,1)/1 is exact), and the 128-bit body equals the scalar tail.  out may alias x and v_out may alias v_prev (every
// thread reads its elements before it writes them): no __restrict__ on those pairs.
__device__ __forceinline__ float dpmpp_one(float xv, float v, float pv, float A, float b, float c, bool has_prev) {
#pragma clang fp contract(off)
    float r = (A * xv) + (b * v);
    if (has_prev) r = __builtin_fmaf(c, pv, r);
    return r;
}
// v of the dynamic mode: clamp(x0, -s, s) / s (the expression of ddim_update_kernel)
__device__ __forceinline__ float dpmpp_v_dynamic(float x0v, float s) { return fminf(fmaxf(x0v, -s), s) / s; }
// v of the static / none modes from x and eps: x0 as step_fixed_one forms it, clamped to [-1, 1] or not
__device__ __forceinline__ float dpmpp_v_fixed(float xv, float ev, float recip, float recipm1, int clamp) {
#pragma clang fp contract(off)
    const float x0v = __builtin_fmaf(recip, xv, -(recipm1 * ev));
    return clamp ? fminf(fmaxf(x0v, -1.0f), 1.0f) : x0v;
}

// FIXED = false: in0 = x0, sp = the threshold; FIXED = true: in0 = eps, x0 is formed here and never goes through memory
template <bool FIXED>
__global__ __launch_bounds__(256) void dpmpp_kernel(const float* __restrict__ in0, const float* __restrict__ sp, const float* x,
                                                    const float* v_prev, float recip, float recipm1, float A, float b, float c,
                                                    int clamp, long n, int vec, float* v_out, float* out) {
    const float s = FIXED ? 1.0f : sp[0];
    const bool hp = v_prev != nullptr;
    const long stride = (long)gridDim.x * 256;
    const long n4 = vec ? (n >> 2) : 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const f32x4 iv = reinterpret_cast<const f32x4*>(in0)[i];
        const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i];
        f32x4 pv = {0.f, 0.f, 0.f, 0.f};
        if (hp) pv = reinterpret_cast<const f32x4*>(v_prev)[i];
        f32x4 r, v;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = FIXED ? dpmpp_v_fixed(xv[k], iv[k], recip, recipm1, clamp) : dpmpp_v_dynamic(iv[k], s);
            r[k] = dpmpp_one(xv[k], v[k], pv[k], A, b, c, hp);
        }
        reinterpret_cast<f32x4*>(v_out)[i] = v;
        reinterpret_cast<f32x4*>(out)[i] = r;
    }
    for (long i = n4 * 4 + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float xv = x[i], pv = hp ? v_prev[i] : 0.f;
        const float v = FIXED ? dpmpp_v_fixed(xv, in0[i], recip, recipm1, clamp) : dpmpp_v_dynamic(in0[i], s);
        const float r = dpmpp_one(xv, v, pv, A, b, c, hp);
        v_out[i] = v;
        out[i] = r;
    }
}

int grid_for(long n) {
    long g = (n + 255) / 256;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" int dawn_ddim_x0(const float* x, const float* eps, float recip, float recipm1, long n, float* x0,
                            unsigned* hist, void* stream) {
    hipLaunchKernelGGL(ddim_x0_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x, eps, recip, recipm1, n,
                       x0, hist);
    DAWN_LAUNCH_CHECK();
    return 0;
}
/* scratch of one threshold selection, laid out [hist1 2048 | hist2 1024 | hist3 1024 | state 4 | hmin 4] (4104 words): zero the
 * histograms / state and set hmin to INT_MAX.  Two runtime fills on the stream -- the host keeps ONE buffer per device instead of
 * allocating + zero-filling five tensors per DDIM step. */
extern "C" int dawn_select_ws_reset(unsigned* ws, void* stream) {
    hipError_t e = hipMemsetAsync(ws, 0, (size_t)(2048 + 1024 + 1024 + 4) * 4, (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(ws + 2048 + 1024 + 1024 + 4), 0x7fffffff, 4, (hipStream_t)stream);
    if (e != hipSuccess) return dawn_set_error(e, __FILE__, __LINE__);
    return 0;
}
extern "C" int dawn_select_scan(const unsigned* hist, int nbins, unsigned long long rank, unsigned* state, int pass,
                                void* stream) {
    if (nbins % 256 != 0) return dawn_set_error_msg(-70, "dawn_select_scan: nbins must be a multiple of 256");
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, nbins, rank, state, pass);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_select_hist(const float* x0, long n, const unsigned* state, int pass, unsigned* hist,
                                void* stream) {
    if (pass < 2 || pass > 4) return dawn_set_error_msg(-71, "dawn_select_hist: pass must be 2, 3 or 4");
    hipLaunchKernelGGL(select_hist_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x0, n, state, pass,
                       hist);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_select_finalize(const unsigned* state, const unsigned* hist3, float weight, float* s_out,
                                    void* stream) {
    hipLaunchKernelGGL(select_finalize_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, hist3, weight, s_out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_ddim_update(const float* x0, const float* eps, const float* s, const float* noise,
                                float sqrt_alpha_next, float c, float sigma, long n, float* x, void* stream) {
    hipLaunchKernelGGL(ddim_update_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x0, eps, s, noise,
                       sqrt_alpha_next, c, sigma, n, x);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_ancestral_update(const float* x0, const float* x_t, const float* s, const float* noise, float c1, float c2,
                                     float std, long n, float* out, void* stream) {
    if (out == x0 || (noise && out == noise))
        return dawn_set_error_msg(-78, "dawn_ancestral_update: out must not alias x0 or noise (out == x_t is allowed)");
    hipLaunchKernelGGL(ancestral_update_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, x0, x_t, s, noise, c1, c2,
                       std, n, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
// [p, p + n) and [q, q + n) share an element (NULL never does)
static bool ranges_overlap(const float* p, const float* q, long n) { return p && q && p < q + n && q < p + n; }
static int step_fixed_launch(bool anc, const char* who, const float* x, const float* eps, const float* noise, float recip,
                             float recipm1, float a, float b, float sg, int clamp, long n, float* x0_out, float* out, void* stream) {
    char msg[160];
    if (!x || !eps || !out || n < 0) {
        snprintf(msg, sizeof(msg), "%s: null argument", who);
        return dawn_set_error_msg(-79, msg);
    }
    if (clamp != 0 && clamp != 1) {
        snprintf(msg, sizeof(msg), "%s: clamp must be 1 (static) or 0 (none)", who);
        return dawn_set_error_msg(-79, msg);
    }
    if (anc && !clamp) {
        snprintf(msg, sizeof(msg), "%s: clamp = 0 does not exist for the ancestral step (p_sample always clips, MT:1113)", who);
        return dawn_set_error_msg(-79, msg);
    }
    const bool bad = (out != x && ranges_overlap(out, x, n)) || ranges_overlap(out, eps, n) || ranges_overlap(out, noise, n) ||
                     ranges_overlap(out, x0_out, n) || ranges_overlap(x0_out, x, n) || ranges_overlap(x0_out, eps, n) ||
                     ranges_overlap(x0_out, noise, n);
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: out must not alias eps, noise or x0_out (out == x is allowed); x0_out must not alias an input", who);
        return dawn_set_error_msg(-80, msg);
    }
    if (n == 0) return 0;
    const uintptr_t bits = (uintptr_t)x | (uintptr_t)eps | (uintptr_t)noise | (uintptr_t)x0_out | (uintptr_t)out;
    const int vec = (bits & 15) == 0 && n >= 4;
    const int grid = grid_for(vec ? (n + 3) / 4 : n);
    if (anc)
        hipLaunchKernelGGL(step_fixed_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, eps, noise, recip, recipm1, a,
                           b, sg, clamp, n, vec, x0_out, out);
    else
        hipLaunchKernelGGL(step_fixed_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, eps, noise, recip, recipm1, a,
                           b, sg, clamp, n, vec, x0_out, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_ddim_step_fixed(const float* x, const float* eps, const float* noise, float recip, float recipm1,
                                    float sqrt_alpha_next, float c, float sigma, int clamp, long n, float* x0_out, float* out,
                                    void* stream) {
    return step_fixed_launch(false, "dawn_ddim_step_fixed", x, eps, noise, recip, recipm1, sqrt_alpha_next, c, sigma, clamp, n, x0_out,
                             out, stream);
}
extern "C" int dawn_ancestral_step_fixed(const float* x_t, const float* eps, const float* noise, float recip, float recipm1, float c1,
                                         float c2, float std, int clamp, long n, float* x0_out, float* out, void* stream) {
    return step_fixed_launch(true, "dawn_ancestral_step_fixed", x_t, eps, noise, recip, recipm1, c1, c2, std, clamp, n, x0_out, out,
                             stream);
}
// in0 = x0 (fixed = false; s = the threshold) or eps (fixed = true; s = NULL).  Allowed aliases: out == x, v_out == v_prev.
static int dpmpp_launch(bool fixed, const char* who, const float* in0, const float* s, const float* x, const float* v_prev, float recip,
                        float recipm1, float A, float b, float c, int clamp, long n, float* v_out, float* out, void* stream) {
    char msg[200];
    if (!in0 || !x || !v_out || !out || (!fixed && !s) || n < 0) {
        snprintf(msg, sizeof(msg), "%s: null argument", who);
        return dawn_set_error_msg(-79, msg);
    }
    if (clamp != 0 && clamp != 1) {
        snprintf(msg, sizeof(msg), "%s: clamp must be 1 (static) or 0 (none)", who);
        return dawn_set_error_msg(-79, msg);
    }
    const bool bad = (out != x && ranges_overlap(out, x, n)) || (v_out != v_prev && ranges_overlap(v_out, v_prev, n)) ||
                     ranges_overlap(out, in0, n) || ranges_overlap(out, v_prev, n) || ranges_overlap(out, v_out, n) ||
                     ranges_overlap(v_out, in0, n) || ranges_overlap(v_out, x, n) ||
                     (s && s >= out && s < out + n) || (s && s >= v_out && s < v_out + n);      // (s[0] is all that is read)
    if (bad) {
        snprintf(msg, sizeof(msg), "%s: out and v_out must not alias each other or an input (out == x and v_out == v_prev are allowed)", who);
        return dawn_set_error_msg(-80, msg);
    }
    if (n == 0) return 0;
    const uintptr_t bits = (uintptr_t)in0 | (uintptr_t)x | (uintptr_t)v_prev | (uintptr_t)v_out | (uintptr_t)out;
    const int vec = (bits & 15) == 0 && n >= 4;
    const int grid = grid_for(vec ? (n + 3) / 4 : n);
    if (fixed)
        hipLaunchKernelGGL(dpmpp_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, in0, s, x, v_prev, recip, recipm1, A, b, c,
                           clamp, n, vec, v_out, out);
    else
        hipLaunchKernelGGL(dpmpp_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, in0, s, x, v_prev, recip, recipm1, A, b, c,
                           clamp, n, vec, v_out, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_dpmpp_update(const float* x0, const float* s, const float* x, const float* v_prev, float A, float b, float c, long n,
                                 float* v_out, float* out, void* stream) {
    return dpmpp_launch(false, "dawn_dpmpp_update", x0, s, x, v_prev, 0.f, 0.f, A, b, c, 1, n, v_out, out, stream);
}
extern "C" int dawn_dpmpp_step_fixed(const float* x, const float* eps, const float* v_prev, float recip, float recipm1, float A, float b,
                                     float c, int clamp, long n, float* v_out, float* out, void* stream) {
    return dpmpp_launch(true, "dawn_dpmpp_step_fixed", eps, nullptr, x, v_prev, recip, recipm1, A, b, c, clamp, n, v_out, out, stream);
}
extern "C" int dawn_cfg_combine(const float* e_null, const float* e_cond, float scale, long n, float* out,
                                void* stream) {
    hipLaunchKernelGGL(cfg_combine_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, e_null, e_cond, scale,
                       n, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_cfg_x0(const float* e_null, const float* e_cond, float scale, const float* x, float recip, float recipm1, long n,
                           float* eps_out, float* x0_out, unsigned* hist1, void* stream) {
    if (x0_out == x || x0_out == eps_out) return dawn_set_error_msg(-73, "dawn_cfg_x0: x0_out must not alias x or eps_out");
    hipLaunchKernelGGL(cfg_x0_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, e_null, e_cond, scale, x, recip,
                       recipm1, n, eps_out, x0_out, hist1);
    DAWN_LAUNCH_CHECK();
    return 0;
}
extern "C" int dawn_philox_normal(float* out, int C, int F, int f0, int Ftotal, int hw, uint64_t seed,
                                  uint32_t stream_id, void* stream) {
    if (hw % 4 != 0) return dawn_set_error_msg(-72, "dawn_philox_normal: h*w must be a multiple of 4");
    hipLaunchKernelGGL(philox_normal_kernel, dim3(grid_for((long)C * F * (hw / 4))), dim3(256), 0, (hipStream_t)stream,
                       out, C, F, f0, Ftotal, hw, (unsigned long long)seed, stream_id);
    DAWN_LAUNCH_CHECK();
    return 0;
}
/* the definition stands in include/dawn_hip.h */
extern "C" int dawn_known_replace(float* x, const float* known, const unsigned char* mask, int F, int f0, int Ftotal, int hw, float a,
                                  float b, const float* noise, uint64_t seed, uint32_t stream_id, void* stream) {
    if (!x || !known || !mask) return dawn_set_error_msg(-86, "dawn_known_replace: null argument (x, known and mask are required)");
    if (F < 0 || f0 < 0 || hw < 0 || (long)f0 + F > (long)Ftotal)
        return dawn_set_error_msg(-87, "dawn_known_replace: frames out of range (F >= 0, f0 >= 0, hw >= 0 and f0 + F <= Ftotal)");
    const long n = (long)3 * F * hw;
    if (ranges_overlap(x, known, n) || ranges_overlap(x, noise, n))
        return dawn_set_error_msg(-88, "dawn_known_replace: x must not overlap known or noise");
    const int mode = b == 0.0f ? 0 : noise ? 1 : 2;                  // b == 0: no noise is read or drawn
    if (mode == 2 && hw % 4 != 0) return dawn_set_error_msg(-72, "dawn_known_replace: h*w must be a multiple of 4 when the generator draws the noise");
    if (F == 0 || hw == 0) return 0;
    int bx = ((hw + 3) / 4 + 255) / 256;
    if (bx > 64) bx = 64;
    const dim3 grid(bx, F < 65535 ? F : 65535, 3);
    if (mode == 0)
        hipLaunchKernelGGL(known_replace_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, x, known, mask, F, f0, Ftotal, hw, a, b,
                           (const float*)nullptr, (unsigned long long)seed, stream_id);
    else if (mode == 1)
        hipLaunchKernelGGL(known_replace_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, known, mask, F, f0, Ftotal, hw, a, b, noise,
                           (unsigned long long)seed, stream_id);
    else
        hipLaunchKernelGGL(known_replace_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, x, known, mask, F, f0, Ftotal, hw, a, b,
                           (const float*)nullptr, (unsigned long long)seed, stream_id);
    DAWN_LAUNCH_CHECK();
    return 0;
}
