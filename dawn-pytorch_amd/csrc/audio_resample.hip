// Audio at any sample rate -> the 16 kHz fp32 mono samples that the HuBERT stage takes: a polyphase Kaiser-windowed-sinc resampler, defined
// here and in include/dawn_hip.h EXACTLY (it stands where the reference runs `ffmpeg -ar 16000`, UVG:223, 416-431; its values are this
// definition's, not swresample's, and nobody has measured the difference at the HuBERT features).
//
// Z = 32 zero crossings per side, BETA = 9 (Kaiser), CUT = 0.92.  For an integer rate in 1000 .. 384000, rate != 16000:
//     g = gcd(16000, rate);  L = 16000 / g;  M = rate / g;  n_out = floor(n_frames * 16000 / rate)            (64-bit integers)
//     rho = rate <= 16000 ? 1 : 16000.0 / rate;  W = Z / rho  (half width in input samples, fp64);  K = ceil(W)
//     h(u) = rho CUT sinc(rho CUT u) I0(BETA sqrt(1 - (u / W)^2)) / I0(BETA) for |u| < W, else 0
//     sinc(t) = sin(pi t) / (pi t), sinc(0) = 1;  I0(x) = sum_k ((x / 2)^k / k!)^2 until a term falls below 2^-60 of the sum
//     coef[r][j + K] = h(r / L - j), r = 0 .. L - 1, j = -K .. K: L rows of 2 K + 1 fp64 values (the workspace)
//     (q, r) = divmod(i M, L) in 64-bit integers;  y[i] = (float) sum_{j = -K .. K, ascending} x[q + j] coef[r][j + K]
// x[k] = 0 outside the signal, x exact (pcm / 32768 or the fp32 sample), the sum in fp64, ONE rounding to fp32, no clipping.  The position
// q + r / L is never formed as one floating-point number: r / L < 1 is, and j is subtracted from it.
//
// Two launches on the caller's stream.  resample_table_kernel: one thread per coefficient, fp64, FMA contraction off (the table is the
// definition's arithmetic, operation by operation).  resample_fir_kernel: a workgroup of 256 threads makes 256 consecutive outputs; it
// stages the input span x[q_first - K .. q_last + K] in LDS once as fp32 (exact for both source types; zeros outside the signal; the PCM
// pointer is 2-byte aligned only, so channel 0 is read with 16-bit loads), and each thread runs its 2 K + 1 taps in fp64 in ascending j.
// With L == 1 (32, 48, 96, 192 kHz) the single coefficient row goes to LDS as well; otherwise each thread streams its own row of the
// table.  Every thread's sum has a fixed order: bit-identical run to run.  Not tuned: profiles/audio_resample.md has the times beside
// the HuBERT stage's.
#include "audio_resample.h"

#include <math.h>
#include <numeric>

namespace {

constexpr int RS_Z = 32;
constexpr double RS_BETA = 9.0, RS_CUT = 0.92;
constexpr int RS_THREADS = 256;
// the longest span: rate 384000 -> 255 * 24 + 1 inputs between the first and the last centre, K <= 769 on each side, + 1 = 7660
constexpr int RS_SPAN_MAX = 7680;
constexpr int RS_TAPS_MAX = 1544;           // room for 2 * 769 + 1 = 1539 (the L == 1 row in LDS; 384 kHz has 1537)

__host__ __device__ inline double bessel_i0(double x) {
#pragma clang fp contract(off)
    const double y = x / 2.0;
    double p = 1.0, sum = 1.0;              // p = y^k / k!
    for (int k = 1; k < 1000; ++k) {
        p = p * y / (double)k;
        const double term = p * p;
        sum += term;
        if (term < 0x1p-60 * sum) break;
    }
    return sum;
}

struct RsPlan {
    long L, M;
    int K, taps;
    double rho, W, i0_beta;
    size_t table_bytes;
};

bool rate_ok(int rate) { return rate >= DAWN_RESAMPLE_MIN_RATE && rate <= DAWN_RESAMPLE_MAX_RATE; }

RsPlan rs_plan(int rate) {                  // rate_ok(rate) && rate != 16000
    RsPlan p;
    const long g = std::gcd(16000L, (long)rate);
    p.L = 16000 / g;
    p.M = rate / g;
    p.rho = rate <= 16000 ? 1.0 : 16000.0 / (double)rate;
    p.W = (double)RS_Z / p.rho;
    p.K = (int)ceil(p.W);
    p.taps = 2 * p.K + 1;
    p.i0_beta = bessel_i0(RS_BETA);
    p.table_bytes = a256((size_t)p.L * p.taps * sizeof(double));
    return p;
}

long rs_len(long n_frames, int rate) {
    if (n_frames < 1 || n_frames > DAWN_RESAMPLE_MAX_FRAMES || !rate_ok(rate)) return 0;
    return n_frames * 16000 / rate;
}

// coef[r * taps + j + K] = h(r / L - j)
__global__ __launch_bounds__(RS_THREADS) void resample_table_kernel(long L, int K, double rho, double W, double i0_beta,
                                                                    double* __restrict__ coef, long total) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * RS_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int taps = 2 * K + 1;
    const long r = idx / taps;
    const int j = (int)(idx - r * taps) - K;
    const double u = (double)r / (double)L - (double)j;
    double h = 0.0;
    if (fabs(u) < W) {
        const double t = rho * RS_CUT * u;
        const double s = t == 0.0 ? 1.0 : sin(M_PI * t) / (M_PI * t);
        const double v = u / W;
        const double in = 1.0 - v * v;
        h = rho * RS_CUT * s * bessel_i0(RS_BETA * sqrt(in > 0.0 ? in : 0.0)) / i0_beta;
    }
    coef[idx] = h;
}

__device__ __forceinline__ float sample_of(const int16_t* __restrict__ x, long k, int channels) {
    return (float)x[k * channels] / 32768.0f;           // exact
}
__device__ __forceinline__ float sample_of(const float* __restrict__ x, long k, int) { return x[k]; }

template <class T>
__global__ __launch_bounds__(RS_THREADS) void resample_fir_kernel(const T* __restrict__ x, long n_frames, int channels, long M, long L, int K,
                                                                  const double* __restrict__ coef, float* __restrict__ out, long n_out) {
    __shared__ float xs[RS_SPAN_MAX];
    __shared__ double cs[RS_TAPS_MAX];
    const int taps = 2 * K + 1;
    const long i0 = (long)blockIdx.x * RS_THREADS;
    const long i_last = min(i0 + RS_THREADS - 1, n_out - 1);
    const long q_first = i0 * M / L, q_last = i_last * M / L;
    const long s0 = q_first - K;                                               // the input index of xs[0]
    const int span = min((int)(q_last - q_first) + taps, RS_SPAN_MAX);          // (the host refuses a plan whose span would not fit)
    for (int t = threadIdx.x; t < span; t += RS_THREADS) {
        const long k = s0 + t;
        xs[t] = k >= 0 && k < n_frames ? sample_of(x, k, channels) : 0.0f;
    }
    const bool one_row = L == 1;
    if (one_row)
        for (int t = threadIdx.x; t < taps; t += RS_THREADS) cs[t] = coef[t];
    __syncthreads();
    const long i = i0 + threadIdx.x;
    if (i >= n_out) return;
    const long p = i * M, q = p / L, r = p - q * L;
    const float* xw = xs + (int)(q - q_first);                                  // xw[j + K] = x[q + j]
    double acc = 0.0;
    if (one_row) {
        for (int t = 0; t < taps; ++t) acc += (double)xw[t] * cs[t];
    } else {
        const double* c = coef + r * taps;
        for (int t = 0; t < taps; ++t) acc += (double)xw[t] * c[t];
    }
    out[i] = (float)acc;
}

int refuse(int code, const char* who, const char* what) {
    char m[240];
    snprintf(m, sizeof m, "%s: %s", who, what);
    return dawn_set_error_msg(code, m);
}

int refuse_rate(const char* who, int rate) {
    char m[200];
    snprintf(m, sizeof m, "rate = %d: %d .. %d", rate, DAWN_RESAMPLE_MIN_RATE, DAWN_RESAMPLE_MAX_RATE);
    return refuse(-332, who, m);
}

// n_frames and rate: the refusals both entries share; *len = dawn_resample16k_len
int length_check(long n_frames, int rate, long* len, const char* who) {
    char m[200];
    if (!rate_ok(rate)) return refuse_rate(who, rate);
    if (n_frames < 1 || n_frames > DAWN_RESAMPLE_MAX_FRAMES) {
        snprintf(m, sizeof m, "n_frames = %ld: 1 .. 2^34", n_frames);
        return refuse(-333, who, m);
    }
    *len = rs_len(n_frames, rate);
    if (*len < 1) {
        snprintf(m, sizeof m, "n_frames = %ld at rate = %d yields n_out = %ld: at least one output sample", n_frames, rate, *len);
        return refuse(-333, who, m);
    }
    return 0;
}

// out, n_out and the workspace, once the source is accepted
int output_check(long n_frames, int rate, long len, const float* out, long n_out, const void* workspace, size_t workspace_bytes,
                 const char* who) {
    char m[200];
    if (((uintptr_t)out & 3) != 0) return refuse(-331, who, "out is not 4-byte aligned");
    if (n_out != len) {
        snprintf(m, sizeof m, "n_out = %ld, dawn_resample16k_len(n_frames = %ld, rate = %d) = %ld", n_out, n_frames, rate, len);
        return refuse(-334, who, m);
    }
    if (rate == 16000) return 0;
    if (!workspace) return refuse(-331, who, "NULL workspace (required unless rate is 16000)");
    if (((uintptr_t)workspace & 7) != 0) return refuse(-331, who, "workspace is not 8-byte aligned");
    const size_t need = rs_plan(rate).table_bytes;
    if (workspace_bytes < need) return refuse_workspace(-335, who, workspace_bytes, need, "dawn_resample16k_workspace_bytes");
    if (overlaps(out, (size_t)n_out * 4, workspace, need)) return refuse(-336, who, "out overlaps the workspace");
    return 0;
}

template <class T>
int launch(const T* x, long n_frames, int channels, int rate, float* out, long n_out, void* workspace, void* stream, const char* who) {
    const RsPlan p = rs_plan(rate);
    const long span = (RS_THREADS - 1) * p.M / p.L + 1 + p.taps;
    if (span > RS_SPAN_MAX || p.taps > RS_TAPS_MAX) return refuse(-337, who, "internal: the input span of a workgroup exceeds its staging buffer");
    const hipStream_t st = (hipStream_t)stream;
    double* coef = (double*)workspace;
    const long total = p.L * p.taps;
    hipLaunchKernelGGL(resample_table_kernel, dim3((unsigned)((total + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, st, p.L, p.K, p.rho,
                       p.W, p.i0_beta, coef, total);
    DAWN_LAUNCH_CHECK();
    hipLaunchKernelGGL(resample_fir_kernel<T>, dim3((unsigned)((n_out + RS_THREADS - 1) / RS_THREADS)), dim3(RS_THREADS), 0, st, x, n_frames,
                       channels, p.M, p.L, p.K, (const double*)coef, out, n_out);
    DAWN_LAUNCH_CHECK();
    return 0;
}

}  // namespace

int resample_pcm_check(const int16_t* pcm, long n_frames, int channels, int rate, long* n_out, const char* who) {
    char m[200];
    if (!pcm) return refuse(-331, who, "NULL pointer (pcm and out are required)");
    if (((uintptr_t)pcm & 1) != 0) return refuse(-331, who, "pcm is not 2-byte aligned");
    if (channels < 1 || channels > 8) {
        snprintf(m, sizeof m, "channels = %d: 1 .. 8", channels);
        return refuse(-332, who, m);
    }
    return length_check(n_frames, rate, n_out, who);
}

extern "C" long dawn_resample16k_len(long n_frames, int rate) { return rs_len(n_frames, rate); }

extern "C" size_t dawn_resample16k_workspace_bytes(int rate) { return rate_ok(rate) && rate != 16000 ? rs_plan(rate).table_bytes : 0; }

extern "C" int dawn_resample16k_pcm16(const int16_t* pcm, long n_frames, int channels, int rate, float* out, long n_out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const char* who = "dawn_resample16k_pcm16";
    if (!pcm || !out) return refuse(-331, who, "NULL pointer (pcm and out are required)");
    long len = 0;
    CK(resample_pcm_check(pcm, n_frames, channels, rate, &len, who));
    CK(output_check(n_frames, rate, len, out, n_out, workspace, workspace_bytes, who));
    if (rate == 16000) return dawn_pcm16_to_samples(pcm, n_frames, channels, out, stream);
    return launch(pcm, n_frames, channels, rate, out, n_out, workspace, stream, who);
}

extern "C" int dawn_resample16k_f32(const float* x, long n_frames, int rate, float* out, long n_out, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    const char* who = "dawn_resample16k_f32";
    if (!x || !out) return refuse(-331, who, "NULL pointer (x and out are required)");
    if (((uintptr_t)x & 3) != 0) return refuse(-331, who, "x is not 4-byte aligned");
    long len = 0;
    CK(length_check(n_frames, rate, &len, who));
    CK(output_check(n_frames, rate, len, out, n_out, workspace, workspace_bytes, who));
    if (rate == 16000) {
        if (out != x && hipMemcpyAsync(out, x, (size_t)n_frames * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
            return dawn_set_error(hipGetLastError(), __FILE__, __LINE__);
        return 0;
    }
    return launch(x, n_frames, 1, rate, out, n_out, workspace, stream, who);
}
