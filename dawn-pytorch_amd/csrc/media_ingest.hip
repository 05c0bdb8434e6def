// Media ingest: what a host holds after decoding -- an interleaved 8-bit image of any size, interleaved 16-bit PCM -- to what
// dawn_generate_clip takes: planar fp32 (3, Ho, Wo) in [0, 1] and fp32 mono samples.  Once per clip, integer arithmetic on the image
// path (bit-identical run to run, and to Pillow's 8-bit bilinear resample: UVG:320-325 Image.open().convert("RGB") ->
// transforms.Resize -> ToTensor), one exact division per PCM sample (soundfile's int16 scaling, channel 0: UVG:226, 451-452).
//
// The resample, per axis with input length n and output length m (Pillow's precompute_coeffs with the bilinear filter, support 1,
// and normalize_coeffs_8bpc), all in fp64 with every operation rounded on its own:
//     scale = n / m;  fs = max(scale, 1);  support = fs;  ss = 1 / fs
//     center = (i + 0.5) * scale;  lo = max((int)(center - support + 0.5), 0);  hi = min((int)(center + support + 0.5), n)
//     w[j] = max(1 - |(j + lo - center + 0.5) * ss|, 0) for j < hi - lo;  ww = w[0] + w[1] + ... left to right
//     k[j] = (int)(0.5 + (w[j] / ww) * 2^22);  out = clip8((2^21 + sum_j in[lo + j] * k[j]) >> 22), the sum in int32
// The tables are made on the device (resample_tables_kernel: one launch, both axes) because the stage contract has no place for a host
// buffer that outlives an asynchronous copy.  Device code contracts a + b * c into an FMA by default, which changes 0.5 + x * 2^22:
// contraction is off in axis_coeffs, and the division is the language's IEEE fp64 division.
//
// PASS ORDER.  Horizontal first (Ws -> Wo, every channel), rounded to BYTES, then vertical on those bytes: always.  A pass whose input
// and output lengths are equal is skipped (not run with unit weights); with both skipped the call is the layout conversion and / 255.
// This is the classic Pillow order.  Observation on Pillow 12.2.0: on some tall and narrow shapes (1023 x 3 -> 8 x 8, 4000 x 6 -> 4 x 4)
// that Pillow runs the vertical pass first and differs from this entry point by one level; on 2160 x 3840 -> 8 x 8, 1080 x 1920 ->
// 12 x 12, 777 x 1333 -> 8 x 16, 257 x 255 -> 256 x 256 and every small shape of tests/ingest_cases.py it agrees bit for bit.
//
// Memory access.  Source rows start at any byte and are row_bytes apart, so nothing about them is aligned.  The horizontal pass stages
// the span of a row that a tile of outputs reads through ALIGNED 32-bit loads into LDS (the first and last word may hold up to three
// bytes outside the span -- bytes of the same aligned word as a byte of the span, never used) and reads its taps from there; a span
// longer than the staging buffer goes through it in rounds, so a window of any length works.  The vertical pass walks down columns with
// the lanes of a wave on consecutive bytes of a row.  None of this is tuned: profiles/media_ingest.md has the times beside the sampler's.
#include "media_ingest.h"

#include <stddef.h>
#include <algorithm>

static_assert(sizeof(dawn_media_args) == 64 && offsetof(dawn_media_args, image) == 8 && offsetof(dawn_media_args, Hs) == 16 &&
                  offsetof(dawn_media_args, row_bytes) == 24 && offsetof(dawn_media_args, pix_bytes) == 32 &&
                  offsetof(dawn_media_args, pcm) == 40 && offsetof(dawn_media_args, n_frames) == 48 &&
                  offsetof(dawn_media_args, channels) == 56,
              "dawn_media_args layout");

namespace {

constexpr int COEF_BITS = 22;               // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int HP_THREADS = 256;
constexpr int HP_STAGE = 8192;              // source bytes staged per round (whole pixels: rounded down to a multiple of pix_bytes)

// One output index of one axis: bounds[2 i] = lo, bounds[2 i + 1] = taps, kk[i * ksize + j] = k[j].  ksize = 2 ceil(fs) + 1 bounds the
// taps (host: axis_ksize); the clamp below only keeps a table row inside its slot should the two ever disagree.
__device__ void axis_coeffs(int n, int m, int ksize, int i, int* __restrict__ bounds, int* __restrict__ kk) {
#pragma clang fp contract(off)
    const double scale = (double)n / (double)m;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs;
    const double ss = 1.0 / fs;
    const double center = ((double)i + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > n) hi = n;
    const int cnt = hi - lo < ksize ? hi - lo : ksize;
    auto weight = [&](int j) {
        double t = ((double)(j + lo) - center + 0.5) * ss;
        if (t < 0.0) t = -t;
        return t < 1.0 ? 1.0 - t : 0.0;
    };
    double ww = 0.0;
    for (int j = 0; j < cnt; ++j) ww += weight(j);
    int* k = kk + (long)i * ksize;
    for (int j = 0; j < cnt; ++j) {
        double w = weight(j);                   // the same bits as in the sum: nothing is stored in between
        if (ww != 0.0) w = w / ww;
        k[j] = (int)(0.5 + w * 4194304.0);
    }
    bounds[2 * i] = lo;
    bounds[2 * i + 1] = cnt;
}

struct AxisTab {
    int n, m, ksize;                            // n == m: the pass is skipped and nothing is written
    int* bounds;
    int* kk;
};

__global__ __launch_bounds__(64) void resample_tables_kernel(AxisTab h, AxisTab v) {
    const AxisTab a = blockIdx.y == 0 ? h : v;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (a.n == a.m || i >= a.m) return;
    axis_coeffs(a.n, a.m, a.ksize, i, a.bounds, a.kk);
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Horizontal pass.  A workgroup owns one source row and a tile of 256 / C outputs (C = 1 grey, 3 colour), a thread one (output, channel).
// tmp = (Hs, Wo, C) bytes in R, G, B order.  bv != NULL: rows that no vertical tap reads are left alone.
__global__ __launch_bounds__(HP_THREADS) void resample_rows_kernel(const unsigned char* __restrict__ src, long row_bytes, int pb, int C, int swap,
                                                                   int Wo, int tiles, const int* __restrict__ bh, const int* __restrict__ kh,
                                                                   int ksize, const int* __restrict__ bv, int Ho,
                                                                   unsigned char* __restrict__ tmp) {
    __shared__ uint32_t stage[HP_STAGE / 4 + 2];
    const int y = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    if (bv) {                                                                  // (the same for the whole workgroup: no barrier is skipped)
        const int last = 2 * (Ho - 1);
        if (y < bv[0] || y >= bv[last] + bv[last + 1]) return;
    }
    const int TX = HP_THREADS / C;
    const int x0 = tile * TX, xe = min(x0 + TX, Wo);
    const int xl = threadIdx.x / C, c = threadIdx.x % C;
    const int x = x0 + xl;
    const bool active = xl < TX && x < xe;
    int lo = 0, cnt = 0;
    if (active) {
        lo = bh[2 * x];
        cnt = min(bh[2 * x + 1], ksize);
    }
    const int coff = pb == 1 ? 0 : (swap ? 2 - c : c);
    const int* k = kh + (long)x * ksize;
    // lo and hi both grow with the output index: the tile reads the source pixels [p_first, p_last)
    const int p_first = bh[2 * x0], p_last = bh[2 * (xe - 1)] + bh[2 * (xe - 1) + 1];
    const unsigned char* row = src + (long)y * row_bytes;
    const int CP = HP_STAGE / pb;
    int acc = 1 << (COEF_BITS - 1);
    for (int p0 = p_first; p0 < p_last; p0 += CP) {
        const int pn = min(CP, p_last - p0);
        const unsigned char* g = row + (long)p0 * pb;
        const int a = (int)((uintptr_t)g & 3);
        const uint32_t* g4 = (const uint32_t*)(g - a);
        const int ndw = (a + pn * pb + 3) >> 2;                                 // <= (3 + HP_STAGE + 3) / 4
        for (int i = threadIdx.x; i < ndw; i += HP_THREADS) stage[i] = g4[i];
        __syncthreads();
        if (active) {
            const int j0 = max(0, p0 - lo), j1 = min(cnt, p0 + pn - lo);
            const unsigned char* s = (const unsigned char*)stage + a + coff;
            for (int j = j0; j < j1; ++j) acc += (int)s[(lo + j - p0) * pb] * k[j];
        }
        __syncthreads();
    }
    if (active) tmp[((long)y * Wo + x) * C + c] = (unsigned char)clip8(acc >> COEF_BITS);
}

// Vertical pass and the way out: a thread owns one (output row, column, channel) and walks down its column of `in` -- the bytes of the
// horizontal pass (in_pix = C) or, where that pass was skipped, the source itself (in_pix = pix_bytes).  Not WEIGHTED: the vertical pass is
// skipped too and the byte is taken as it is.  out3 = three planes in R, G, B order; grey goes to all three.
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void resample_cols_kernel(const unsigned char* __restrict__ in, long in_row, int in_pix, int C, int swap, int Wo,
                                                            int blocks_x, const int* __restrict__ bv, const int* __restrict__ kv, int ksize,
                                                            float* __restrict__ out3, long plane) {
    const int yo = blockIdx.x / blocks_x;
    const int e = (blockIdx.x % blocks_x) * 256 + threadIdx.x;
    if (e >= Wo * C) return;
    const int xo = e / C, c = e % C;
    const int coff = in_pix == 1 ? 0 : (swap ? 2 - c : c);
    const unsigned char* col = in + (long)xo * in_pix + coff;
    int v;
    if (WEIGHTED) {
        const int lo = bv[2 * yo], cnt = min(bv[2 * yo + 1], ksize);
        const int* k = kv + (long)yo * ksize;
        const unsigned char* p = col + (long)lo * in_row;
        int acc = 1 << (COEF_BITS - 1);
        for (int j = 0; j < cnt; ++j, p += in_row) acc += (int)*p * k[j];
        v = clip8(acc >> COEF_BITS);
    } else {
        v = col[(long)yo * in_row];
    }
    const float f = (float)v / 255.0f;                                         // one correctly rounded division: ToTensor()'s value
    float* o = out3 + (long)yo * Wo + xo;
    if (C == 1) {
        o[0] = f;
        o[plane] = f;
        o[2 * plane] = f;
    } else {
        o[(long)c * plane] = f;
    }
}

__global__ __launch_bounds__(256) void pcm16_kernel(const int16_t* __restrict__ pcm, long n, int channels, float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (float)pcm[i * channels] / 32768.0f;
}

// taps a table row has room for: Pillow's ksize = (int)ceil(support) * 2 + 1
int axis_ksize(int n, int m) {
    const double scale = (double)n / (double)m;
    const double fs = scale < 1.0 ? 1.0 : scale;
    int c = (int)fs;
    if ((double)c < fs) ++c;
    return 2 * c + 1;
}

// The workspace: [bounds_h | k_h | bounds_v | k_v | bytes of the horizontal pass], each rounded up to 256 bytes.  Every piece is sized
// whether or not its pass runs, and a coefficient table by the bound m * ksize <= 2 n + 3 m, so that the total grows with each argument.
struct IngestPlan {
    int ksize_h, ksize_v;
    size_t bh, kh, bv, kv, tmp, total;
};

bool sides_ok(int Hs, int Ws, int Ho, int Wo) {
    return Hs >= 1 && Ws >= 1 && Ho >= 1 && Wo >= 1 && Hs <= DAWN_INGEST_MAX_SIDE && Ws <= DAWN_INGEST_MAX_SIDE &&
           Ho <= DAWN_INGEST_MAX_SIDE && Wo <= DAWN_INGEST_MAX_SIDE;
}

IngestPlan ingest_plan(int Hs, int Ws, int Ho, int Wo) {
    IngestPlan p;
    p.ksize_h = axis_ksize(Ws, Wo);
    p.ksize_v = axis_ksize(Hs, Ho);
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += a256(bytes); return at; };
    p.bh = take((size_t)Wo * 8);
    p.kh = take(((size_t)2 * Ws + (size_t)3 * Wo) * 4);
    p.bv = take((size_t)Ho * 8);
    p.kv = take(((size_t)2 * Hs + (size_t)3 * Ho) * 4);
    p.tmp = take((size_t)Hs * Wo * 3);
    p.total = o;
    return p;
}

int refuse(int code, const char* who, const char* what) {
    char m[240];
    snprintf(m, sizeof m, "%s: %s", who, what);
    return dawn_set_error_msg(code, m);
}

}  // namespace

extern "C" size_t dawn_image_ingest_workspace_bytes(int Hs, int Ws, int Ho, int Wo) {
    return sides_ok(Hs, Ws, Ho, Wo) ? ingest_plan(Hs, Ws, Ho, Wo).total : 0;
}

int media_image_check(const unsigned char* src, int Hs, int Ws, long row_bytes, int pix_bytes, int order, int Ho, int Wo, long plane,
                      const char* who) {
    char m[200];
    if (!src) return refuse(-311, who, "NULL pointer (src, out3 and workspace are required)");
    if (!sides_ok(Hs, Ws, Ho, Wo)) {
        snprintf(m, sizeof m, "Hs = %d, Ws = %d, Ho = %d, Wo = %d: every side is 1 .. %d", Hs, Ws, Ho, Wo, DAWN_INGEST_MAX_SIDE);
        return refuse(-312, who, m);
    }
    if (pix_bytes != 1 && pix_bytes != 3 && pix_bytes != 4) {
        snprintf(m, sizeof m, "pix_bytes = %d: 1 (grey), 3 (RGB / BGR) or 4 (a fourth byte that is not read)", pix_bytes);
        return refuse(-313, who, m);
    }
    if (pix_bytes != 1 && order != DAWN_PIXELS_RGB && order != DAWN_PIXELS_BGR) {
        snprintf(m, sizeof m, "order = %d: DAWN_PIXELS_RGB or DAWN_PIXELS_BGR", order);
        return refuse(-313, who, m);
    }
    if (row_bytes < (long)Ws * pix_bytes) {
        snprintf(m, sizeof m, "row_bytes = %ld, a row of Ws = %d pixels holds %ld", row_bytes, Ws, (long)Ws * pix_bytes);
        return refuse(-314, who, m);
    }
    if (plane < (long)Ho * Wo) {
        snprintf(m, sizeof m, "plane = %ld floats, an output plane holds %ld", plane, (long)Ho * Wo);
        return refuse(-315, who, m);
    }
    return 0;
}

int media_pcm_check(const int16_t* pcm, long n_frames, int channels, const float* out, const char* who) {
    char m[200];
    if (!pcm || !out) return refuse(-318, who, "NULL pointer (pcm and out are required)");
    if (n_frames < 1) {
        snprintf(m, sizeof m, "n_frames = %ld: at least one", n_frames);
        return refuse(-319, who, m);
    }
    if (channels < 1 || channels > 8) {
        snprintf(m, sizeof m, "channels = %d: 1 .. 8", channels);
        return refuse(-319, who, m);
    }
    if (((uintptr_t)pcm & 1) != 0) return refuse(-319, who, "pcm is not 2-byte aligned");
    return 0;
}

extern "C" int dawn_image_ingest(const unsigned char* src, int Hs, int Ws, long row_bytes, int pix_bytes, int order, int Ho, int Wo,
                                 float* out3, long plane, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dawn_image_ingest";
    if (!src || !out3 || !workspace) return refuse(-311, who, "NULL pointer (src, out3 and workspace are required)");
    CK(media_image_check(src, Hs, Ws, row_bytes, pix_bytes, order, Ho, Wo, plane, who));
    const IngestPlan p = ingest_plan(Hs, Ws, Ho, Wo);
    if (workspace_bytes < p.total) return refuse_workspace(-316, who, workspace_bytes, p.total, "dawn_image_ingest_workspace_bytes");
    if (overlaps(out3, ((size_t)2 * plane + (size_t)Ho * Wo) * 4, workspace, p.total)) return refuse(-317, who, "out3 overlaps the workspace");
    char* ws = (char*)workspace;
    int *bh = (int*)(ws + p.bh), *kh = (int*)(ws + p.kh), *bv = (int*)(ws + p.bv), *kv = (int*)(ws + p.kv);
    unsigned char* tmp = (unsigned char*)(ws + p.tmp);
    const bool need_h = Ws != Wo, need_v = Hs != Ho;
    const int C = pix_bytes == 1 ? 1 : 3;
    const int swap = pix_bytes != 1 && order == DAWN_PIXELS_BGR;
    const hipStream_t st = (hipStream_t)stream;
    if (need_h || need_v) {
        const AxisTab th = {Ws, Wo, p.ksize_h, bh, kh}, tv = {Hs, Ho, p.ksize_v, bv, kv};
        hipLaunchKernelGGL(resample_tables_kernel, dim3(dawn_cdiv(std::max(Wo, Ho), 64), 2), dim3(64), 0, st, th, tv);
        DAWN_LAUNCH_CHECK();
    }
    if (need_h) {
        const int tiles = dawn_cdiv(Wo, HP_THREADS / C);
        hipLaunchKernelGGL(resample_rows_kernel, dim3((unsigned)Hs * (unsigned)tiles), dim3(HP_THREADS), 0, st, src, row_bytes, pix_bytes, C, swap, Wo,
                           tiles, bh, kh, p.ksize_h, need_v ? bv : (const int*)nullptr, Ho, tmp);
        DAWN_LAUNCH_CHECK();
    }
    // what the last kernel reads: the bytes of the horizontal pass (R, G, B order already), or the source
    const unsigned char* in = need_h ? tmp : src;
    const long in_row = need_h ? (long)Wo * C : row_bytes;
    const int in_pix = need_h ? C : pix_bytes, in_swap = need_h ? 0 : swap;
    const int blocks_x = dawn_cdiv((long)Wo * C, 256);
    const dim3 grid((unsigned)Ho * (unsigned)blocks_x);
    if (need_v)
        hipLaunchKernelGGL(resample_cols_kernel<true>, grid, dim3(256), 0, st, in, in_row, in_pix, C, in_swap, Wo, blocks_x, bv, kv, p.ksize_v, out3,
                           plane);
    else
        hipLaunchKernelGGL(resample_cols_kernel<false>, grid, dim3(256), 0, st, in, in_row, in_pix, C, in_swap, Wo, blocks_x, (const int*)nullptr,
                           (const int*)nullptr, 0, out3, plane);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_pcm16_to_samples(const int16_t* pcm, long n_frames, int channels, float* out, void* stream) {
    CK(media_pcm_check(pcm, n_frames, channels, out, "dawn_pcm16_to_samples"));
    const long blocks = (n_frames + 255) / 256;
    hipLaunchKernelGGL(pcm16_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, pcm, n_frames, channels,
                       out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
