// LFG motion encode: the five kernels between a driving video and the flow / occlusion latent that are not convolutions.
// The reference runs RegionPredictor (RP = LFG/modules/region_predictor.py), BGMotionPredictor (BG = bg_motion_predictor.py) and
// Generator.forward's PixelwiseFlowPredictor (PF = pixelwise_flow_predictor.py, UTIL = util.py) frame by frame on tensors that repeat the
// source image T times (FD:248-262); here the frames of a clip are a batch, the source side is computed once, and what the reference
// materialises per frame -- the (T,R,h,w) heatmap, eleven sparse-motion grids, eleven warped copies of the source -- lives in registers.
//
//   dawn_antialias_down   UTIL:217-264  AntiAliasInterpolation2d, only the kept pixels, separable, into conv rows
//   dawn_region_moments   RP:60-117     softmax over the pixels, mean, covariance (fp64 sums), closed-form 2x2 eigen-decomposition
//   dawn_bg_params        BG:42-57      spatial mean, fc, 3x3 matrix (bg_type 'affine')
//   dawn_motion_inputs    PF:48-120     heatmap differences and the source warped by every sparse motion, as the hourglass's input rows
//   dawn_flow_combine     PF:124-135    softmax over the masks, the dense flow, the occlusion map, in the latent's planar layout
//
// The three conv stacks between them run on dawn_conv_gemm / dawn_affine_act / dawn_bn_relu_pool2 (motion_encoder.py).  Every entry
// follows the stage contract: launches on `stream` only, no allocation, no synchronisation, every argument checked before the first
// launch, a refusal names the argument.  None of this is tuned: profiles/motion_encode.md has the times beside the conv stacks'.
//
// Coordinates.  make_coordinate_grid (UTIL:51-67) in fp32 with every operation rounded on its own: g(j, n) = 2 * (j / (n - 1)) - 1, so
// contraction is off where it is formed.  Sparse motion k of frame t (PF:66-93), recomputed wherever it is needed:
//     k = 0      (X, Y, Z) = bg[t] . (gx, gy, 1);  motion = (X / Z, Y / Z)
//     k >= 1     motion = M . (g - shift_d) + shift_s,   M = A_s . inverse(A_d),  M *= sign(M[0][0])     (revert_axis_swap; sign(0) = 0)
// M and the two inverse covariances of the heatmaps are formed once per workgroup in fp64 (2x2 inverses in closed form) and rounded
// to fp32; the per-pixel arithmetic is fp32 in the reference's order.
#include "dawn_host.h"

#include <math.h>

namespace {

constexpr int ME_MAX_R = 15;                                      // regions: (R + 1) quads of channels fit 64 columns
constexpr int ME_PARAM = 16;                                      // floats per region in LDS: M[4], shift_d[2], shift_s[2], Cd^-1[4], Cs^-1[4]
constexpr int AA_MAX_S = 8;                                       // 1 / scale
constexpr int AA_TILE = 16;                                       // outputs per side of a workgroup's tile
constexpr int AA_MAX_K = 4 * (AA_MAX_S - 1) + 1;                  // taps: 2 * round(4 sigma) + 1 with sigma = (s - 1) / 2
constexpr int AA_MAX_ROWS = AA_MAX_S * (AA_TILE - 1) + AA_MAX_K;  // input rows under a tile

int refuse(int code, const char* who, const char* what) {
    char m[240];
    snprintf(m, sizeof m, "%s: %s", who, what);
    return dawn_set_error_msg(code, m);
}

struct AaTaps {
    float g[AA_MAX_K];       // the reference's fp32 1-D factors exp(-(i - mean)^2 / (2 sigma^2))
    float sum;               // the sum of the fp32 products g[i] * g[j], taken in double and rounded once
};

__device__ __forceinline__ float grid_coord(int j, int n) {
#pragma clang fp contract(off)
    return 2.0f * ((float)j / (float)(n - 1)) - 1.0f;
}

// ---------------------------------------------------------------------------------------------------------------- antialias_down
// A workgroup owns a 16 x 16 tile of outputs of one frame.  Pass 1: the horizontal taps of every input row under the tile, at the
// tile's 16 kept columns, into LDS (zero where the row or the tap lies in the padding).  Pass 2: the vertical taps from LDS, / sum.
template <bool U8>
__global__ __launch_bounds__(256) void antialias_down_kernel(const void* __restrict__ in, long frame_stride, long chan_stride, int H, int W,
                                                             int s, int K, AaTaps taps, int ho, int wo, int tiles_x,
                                                             float* __restrict__ out, int ld_out, int c_pad) {
    __shared__ float hbuf[AA_MAX_ROWS * AA_TILE * 3];
    const int t = blockIdx.y;
    const int yo0 = (blockIdx.x / tiles_x) * AA_TILE, xo0 = (blockIdx.x % tiles_x) * AA_TILE;
    const int ka = K / 2;
    const int rows = s * (AA_TILE - 1) + K;
    const int y_base = s * yo0 - ka;
    for (int i = threadIdx.x; i < rows * AA_TILE * 3; i += 256) {
        const int xl = i % AA_TILE, c = (i / AA_TILE) % 3, r = i / (AA_TILE * 3);
        const int y = y_base + r, xo = xo0 + xl;
        float acc = 0.f;
        if (y >= 0 && y < H && xo < wo) {
            const int xb = s * xo - ka;
            for (int j = 0; j < K; ++j) {
                const int x = xb + j;
                if (x < 0 || x >= W) continue;
                float v;
                if (U8) v = (float)((const unsigned char*)in)[(long)t * frame_stride + ((long)y * W + x) * 3 + c] / 255.0f;
                else v = ((const float*)in)[(long)t * frame_stride + (long)c * chan_stride + (long)y * W + x];
                acc = fmaf(taps.g[j], v, acc);
            }
        }
        hbuf[(r * AA_TILE + xl) * 3 + c] = acc;
    }
    __syncthreads();
    const int xl = threadIdx.x % AA_TILE, yl = threadIdx.x / AA_TILE;
    const int yo = yo0 + yl, xo = xo0 + xl;
    if (yo >= ho || xo >= wo) return;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int j = 0; j < K; ++j) {
        const float* p = &hbuf[((s * yl + j) * AA_TILE + xl) * 3];
        a0 = fmaf(taps.g[j], p[0], a0);
        a1 = fmaf(taps.g[j], p[1], a1);
        a2 = fmaf(taps.g[j], p[2], a2);
    }
    float* o = out + (((long)t * ho + yo) * wo + xo) * ld_out;
    o[0] = a0 / taps.sum;
    o[1] = a1 / taps.sum;
    o[2] = a2 / taps.sum;
    for (int c = 3; c < c_pad; ++c) o[c] = 0.f;
}

// ---------------------------------------------------------------------------------------------------------------- region_moments
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    return v;
}

// One workgroup per (frame, region).  Pass 1: the maximum.  Pass 2: e = exp((x - max) / temperature) in fp64 and the six sums
// S, Sx, Sy, Sxx, Sxy, Syy of e, e g, e g g^T; shift = (Sx, Sy) / S, covar = (Sxx, Sxy, Syy) / S - shift shift^T (fp64: the
// cancellation costs nothing there).  affine = U diag(sqrt(s)): covar = [[a, b], [b, c]], hd = (a - c) / 2, rad = sqrt(hd^2 + b^2),
// s1 = (a + c) / 2 + rad, s2 = det / s1; u1 = the unit eigenvector of s1 -- (hd + rad, b) where hd >= 0, (b, rad - hd) otherwise, (1, 0)
// where both vanish -- with u1.x > 0, or u1.x == 0 and u1.y > 0; u2 = (u1.y, -u1.x), so det U = -1.
__global__ __launch_bounds__(256) void region_moments_kernel(const float* __restrict__ x, int ld, int h, int w, int R, double temperature,
                                                             float* __restrict__ shift, float* __restrict__ covar, float* __restrict__ affine) {
    __shared__ float redf[4];
    __shared__ double redd[4][6];
    const int t = blockIdx.x / R, r = blockIdx.x % R;
    const int hw = h * w;
    const float* xp = x + (long)t * hw * ld + r;
    float m = -INFINITY;
    for (int p = threadIdx.x; p < hw; p += 256) m = fmaxf(m, xp[(long)p * ld]);
    m = block_max(m, redf);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = threadIdx.x; p < hw; p += 256) {
        const double e = exp(((double)xp[(long)p * ld] - (double)m) / temperature);
        const double gx = (double)grid_coord(p % w, w), gy = (double)grid_coord(p / w, h);
        acc[0] += e;
        acc[1] += e * gx;
        acc[2] += e * gy;
        acc[3] += e * gx * gx;
        acc[4] += e * gx * gy;
        acc[5] += e * gy * gy;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = wave_sum_d(acc[i]);
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < 6; ++i) redd[threadIdx.x >> 6][i] = acc[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[6];
    for (int i = 0; i < 6; ++i) s[i] = (redd[0][i] + redd[1][i]) + (redd[2][i] + redd[3][i]);
    const double mx = s[1] / s[0], my = s[2] / s[0];
    const double a = s[3] / s[0] - mx * mx, b = s[4] / s[0] - mx * my, c = s[5] / s[0] - my * my;
    const long o = (long)t * R + r;
    shift[o * 2] = (float)mx;
    shift[o * 2 + 1] = (float)my;
    covar[o * 4] = (float)a;
    covar[o * 4 + 1] = (float)b;
    covar[o * 4 + 2] = (float)b;
    covar[o * 4 + 3] = (float)c;
    const double hd = 0.5 * (a - c), rad = sqrt(hd * hd + b * b);
    const double s1 = 0.5 * (a + c) + rad;
    double s2 = s1 > 0.0 ? (a * c - b * b) / s1 : 0.0;
    if (s2 < 0.0) s2 = 0.0;
    double ux = hd >= 0.0 ? hd + rad : b, uy = hd >= 0.0 ? b : rad - hd;
    const double n = sqrt(ux * ux + uy * uy);
    if (n > 0.0) {
        ux /= n;
        uy /= n;
    } else {
        ux = 1.0;
        uy = 0.0;
    }
    if (ux < 0.0 || (ux == 0.0 && uy < 0.0)) {
        ux = -ux;
        uy = -uy;
    }
    const double q1 = sqrt(s1 > 0.0 ? s1 : 0.0), q2 = sqrt(s2);
    affine[o * 4] = (float)(ux * q1);
    affine[o * 4 + 1] = (float)(uy * q2);
    affine[o * 4 + 2] = (float)(uy * q1);
    affine[o * 4 + 3] = (float)(-ux * q2);
}

// ---------------------------------------------------------------------------------------------------------------- bg_params
// One workgroup per frame: a thread owns channels c, c + 256, ...: their spatial means (fp64) times the six rows of fc, summed over
// the workgroup in fp64, + bias; the third row of the matrix is (0, 0, 1).
__global__ __launch_bounds__(256) void bg_params_kernel(const float* __restrict__ x, int ld, int npix, int C, const float* __restrict__ fcw,
                                                        const float* __restrict__ fcb, float* __restrict__ out) {
    __shared__ double redd[4][6];
    const int t = blockIdx.x;
    const float* xp = x + (long)t * npix * ld;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int c = threadIdx.x; c < C; c += 256) {
        double sum = 0.0;
        for (int p = 0; p < npix; ++p) sum += (double)xp[(long)p * ld + c];
        const double mean = sum / (double)npix;
#pragma unroll
        for (int o = 0; o < 6; ++o) acc[o] += mean * (double)fcw[(long)o * C + c];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = wave_sum_d(acc[i]);
    if ((threadIdx.x & 63) == 0)
        for (int i = 0; i < 6; ++i) redd[threadIdx.x >> 6][i] = acc[i];
    __syncthreads();
    if (threadIdx.x >= 9) return;
    const int i = threadIdx.x;
    float v = i == 8 ? 1.0f : 0.0f;
    if (i < 6) v = (float)((redd[0][i] + redd[1][i]) + (redd[2][i] + redd[3][i]) + (double)fcb[i]);
    out[(long)t * 9 + i] = v;
}

// ---------------------------------------------------------------------------------------------------------------- sparse motions
struct MotionParams {
    const float* d_shift;    // (T, R, 2)   driving, per frame
    const float* d_covar;    // (T, R, 2, 2)
    const float* d_affine;   // (T, R, 2, 2)
    const float* s_shift;    // (R, 2)      source, once per clip
    const float* s_covar;    // (R, 2, 2)
    const float* s_affine;   // (R, 2, 2)
    const float* bg;         // (T, 3, 3)
    int R;
};

// Frame t's per-region constants into P[R][ME_PARAM] and its background matrix into B[9] (threads 0 .. R - 1 and 64 .. 72), then a barrier.
// COVAR false: the covariances are neither read nor inverted (dawn_flow_combine has none).
template <bool COVAR>
__device__ __forceinline__ void motion_prepare(const MotionParams& a, int t, float* P, float* B) {
    const int k = threadIdx.x;
    if (k < a.R) {
        const float* Ad = a.d_affine + ((long)t * a.R + k) * 4;
        const float* As = a.s_affine + (long)k * 4;
        const double det = (double)Ad[0] * Ad[3] - (double)Ad[1] * Ad[2];
        const double i0 = Ad[3] / det, i1 = -Ad[1] / det, i2 = -Ad[2] / det, i3 = Ad[0] / det;
        float M[4] = {(float)(As[0] * i0 + As[1] * i2), (float)(As[0] * i1 + As[1] * i3), (float)(As[2] * i0 + As[3] * i2),
                      (float)(As[2] * i1 + As[3] * i3)};
        const float sg = M[0] > 0.f ? 1.f : (M[0] < 0.f ? -1.f : 0.f);
        float* p = P + k * ME_PARAM;
        for (int i = 0; i < 4; ++i) p[i] = M[i] * sg;
        p[4] = a.d_shift[((long)t * a.R + k) * 2];
        p[5] = a.d_shift[((long)t * a.R + k) * 2 + 1];
        p[6] = a.s_shift[k * 2];
        p[7] = a.s_shift[k * 2 + 1];
        if (COVAR) {
            const float* Cd = a.d_covar + ((long)t * a.R + k) * 4;
            const float* Cs = a.s_covar + (long)k * 4;
            const double dd = (double)Cd[0] * Cd[3] - (double)Cd[1] * Cd[2], ds = (double)Cs[0] * Cs[3] - (double)Cs[1] * Cs[2];
            p[8] = (float)(Cd[3] / dd);
            p[9] = (float)(-Cd[1] / dd);
            p[10] = (float)(-Cd[2] / dd);
            p[11] = (float)(Cd[0] / dd);
            p[12] = (float)(Cs[3] / ds);
            p[13] = (float)(-Cs[1] / ds);
            p[14] = (float)(-Cs[2] / ds);
            p[15] = (float)(Cs[0] / ds);
        }
    }
    if (k >= 64 && k < 73) B[k - 64] = a.bg[(long)t * 9 + (k - 64)];
    __syncthreads();
}

// sparse motion k (0 = background) at the grid point (gx, gy)
__device__ __forceinline__ void sparse_motion(const float* P, const float* B, int k, float gx, float gy, float& mx, float& my) {
#pragma clang fp contract(off)
    if (k == 0) {
        const float X = B[0] * gx + B[1] * gy + B[2], Y = B[3] * gx + B[4] * gy + B[5], Z = B[6] * gx + B[7] * gy + B[8];
        mx = X / Z;
        my = Y / Z;
        return;
    }
    const float* p = P + (k - 1) * ME_PARAM;
    const float dx = gx - p[4], dy = gy - p[5];
    mx = (p[0] * dx + p[1] * dy) + p[6];
    my = (p[2] * dx + p[3] * dy) + p[7];
}

// grid_sample(bilinear, zeros, align_corners=False) corner set, in ATen's nw, ne, sw, se order (the arithmetic of flow_decode.hip)
struct Corners { int i[4]; float w[4]; };
__device__ __forceinline__ Corners corners_at(float gx, float gy, int Hs, int Ws) {
    float ix = ((gx + 1.0f) * (float)Ws - 1.0f) * 0.5f;
    float iy = ((gy + 1.0f) * (float)Hs - 1.0f) * 0.5f;
    ix = fminf(fmaxf(ix, -2.0f), (float)Ws + 1.0f);          // far outside (or NaN): every corner is outside; keeps the int conversion defined
    iy = fminf(fmaxf(iy, -2.0f), (float)Hs + 1.0f);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float ex = ix - fx0, ey = iy - fy0;
    const float wx1 = (fx0 + 1.0f) - ix, wy1 = (fy0 + 1.0f) - iy;
    Corners c;
    c.w[0] = wx1 * wy1; c.w[1] = ex * wy1; c.w[2] = wx1 * ey; c.w[3] = ex * ey;
    const bool xi0 = x0 >= 0 && x0 < Ws, xi1 = x1 >= 0 && x1 < Ws, yi0 = y0 >= 0 && y0 < Hs, yi1 = y1 >= 0 && y1 < Hs;
    c.i[0] = (xi0 && yi0) ? y0 * Ws + x0 : -1;
    c.i[1] = (xi1 && yi0) ? y0 * Ws + x1 : -1;
    c.i[2] = (xi0 && yi1) ? y1 * Ws + x0 : -1;
    c.i[3] = (xi1 && yi1) ? y1 * Ws + x1 : -1;
    return c;
}

constexpr int MI_PIX = 64;          // pixels of one frame per workgroup

// A workgroup owns 64 pixels of one frame; an item is one (pixel, k): the four channels 4k .. 4k + 3 of the pixel's row, one 16-byte
// store.  k > R: the zero channels that pad the row to c_pad.
__global__ __launch_bounds__(256) void motion_inputs_kernel(MotionParams a, const float* __restrict__ src, int ld_src, int h, int w,
                                                            float* __restrict__ out, int ld_out, int c_pad) {
    __shared__ float P[ME_MAX_R * ME_PARAM];
    __shared__ float B[9];
    const int t = blockIdx.y;
    motion_prepare<true>(a, t, P, B);
    const int hw = h * w, KQ = c_pad / 4;
    const int p0 = blockIdx.x * MI_PIX;
    const int np = min(MI_PIX, hw - p0);
    for (int i = threadIdx.x; i < np * KQ; i += 256) {
        const int k = i % KQ, p = p0 + i / KQ;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (k <= a.R) {
            const float gx = grid_coord(p % w, w), gy = grid_coord(p / w, h);
            if (k > 0) {
                const float* q = P + (k - 1) * ME_PARAM;
                const float dx = gx - q[4], dy = gy - q[5], sx = gx - q[6], sy = gy - q[7];
                const float ud = (dx * q[8] + dy * q[10]) * dx + (dx * q[9] + dy * q[11]) * dy;
                const float us = (sx * q[12] + sy * q[14]) * sx + (sx * q[13] + sy * q[15]) * sy;
                v[0] = expf(-0.5f * ud) - expf(-0.5f * us);
            }
            float mx, my;
            sparse_motion(P, B, k, gx, gy, mx, my);
            const Corners cr = corners_at(mx, my, h, w);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (cr.i[j] < 0) continue;
                const float* s = src + (long)cr.i[j] * ld_src;
                v[1] += s[0] * cr.w[j];
                v[2] += s[1] * cr.w[j];
                v[3] += s[2] * cr.w[j];
            }
        }
        *reinterpret_cast<f32x4*>(out + ((long)t * hw + p) * ld_out + 4 * k) = v;
    }
}

// A thread owns one pixel of one frame: softmax over the R + 1 mask channels of its row, the eleven motions again, their weighted
// sum in k order, the sigmoid of channel R + 1.
__global__ __launch_bounds__(256) void flow_combine_kernel(MotionParams a, const float* __restrict__ x, int ld, int h, int w,
                                                           float* __restrict__ grid, long grid_plane, float* __restrict__ conf, int conf_x0) {
    __shared__ float P[ME_MAX_R * ME_PARAM];
    __shared__ float B[9];
    const int t = blockIdx.y;
    motion_prepare<false>(a, t, P, B);
    const int hw = h * w;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const float* row = x + ((long)t * hw + p) * ld;
    float e[ME_MAX_R + 1];
    float m = row[0];
    for (int k = 1; k <= a.R; ++k) m = fmaxf(m, row[k]);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k <= ME_MAX_R; ++k) {
        e[k] = k <= a.R ? expf(row[k] - m) : 0.f;
        sum += e[k];
    }
    const float gx = grid_coord(p % w, w), gy = grid_coord(p / w, h);
    float fx = 0.f, fy = 0.f;
#pragma unroll
    for (int k = 0; k <= ME_MAX_R; ++k) {
        if (k > a.R) break;
        float mx, my;
        sparse_motion(P, B, k, gx, gy, mx, my);
        const float wk = e[k] / sum;
        fx += mx * wk;
        fy += my * wk;
    }
    const float oc = 1.0f / (1.0f + expf(-row[a.R + 1]));
    const long o = (long)t * hw + p;
    grid[o] = fx;
    grid[grid_plane + o] = fy;
    conf[o] = conf_x0 ? 2.0f * oc - 1.0f : oc;
}

int check_motion(const char* who, const float* d_shift, const float* d_covar, const float* d_affine, const float* s_shift,
                 const float* s_covar, const float* s_affine, const float* bg, int R, int T, int h, int w) {
    char m[200];
    if (!d_shift) return refuse(-421, who, "drv_shift is NULL");
    if (!d_covar) return refuse(-421, who, "drv_covar is NULL");
    if (!d_affine) return refuse(-421, who, "drv_affine is NULL");
    if (!s_shift) return refuse(-421, who, "src_shift is NULL");
    if (!s_covar) return refuse(-421, who, "src_covar is NULL");
    if (!s_affine) return refuse(-421, who, "src_affine is NULL");
    if (!bg) return refuse(-421, who, "bg_params is NULL");
    if (R < 1 || R > ME_MAX_R) {
        snprintf(m, sizeof m, "R = %d: 1 .. %d regions", R, ME_MAX_R);
        return refuse(-422, who, m);
    }
    if (T < 1 || T > 65535) {
        snprintf(m, sizeof m, "T = %d: 1 .. 65535 frames per call", T);
        return refuse(-423, who, m);
    }
    if (h < 2 || w < 2 || h > 4096 || w > 4096) {
        snprintf(m, sizeof m, "h = %d, w = %d: every side is 2 .. 4096 (the coordinate grid divides by side - 1)", h, w);
        return refuse(-424, who, m);
    }
    return 0;
}

}  // namespace

extern "C" int dawn_antialias_down(const void* in, int in_kind, long frame_stride, long chan_stride, int T, int H, int W, int s, float* out,
                                   int ld_out, int c_pad, void* stream) {
    const char* who = "dawn_antialias_down";
    char m[200];
    if (!in) return refuse(-401, who, "in is NULL");
    if (!out) return refuse(-401, who, "out is NULL");
    if (in_kind != 0 && in_kind != 1) {
        snprintf(m, sizeof m, "in_kind = %d: 0 (fp32 planes) or 1 (uint8 H x W x 3 frames)", in_kind);
        return refuse(-402, who, m);
    }
    if (T < 1 || T > 65535) {
        snprintf(m, sizeof m, "T = %d: 1 .. 65535 frames per call", T);
        return refuse(-403, who, m);
    }
    if (H < 1 || W < 1 || H > 32768 || W > 32768) {
        snprintf(m, sizeof m, "H = %d, W = %d: every side is 1 .. 32768", H, W);
        return refuse(-404, who, m);
    }
    if (s < 1 || s > AA_MAX_S) {
        snprintf(m, sizeof m, "s = %d: the integer 1 / scale, 1 .. %d", s, AA_MAX_S);
        return refuse(-405, who, m);
    }
    if (in_kind == 0 && (chan_stride < (long)H * W || frame_stride < (long)H * W)) {
        snprintf(m, sizeof m, "frame_stride = %ld, chan_stride = %ld floats: a plane holds %ld", frame_stride, chan_stride, (long)H * W);
        return refuse(-406, who, m);
    }
    if (in_kind == 1 && frame_stride < (long)H * W * 3) {
        snprintf(m, sizeof m, "frame_stride = %ld bytes: a frame holds %ld", frame_stride, (long)H * W * 3);
        return refuse(-406, who, m);
    }
    if (c_pad < 3 || ld_out < c_pad) {
        snprintf(m, sizeof m, "c_pad = %d, ld_out = %d: 3 <= c_pad <= ld_out", c_pad, ld_out);
        return refuse(-407, who, m);
    }
    const int K = 4 * (s - 1) + 1;
    AaTaps taps;
    const double sigma = 0.5 * (double)(s - 1), mean = 0.5 * (double)(K - 1);
    for (int i = 0; i < AA_MAX_K; ++i) taps.g[i] = i < K ? (float)exp(-((double)i - mean) * ((double)i - mean) / (2.0 * sigma * sigma)) : 0.f;
    if (s == 1) taps.g[0] = 1.f;                                 // scale 1: the reference returns its input (UTIL:257-258); here the layout change alone
    // The reference divides by torch.sum of the K x K fp32 products, which is blocked and good to ~4e-8; a running fp32 sum of the 841
    // products of s = 8 is not (-2.8e-6, and 6.5e-7 at s = 4: a scale error on every output), so the products are summed in double.
    double sum = 0.0;
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) sum += (double)(taps.g[i] * taps.g[j]);
    taps.sum = (float)sum;
    const int ho = (H + s - 1) / s, wo = (W + s - 1) / s;
    const int tiles_x = dawn_cdiv(wo, AA_TILE), tiles_y = dawn_cdiv(ho, AA_TILE);
    const dim3 grid((unsigned)tiles_x * (unsigned)tiles_y, (unsigned)T);
    if (in_kind == 1)
        hipLaunchKernelGGL(antialias_down_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, frame_stride, chan_stride, H, W, s, K, taps, ho,
                           wo, tiles_x, out, ld_out, c_pad);
    else
        hipLaunchKernelGGL(antialias_down_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, frame_stride, chan_stride, H, W, s, K, taps, ho,
                           wo, tiles_x, out, ld_out, c_pad);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_region_moments(const float* x, int ld, int T, int h, int w, int R, double temperature, float* shift, float* covar,
                                   float* affine, void* stream) {
    const char* who = "dawn_region_moments";
    char m[200];
    if (!x) return refuse(-411, who, "x is NULL");
    if (!shift) return refuse(-411, who, "shift is NULL");
    if (!covar) return refuse(-411, who, "covar is NULL");
    if (!affine) return refuse(-411, who, "affine is NULL");
    if (R < 1 || R > ME_MAX_R) {
        snprintf(m, sizeof m, "R = %d: 1 .. %d regions", R, ME_MAX_R);
        return refuse(-412, who, m);
    }
    if (ld < R) {
        snprintf(m, sizeof m, "ld = %d: a row holds R = %d values", ld, R);
        return refuse(-412, who, m);
    }
    if (T < 1 || (long)T * R > 0x7fffffffL) {
        snprintf(m, sizeof m, "T = %d: at least one frame, T * R below 2^31", T);
        return refuse(-413, who, m);
    }
    if (h < 2 || w < 2 || h > 4096 || w > 4096) {
        snprintf(m, sizeof m, "h = %d, w = %d: every side is 2 .. 4096 (the coordinate grid divides by side - 1)", h, w);
        return refuse(-414, who, m);
    }
    if (!(temperature > 0.0)) {
        snprintf(m, sizeof m, "temperature = %g: positive", temperature);
        return refuse(-415, who, m);
    }
    hipLaunchKernelGGL(region_moments_kernel, dim3((unsigned)(T * R)), dim3(256), 0, (hipStream_t)stream, x, ld, h, w, R, temperature, shift, covar,
                       affine);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_bg_params(const float* x, int ld, int T, int npix, int C, const float* fc_w, const float* fc_b, float* out, void* stream) {
    const char* who = "dawn_bg_params";
    char m[200];
    if (!x) return refuse(-431, who, "x is NULL");
    if (!fc_w) return refuse(-431, who, "fc_w is NULL");
    if (!fc_b) return refuse(-431, who, "fc_b is NULL");
    if (!out) return refuse(-431, who, "out is NULL");
    if (T < 1) {
        snprintf(m, sizeof m, "T = %d: at least one frame", T);
        return refuse(-432, who, m);
    }
    if (npix < 1) {
        snprintf(m, sizeof m, "npix = %d: at least one pixel", npix);
        return refuse(-433, who, m);
    }
    if (C < 1 || ld < C) {
        snprintf(m, sizeof m, "C = %d, ld = %d: 1 <= C <= ld", C, ld);
        return refuse(-434, who, m);
    }
    hipLaunchKernelGGL(bg_params_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, x, ld, npix, C, fc_w, fc_b, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_motion_inputs(const float* drv_shift, const float* drv_covar, const float* drv_affine, const float* src_shift,
                                  const float* src_covar, const float* src_affine, const float* bg_params, int R, const float* src_rows,
                                  int ld_src, int T, int h, int w, float* out, int ld_out, int c_pad, void* stream) {
    const char* who = "dawn_motion_inputs";
    char m[200];
    CK(check_motion(who, drv_shift, drv_covar, drv_affine, src_shift, src_covar, src_affine, bg_params, R, T, h, w));
    if (!src_rows) return refuse(-421, who, "src_rows is NULL");
    if (!out) return refuse(-421, who, "out is NULL");
    if (ld_src < 3) {
        snprintf(m, sizeof m, "ld_src = %d: a source row holds 3 channels", ld_src);
        return refuse(-425, who, m);
    }
    if (c_pad < 4 * (R + 1) || c_pad > 64 || c_pad % 4 != 0 || ld_out < c_pad || ld_out % 4 != 0 || ((uintptr_t)out & 15) != 0) {
        snprintf(m, sizeof m, "c_pad = %d, ld_out = %d: 4 (R + 1) = %d <= c_pad <= 64, c_pad <= ld_out, both multiples of 4, out 16-byte aligned",
                 c_pad, ld_out, 4 * (R + 1));
        return refuse(-426, who, m);
    }
    const MotionParams a = {drv_shift, drv_covar, drv_affine, src_shift, src_covar, src_affine, bg_params, R};
    hipLaunchKernelGGL(motion_inputs_kernel, dim3((unsigned)dawn_cdiv((long)h * w, MI_PIX), (unsigned)T), dim3(256), 0, (hipStream_t)stream, a,
                       src_rows, ld_src, h, w, out, ld_out, c_pad);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_flow_combine(const float* x, int ld, const float* drv_shift, const float* drv_affine, const float* src_shift,
                                 const float* src_affine, const float* bg_params, int R, int T, int h, int w, float* grid, long grid_plane,
                                 float* conf, int conf_x0, void* stream) {
    const char* who = "dawn_flow_combine";
    char m[200];
    if (!x) return refuse(-421, who, "x is NULL");
    // no covariances here: the shifts stand in for them in the shared check, and the kernel never reads them (motion_prepare<false>)
    CK(check_motion(who, drv_shift, drv_shift, drv_affine, src_shift, src_shift, src_affine, bg_params, R, T, h, w));
    if (!grid) return refuse(-421, who, "grid is NULL");
    if (!conf) return refuse(-421, who, "conf is NULL");
    if (ld < R + 2) {
        snprintf(m, sizeof m, "ld = %d: a row holds the R + 1 masks and the occlusion channel, %d values", ld, R + 2);
        return refuse(-427, who, m);
    }
    if (grid_plane < (long)T * h * w) {
        snprintf(m, sizeof m, "grid_plane = %ld floats: the x plane of this call holds %ld", grid_plane, (long)T * h * w);
        return refuse(-428, who, m);
    }
    if (conf_x0 != 0 && conf_x0 != 1) {
        snprintf(m, sizeof m, "conf_x0 = %d: 0 (the occlusion map) or 1 (2 * map - 1, the diffusion's x0 plane)", conf_x0);
        return refuse(-429, who, m);
    }
    const MotionParams a = {drv_shift, nullptr, drv_affine, src_shift, nullptr, src_affine, bg_params, R};
    hipLaunchKernelGGL(flow_combine_kernel, dim3((unsigned)dawn_cdiv((long)h * w, 256), (unsigned)T), dim3(256), 0, (hipStream_t)stream, a, x, ld, h,
                       w, grid, grid_plane, conf, conf_x0);
    DAWN_LAUNCH_CHECK();
    return 0;
}
