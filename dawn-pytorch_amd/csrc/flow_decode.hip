// LFG flow decode: the non-GEMM pieces of Generator.forward_with_flow (GEN = LFG/modules/generator.py
// :138-171, blocks UTIL = LFG/modules/util.py:70-150), batched over the T frames of a clip instead of the reference's
// T sequential batch-1 calls (FD:372-385).  Activations are channels-last (rows = T*H*W, C), the layout of dawn_conv_gemm,
// which runs every 3x3 convolution of the decoder on the split-operand bf16 matrix pipe.  Everything here is HBM-bound
// elementwise / gather work except the final 7x7 C->3 convolution, whose 3-wide output has no use for MFMA tiles and runs
// on the vector ALUs from LDS (0.25 of the decoder's 15.7 TFLOP per 200-frame 256^2 clip).
//
// Warp semantics (GEN:62-90): flow (h,w) and occlusion (h,w) live at the latent resolution; a skip tensor at (Hs,Ws) is
// sampled with F.interpolate(flow, bilinear, align_corners=False) -> F.grid_sample(skip, bilinear, zeros,
// align_corners=False), the occlusion map is bilinearly resized the same way, and
//     out = warp(skip) * occ + prev * (1 - occ)          (prev absent: out = warp(skip) * occ).
// The source of every warp (source image, encoder skips) is ONE frame per clip: it stays L2/MALL-resident while the T
// frames stream through.
#include "dawn_common.h"
#include "../../include/dawn_hip.h"

#include <stdio.h>

namespace {

// F.interpolate(mode='bilinear', align_corners=False) source index and weights for output index `dst`
// (ATen area_pixel_compute_source_index: src = scale*(dst+0.5)-0.5 clamped at 0; scale = in/out).
struct Lerp { int i0, i1; float l0, l1; };
__device__ __forceinline__ Lerp lerp_index(int dst, int in_size, float scale) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    Lerp r;
    r.i0 = (int)src;
    if (r.i0 > in_size - 1) r.i0 = in_size - 1;
    r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.0f - r.l1;
    return r;
}

// bilinear sample of a (h,w) plane at output pixel (Y,X) of an (Hs,Ws) grid; identity when the sizes match
__device__ __forceinline__ float plane_at(const float* __restrict__ p, int w, const Lerp& ly, const Lerp& lx) {
    const float v00 = p[ly.i0 * w + lx.i0], v01 = p[ly.i0 * w + lx.i1];
    const float v10 = p[ly.i1 * w + lx.i0], v11 = p[ly.i1 * w + lx.i1];
    return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}

// grid_sample(bilinear, zeros, align_corners=False) corner set for one output pixel: pixel indices (-1 = outside,
// contributes 0) and weights, in ATen's nw, ne, sw, se order.
struct Corners { int i[4]; float w[4]; };
__device__ __forceinline__ Corners corners_at(float gx, float gy, int Hs, int Ws) {
    float ix = ((gx + 1.0f) * (float)Ws - 1.0f) * 0.5f;
    float iy = ((gy + 1.0f) * (float)Hs - 1.0f) * 0.5f;
    // far-outside coordinates: every corner is outside anyway; clamp so the int conversion is defined
    ix = fminf(fmaxf(ix, -2.0f), (float)Ws + 1.0f);
    iy = fminf(fmaxf(iy, -2.0f), (float)Hs + 1.0f);
    const float fx0 = floorf(ix), fy0 = floorf(iy);
    const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
    const float ex = ix - fx0, ey = iy - fy0;            // == ix - x_nw ; (x_se - ix) == 1 - ex exactly as ATen computes it
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

// flow / occlusion of frame t at output pixel (Y,X): grid planes gxp, gyp (h*w each), conf plane
__device__ __forceinline__ void motion_at(const float* __restrict__ gxp, const float* __restrict__ gyp,
                                          const float* __restrict__ cfp, int h, int w, int Hs, int Ws, int Y, int X,
                                          float& gx, float& gy, float& oc) {
    if (Hs == h && Ws == w) {
        gx = gxp[Y * w + X]; gy = gyp[Y * w + X]; oc = cfp[Y * w + X];
        return;
    }
    const Lerp ly = lerp_index(Y, h, (float)h / (float)Hs), lx = lerp_index(X, w, (float)w / (float)Ws);
    gx = plane_at(gxp, w, ly, lx);
    gy = plane_at(gyp, w, ly, lx);
    oc = plane_at(cfp, w, ly, lx);
}

// ---- eval-mode BatchNorm (+ReLU) as a per-channel affine: out = act(x*a[c] + b[c])          UTIL:83-88, 108-109
__global__ __launch_bounds__(256) void affine_act_kernel(const float* __restrict__ x, int ld, const float* __restrict__ a,
                                                         const float* __restrict__ b, int act, float* __restrict__ out,
                                                         long rows, int C) {
    const int q = C >> 2;
    const long total = rows * q;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / q;
        const int c = (int)(i - row * q) * 4;
        f32x4 v = *reinterpret_cast<const f32x4*>(x + row * ld + c);
        v = v * *reinterpret_cast<const f32x4*>(a + c) + *reinterpret_cast<const f32x4*>(b + c);
        if (act == 1) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        *reinterpret_cast<f32x4*>(out + row * C + c) = v;
    }
}

// ---- DownBlock2d tail: out (F,H/2,W/2,C) = AvgPool2x2(ReLU(x*a+b))                         UTIL:129-133
__global__ __launch_bounds__(256) void bn_relu_pool2_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                            const float* __restrict__ b, float* __restrict__ out, int F,
                                                            int H, int W, int C) {
    const int q = C >> 2, Ho = H >> 1, Wo = W >> 1;
    const long total = (long)F * Ho * Wo * q;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long pix = i / q;
        const int c = (int)(i - pix * q) * 4;
        const int xo = (int)(pix % Wo);
        const long r = pix / Wo;
        const int yo = (int)(r % Ho);
        const long f = r / Ho;
        const f32x4 av = *reinterpret_cast<const f32x4*>(a + c), bv = *reinterpret_cast<const f32x4*>(b + c);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                f32x4 v = *reinterpret_cast<const f32x4*>(x + ((f * H + 2 * yo + dy) * W + 2 * xo + dx) * C + c) * av + bv;
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                s += v;
            }
        *reinterpret_cast<f32x4*>(out + pix * C + c) = s * 0.25f;
    }
}

// ---- apply_optical (GEN:71-90) on a channels-last skip: one thread = one output pixel x 4 channels.
// prev (optional) is the running decoder activation; prev_a/prev_b (optional) apply the UpBlock2d's BatchNorm + ReLU
// to it on the fly (UTIL:108-109), so that conv output never takes a separate normalisation pass.  up2 = also apply
// the NEXT UpBlock2d's nearest x2 upsampling (UTIL:106) by writing each result to its 2x2 output pixels.
__global__ __launch_bounds__(256) void warp_blend_kernel(const float* __restrict__ skip, int Hs, int Ws, int C,
                                                         const float* __restrict__ grid, long grid_plane,
                                                         const float* __restrict__ conf, int T, int h, int w,
                                                         const float* __restrict__ prev, const float* __restrict__ prev_a,
                                                         const float* __restrict__ prev_b, int up2,
                                                         float* __restrict__ out) {
    const int q = C >> 2;
    const long total = (long)T * Hs * Ws * q;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long pix = i / q;
        const int c = (int)(i - pix * q) * 4;
        const int X = (int)(pix % Ws);
        const long r = pix / Ws;
        const int Y = (int)(r % Hs);
        const int t = (int)(r / Hs);
        float gx, gy, oc;
        motion_at(grid + (long)t * h * w, grid + grid_plane + (long)t * h * w, conf + (long)t * h * w, h, w, Hs, Ws, Y, X, gx,
                  gy, oc);
        const Corners cr = corners_at(gx, gy, Hs, Ws);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cr.i[k] >= 0) v += *reinterpret_cast<const f32x4*>(skip + (long)cr.i[k] * C + c) * cr.w[k];
        v = v * oc;
        if (prev) {
            f32x4 p = *reinterpret_cast<const f32x4*>(prev + pix * C + c);
            if (prev_a) {
                p = p * *reinterpret_cast<const f32x4*>(prev_a + c) + *reinterpret_cast<const f32x4*>(prev_b + c);
                p.x = fmaxf(p.x, 0.f); p.y = fmaxf(p.y, 0.f); p.z = fmaxf(p.z, 0.f); p.w = fmaxf(p.w, 0.f);
            }
            v += p * (1.0f - oc);
        }
        if (!up2) {
            *reinterpret_cast<f32x4*>(out + pix * C + c) = v;
        } else {
            float* o = out + (((long)t * 2 * Hs + 2 * Y) * (2 * Ws) + 2 * X) * C + c;
            *reinterpret_cast<f32x4*>(o) = v;
            *reinterpret_cast<f32x4*>(o + C) = v;
            *reinterpret_cast<f32x4*>(o + (long)2 * Ws * C) = v;
            *reinterpret_cast<f32x4*>(o + (long)2 * Ws * C + C) = v;
        }
    }
}

// u8_of: one value of the frame egress (see frames_to_u8_kernel below for the arithmetic it restates)
__device__ __forceinline__ unsigned u8_of(float x, double m) {
    float v = (float)((double)x + m);
    v = fminf(fmaxf(v, 0.0f), 1.0f);
    return (unsigned)(v * 255.0f);
}

// ---- yuv420p egress: BT.601 limited range in 8-bit fixed point, on the RGB bytes u8_of defines (>> = arithmetic shift):
//   Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 per pixel;  R', G', B' = (sum of the 2x2 block + 2) >> 2 (centre-sited box);
//   U = ((-38 R' - 74 G' + 112 B' + 128) >> 8) + 128;  V = ((112 R' - 94 G' - 18 B' + 128) >> 8) + 128.
// Y stays in [16,235], U and V in [16,240] for every input: no clamp.  I420: per frame Y (H*W), U (H/2 * W/2), V (the same).
__device__ __forceinline__ unsigned yuv_y(unsigned R, unsigned G, unsigned B) { return ((66u * R + 129u * G + 25u * B + 128u) >> 8) + 16u; }
__device__ __forceinline__ unsigned yuv_u(int R, int G, int B) { return (unsigned)(((-38 * R - 74 * G + 112 * B + 128) >> 8) + 128); }
__device__ __forceinline__ unsigned yuv_v(int R, int G, int B) { return (unsigned)(((112 * R - 94 * G - 18 * B + 128) >> 8) + 128); }

// four RGB pixels packed as 12 bytes in three words -> byte k
__device__ __forceinline__ unsigned rgb12_byte(const unsigned (&q)[3], int k) { return (q[k >> 2] >> (8 * (k & 3))) & 255u; }
// the four Y bytes of such a group as one word
__device__ __forceinline__ unsigned yuv_y4(const unsigned (&q)[3]) {
    unsigned y = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) y |= yuv_y(rgb12_byte(q, 3 * p), rgb12_byte(q, 3 * p + 1), rgb12_byte(q, 3 * p + 2)) << (8 * p);
    return y;
}
// two rows of such groups = two 2x2 blocks: their U bytes (low half) and V bytes (high half)
__device__ __forceinline__ unsigned yuv_uv2(const unsigned (&a)[3], const unsigned (&b)[3]) {
    unsigned uv = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        int c[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            c[ch] = (int)(rgb12_byte(a, 6 * j + ch) + rgb12_byte(a, 6 * j + 3 + ch) + rgb12_byte(b, 6 * j + ch) +
                          rgb12_byte(b, 6 * j + 3 + ch) + 2u) >> 2;
        uv |= (yuv_u(c[0], c[1], c[2]) << (8 * j)) | (yuv_v(c[0], c[1], c[2]) << (16 + 8 * j));
    }
    return uv;
}

// ---- final 7x7 conv C->3 + bias, sigmoid, and the last apply_optical against the source image (GEN:163-167), plus the
// `deformed` output (GEN:152).  Tile = 32 x 16 output pixels of one frame, 256 threads, 2 pixels per thread (rows y and
// y+8).  The input streams through LDS 8 channels at a time as a zero-padded (16+6) x (32+6) patch laid out
// [channel quad][pixel][4] (consecutive lanes -> consecutive 16-byte slots: conflict-free b128 reads); the weights
// [tap][channel quad][3 outputs][4 channels] stay in LDS for the whole block and are read as wave-uniform broadcasts.
//
// The kernel is a template over where the result goes; everything up to the blended value is the same source in both forms:
//   FcOutF32  out_vid / warped_vid planar fp32 (dawn_final_conv_blend);
//   FcOutU8   the frame egress of dawn_frames_to_u8 applied to the value out_vid would have received, written as (T,H,W,3)
//             bytes (dawn_final_conv_blend_u8): no fp32 frame goes to memory.  A 32 x 16 tile is 16 rows of 96 contiguous
//             bytes: they are staged in the patch region of LDS (free once the last channel chunk is consumed) and leave as
//             24 4-byte stores per row; tiles cut by the image edge store their bytes one by one.
//   FcOutYuv420  the same RGB bytes (RGB order) converted to I420 (dawn_final_conv_blend_yuv420; definition at yuv_y above): every
//             tile, edge-cut ones too, stages its bytes in that tile, and its valid part is converted from LDS.  Even H and W % 4 == 0
//             with a tile origin at multiples of (16,32) make the valid part whole groups of 4 pixels x 2 rows: no chroma block
//             straddles a tile or the image edge, Y leaves as 4-byte words (8 per tile row) and U, V as 2-byte pairs (the chroma
//             planes and their rows are 2-byte aligned, no more, when W % 8 != 0).
constexpr int FC_TW = 32, FC_TH = 16, FC_PW = FC_TW + 6, FC_PH = FC_TH + 6, FC_PP = FC_PW * FC_PH;

// The last blend as the fp32 kernel has always evaluated it: two rounded products and a rounded sum.  Spelled out because the
// compiler's choice between that and a fused multiply-add depends on what consumes the value (it fused in the byte form), and
// the two forms must produce the same fp32 value bit for bit.
__device__ __forceinline__ float fc_blend(float wv, float oc, float s) {
#pragma clang fp contract(off)
    return wv * oc + s * (1.0f - oc);
}

struct FcOutF32 { float* out_vid; float* warped_vid; long out_plane; };
struct FcOutU8 { unsigned char* frames; double m0, m1, m2; int bgr; };
struct FcOutYuv420 { unsigned char* frames; double m0, m1, m2; };

template <class Out>
__global__ __launch_bounds__(256) void final_conv_blend_kernel(const float* __restrict__ x, int T, int H, int W, int C,
                                                               const float* __restrict__ w7, const float* __restrict__ bias3,
                                                               const float* __restrict__ src, const float* __restrict__ grid,
                                                               long grid_plane, const float* __restrict__ conf, int h, int w,
                                                               const Out dst) {
    constexpr bool U8 = __is_same(Out, FcOutU8), YUV = __is_same(Out, FcOutYuv420), F32 = __is_same(Out, FcOutF32);
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* Ws_ = sm;                                   // [49][C/4][3][4]
    float* Ps = sm + 49 * C * 3;                       // [2][FC_PP][4]
    const int tid = threadIdx.x;
    const int tiles_x = (W + FC_TW - 1) / FC_TW, tiles_y = (H + FC_TH - 1) / FC_TH;
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y;
    const int t = b / tiles_y;
    const int X0 = tx * FC_TW, Y0 = ty * FC_TH;
    for (int i = tid; i < 49 * C * 3; i += 256) Ws_[i] = w7[i];
    const int lx = tid & 31, ly = tid >> 5;            // pixels (Y0+ly, X0+lx) and (Y0+ly+8, X0+lx)
    float acc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
    const int nq = C >> 2;
    for (int c0 = 0; c0 < C; c0 += 8) {
        __syncthreads();                               // previous chunk consumed (first pass: weights visible below)
        for (int i = tid; i < 2 * FC_PP; i += 256) {
            const int qd = i / FC_PP, p = i - qd * FC_PP;
            const int py = p / FC_PW, px = p - py * FC_PW;
            const int y = Y0 + py - 3, xx = X0 + px - 3;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (y >= 0 && y < H && xx >= 0 && xx < W)
                v = *reinterpret_cast<const f32x4*>(x + (((long)t * H + y) * W + xx) * C + c0 + 4 * qd);
            *reinterpret_cast<f32x4*>(Ps + (size_t)i * 4) = v;
        }
        __syncthreads();
        const int q0 = c0 >> 2;
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const int tap = ky * 7 + kx;
#pragma unroll
                for (int qd = 0; qd < 2; ++qd) {
                    const float* wp = Ws_ + ((size_t)(tap * nq + q0 + qd) * 3) * 4;
                    const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4),
                                w2 = *reinterpret_cast<const f32x4*>(wp + 8);
#pragma unroll
                    for (int pI = 0; pI < 2; ++pI) {
                        const f32x4 v = *reinterpret_cast<const f32x4*>(
                            Ps + ((size_t)qd * FC_PP + (ly + 8 * pI + ky) * FC_PW + lx + kx) * 4);
                        acc[pI][0] += v.x * w0.x + v.y * w0.y + v.z * w0.z + v.w * w0.w;
                        acc[pI][1] += v.x * w1.x + v.y * w1.y + v.z * w1.z + v.w * w1.w;
                        acc[pI][2] += v.x * w2.x + v.y * w2.y + v.z * w2.z + v.w * w2.w;
                    }
                }
            }
        }
    }
    const float* gxp = grid + (long)t * h * w;
    const float* gyp = gxp + grid_plane;
    const float* cfp = conf + (long)t * h * w;
    unsigned char* tile = reinterpret_cast<unsigned char*>(Ps);      // U8, YUV: [FC_TH][FC_TW * 3] bytes
    const bool full = X0 + FC_TW <= W && Y0 + FC_TH <= H;
    if constexpr (U8 || YUV) __syncthreads();          // last chunk consumed: the patch region becomes the byte tile
#pragma unroll
    for (int pI = 0; pI < 2; ++pI) {
        const int Y = Y0 + ly + 8 * pI, X = X0 + lx;
        if (Y >= H || X >= W) continue;
        float gx, gy, oc;
        motion_at(gxp, gyp, cfp, h, w, H, W, Y, X, gx, gy, oc);
        const Corners cr = corners_at(gx, gy, H, W);
        const long o = ((long)t * H + Y) * W + X;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float wv = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cr.i[k] >= 0) wv += src[(long)ch * H * W + cr.i[k]] * cr.w[k];
            const float s = 1.0f / (1.0f + expf(-(acc[pI][ch] + bias3[ch])));
            const float v = fc_blend(wv, oc, s);
            if constexpr (F32) {
                dst.warped_vid[ch * dst.out_plane + o] = wv;
                dst.out_vid[ch * dst.out_plane + o] = v;
            } else if constexpr (YUV) {
                tile[(ly + 8 * pI) * (FC_TW * 3) + lx * 3 + ch] =
                    (unsigned char)u8_of(v, ch == 0 ? dst.m0 : (ch == 1 ? dst.m1 : dst.m2));
            } else {
                const unsigned char u = (unsigned char)u8_of(v, ch == 0 ? dst.m0 : (ch == 1 ? dst.m1 : dst.m2));
                const int k = dst.bgr ? 2 - ch : ch;
                if (full) tile[(ly + 8 * pI) * (FC_TW * 3) + lx * 3 + k] = u;
                else dst.frames[o * 3 + k] = u;
            }
        }
    }
    if constexpr (U8) {
        __syncthreads();
        if (full) {
            const unsigned* tw = reinterpret_cast<const unsigned*>(tile);
            constexpr int RW = FC_TW * 3 / 4;          // 24 words per tile row
            for (int i = tid; i < FC_TH * RW; i += 256) {
                const int r = i / RW, c = i - r * RW;
                reinterpret_cast<unsigned*>(dst.frames + (((long)t * H + Y0 + r) * W + X0) * 3)[c] = tw[i];
            }
        }
    }
    if constexpr (YUV) {
        __syncthreads();
        const unsigned* tw = reinterpret_cast<const unsigned*>(tile);
        constexpr int RW = FC_TW * 3 / 4, GW = FC_TW / 4;           // 24 words, 8 groups of 4 pixels per tile row
        const int vg = ((W - X0 < FC_TW ? W - X0 : FC_TW)) >> 2;    // valid groups per row, valid rows
        const int vr = H - Y0 < FC_TH ? H - Y0 : FC_TH;
        unsigned char* fr = dst.frames + (long)t * ((long)H * W / 2 * 3);
        if (tid < FC_TH * GW) {                                     // waves 0-1: Y, one word per thread
            const int r = tid / GW, c = tid - r * GW;
            if (r < vr && c < vg) {
                const unsigned q[3] = {tw[r * RW + 3 * c], tw[r * RW + 3 * c + 1], tw[r * RW + 3 * c + 2]};
                reinterpret_cast<unsigned*>(fr + (long)(Y0 + r) * W + X0)[c] = yuv_y4(q);
            }
        } else if (tid < FC_TH * GW + FC_TH / 2 * GW) {             // wave 2: chroma, two 2x2 blocks per thread
            const int j = tid - FC_TH * GW, r = j / GW, c = j - r * GW;
            if (2 * r < vr && c < vg) {
                const unsigned* p = tw + 2 * r * RW + 3 * c;
                const unsigned a[3] = {p[0], p[1], p[2]}, b[3] = {p[RW], p[RW + 1], p[RW + 2]};
                const unsigned uv = yuv_uv2(a, b);
                const long HW = (long)H * W;
                const long co = (long)((Y0 >> 1) + r) * (W >> 1) + (X0 >> 1) + 2 * c;
                *reinterpret_cast<unsigned short*>(fr + HW + co) = (unsigned short)(uv & 0xffffu);
                *reinterpret_cast<unsigned short*>(fr + HW + (HW >> 2) + co) = (unsigned short)(uv >> 16);
            }
        }
    }
}

// ---- frame egress (UVG:383-397, 533-548 `_process_output_frame`): the decoded clip (3,T,H,W) fp32 in
// [0,1] -> (T,H,W,3) uint8, RGB or BGR (cv2.VideoWriter / cv2.imwrite order), with numpy's exact arithmetic:
//   frame += mean/255 (float64 add, stored back as float32) ; clip(0,1) ; (frame*255) in float32 ; astype(uint8) = trunc.
// 4 pixels per thread: three 16-byte plane reads, three packed 4-byte stores; one D2H copy of T*H*W*3 bytes follows
// instead of the reference's T device->host copies of fp32 frames.
__global__ __launch_bounds__(256) void frames_to_u8_kernel(const float* __restrict__ vid, long plane, long npix4, double m0,
                                                           double m1, double m2, int bgr, unsigned* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < npix4; i += (long)gridDim.x * 256) {
        const f32x4 r = *reinterpret_cast<const f32x4*>(vid + 4 * i);
        const f32x4 g = *reinterpret_cast<const f32x4*>(vid + plane + 4 * i);
        const f32x4 b = *reinterpret_cast<const f32x4*>(vid + 2 * plane + 4 * i);
        unsigned c[12];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const unsigned R = u8_of(r[p], m0), G = u8_of(g[p], m1), B = u8_of(b[p], m2);
            c[3 * p] = bgr ? B : R; c[3 * p + 1] = G; c[3 * p + 2] = bgr ? R : B;
        }
#pragma unroll
        for (int w = 0; w < 3; ++w)
            out[3 * i + w] = c[4 * w] | (c[4 * w + 1] << 8) | (c[4 * w + 2] << 16) | (c[4 * w + 3] << 24);
    }
}

// ---- the same egress to I420 (definition at yuv_y above) for a clip that exists as fp32 planes: (3,T,H,W) -> (T, 3HW/2) bytes.
// A thread owns two rows x four columns: six 16-byte loads, two 4-byte Y stores, one 2-byte U and one 2-byte V store.
__global__ __launch_bounds__(256) void frames_to_yuv420_kernel(const float* __restrict__ vid, long plane, int T, int H, int W,
                                                               double m0, double m1, double m2, unsigned char* __restrict__ out) {
    const int gw = W >> 2, hh = H >> 1;
    const long total = (long)T * hh * gw, HW = (long)H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % gw);
        const long r2 = i / gw;
        const int by = (int)(r2 % hh);
        const long t = r2 / hh;
        const float* v0 = vid + (t * H + 2 * by) * W + 4 * c;
        unsigned q[2][3];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const f32x4 r = *reinterpret_cast<const f32x4*>(v0 + dy * W);
            const f32x4 g = *reinterpret_cast<const f32x4*>(v0 + dy * W + plane);
            const f32x4 b = *reinterpret_cast<const f32x4*>(v0 + dy * W + 2 * plane);
            unsigned k[12];
#pragma unroll
            for (int p = 0; p < 4; ++p) { k[3 * p] = u8_of(r[p], m0); k[3 * p + 1] = u8_of(g[p], m1); k[3 * p + 2] = u8_of(b[p], m2); }
#pragma unroll
            for (int w = 0; w < 3; ++w) q[dy][w] = k[4 * w] | (k[4 * w + 1] << 8) | (k[4 * w + 2] << 16) | (k[4 * w + 3] << 24);
        }
        unsigned char* fr = out + t * (HW / 2 * 3);
        reinterpret_cast<unsigned*>(fr + (long)(2 * by) * W)[c] = yuv_y4(q[0]);
        reinterpret_cast<unsigned*>(fr + (long)(2 * by + 1) * W)[c] = yuv_y4(q[1]);
        const unsigned uv = yuv_uv2(q[0], q[1]);
        const long co = (long)by * (W >> 1) + 2 * c;
        *reinterpret_cast<unsigned short*>(fr + HW + co) = (unsigned short)(uv & 0xffffu);
        *reinterpret_cast<unsigned short*>(fr + HW + (HW >> 2) + co) = (unsigned short)(uv >> 16);
    }
}

int grid_for(long total) {
    long g = (total + 255) / 256;
    return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

// the I420 outputs' argument rule: even H, W % 4 == 0 (every frame and Y row 4-byte aligned, chroma rows of even length) and a
// 4-byte aligned buffer
int bad_yuv420(const char* who, int H, int W, const void* out) {
    if (H > 0 && W > 0 && H % 2 == 0 && W % 4 == 0 && out && ((uintptr_t)out & 3) == 0) return 0;
    char msg[200];
    snprintf(msg, sizeof msg, "%s: yuv420p needs an even H, W %% 4 == 0 and a non-NULL 4-byte aligned output (H = %d, W = %d)", who, H, W);
    return dawn_set_error_msg(-84, msg);
}

}  // namespace

extern "C" int dawn_affine_act(const float* x, int ld, const float* a, const float* b, int act, float* out, long rows,
                               int C, void* stream) {
    if (C % 4 != 0 || ld % 4 != 0) return dawn_set_error_msg(-70, "dawn_affine_act: C and ld must be multiples of 4");
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(affine_act_kernel, dim3(grid_for(rows * (C / 4))), dim3(256), 0, (hipStream_t)stream, x, ld, a, b,
                       act, out, rows, C);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_bn_relu_pool2(const float* x, const float* a, const float* b, float* out, int F, int H, int W, int C,
                                  void* stream) {
    if (C % 4 != 0 || (H & 1) || (W & 1)) return dawn_set_error_msg(-71, "dawn_bn_relu_pool2: C % 4, even H and W");
    hipLaunchKernelGGL(bn_relu_pool2_kernel, dim3(grid_for((long)F * (H / 2) * (W / 2) * (C / 4))), dim3(256), 0,
                       (hipStream_t)stream, x, a, b, out, F, H, W, C);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_warp_blend(const float* skip, int Hs, int Ws, int C, const float* grid, long grid_plane,
                               const float* conf, int T, int h, int w, const float* prev, const float* prev_a,
                               const float* prev_b, int up2, float* out, void* stream) {
    if (C % 4 != 0) return dawn_set_error_msg(-72, "dawn_warp_blend: C must be a multiple of 4");
    if ((prev_a == nullptr) != (prev_b == nullptr) || (prev_a && !prev))
        return dawn_set_error_msg(-73, "dawn_warp_blend: prev_a/prev_b come as a pair and need prev");
    if (T <= 0) return 0;
    hipLaunchKernelGGL(warp_blend_kernel, dim3(grid_for((long)T * Hs * Ws * (C / 4))), dim3(256), 0, (hipStream_t)stream,
                       skip, Hs, Ws, C, grid, grid_plane, conf, T, h, w, prev, prev_a, prev_b, up2, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}

namespace {
template <class Out>
int launch_final_conv(const char* who, const float* x, int T, int H, int W, int C, const float* w7, const float* bias3,
                      const float* src, const float* grid, long grid_plane, const float* conf, int h, int w, const Out& dst,
                      void* stream) {
    char msg[160];
    if (C % 8 != 0) {
        snprintf(msg, sizeof msg, "%s: C must be a multiple of 8", who);
        return dawn_set_error_msg(-74, msg);
    }
    const size_t lds = ((size_t)49 * C * 3 + (size_t)2 * FC_PP * 4) * sizeof(float);
    if (lds > 160 * 1024) {
        snprintf(msg, sizeof msg, "%s: C too large for the LDS-resident weights", who);
        return dawn_set_error_msg(-75, msg);
    }
    if (T <= 0) return 0;
    const long nblk = (long)T * ((H + FC_TH - 1) / FC_TH) * ((W + FC_TW - 1) / FC_TW);
    if (nblk > 0x7fffffffL) {
        snprintf(msg, sizeof msg, "%s: too many tiles for one launch", who);
        return dawn_set_error_msg(-76, msg);
    }
    (void)hipFuncSetAttribute((const void*)final_conv_blend_kernel<Out>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(final_conv_blend_kernel<Out>, dim3((unsigned)nblk), dim3(256), lds, (hipStream_t)stream, x, T, H, W, C,
                       w7, bias3, src, grid, grid_plane, conf, h, w, dst);
    DAWN_LAUNCH_CHECK();
    return 0;
}
}  // namespace

extern "C" int dawn_final_conv_blend(const float* x, int T, int H, int W, int C, const float* w7, const float* bias3,
                                     const float* src, const float* grid, long grid_plane, const float* conf, int h, int w,
                                     float* out_vid, float* warped_vid, long out_plane, void* stream) {
    return launch_final_conv("dawn_final_conv_blend", x, T, H, W, C, w7, bias3, src, grid, grid_plane, conf, h, w,
                             FcOutF32{out_vid, warped_vid, out_plane}, stream);
}

extern "C" int dawn_final_conv_blend_u8(const float* x, int T, int H, int W, int C, const float* w7, const float* bias3,
                                        const float* src, const float* grid, long grid_plane, const float* conf, int h, int w,
                                        double mean0, double mean1, double mean2, int bgr, unsigned char* frames,
                                        void* stream) {
    if (W % 4 != 0 || ((uintptr_t)frames & 3) != 0)
        return dawn_set_error_msg(-78, "dawn_final_conv_blend_u8: W must be a multiple of 4 and frames 4-byte aligned");
    return launch_final_conv("dawn_final_conv_blend_u8", x, T, H, W, C, w7, bias3, src, grid, grid_plane, conf, h, w,
                             FcOutU8{frames, mean0, mean1, mean2, bgr}, stream);
}

extern "C" int dawn_final_conv_blend_yuv420(const float* x, int T, int H, int W, int C, const float* w7, const float* bias3,
                                            const float* src, const float* grid, long grid_plane, const float* conf, int h, int w,
                                            double mean0, double mean1, double mean2, unsigned char* frames, void* stream) {
    if (const int rc = bad_yuv420("dawn_final_conv_blend_yuv420", H, W, frames)) return rc;
    return launch_final_conv("dawn_final_conv_blend_yuv420", x, T, H, W, C, w7, bias3, src, grid, grid_plane, conf, h, w,
                             FcOutYuv420{frames, mean0, mean1, mean2}, stream);
}

extern "C" int dawn_frames_to_yuv420(const float* vid, long plane, int T, int H, int W, double mean0, double mean1, double mean2,
                                     unsigned char* out, void* stream) {
    if (const int rc = bad_yuv420("dawn_frames_to_yuv420", H, W, out)) return rc;
    if (!vid || plane % 4 != 0 || ((uintptr_t)vid & 15) != 0)
        return dawn_set_error_msg(-85, "dawn_frames_to_yuv420: vid must be non-NULL and 16-byte aligned, the plane stride a multiple of 4");
    if (T <= 0) return 0;
    hipLaunchKernelGGL(frames_to_yuv420_kernel, dim3(grid_for((long)T * (H / 2) * (W / 4))), dim3(256), 0, (hipStream_t)stream, vid,
                       plane, T, H, W, mean0, mean1, mean2, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}

extern "C" int dawn_frames_to_u8(const float* vid, long plane, long npix, double mean0, double mean1, double mean2, int bgr,
                                 unsigned char* out, void* stream) {
    if (npix % 4 != 0 || plane % 4 != 0)
        return dawn_set_error_msg(-77, "dawn_frames_to_u8: pixel count and plane stride must be multiples of 4");
    if (npix <= 0) return 0;
    hipLaunchKernelGGL(frames_to_u8_kernel, dim3(grid_for(npix / 4)), dim3(256), 0, (hipStream_t)stream, vid, plane, npix / 4,
                       mean0, mean1, mean2, bgr, reinterpret_cast<unsigned*>(out));
    DAWN_LAUNCH_CHECK();
    return 0;
}
