// yuv420p ingest: dawn_yuv420_to_frames, the inverse of the yuv420p egress (flow_decode.hip) -- I420 frames as a video decoder or a
// .y4m file delivers them to the uint8 RGB frames that dawn_antialias_down reads (in_kind = 1).  include/dawn_hip.h states the
// arithmetic: BT.601 limited range in 8-bit fixed point, chroma replicated over its 2x2 block, clamp to 0 .. 255.
//
// Memory access.  A pure stream: 1.5 bytes in, 3 bytes out per pixel, nothing is read twice.  A work item owns a block of two rows,
// so that it loads a chroma sample once for the four pixels that share it, and consecutive work items own consecutive blocks of a row
// pair, so that the lanes of a wave read and write contiguous memory in every instruction.
//   wide path (W % 8 == 0; in, frame_stride, out multiples of 8): 2 x 8 pixels -- one 8-byte load per Y row, one 4-byte load of U and
//     of V, 24 output bytes per row as three 8-byte stores.  Every address is aligned by construction: a Y row starts at a multiple
//     of W, the chroma planes at H W and 5 H W / 4 (H W / 4 is a multiple of 4), a chroma row at a multiple of W / 2, an output row
//     at a multiple of 24.
//   narrow path (everything else): 2 x 4 pixels -- the same loads at half the width, assembled from bytes because neither W % 4 == 0 nor
//     the caller's frame_stride makes them aligned, 12 output bytes per row as three 4-byte stores (out is 4-byte aligned and an
//     output row starts at a multiple of 12).
// Not tuned: profiles/motion_stage.md has the measured time.
#include "dawn_common.h"

#include <stdio.h>

namespace {

constexpr int YUV_THREADS = 256;

// clamp8(v >> 8), written as the clamp of v to 0 .. 0xffff followed by the shift: the same value for every int (v < 0 gives 0, v > 0xffff
// gives 255, and in between v >> 8 is 0 .. 255 already).  The order matters to the compiler only: hipcc turns shift-then-clamp into
// v_ashr_pk_u8_i32, and on an MI355X that instruction was seen to return 255, not 0, for a negative input (the exhaustive test of
// tests/test_hip_motion_stage.py caught it: R = 255 where the definition gives 0).  This form compiles to v_med3_i32 and a shift.
__device__ __forceinline__ unsigned clamp8_shr8(int v) { return (unsigned)(v < 0 ? 0 : (v > 0xffff ? 0xffff : v)) >> 8; }

// the three bytes of one pixel, R in the low byte
__device__ __forceinline__ unsigned yuv_rgb(int y, int d, int e) {
    const int c = 298 * (y - 16) + 128;
    const unsigned r = clamp8_shr8(c + 409 * e);
    const unsigned g = clamp8_shr8(c - 100 * d - 208 * e);
    const unsigned b = clamp8_shr8(c + 516 * d);
    return r | g << 8 | b << 16;
}

// NPIX pixels of one row: y = their NPIX luma bytes (little-endian), u / v = the NPIX / 2 chroma bytes -> 3 NPIX / 4 words
template <int NPIX>
__device__ __forceinline__ void yuv_row(unsigned long long y, unsigned u, unsigned v, unsigned (&out)[3 * NPIX / 4]) {
#pragma unroll
    for (int q = 0; q < NPIX / 4; ++q) {                      // four pixels -> three words
        unsigned p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = 4 * q + k;
            p[k] = yuv_rgb((int)((y >> (8 * i)) & 0xff), (int)((u >> (8 * (i / 2))) & 0xff) - 128, (int)((v >> (8 * (i / 2))) & 0xff) - 128);
        }
        out[3 * q] = p[0] | p[1] << 24;
        out[3 * q + 1] = p[1] >> 8 | p[2] << 16;
        out[3 * q + 2] = p[2] >> 16 | p[3] << 8;
    }
}

template <typename T>
__device__ __forceinline__ T load_unaligned(const unsigned char* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

// one work item per 2 x 8 block; blocks = T * (H / 2) * (W / 8)
__global__ __launch_bounds__(YUV_THREADS) void yuv420_to_frames_wide_kernel(const unsigned char* __restrict__ in, long frame_stride, long blocks,
                                                                            int H, int W, unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * YUV_THREADS + threadIdx.x;
    if (i >= blocks) return;
    const int bw = W >> 3, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long t = r / bh;
    const long HW = (long)H * W;
    const unsigned char* f = in + t * frame_stride;
    const unsigned char* yp = f + (long)(2 * by) * W + 8 * bx;
    const long coff = (long)by * (W >> 1) + 4 * bx;
    const unsigned u = *(const unsigned*)(f + HW + coff);
    const unsigned v = *(const unsigned*)(f + HW + (HW >> 2) + coff);
    unsigned char* op = out + (t * HW + (long)(2 * by) * W + 8 * bx) * 3;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        unsigned w[6];
        yuv_row<8>(*(const unsigned long long*)(yp + (long)row * W), u, v, w);
        uint2* o = (uint2*)(op + (long)row * W * 3);
        o[0] = uint2{w[0], w[1]};
        o[1] = uint2{w[2], w[3]};
        o[2] = uint2{w[4], w[5]};
    }
}

// one work item per 2 x 4 block; blocks = T * (H / 2) * (W / 4); no alignment assumed of the input
__global__ __launch_bounds__(YUV_THREADS) void yuv420_to_frames_narrow_kernel(const unsigned char* __restrict__ in, long frame_stride, long blocks,
                                                                              int H, int W, unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * YUV_THREADS + threadIdx.x;
    if (i >= blocks) return;
    const int bw = W >> 2, bh = H >> 1;
    const int bx = (int)(i % bw);
    const long r = i / bw;
    const int by = (int)(r % bh);
    const long t = r / bh;
    const long HW = (long)H * W;
    const unsigned char* f = in + t * frame_stride;
    const unsigned char* yp = f + (long)(2 * by) * W + 4 * bx;
    const long coff = (long)by * (W >> 1) + 2 * bx;
    const unsigned u = load_unaligned<unsigned short>(f + HW + coff);
    const unsigned v = load_unaligned<unsigned short>(f + HW + (HW >> 2) + coff);
    unsigned char* op = out + (t * HW + (long)(2 * by) * W + 4 * bx) * 3;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        unsigned w[3];
        yuv_row<4>(load_unaligned<unsigned>(yp + (long)row * W), u, v, w);
        unsigned* o = (unsigned*)(op + (long)row * W * 3);
        o[0] = w[0];
        o[1] = w[1];
        o[2] = w[2];
    }
}

}  // namespace

extern "C" int dawn_yuv420_to_frames(const unsigned char* in, long frame_stride, int T, int H, int W, unsigned char* out, void* stream) {
    char m[240];
    if (!in || !out) {
        snprintf(m, sizeof m, "dawn_yuv420_to_frames: %s is NULL", !in ? "in" : "out");
        return dawn_set_error_msg(-380, m);
    }
    if (T < 1) {
        snprintf(m, sizeof m, "dawn_yuv420_to_frames: T = %d frames, at least 1 needed", T);
        return dawn_set_error_msg(-381, m);
    }
    if (H < 2 || H % 2 != 0 || H > 65536) {
        snprintf(m, sizeof m, "dawn_yuv420_to_frames: H = %d must be even, 2 .. 65536 (a chroma sample covers two rows)", H);
        return dawn_set_error_msg(-381, m);
    }
    if (W < 4 || W % 4 != 0 || W > 65536) {
        snprintf(m, sizeof m, "dawn_yuv420_to_frames: W = %d must be a multiple of 4, 4 .. 65536 (output rows leave as 4-byte stores)", W);
        return dawn_set_error_msg(-381, m);
    }
    const long HW = (long)H * W;
    if (frame_stride < HW / 2 * 3) {
        snprintf(m, sizeof m, "dawn_yuv420_to_frames: frame_stride = %ld bytes, an I420 frame of %d x %d has %ld", frame_stride, H, W, HW / 2 * 3);
        return dawn_set_error_msg(-382, m);
    }
    if (((uintptr_t)out & 3) != 0) return dawn_set_error_msg(-383, "dawn_yuv420_to_frames: out is not 4-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const bool wide = W % 8 == 0 && (((uintptr_t)in | (uintptr_t)out | (uintptr_t)frame_stride) & 7) == 0;
    const long blocks = (long)T * (H / 2) * (W / (wide ? 8 : 4));
    const long groups = (blocks + YUV_THREADS - 1) / YUV_THREADS;
    if (groups > 0x7fffffffL) {
        snprintf(m, sizeof m, "dawn_yuv420_to_frames: T = %d frames of %d x %d are more than one launch takes", T, H, W);
        return dawn_set_error_msg(-381, m);
    }
    if (wide)
        hipLaunchKernelGGL(yuv420_to_frames_wide_kernel, dim3((unsigned)groups), dim3(YUV_THREADS), 0, st, in, frame_stride, blocks, H, W, out);
    else
        hipLaunchKernelGGL(yuv420_to_frames_narrow_kernel, dim3((unsigned)groups), dim3(YUV_THREADS), 0, st, in, frame_stride, blocks, H, W, out);
    DAWN_LAUNCH_CHECK();
    return 0;
}
