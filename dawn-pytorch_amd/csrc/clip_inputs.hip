// The clip inputs of FlowDiffusion.sample_one_video (FD:327-350) that are neither a stage's output nor the denoiser's: the 16
// face-location channels of fea272 (bbox mask FD:182-201 through Face_loc_Encoder FD:39-50) and the condition rows (FD:332-350).
// Once per clip, plain fp32 VALU work: no matrix pipe, no atomics, a fixed summation order (bit-identical run to run).
#include "clip_inputs.h"

#include <math.h>

namespace {

// ---- dawn_face_loc_embed: mask -> conv1 (1 -> 8, 3x3 / s2 / p1) + ReLU -> conv2 (8 -> 16, 3x3 / s2 / p1) + ReLU in one launch.
// A workgroup owns a 16 x 16 tile of conv2 outputs; the conv1 values it reads are rows / columns 2 o0 - 1 .. 2 (o0 + 15) + 1 of the
// (size / 2)^2 conv1 image: a 33 x 33 tile per channel, computed from the analytic mask into LDS.  Positions outside the conv1 image
// are conv2's padding: ZERO, not relu(b1).
constexpr int FL_T = 16;                    // conv2 outputs per tile side
constexpr int FL_H = 2 * FL_T + 1;          // conv1 values per tile side
constexpr int FL_C1 = 8, FL_C2 = 16;

struct MaskBounds { int lt_x, lt_y, rb_x, rb_y; };

__global__ __launch_bounds__(256) void face_loc_embed_kernel(MaskBounds mb, int size, const float* __restrict__ w1,
                                                             const float* __restrict__ b1, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, float* __restrict__ out, long plane) {
    __shared__ float h1[FL_C1][FL_H][FL_H];
    __shared__ __attribute__((aligned(16))) float w2t[FL_C1 * 9][FL_C2];      // [c * 9 + ky * 3 + kx][o]: 16 outputs of one tap side by side
    __shared__ float w1s[FL_C1][9], b1s[FL_C1], b2s[FL_C2];
    const int tid = threadIdx.x;
    const int s2 = size >> 1, s4 = size >> 2;
    const int ox0 = blockIdx.x * FL_T, oy0 = blockIdx.y * FL_T;
    for (int i = tid; i < FL_C2 * FL_C1 * 9; i += 256) {                      // w2 (16, 8, 3, 3) as the checkpoint holds it
        const int o = i / (FL_C1 * 9), k = i % (FL_C1 * 9);
        w2t[k][o] = w2[i];
    }
    if (tid < FL_C1 * 9) w1s[tid / 9][tid % 9] = w1[tid];
    if (tid < FL_C1) b1s[tid] = b1[tid];
    if (tid < FL_C2) b2s[tid] = b2[tid];
    __syncthreads();
    // conv1 tile: one position per thread and pass, its nine mask values once, then the eight channels
    for (int i = tid; i < FL_H * FL_H; i += 256) {
        const int ly = i / FL_H, lx = i % FL_H;
        const int y = 2 * oy0 - 1 + ly, x = 2 * ox0 - 1 + lx;                 // conv1 coordinates
        const bool inside = y >= 0 && y < s2 && x >= 0 && x < s2;
        float m[9];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int r = 2 * y - 1 + ky, c = 2 * x - 1 + kx;             // mask pixel; outside the image: conv1's zero padding
                m[ky * 3 + kx] = (r >= 0 && r < size && c >= 0 && c < size && r >= mb.lt_y && r <= mb.rb_y && c >= mb.lt_x && c <= mb.rb_x)
                                     ? 1.0f : 0.0f;
            }
#pragma unroll
        for (int ch = 0; ch < FL_C1; ++ch) {
            float a = b1s[ch];
#pragma unroll
            for (int k = 0; k < 9; ++k) a = fmaf(w1s[ch][k], m[k], a);
            h1[ch][ly][lx] = inside ? fmaxf(a, 0.0f) : 0.0f;
        }
    }
    __syncthreads();
    const int tx = tid % FL_T, ty = tid / FL_T;
    const int ox = ox0 + tx, oy = oy0 + ty;
    if (ox >= s4 || oy >= s4) return;                                          // partial tiles (no barrier follows)
    float acc[FL_C2];
#pragma unroll
    for (int o = 0; o < FL_C2; ++o) acc[o] = b2s[o];
    for (int c = 0; c < FL_C1; ++c)                                            // fixed order: channel, ky, kx
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const float v = h1[c][2 * ty + ky][2 * tx + kx];
                const f32x4* wv = (const f32x4*)w2t[c * 9 + ky * 3 + kx];      // the same address in every lane: a broadcast read
#pragma unroll
                for (int q = 0; q < FL_C2 / 4; ++q) {
                    const f32x4 w = wv[q];
                    acc[4 * q + 0] = fmaf(w[0], v, acc[4 * q + 0]);
                    acc[4 * q + 1] = fmaf(w[1], v, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(w[2], v, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(w[3], v, acc[4 * q + 3]);
                }
            }
    float* dst = out + (long)oy * s4 + ox;                                     // 16 lanes side by side along x
#pragma unroll
    for (int o = 0; o < FL_C2; ++o) dst[(long)o * plane] = fmaxf(acc[o], 0.0f);
}

// ---- dawn_cond_rows: cond[t] = [audio[t] | pose[t] - init_pose | eye[t] - init_eye] for the rows [t0, t1)
struct CondArgs {
    const float* audio; const float* pose; const float* eye; float* cond;
    int n_aud, n_pose, P;                   // n_pose == P or P - 1 (the last pose column is then init_pose[P - 1])
    int ld_audio, ld_pose, ld_eye, ld_cond;
    int copy_audio;                         // 0: the audio rows are the audio columns of `cond` already
    int pose_row0, eye_row0;                // 1: the subtrahend is row 0 of the input (no host value)
    float ip[DAWN_COND_MAX_INIT], ie[2];
};

__global__ __launch_bounds__(256) void cond_rows_kernel(CondArgs a, long t0, long t1) {
    const int c0 = a.copy_audio ? 0 : a.n_aud;
    const int ncol = a.n_aud + a.P + 2 - c0;
    const long total = (t1 - t0) * ncol;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long t = t0 + i / ncol;
        const int c = c0 + (int)(i % ncol);
        float v;
        if (c < a.n_aud) {
            v = a.audio[t * a.ld_audio + c];
        } else if (c < a.n_aud + a.P) {
            const int j = c - a.n_aud;
            const float sub = a.pose_row0 ? a.pose[j] : a.ip[j];
            const float x = j < a.n_pose ? a.pose[t * a.ld_pose + j] : a.ip[j];      // FD:348-349: the appended init_pose column
            v = x - sub;
        } else {
            const int j = c - a.n_aud - a.P;
            v = a.eye[t * a.ld_eye + j] - (a.eye_row0 ? a.eye[j] : a.ie[j]);
        }
        a.cond[t * a.ld_cond + c] = v;
    }
}

inline bool finite_all(const float* v, int n) {
    for (int i = 0; i < n; ++i)
        if (!isfinite(v[i])) return false;
    return true;
}

// trunc toward zero as .to(torch.int32) does; beyond int's range (where the cast is undefined) the nearest int: no pixel either way
inline int trunc_int(float v) {
    if (v >= 2147483520.0f) return 2147483520;
    if (v <= -2147483648.0f) return (int)(-2147483647 - 1);
    return (int)v;
}

int bounds_checked(const float* bbox6, int size, const char* who, MaskBounds* mb) {
    char m[200];
    if (!bbox6) {
        snprintf(m, sizeof m, "%s: NULL bbox6", who);
        return dawn_set_error_msg(-271, m);
    }
    if (size < 4 || size % 4 != 0) {
        snprintf(m, sizeof m, "%s: size = %d, a multiple of 4 from 4 up is needed (two stride-2 convolutions)", who, size);
        return dawn_set_error_msg(-272, m);
    }
    if (!finite_all(bbox6, 6) || bbox6[4] == 0.0f || bbox6[5] == 0.0f) {
        snprintf(m, sizeof m, "%s: bbox6 must be finite with non-zero H_src and W_src", who);
        return dawn_set_error_msg(-273, m);
    }
    // FD:187-193 in fp32, every operation rounded on its own (volatile: the +1 must not fuse into the multiplication)
    const float fs = (float)size;
    volatile float q0 = bbox6[0] / bbox6[4], q1 = bbox6[1] / bbox6[4], q2 = bbox6[2] / bbox6[5], q3 = bbox6[3] / bbox6[5];
    volatile float x_min = q0 * fs, x_max = q1 * fs, y_min = q2 * fs, y_max = q3 * fs;
    volatile float x_hi = x_max + 1.0f, y_hi = y_max + 1.0f;
    mb->lt_x = trunc_int(x_min);
    mb->lt_y = trunc_int(y_min);
    mb->rb_x = trunc_int(x_hi);
    mb->rb_y = trunc_int(y_hi);
    return 0;
}

}  // namespace

extern "C" int dawn_bbox_mask_bounds(const float* bbox6, int size, int* bounds4) {
    if (!bounds4) return dawn_set_error_msg(-271, "dawn_bbox_mask_bounds: NULL bounds4");
    MaskBounds mb;
    CK(bounds_checked(bbox6, size, "dawn_bbox_mask_bounds", &mb));
    bounds4[0] = mb.lt_x; bounds4[1] = mb.lt_y; bounds4[2] = mb.rb_x; bounds4[3] = mb.rb_y;
    return 0;
}

int clip_face_loc_check(const float* bbox6, int size, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* out, long plane, const char* who, int* bounds4) {
    MaskBounds mb;
    CK(bounds_checked(bbox6, size, who, &mb));
    char m[200];
    if (!w1 || !b1 || !w2 || !b2 || !out) {
        snprintf(m, sizeof m, "%s: NULL pointer (w1, b1, w2, b2 and out are required)", who);
        return dawn_set_error_msg(-271, m);
    }
    const long s4 = size / 4;
    if (plane < s4 * s4) {
        snprintf(m, sizeof m, "%s: plane = %ld floats, an output plane holds %ld", who, plane, s4 * s4);
        return dawn_set_error_msg(-274, m);
    }
    bounds4[0] = mb.lt_x; bounds4[1] = mb.lt_y; bounds4[2] = mb.rb_x; bounds4[3] = mb.rb_y;
    return 0;
}

extern "C" int dawn_face_loc_embed(const float* bbox6, int size, const float* w1, const float* b1, const float* w2, const float* b2,
                                   float* out, long plane, void* stream) {
    int b[4];
    CK(clip_face_loc_check(bbox6, size, w1, b1, w2, b2, out, plane, "dawn_face_loc_embed", b));
    const MaskBounds mb = {b[0], b[1], b[2], b[3]};
    const int tiles = dawn_cdiv(size / 4, FL_T);
    hipLaunchKernelGGL(face_loc_embed_kernel, dim3(tiles, tiles), dim3(256), 0, (hipStream_t)stream, mb, size, w1, b1, w2, b2, out, plane);
    DAWN_LAUNCH_CHECK();
    return 0;
}

int clip_cond_rows_check(const float* audio, int n_aud, int ld_audio, const float* pose, int n_pose, int ld_pose, const float* eye,
                         int ld_eye, const float* init_pose, int n_init, const float* init_eye, long T, const float* cond, int ld_cond,
                         const char* who) {
    char m[240];
    if (!audio || !pose || !eye || !cond) {
        snprintf(m, sizeof m, "%s: NULL pointer (audio, pose, eye and cond are required)", who);
        return dawn_set_error_msg(-275, m);
    }
    if (T < 1 || n_aud < 0 || n_pose < 1) {
        snprintf(m, sizeof m, "%s: T = %ld rows, n_aud = %d, n_pose = %d: at least one row and one pose column", who, T, n_aud, n_pose);
        return dawn_set_error_msg(-276, m);
    }
    if (init_pose && (n_init < 1 || n_init > DAWN_COND_MAX_INIT)) {
        snprintf(m, sizeof m, "%s: n_init = %d, an init_pose holds 1..%d values", who, n_init, DAWN_COND_MAX_INIT);
        return dawn_set_error_msg(-277, m);
    }
    const int P = init_pose ? n_init : n_pose;
    if (n_pose != P && n_pose != P - 1) {
        snprintf(m, sizeof m, "%s: n_pose = %d against an init_pose of %d: the pose has as many columns or one fewer", who, n_pose, P);
        return dawn_set_error_msg(-277, m);
    }
    if ((init_pose && !finite_all(init_pose, n_init)) || (init_eye && !finite_all(init_eye, 2))) {
        snprintf(m, sizeof m, "%s: init_pose / init_eye must be finite", who);
        return dawn_set_error_msg(-278, m);
    }
    const long width = (long)n_aud + P + 2;
    if (ld_audio < n_aud || ld_pose < n_pose || ld_eye < 2 || ld_cond < width) {
        snprintf(m, sizeof m, "%s: a row stride is smaller than its width (audio %d / %d, pose %d / %d, eye %d / 2, cond %d / %ld)", who,
                 ld_audio, n_aud, ld_pose, n_pose, ld_eye, ld_cond, width);
        return dawn_set_error_msg(-279, m);
    }
    // an input is either exactly the columns of `cond` it lands in, or apart from `cond` altogether
    const size_t cond_bytes = ((size_t)(T - 1) * ld_cond + width) * 4;
    const struct { const float* p; int w, ld, col; const char* name; } in[3] = {
        {audio, n_aud, ld_audio, 0, "audio"}, {pose, n_pose, ld_pose, n_aud, "pose"}, {eye, 2, ld_eye, n_aud + P, "eye"}};
    for (const auto& o : in) {
        if (o.w == 0 || (o.p == cond + o.col && (o.ld == ld_cond || T == 1))) continue;      // (one row: no stride is read)
        if (overlaps(o.p, ((size_t)(T - 1) * o.ld + o.w) * 4, cond, cond_bytes)) {
            snprintf(m, sizeof m, "%s: %s overlaps cond without being its own columns of it (same address, ld == ld_cond)", who, o.name);
            return dawn_set_error_msg(-280, m);
        }
    }
    return 0;
}

extern "C" int dawn_cond_rows(const float* audio, int n_aud, int ld_audio, const float* pose, int n_pose, int ld_pose, const float* eye,
                              int ld_eye, const float* init_pose, int n_init, const float* init_eye, long T, float* cond, int ld_cond,
                              void* stream) {
    CK(clip_cond_rows_check(audio, n_aud, ld_audio, pose, n_pose, ld_pose, eye, ld_eye, init_pose, n_init, init_eye, T, cond, ld_cond,
                            "dawn_cond_rows"));
    CondArgs a = {};
    a.audio = audio; a.pose = pose; a.eye = eye; a.cond = cond;
    a.n_aud = n_aud; a.n_pose = n_pose; a.P = init_pose ? n_init : n_pose;
    a.ld_audio = ld_audio; a.ld_pose = ld_pose; a.ld_eye = ld_eye; a.ld_cond = ld_cond;
    a.copy_audio = !(audio == cond && (ld_audio == ld_cond || T == 1));
    a.pose_row0 = init_pose == nullptr;
    a.eye_row0 = init_eye == nullptr;
    for (int j = 0; init_pose && j < n_init; ++j) a.ip[j] = init_pose[j];
    for (int j = 0; init_eye && j < 2; ++j) a.ie[j] = init_eye[j];
    const int ncol = a.copy_audio ? n_aud + a.P + 2 : a.P + 2;
    const hipStream_t st = (hipStream_t)stream;
    auto launch = [&](long t0, long t1) {
        const long blocks = ((t1 - t0) * ncol + 255) / 256;
        hipLaunchKernelGGL(cond_rows_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, a, t0, t1);
    };
    if (a.pose_row0 || a.eye_row0) {
        // Row 0 is a subtrahend of every row and, in place, an output: the rows after it go first and read it unwritten, then row 0 on
        // its own in a second launch (stream order; nothing depends on the order of workgroups inside a grid)
        if (T > 1) {
            launch(1, T);
            DAWN_LAUNCH_CHECK();
        }
        launch(0, 1);
    } else {
        launch(0, T);
    }
    DAWN_LAUNCH_CHECK();
    return 0;
}
