// C-side LFG motion-encode stage (SURVEY 8f N5 as a whole path): dawn_motion_*, dawn_reenact_*.  The launch sequence of
// dawn-pytorch_amd/motion_encoder.py -- MotionEncoder._encode: the source work once per clip, then RegionPredictor, the background
// encoder and the PixelwiseFlowPredictor on the driving frames, chunk by chunk -- issued through the per-op entry points of this
// library with the same arguments, so that a non-Python host turns a driving video into the flow / occlusion latent with nothing but
// this .so, and so that the GPU tests can require both paths to agree bit for bit (tests/test_hip_motion_stage.py).
//
// Conventions as in dawn_decoder.hip: no allocation on the device (the caller provides the workspace, sized by dry passes of the same
// code), every launch on the caller's stream, no synchronisation, int return codes + dawn_last_error().  One kernel lives here: the
// copy that repeats the source half of the background encoder's first conv for the frames of a chunk (Python: expand().reshape()).
//
// The workspace: first the pieces that live for the whole clip -- the downsampled source, its region parameters, the repeated source
// rows, a chunk of RGB bytes (driving kind 2) -- then whatever the pass at hand allocates and frees again.  Every pass frees all it took,
// so the arena is in the same state in front of every chunk, and the size query runs the dry pass for EVERY chunk length 1 .. chunk:
// a ragged last chunk replays a sequence that has been measured, whatever first-fit makes of it.
#include "dawn_host.h"

#include <stddef.h>
#include <vector>

static_assert(sizeof(dawn_motion_cfg) == 192 && offsetof(dawn_motion_cfg, temperature) == 8 && offsetof(dawn_motion_cfg, rp_blocks) == 16 &&
                  offsetof(dawn_motion_cfg, rp_down) == 28 && offsetof(dawn_motion_cfg, pf_up) == 156,
              "dawn_motion_cfg layout (ctx.MotionCfg, the bundle's motion/cfg blob)");
static_assert(sizeof(dawn_reenact_args) == 120 && offsetof(dawn_reenact_args, drv) == 40 && offsetof(dawn_reenact_args, drv_frame_stride) == 56 &&
                  offsetof(dawn_reenact_args, mean3) == 88 && offsetof(dawn_reenact_args, conf_out) == 112,
              "dawn_reenact_args layout (ctx.ReenactArgs)");

namespace {

int pad16(int n) { return (n + 15) / 16 * 16; }

struct MConv {                    // motion_encoder._Conv: pack_kn image (an up block: the four phase images), optional pack_bf3 image, bias,
    const float *w = nullptr, *bias = nullptr, *a = nullptr, *b = nullptr;     // and the BatchNorm that follows as scale / shift
    const void* ws = nullptr;
    int N = 0;                    // padded output channels
};
struct Hourglass { std::vector<MConv> downs, ups; };
struct Buf { float* p; int C; };  // channels-last rows and their (padded) width

// out[r][i] = src[i], r < reps, i < n4: the rows of one image repeated for the frames of a chunk
__global__ __launch_bounds__(256) void rows_repeat_kernel(const f32x4* __restrict__ src, long n4, int reps, f32x4* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = src[i];
        for (int r = 0; r < reps; ++r) out[(long)r * n4 + i] = v;
    }
}

}  // namespace

struct dawn_motion {
    dawn_motion_cfg cfg;
    Hourglass rp, pf;
    MConv rp_regions, bg_src0, bg_drv0, pf_out;
    std::vector<MConv> bg_downs;  // [0]: only a / b (the BatchNorm after the split first conv)
    const float *fc_w = nullptr, *fc_b = nullptr;
    int c_in_pf = 0;
};                                // immutable after dawn_motion_create

namespace {

void load_conv(DawnWeights& Wt, const std::string& p, int N, bool ws, bool bias, bool norm, MConv& c) {
    c.N = N;
    c.w = Wt.getf(p + "w");
    if (ws) c.ws = Wt.get(p + "ws");
    if (bias) c.bias = Wt.getf(p + "bias");
    if (norm) {
        c.a = Wt.getf(p + "a");
        c.b = Wt.getf(p + "b");
    }
}

void load_hourglass(DawnWeights& Wt, const std::string& p, int n, const int* down, const int* up, Hourglass& g) {
    g.downs.resize(n);
    g.ups.resize(n);
    for (int i = 0; i < n; ++i) {
        load_conv(Wt, p + "down." + std::to_string(i) + ".", pad16(down[i]), true, true, true, g.downs[i]);
        load_conv(Wt, p + "up." + std::to_string(i) + ".", pad16(up[i]), false, true, true, g.ups[i]);
    }
}

#define ALLOC(ptr, floats) DAWN_ALLOC(A, ptr, floats, -392, "dawn_motion: workspace too small (dawn_motion_workspace_bytes)")

// ops.conv_gemm as motion_encoder.py calls it: K x K, stride 1; mode 1 = an up block's nearest-x2 + 3x3 as four 2 x 2 phases
int conv(const MConv& c, Buf in0, Buf in1, int F, int Hi, int Wi, int K, int pad, int mode, const float* res, float* out, bool dry,
         void* stream) {
    if (dry) return 0;
    dawn_conv_desc d = {};
    d.in0 = in0.p; d.C0 = in0.C; d.ld0 = in0.C;
    d.in1 = in1.p; d.C1 = in1.p ? in1.C : 0; d.ld1 = in1.p ? in1.C : 0;
    d.F = F; d.Hi = Hi; d.Wi = Wi; d.Ho = mode ? 2 * Hi : Hi; d.Wo = mode ? 2 * Wi : Wi;
    d.KH = K; d.KW = K; d.stride = 1; d.pad = pad; d.mode = mode;
    d.w = c.w; d.bias = c.bias; d.N = c.N;
    d.res = res; d.ld_res = res ? c.N : 0;
    d.out = out; d.ld_out = c.N;
    d.w_bf3 = c.ws;
    return dawn_conv_gemm(&d, stream);
}

// _Hourglass.forward: x (F h w, x.C) -> *out = the last decoder level (the caller frees it); the second source of the 7x7 conv that
// follows is x itself
int hourglass(const Hourglass& g, DawnArena& A, Buf x, int F, int h, int w, Buf* out, bool dry, void* stream) {
    const int n = (int)g.downs.size();
    std::vector<Buf> outs{x};
    Buf cur = x;
    for (const MConv& d : g.downs) {
        ALLOC(z, (size_t)F * h * w * d.N);
        CK(conv(d, cur, Buf{nullptr, 0}, F, h, w, 3, 1, 0, nullptr, z, dry, stream));
        ALLOC(nxt, (size_t)F * (h / 2) * (w / 2) * d.N);
        if (!dry) CK(dawn_bn_relu_pool2(z, d.a, d.b, nxt, F, h, w, d.N, stream));
        A.free(z);
        h /= 2; w /= 2;
        cur = Buf{nxt, d.N};
        outs.push_back(cur);
    }
    Buf o = outs.back(), skip{nullptr, 0};
    outs.pop_back();
    for (int j = 0; j < n; ++j) {
        const MConv& u = g.ups[j];
        ALLOC(y, (size_t)F * 4 * h * w * u.N);
        CK(conv(u, o, skip, F, h, w, 2, 0, 1, nullptr, y, dry, stream));
        A.free(o.p);
        if (skip.p) A.free(skip.p);
        h *= 2; w *= 2;
        ALLOC(act, (size_t)F * h * w * u.N);
        if (!dry) CK(dawn_affine_act(y, u.N, u.a, u.b, 1, act, (long)F * h * w, u.N, stream));
        A.free(y);
        o = Buf{act, u.N};
        skip = outs.back();
        outs.pop_back();
    }
    *out = o;
    return 0;
}

// MotionEncoder._regions: down (F h w, 16) -> the region parameters of F frames
int regions(const dawn_motion* m, DawnArena& A, Buf down, int F, int h, int w, float* shift, float* covar, float* affine, bool dry,
            void* stream) {
    Buf top;
    CK(hourglass(m->rp, A, down, F, h, w, &top, dry, stream));
    const MConv& c = m->rp_regions;
    ALLOC(x, (size_t)F * h * w * c.N);
    CK(conv(c, top, down, F, h, w, 7, 3, 0, nullptr, x, dry, stream));
    A.free(top.p);
    if (!dry) CK(dawn_region_moments(x, c.N, F, h, w, m->cfg.R, m->cfg.temperature, shift, covar, affine, stream));
    A.free(x);
    return 0;
}

struct Clip {                     // what lives for the whole clip, in allocation order
    float *src_down, *s_shift, *s_covar, *s_affine, *bg_rep;
    unsigned char* rgb;
};

int persist(const dawn_motion* m, DawnArena& A, int H, int W, int chunk, Clip* c) {
    const int s = m->cfg.s, R = m->cfg.R, h = (H + s - 1) / s, w = (W + s - 1) / s;
    ALLOC(src_down, (size_t)h * w * 16);
    ALLOC(s_shift, (size_t)R * 2);
    ALLOC(s_covar, (size_t)R * 4);
    ALLOC(s_affine, (size_t)R * 4);
    ALLOC(bg_rep, (size_t)chunk * H * W * m->bg_src0.N);
    ALLOC(rgb, ((size_t)chunk * H * W * 3 + 3) / 4);
    *c = Clip{src_down, s_shift, s_covar, s_affine, bg_rep, (unsigned char*)rgb};
    return 0;
}

// once per clip: the source's downsampled image, its region parameters, its half of the background encoder's first conv
int source_pass(const dawn_motion* m, DawnArena& A, const Clip& c, int H, int W, const void* src, int kind, int chunk, bool dry, void* stream) {
    const int s = m->cfg.s, h = (H + s - 1) / s, w = (W + s - 1) / s;
    const long fs = (long)3 * H * W, cs = kind == 0 ? (long)H * W : 1;
    if (!dry) CK(dawn_antialias_down(src, kind, fs, cs, 1, H, W, s, c.src_down, 16, 16, stream));
    CK(regions(m, A, Buf{c.src_down, 16}, 1, h, w, c.s_shift, c.s_covar, c.s_affine, dry, stream));
    ALLOC(full, (size_t)H * W * 16);
    if (!dry) CK(dawn_antialias_down(src, kind, fs, cs, 1, H, W, 1, full, 16, 16, stream));
    const MConv& c0 = m->bg_src0;
    ALLOC(bg_src, (size_t)H * W * c0.N);
    CK(conv(c0, Buf{full, 16}, Buf{nullptr, 0}, 1, H, W, 3, 1, 0, nullptr, bg_src, dry, stream));
    A.free(full);
    if (!dry) {
        const long n4 = (long)H * W * c0.N / 4;
        const long g = (n4 + 255) / 256;
        hipLaunchKernelGGL(rows_repeat_kernel, dim3((unsigned)(g > 65536 ? 65536 : g)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)bg_src,
                           n4, chunk, (f32x4*)c.bg_rep);
        DAWN_LAUNCH_CHECK();
    }
    A.free(bg_src);
    return 0;
}

struct Driving { const void* p; int kind; long fs, cs; };
struct Out { float* grid; long plane; float* conf; int x0; };

// the n frames from t0 on
int chunk_pass(const dawn_motion* m, DawnArena& A, const Clip& c, int H, int W, int n, int t0, const Driving& dv, const Out& o, bool dry,
               void* stream) {
    const int s = m->cfg.s, R = m->cfg.R, h = (H + s - 1) / s, w = (W + s - 1) / s;
    const void* fr = nullptr;
    int kind = dv.kind;
    long fs = dv.fs, cs = dv.cs;
    if (!dry) {
        if (dv.kind == 2) {
            CK(dawn_yuv420_to_frames((const unsigned char*)dv.p + (long)t0 * dv.fs, dv.fs, n, H, W, c.rgb, stream));
            fr = c.rgb; kind = 1; fs = (long)3 * H * W; cs = 1;
        } else if (dv.kind == 1) {
            fr = (const unsigned char*)dv.p + (long)t0 * dv.fs; cs = 1;
        } else {
            fr = (const float*)dv.p + (long)t0 * dv.fs;
        }
    }
    ALLOC(d_shift, (size_t)n * R * 2);
    ALLOC(d_covar, (size_t)n * R * 4);
    ALLOC(d_affine, (size_t)n * R * 4);
    ALLOC(down, (size_t)n * h * w * 16);
    if (!dry) CK(dawn_antialias_down(fr, kind, fs, cs, n, H, W, s, down, 16, 16, stream));
    CK(regions(m, A, Buf{down, 16}, n, h, w, d_shift, d_covar, d_affine, dry, stream));
    A.free(down);
    // the background encoder: the first conv's driving half on top of the repeated source half, then the remaining blocks
    ALLOC(full, (size_t)n * H * W * 16);
    if (!dry) CK(dawn_antialias_down(fr, kind, fs, cs, n, H, W, 1, full, 16, 16, stream));
    const MConv& d0 = m->bg_drv0;
    ALLOC(z0, (size_t)n * H * W * d0.N);
    CK(conv(d0, Buf{full, 16}, Buf{nullptr, 0}, n, H, W, 3, 1, 0, c.bg_rep, z0, dry, stream));
    A.free(full);
    int Hc = H / 2, Wc = W / 2;
    ALLOC(p0, (size_t)n * Hc * Wc * d0.N);
    if (!dry) CK(dawn_bn_relu_pool2(z0, m->bg_downs[0].a, m->bg_downs[0].b, p0, n, H, W, d0.N, stream));
    A.free(z0);
    Buf cur{p0, d0.N};
    for (size_t i = 1; i < m->bg_downs.size(); ++i) {
        const MConv& d = m->bg_downs[i];
        ALLOC(z, (size_t)n * Hc * Wc * d.N);
        CK(conv(d, cur, Buf{nullptr, 0}, n, Hc, Wc, 3, 1, 0, nullptr, z, dry, stream));
        A.free(cur.p);
        ALLOC(nxt, (size_t)n * (Hc / 2) * (Wc / 2) * d.N);
        if (!dry) CK(dawn_bn_relu_pool2(z, d.a, d.b, nxt, n, Hc, Wc, d.N, stream));
        A.free(z);
        Hc /= 2; Wc /= 2;
        cur = Buf{nxt, d.N};
    }
    ALLOC(bg, (size_t)n * 9);
    if (!dry) CK(dawn_bg_params(cur.p, cur.C, n, Hc * Wc, cur.C, m->fc_w, m->fc_b, bg, stream));
    A.free(cur.p);
    // the pixelwise flow predictor
    ALLOC(rows, (size_t)n * h * w * m->c_in_pf);
    if (!dry)
        CK(dawn_motion_inputs(d_shift, d_covar, d_affine, c.s_shift, c.s_covar, c.s_affine, bg, R, c.src_down, 16, n, h, w, rows, m->c_in_pf,
                              m->c_in_pf, stream));
    Buf top;
    CK(hourglass(m->pf, A, Buf{rows, m->c_in_pf}, n, h, w, &top, dry, stream));
    const MConv& co = m->pf_out;
    ALLOC(x, (size_t)n * h * w * co.N);
    CK(conv(co, top, Buf{rows, m->c_in_pf}, n, h, w, 7, 3, 0, nullptr, x, dry, stream));
    A.free(top.p);
    A.free(rows);
    if (!dry)
        CK(dawn_flow_combine(x, co.N, d_shift, d_affine, c.s_shift, c.s_affine, bg, R, n, h, w, o.grid + (long)t0 * h * w, o.plane,
                             o.conf + (long)t0 * h * w, o.x0, stream));
    A.free(x);
    A.free(bg);
    A.free(d_affine);
    A.free(d_covar);
    A.free(d_shift);
    return 0;
}

// the sizes the stage takes; `who` names the entry in the message
int check_size(const dawn_motion* m, int H, int W, int chunk, const char* who) {
    char msg[240];
    if (!m) {
        snprintf(msg, sizeof msg, "%s: NULL handle", who);
        return dawn_set_error_msg(-391, msg);
    }
    if (chunk < 1 || chunk > 4096) {
        snprintf(msg, sizeof msg, "%s: chunk = %d frames, 1 .. 4096", who, chunk);
        return dawn_set_error_msg(-393, msg);
    }
    const int kb = 1 << m->cfg.bg_blocks;
    if (H < 1 || W < 1 || H > 32768 || W > 32768 || H % kb || W % kb) {
        snprintf(msg, sizeof msg, "%s: H x W = %d x %d must be positive multiples of %d (the background encoder pools %d times)", who, H, W, kb,
                 m->cfg.bg_blocks);
        return dawn_set_error_msg(-394, msg);
    }
    const int s = m->cfg.s, h = (H + s - 1) / s, w = (W + s - 1) / s;
    const int kh = 1 << (m->cfg.rp_blocks > m->cfg.pf_blocks ? m->cfg.rp_blocks : m->cfg.pf_blocks);
    if (h < 2 || w < 2 || h % kh || w % kh) {
        snprintf(msg, sizeof msg, "%s: the %d x %d map of %d x %d frames (1 / %d) must be a multiple of %d, at least 2 (the hourglasses' skip "
                                  "sizes would not match)", who, h, w, H, W, s, kh);
        return dawn_set_error_msg(-395, msg);
    }
    int widest = m->bg_src0.N > 16 ? m->bg_src0.N : 16;
    if ((long)chunk * H * W > 0x7fffffffL / widest) {
        snprintf(msg, sizeof msg, "%s: chunk = %d frames of %d x %d: rows * %d channels must fit an int", who, chunk, H, W, widest);
        return dawn_set_error_msg(-393, msg);
    }
    return 0;
}

size_t workspace_need(const dawn_motion* m, int H, int W, int chunk) {
    DawnArena dry;
    dry.reset(nullptr, 0, true);
    Clip c;
    if (persist(m, dry, H, W, chunk, &c)) return 0;
    if (source_pass(m, dry, c, H, W, nullptr, 0, chunk, true, nullptr)) return 0;
    for (int n = 1; n <= chunk; ++n)
        if (chunk_pass(m, dry, c, H, W, n, 0, Driving{nullptr, 0, 0, 0}, Out{nullptr, 0, nullptr, 0}, true, nullptr)) return 0;
    return dry.high;
}

}  // namespace

extern "C" int dawn_motion_create(const dawn_motion_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_motion** out) {
    if (!cfg || !out || (!weights && n_weights > 0)) return dawn_set_error_msg(-391, "dawn_motion_create: NULL argument");
    char msg[240];
    if (cfg->R < 1 || cfg->R > 15 || cfg->s < 1 || cfg->s > 8 || !(cfg->temperature > 0.0)) {
        snprintf(msg, sizeof msg, "dawn_motion_create: R = %d regions (1 .. 15), s = %d (1 .. 8), temperature = %g (positive)", cfg->R, cfg->s,
                 cfg->temperature);
        return dawn_set_error_msg(-396, msg);
    }
    const int counts[3] = {cfg->rp_blocks, cfg->bg_blocks, cfg->pf_blocks};
    const char* const what[3] = {"rp_blocks", "bg_blocks", "pf_blocks"};
    for (int i = 0; i < 3; ++i)
        if (counts[i] < 1 || counts[i] > DAWN_MOTION_MAX_BLOCKS) {
            snprintf(msg, sizeof msg, "dawn_motion_create: %s = %d, 1 .. %d blocks", what[i], counts[i], DAWN_MOTION_MAX_BLOCKS);
            return dawn_set_error_msg(-396, msg);
        }
    const int* const widths[5] = {cfg->rp_down, cfg->rp_up, cfg->bg_down, cfg->pf_down, cfg->pf_up};
    const char* const wname[5] = {"rp_down", "rp_up", "bg_down", "pf_down", "pf_up"};
    const int wcount[5] = {cfg->rp_blocks, cfg->rp_blocks, cfg->bg_blocks, cfg->pf_blocks, cfg->pf_blocks};
    for (int k = 0; k < 5; ++k)
        for (int i = 0; i < wcount[k]; ++i)
            if (widths[k][i] < 1 || widths[k][i] > 4096) {
                snprintf(msg, sizeof msg, "dawn_motion_create: %s[%d] = %d channels, 1 .. 4096", wname[k], i, widths[k][i]);
                return dawn_set_error_msg(-396, msg);
            }
    dawn_motion* m = new dawn_motion();
    m->cfg = *cfg;
    m->c_in_pf = pad16(4 * (cfg->R + 1));
    DawnWeights Wt(weights, n_weights, "dawn_motion_create: missing packed weight", -390);
    load_hourglass(Wt, "rp.", cfg->rp_blocks, cfg->rp_down, cfg->rp_up, m->rp);
    load_conv(Wt, "rp.regions.", pad16(cfg->R), false, true, false, m->rp_regions);
    const int N0 = pad16(cfg->bg_down[0]);
    load_conv(Wt, "bg.src0.", N0, true, true, false, m->bg_src0);
    load_conv(Wt, "bg.drv0.", N0, true, false, false, m->bg_drv0);
    m->bg_downs.resize(cfg->bg_blocks);
    m->bg_downs[0].N = N0;
    m->bg_downs[0].a = Wt.getf("bg.down.0.a");
    m->bg_downs[0].b = Wt.getf("bg.down.0.b");
    for (int i = 1; i < cfg->bg_blocks; ++i) load_conv(Wt, "bg.down." + std::to_string(i) + ".", pad16(cfg->bg_down[i]), true, true, true, m->bg_downs[i]);
    m->fc_w = Wt.getf("fc.w");
    m->fc_b = Wt.getf("fc.b");
    load_hourglass(Wt, "pf.", cfg->pf_blocks, cfg->pf_down, cfg->pf_up, m->pf);
    load_conv(Wt, "pf.out.", pad16(cfg->R + 2), false, true, false, m->pf_out);
    if (!Wt.ok()) {
        delete m;
        return Wt.code();
    }
    *out = m;
    return 0;
}

extern "C" void dawn_motion_destroy(dawn_motion* m) { delete m; }

extern "C" size_t dawn_motion_workspace_bytes(const dawn_motion* m, int H, int W, int chunk) {
    if (check_size(m, H, W, chunk, "dawn_motion_workspace_bytes")) return 0;
    return workspace_need(m, H, W, chunk);
}

extern "C" int dawn_motion_encode_clip(dawn_motion* m, int H, int W, int T, const void* src, int src_kind, const void* drv, int drv_kind,
                                       long drv_frame_stride, long drv_chan_stride, int chunk, float* grid, long grid_plane, float* conf,
                                       int conf_x0, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dawn_motion_encode_clip";
    char msg[240];
    if (!m || !src || !drv || !grid || !conf) {
        snprintf(msg, sizeof msg, "%s: NULL argument (%s)", who, !m ? "the handle" : !src ? "src" : !drv ? "drv" : !grid ? "grid" : "conf");
        return dawn_set_error_msg(-391, msg);
    }
    if (T < 1) {
        snprintf(msg, sizeof msg, "%s: T = %d frames, at least 1 needed", who, T);
        return dawn_set_error_msg(-393, msg);
    }
    if (chunk < 1) {
        snprintf(msg, sizeof msg, "%s: chunk = %d frames, at least 1 needed", who, chunk);
        return dawn_set_error_msg(-393, msg);
    }
    if (src_kind < 0 || src_kind > 1 || drv_kind < 0 || drv_kind > 2) {
        snprintf(msg, sizeof msg, "%s: src_kind = %d (0 fp32 planes, 1 uint8 RGB), drv_kind = %d (0, 1, or 2 I420 frames)", who, src_kind, drv_kind);
        return dawn_set_error_msg(-397, msg);
    }
    const int ce = chunk < T ? chunk : T;
    CK(check_size(m, H, W, ce > 4096 ? 4096 : ce, who));
    const int n_chunk = ce > 4096 ? 4096 : ce;
    const long HW = (long)H * W;
    const long fs_min = drv_kind == 0 ? HW : drv_kind == 1 ? 3 * HW : HW / 2 * 3;
    if ((T > 1 || drv_kind != 0) && drv_frame_stride < fs_min) {
        snprintf(msg, sizeof msg, "%s: drv_frame_stride = %ld, a frame of kind %d takes at least %ld", who, drv_frame_stride, drv_kind, fs_min);
        return dawn_set_error_msg(-398, msg);
    }
    if (drv_kind == 0 && drv_chan_stride < HW) {
        snprintf(msg, sizeof msg, "%s: drv_chan_stride = %ld floats, a plane has %ld", who, drv_chan_stride, HW);
        return dawn_set_error_msg(-398, msg);
    }
    if (drv_kind == 2 && (H % 2 != 0 || W % 4 != 0)) {
        snprintf(msg, sizeof msg, "%s: I420 driving frames (drv_kind 2) need an even H and W %% 4 == 0 (H = %d, W = %d)", who, H, W);
        return dawn_set_error_msg(-394, msg);
    }
    const int s = m->cfg.s, h = (H + s - 1) / s, w = (W + s - 1) / s;
    if (grid_plane < (long)T * h * w) {
        snprintf(msg, sizeof msg, "%s: grid_plane = %ld floats, T h w = %ld", who, grid_plane, (long)T * h * w);
        return dawn_set_error_msg(-398, msg);
    }
    const size_t need = workspace_need(m, H, W, n_chunk);
    if (!workspace || workspace_bytes < need) return refuse_workspace(-392, who, workspace ? workspace_bytes : 0, need, "dawn_motion_workspace_bytes");
    const size_t plane = (size_t)T * h * w * 4;
    if (overlaps(grid, (size_t)grid_plane * 4 + plane, workspace, workspace_bytes) || overlaps(conf, plane, workspace, workspace_bytes)) {
        snprintf(msg, sizeof msg, "%s: grid / conf overlap the workspace", who);
        return dawn_set_error_msg(-399, msg);
    }
    DawnArena A;
    A.reset(workspace, workspace_bytes, false);
    Clip c;
    CK(persist(m, A, H, W, n_chunk, &c));
    CK(source_pass(m, A, c, H, W, src, src_kind, n_chunk, false, stream));
    const Driving dv{drv, drv_kind, drv_frame_stride, drv_chan_stride};
    const Out o{grid, grid_plane, conf, conf_x0 ? 1 : 0};
    for (int t0 = 0; t0 < T; t0 += n_chunk) {
        const int n = T - t0 < n_chunk ? T - t0 : n_chunk;
        CK(chunk_pass(m, A, c, H, W, n, t0, dv, o, false, stream));
    }
    return 0;
}

namespace {

struct ReenactLayout {
    size_t grid, conf, skip, stage, total, skip_bytes, clip_bytes;
    int h, w;
};

int reenact_check(const dawn_reenact_args* a, const char* who, ReenactLayout* L) {
    char msg[240];
    if (!a) {
        snprintf(msg, sizeof msg, "%s: NULL args", who);
        return dawn_set_error_msg(-391, msg);
    }
    if (a->size != sizeof(dawn_reenact_args)) {
        snprintf(msg, sizeof msg, "%s: args->size = %zu, sizeof(dawn_reenact_args) = %zu here", who, a->size, sizeof(dawn_reenact_args));
        return dawn_set_error_msg(-391, msg);
    }
    if (!a->motion || !a->decoder || !a->img3 || !a->drv) {
        snprintf(msg, sizeof msg, "%s: NULL argument (%s)", who, !a->motion ? "motion" : !a->decoder ? "decoder" : !a->img3 ? "img3" : "drv");
        return dawn_set_error_msg(-391, msg);
    }
    if ((a->grid_out == nullptr) != (a->conf_out == nullptr)) {
        snprintf(msg, sizeof msg, "%s: grid_out and conf_out come as a pair", who);
        return dawn_set_error_msg(-391, msg);
    }
    if (a->T < 1 || a->motion_chunk < 1 || a->chunk < 1) {
        snprintf(msg, sizeof msg, "%s: T = %d, motion_chunk = %d, chunk = %d: at least 1 each", who, a->T, a->motion_chunk, a->chunk);
        return dawn_set_error_msg(-393, msg);
    }
    if (a->format != DAWN_FRAMES_RGB && a->format != DAWN_FRAMES_YUV420) {
        snprintf(msg, sizeof msg, "%s: format = %d (DAWN_FRAMES_RGB or DAWN_FRAMES_YUV420)", who, a->format);
        return dawn_set_error_msg(-397, msg);
    }
    if (a->W % 4 != 0 || (a->format == DAWN_FRAMES_YUV420 && a->H % 2 != 0)) {
        snprintf(msg, sizeof msg, "%s: frames of %d x %d: W %% 4 == 0 is needed, and an even H for yuv420", who, a->H, a->W);
        return dawn_set_error_msg(-394, msg);
    }
    if (a->format == DAWN_FRAMES_YUV420 && a->bgr) {
        snprintf(msg, sizeof msg, "%s: bgr goes with DAWN_FRAMES_RGB only", who);
        return dawn_set_error_msg(-397, msg);
    }
    const int mc = a->motion_chunk < a->T ? a->motion_chunk : a->T, dc = a->chunk < a->T ? a->chunk : a->T;
    const size_t mws = dawn_motion_workspace_bytes(a->motion, a->H, a->W, mc);
    if (mws == 0) return -394;                                   // (the query left its message)
    L->skip_bytes = dawn_decoder_skip_bytes(a->decoder, a->H, a->W);
    const size_t dws = dawn_decoder_workspace_bytes(a->decoder, a->H, a->W, dc);
    if (L->skip_bytes == 0 || dws == 0) return -394;
    const dawn_motion_cfg& c = a->motion->cfg;
    L->h = (a->H + c.s - 1) / c.s;
    L->w = (a->W + c.s - 1) / c.s;
    const size_t plane = (size_t)a->T * L->h * L->w * 4;
    size_t off = 0;
    L->grid = off; off += a->grid_out ? 0 : a256(2 * plane);
    L->conf = off; off += a->conf_out ? 0 : a256(plane);
    L->skip = off; off += a256(L->skip_bytes);
    L->stage = off;
    L->total = off + (mws > dws ? mws : dws);
    const size_t HW = (size_t)a->H * a->W;
    L->clip_bytes = (size_t)a->T * (a->format == DAWN_FRAMES_YUV420 ? HW / 2 * 3 : HW * 3);
    return 0;
}

}  // namespace

extern "C" int dawn_reenact_bytes(const dawn_reenact_args* args, size_t* clip_bytes, size_t* workspace_bytes) {
    if (!clip_bytes || !workspace_bytes) return dawn_set_error_msg(-391, "dawn_reenact_bytes: NULL argument");
    ReenactLayout L;
    CK(reenact_check(args, "dawn_reenact_bytes", &L));
    *clip_bytes = L.clip_bytes;
    *workspace_bytes = L.total;
    return 0;
}

extern "C" int dawn_reenact_clip(const dawn_reenact_args* args, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dawn_reenact_clip";
    ReenactLayout L;
    CK(reenact_check(args, who, &L));
    const dawn_reenact_args& a = *args;
    if (!a.frames_out || ((uintptr_t)a.frames_out & 3) != 0) return dawn_set_error_msg(-391, "dawn_reenact_clip: frames_out must be a non-NULL 4-byte aligned buffer");
    if (!workspace || workspace_bytes < L.total || ((uintptr_t)workspace & 255) != 0) {
        if (workspace && ((uintptr_t)workspace & 255) != 0) return dawn_set_error_msg(-392, "dawn_reenact_clip: the workspace is not 256-byte aligned");
        return refuse_workspace(-392, who, workspace ? workspace_bytes : 0, L.total, "dawn_reenact_bytes");
    }
    const size_t plane = (size_t)a.T * L.h * L.w * 4;
    if (overlaps(a.frames_out, L.clip_bytes, workspace, workspace_bytes) ||
        (a.grid_out && (overlaps(a.grid_out, 2 * plane, workspace, workspace_bytes) || overlaps(a.conf_out, plane, workspace, workspace_bytes))))
        return dawn_set_error_msg(-399, "dawn_reenact_clip: an output overlaps the workspace");
    char* ws = (char*)workspace;
    float* grid = a.grid_out ? a.grid_out : (float*)(ws + L.grid);
    float* conf = a.conf_out ? a.conf_out : (float*)(ws + L.conf);
    void* skip = ws + L.skip;
    void* stage = ws + L.stage;
    const size_t stage_bytes = workspace_bytes - L.stage;
    const long gp = (long)a.T * L.h * L.w;
    CK(dawn_motion_encode_clip(a.motion, a.H, a.W, a.T, a.img3, 0, a.drv, a.drv_kind, a.drv_frame_stride, a.drv_chan_stride, a.motion_chunk, grid,
                               gp, conf, 0, stage, stage_bytes, stream));
    CK(dawn_decoder_encode(a.decoder, a.H, a.W, a.img3, skip, L.skip_bytes, nullptr, stage, stage_bytes, stream));
    if (a.format == DAWN_FRAMES_YUV420)
        return dawn_decode_clip_conf_yuv420(a.decoder, a.H, a.W, a.T, L.h, L.w, a.img3, skip, grid, gp, conf, a.chunk, a.frames_out, a.mean3, stage,
                                            stage_bytes, stream);
    return dawn_decode_clip_conf(a.decoder, a.H, a.W, a.T, L.h, L.w, a.img3, skip, grid, gp, conf, a.chunk, nullptr, nullptr, 0, a.frames_out, a.mean3,
                                 a.bgr ? 1 : 0, stage, stage_bytes, stream);
}
