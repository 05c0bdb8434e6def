// C-side LFG flow decoder (SURVEY 8f N1 + N2 as a whole path): dawn_decoder_* / dawn_decode_clip.  The launch sequence of
// dawn-pytorch_amd/flow_decoder.py -- FlowDecoder.encode (GEN:140-146, once per clip) and _decode_frames / decode_clip
// (GEN:152-167 for a chunk of frames, loop FD:372-385) -- issued through the per-op entry points of this library with the same
// arguments, so that a non-Python host turns the sampler's latent into frames with nothing but this .so, and so that the GPU
// tests can require both paths to agree bit for bit (tests/test_hip_decode_u8.py).
//
// Conventions as in dawn_ctx.hip: no allocation on the device (the caller provides the per-clip skip memory and the workspace,
// sized by a dry pass of the same code), every launch on the caller's stream, no synchronisation, int return codes +
// dawn_last_error().  Three copy / elementwise kernels live here: the bias rows of the first convolution, the (C,h,w) transpose of
// `fea`, and the occlusion map (p + 1) * 0.5 of a latent chunk.
#include "dawn_host.h"

#include <vector>

namespace {

struct Conv3 {                    // flow_decoder._Conv: 3x3 conv (pack_kn image, optional pack_bf3 image, bias), BatchNorm that follows
    const float *w = nullptr, *bias = nullptr, *a = nullptr, *b = nullptr;
    const void* ws = nullptr;
    int Cin = 0, N = 0;
};
struct Bott { const float *a1, *b1, *a2, *b2; Conv3 c1, c2; };

// fea_pre of dawn_init_conv_x for a conv without a hoisted part: every row = the bias (FlowDecoder._bias_maps)
__global__ __launch_bounds__(256) void bias_rows_kernel(const float* __restrict__ bias, long rows, int C, float* __restrict__ out) {
    const long total = rows * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) out[i] = bias[i % C];
}

// (HW, C) channels-last rows -> (C, HW) planes (compute_fea's permute(2,0,1), a copy)
__global__ __launch_bounds__(256) void hwc_to_chw_kernel(const float* __restrict__ in, long HW, int C, float* __restrict__ out) {
    const long total = HW * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long c = i / HW, p = i - c * HW;
        out[i] = in[p * C + c];
    }
}

// occlusion map of a latent chunk as torch evaluates (pred[:, 2] + 1) * 0.5: a rounded sum, then a rounded product
__global__ __launch_bounds__(256) void conf_of_latent_kernel(const float* __restrict__ p, long n, float* __restrict__ out) {
#pragma clang fp contract(off)
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) out[i] = (p[i] + 1.0f) * 0.5f;
}

int grid_for(long total) {
    long g = (total + 255) / 256;
    return (int)(g > 65536 ? 65536 : (g < 1 ? 1 : g));
}

}  // namespace

struct dawn_decoder {
    dawn_decoder_cfg cfg;
    const float *first_w3 = nullptr, *first_bias = nullptr, *first_a = nullptr, *first_b = nullptr, *final_w7 = nullptr,
                *final_bias = nullptr;
    std::vector<Conv3> downs, ups;
    std::vector<Bott> bott;
};                                // immutable after dawn_decoder_create: every call sub-allocates its workspace with an arena of its own

namespace {

// the conv under prefix p; norm: with the scale / shift of the BatchNorm that follows it
void load_conv(DawnWeights& Wt, const std::string& p, int Cin, int N, bool norm, Conv3& c) {
    c.Cin = Cin; c.N = N;
    c.w = Wt.getf(p + "w");
    c.bias = Wt.getf(p + "bias");
    c.ws = Wt.opt(p + "ws");
    if (norm) {
        c.a = Wt.getf(p + "a");
        c.b = Wt.getf(p + "b");
    }
}

size_t skip_floats(const dawn_decoder* d, int lvl, int H, int W) { return (size_t)(H >> lvl) * (W >> lvl) * d->cfg.widths[lvl]; }

// skip `lvl` inside the per-clip skip memory: levels one after the other, each 256-byte aligned
const float* skip_at(const dawn_decoder* d, const void* mem, int lvl, int H, int W) {
    size_t off = 0;
    for (int i = 0; i < lvl; ++i) off += a256(skip_floats(d, i, H, W) * 4);
    return (const float*)((const char*)mem + off);
}

int bad_size(const dawn_decoder* d, int H, int W, const char* who) {
    const int k = 1 << d->cfg.n_down;
    if (H <= 0 || W <= 0 || H % k || W % k) {
        char m[160];
        snprintf(m, sizeof m, "%s: image size %dx%d is not a positive multiple of %d", who, H, W, k);
        return dawn_set_error_msg(-231, m);
    }
    return 0;
}

// FlowDecoder._conv3: 3x3 / stride 1 / pad 1 through dawn_conv_gemm (split-operand kernel when the bf16 image is there)
int conv3(const Conv3& c, const float* x, int F, int H, int W, const float* res, float* out, bool dry, void* stream) {
    if (dry) return 0;
    dawn_conv_desc d = {};
    d.in0 = x; d.C0 = c.Cin; d.ld0 = c.Cin;
    d.F = F; d.Hi = H; d.Wi = W; d.Ho = H; d.Wo = W;
    d.KH = 3; d.KW = 3; d.stride = 1; d.pad = 1; d.mode = 0;
    d.w = c.w; d.bias = c.bias; d.N = c.N;
    d.res = res; d.ld_res = res ? c.N : 0;
    d.out = out; d.ld_out = c.N;
    d.w_bf3 = c.ws;
    return dawn_conv_gemm(&d, stream);
}

#define ALLOC(ptr, floats) DAWN_ALLOC(A, ptr, floats, -232, "dawn_decoder: workspace too small (dawn_decoder_workspace_bytes)")

// FlowDecoder.encode (+ compute_fea's transpose).  dry: sizes the workspace, launches nothing.
int encode(const dawn_decoder* d, DawnArena& A, int H, int W, const float* img3, void* skip_mem, float* fea_out, bool dry,
           void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const int C0 = d->cfg.widths[0], n = d->cfg.n_down;
    const long HW = (long)H * W;
    ALLOC(bmap, HW * C0);
    ALLOC(y, HW * C0);
    float* cur = const_cast<float*>(skip_at(d, skip_mem, 0, H, W));
    if (!dry) {
        hipLaunchKernelGGL(bias_rows_kernel, dim3(grid_for(HW * C0)), dim3(256), 0, st, d->first_bias, HW, C0, bmap);
        DAWN_LAUNCH_CHECK();
        CK(dawn_init_conv_x_ex(img3, HW, d->first_w3, bmap, 1, H, W, C0, y, stream));
        CK(dawn_affine_act(y, C0, d->first_a, d->first_b, 1, cur, HW, C0, stream));
    }
    A.free(y);
    A.free(bmap);
    int Hc = H, Wc = W;
    for (int i = 0; i < n; ++i) {
        const Conv3& c = d->downs[i];
        ALLOC(z, (long)Hc * Wc * c.N);
        float* nxt = const_cast<float*>(skip_at(d, skip_mem, i + 1, H, W));
        CK(conv3(c, cur, 1, Hc, Wc, nullptr, z, dry, stream));
        if (!dry) CK(dawn_bn_relu_pool2(z, c.a, c.b, nxt, 1, Hc, Wc, c.N, stream));
        A.free(z);
        Hc /= 2; Wc /= 2;
        cur = nxt;
    }
    if (fea_out && !dry) {
        const int Cb = d->cfg.widths[n];
        hipLaunchKernelGGL(hwc_to_chw_kernel, dim3(grid_for((long)Hc * Wc * Cb)), dim3(256), 0, st, cur, (long)Hc * Wc, Cb, fea_out);
        DAWN_LAUNCH_CHECK();
    }
    return 0;
}

struct Outputs {
    float *out_vid, *warped_vid;
    long out_plane;
    unsigned char* frames;
    double m[3];
    int bgr;
    unsigned char* yuv;               // I420 frames (T, 3HW/2): the only output when set
};

// FlowDecoder._decode_frames for the frames [t0, t0 + n) of the clip.  g = grid planes of the chunk (gp floats apart); cf = the
// chunk's occlusion map, or NULL: formed here from the latent's third plane `lat2`.
int decode_chunk(const dawn_decoder* d, DawnArena& A, int H, int W, int n, int t0, int h, int w, const float* img3, const void* skip_mem,
                 const float* g, long gp, const float* cf, const float* lat2, const Outputs& o, bool dry, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    const int nd = d->cfg.n_down;
    float* cfbuf = nullptr;
    if (!cf) {
        ALLOC(buf, (size_t)n * h * w);
        cfbuf = buf;
        if (!dry) {
            hipLaunchKernelGGL(conf_of_latent_kernel, dim3(grid_for((long)n * h * w)), dim3(256), 0, st, lat2, (long)n * h * w, cfbuf);
            DAWN_LAUNCH_CHECK();
        }
        cf = cfbuf;
    }
    int Hc = H >> nd, Wc = W >> nd;
    const int Cb = d->cfg.widths[nd];
    const long rb = (long)n * Hc * Wc;
    ALLOC(x, rb * Cb);
    if (!dry) CK(dawn_warp_blend(skip_at(d, skip_mem, nd, H, W), Hc, Wc, Cb, g, gp, cf, n, h, w, nullptr, nullptr, nullptr, 0, x, stream));
    for (const Bott& b : d->bott) {
        ALLOC(y, rb * Cb);
        if (!dry) CK(dawn_affine_act(x, Cb, b.a1, b.b1, 1, y, rb, Cb, stream));
        ALLOC(z, rb * Cb);
        CK(conv3(b.c1, y, n, Hc, Wc, nullptr, z, dry, stream));
        A.free(y);
        ALLOC(y2, rb * Cb);
        if (!dry) CK(dawn_affine_act(z, Cb, b.a2, b.b2, 1, y2, rb, Cb, stream));
        A.free(z);
        ALLOC(xn, rb * Cb);
        CK(conv3(b.c2, y2, n, Hc, Wc, x, xn, dry, stream));
        A.free(y2);
        A.free(x);
        x = xn;
    }
    float* prev = x;
    const float *pa = nullptr, *pb = nullptr;
    for (int i = 0; i < nd; ++i) {
        const Conv3& up = d->ups[i];
        ALLOC(u, (long)n * Hc * Wc * 4 * up.Cin);
        if (!dry) CK(dawn_warp_blend(skip_at(d, skip_mem, nd - i, H, W), Hc, Wc, up.Cin, g, gp, cf, n, h, w, prev, pa, pb, 1, u, stream));
        A.free(prev);
        Hc *= 2; Wc *= 2;
        ALLOC(pn, (long)n * Hc * Wc * up.N);
        CK(conv3(up, u, n, Hc, Wc, nullptr, pn, dry, stream));
        A.free(u);
        prev = pn;
        pa = up.a; pb = up.b;
    }
    const int C0 = d->cfg.widths[0];
    ALLOC(xf, (long)n * H * W * C0);
    if (!dry) CK(dawn_warp_blend(skip_at(d, skip_mem, 0, H, W), H, W, C0, g, gp, cf, n, h, w, prev, pa, pb, 0, xf, stream));
    A.free(prev);
    if (!dry) {
        const long fpix = (long)H * W;
        if (o.yuv) {
            CK(dawn_final_conv_blend_yuv420(xf, n, H, W, C0, d->final_w7, d->final_bias, img3, g, gp, cf, h, w, o.m[0], o.m[1], o.m[2],
                                            o.yuv + (long)t0 * (fpix / 2 * 3), stream));
        } else if (o.out_vid) {
            float* ov = o.out_vid + (long)t0 * fpix;
            CK(dawn_final_conv_blend(xf, n, H, W, C0, d->final_w7, d->final_bias, img3, g, gp, cf, h, w, ov,
                                     o.warped_vid + (long)t0 * fpix, o.out_plane, stream));
            if (o.frames)
                CK(dawn_frames_to_u8(ov, o.out_plane, (long)n * fpix, o.m[0], o.m[1], o.m[2], o.bgr, o.frames + (long)t0 * fpix * 3, stream));
        } else {
            CK(dawn_final_conv_blend_u8(xf, n, H, W, C0, d->final_w7, d->final_bias, img3, g, gp, cf, h, w, o.m[0], o.m[1], o.m[2],
                                        o.bgr, o.frames + (long)t0 * fpix * 3, stream));
        }
    }
    A.free(xf);
    if (cfbuf) A.free(cfbuf);
    return 0;
}

int decode_clip(dawn_decoder* d, const char* who, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                const float* grid, long grid_plane, const float* conf, const float* lat2, int chunk, float* out_vid, float* warped_vid,
                long out_plane, unsigned char* frames_u8, const double* mean3, int bgr, void* workspace, size_t workspace_bytes,
                void* stream, unsigned char* frames_yuv = nullptr, bool yuv = false) {
    char m[200];
    if (!d) return dawn_set_error_msg(-233, "dawn_decode_clip: NULL decoder");
    CK(bad_size(d, H, W, who));
    if (yuv && (H % 2 != 0 || W % 4 != 0 || !frames_yuv || ((uintptr_t)frames_yuv & 3) != 0)) {
        snprintf(m, sizeof m, "%s: frames_yuv420 needs an even H, W %% 4 == 0 and a non-NULL 4-byte aligned buffer (H = %d, W = %d)", who, H, W);
        return dawn_set_error_msg(-240, m);
    }
    if ((out_vid == nullptr) != (warped_vid == nullptr)) {
        snprintf(m, sizeof m, "%s: out_vid and warped_vid come as a pair", who);
        return dawn_set_error_msg(-234, m);
    }
    if (!out_vid && !frames_u8 && !yuv) {
        snprintf(m, sizeof m, "%s: no output requested (out_vid / warped_vid and frames_u8 are all NULL)", who);
        return dawn_set_error_msg(-235, m);
    }
    if (frames_u8 && (W % 4 != 0 || ((uintptr_t)frames_u8 & 3) != 0)) {
        snprintf(m, sizeof m, "%s: frames_u8 needs W %% 4 == 0 and a 4-byte aligned buffer", who);
        return dawn_set_error_msg(-236, m);
    }
    if (chunk <= 0 || T < 0 || h <= 0 || w <= 0 || h > H || w > W || !grid || !img3 || !skip_mem || (out_vid && out_plane % 4 != 0)) {
        snprintf(m, sizeof m, "%s: bad argument (chunk, T, a latent larger than the image, NULL input, or out_plane %% 4 != 0)", who);
        return dawn_set_error_msg(-237, m);
    }
    const size_t need = dawn_decoder_workspace_bytes(d, H, W, chunk < T ? chunk : (T > 0 ? T : 1));
    if (workspace_bytes < need || !workspace) return refuse_workspace(-232, who, workspace_bytes, need, "dawn_decoder_workspace_bytes");
    Outputs o = {out_vid, warped_vid, out_plane, frames_u8, {0.0, 0.0, 0.0}, bgr ? 1 : 0, frames_yuv};
    if (mean3) { o.m[0] = mean3[0]; o.m[1] = mean3[1]; o.m[2] = mean3[2]; }
    for (int t0 = 0; t0 < T; t0 += chunk) {
        const int n = T - t0 < chunk ? T - t0 : chunk;
        const long off = (long)t0 * h * w;
        DawnArena A;
        A.reset(workspace, workspace_bytes, false);
        CK(decode_chunk(d, A, H, W, n, t0, h, w, img3, skip_mem, grid + off, grid_plane, conf ? conf + off : nullptr,
                        lat2 ? lat2 + off : nullptr, o, false, stream));
    }
    return 0;
}

}  // namespace

extern "C" int dawn_decoder_create(const dawn_decoder_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_decoder** out) {
    if (!cfg || !out || (!weights && n_weights > 0)) return dawn_set_error_msg(-238, "dawn_decoder_create: NULL argument");
    if (cfg->n_down < 0 || cfg->n_down > 7 || cfg->n_bottleneck < 0)
        return dawn_set_error_msg(-239, "dawn_decoder_create: n_down must be 0..7 and n_bottleneck >= 0");
    for (int i = 0; i <= cfg->n_down; ++i)
        if (cfg->widths[i] <= 0 || cfg->widths[i] % 8 != 0) {
            char m[120];
            snprintf(m, sizeof m, "dawn_decoder_create: widths[%d] = %d must be a positive multiple of 8", i, cfg->widths[i]);
            return dawn_set_error_msg(-239, m);
        }
    dawn_decoder* d = new dawn_decoder();
    d->cfg = *cfg;
    DawnWeights Wt(weights, n_weights, "dawn_decoder_create: missing packed weight", -230);
    auto F = [&](const std::string& n) { return Wt.getf(n); };
    d->first_w3 = F("first_w3"); d->first_bias = F("first_bias"); d->first_a = F("first.a"); d->first_b = F("first.b");
    d->final_w7 = F("final_w7"); d->final_bias = F("final_bias");
    const int n = cfg->n_down;
    d->downs.resize(n); d->ups.resize(n); d->bott.resize(cfg->n_bottleneck);
    for (int i = 0; i < n; ++i) {
        const std::string s = std::to_string(i);
        load_conv(Wt, "downs." + s + ".", cfg->widths[i], cfg->widths[i + 1], true, d->downs[i]);
        load_conv(Wt, "ups." + s + ".", cfg->widths[n - i], cfg->widths[n - i - 1], true, d->ups[i]);
    }
    const int Cb = cfg->widths[n];
    for (int i = 0; i < cfg->n_bottleneck; ++i) {
        const std::string p = "bott." + std::to_string(i) + ".";
        Bott& b = d->bott[i];
        b.a1 = F(p + "a1"); b.b1 = F(p + "b1"); b.a2 = F(p + "a2"); b.b2 = F(p + "b2");
        load_conv(Wt, p + "c1.", Cb, Cb, false, b.c1);
        load_conv(Wt, p + "c2.", Cb, Cb, false, b.c2);
    }
    if (!Wt.ok()) {
        delete d;
        return Wt.code();
    }
    *out = d;
    return 0;
}

extern "C" void dawn_decoder_destroy(dawn_decoder* dec) { delete dec; }

extern "C" size_t dawn_decoder_skip_bytes(dawn_decoder* dec, int H, int W) {
    if (!dec || bad_size(dec, H, W, "dawn_decoder_skip_bytes")) return 0;
    size_t b = 0;
    for (int i = 0; i <= dec->cfg.n_down; ++i) b += a256(skip_floats(dec, i, H, W) * 4);
    return b;
}

extern "C" size_t dawn_decoder_workspace_bytes(dawn_decoder* dec, int H, int W, int chunk) {
    if (!dec || chunk <= 0 || bad_size(dec, H, W, "dawn_decoder_workspace_bytes")) return 0;
    DawnArena dry;                 // a dry pass of the launch sequence on an arena of its own: the query leaves the decoder untouched
    dry.reset(nullptr, 0, true);
    if (encode(dec, dry, H, W, nullptr, nullptr, nullptr, true, nullptr)) return 0;
    const size_t need = dry.high;
    dry.reset(nullptr, 0, true);
    Outputs o = {};
    if (decode_chunk(dec, dry, H, W, chunk, 0, H, W, nullptr, nullptr, nullptr, 0, nullptr, nullptr, o, true, nullptr)) return 0;
    return need > dry.high ? need : dry.high;
}

extern "C" int dawn_decoder_encode(dawn_decoder* dec, int H, int W, const float* img3, void* skip_mem, size_t skip_bytes,
                                   float* fea_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dec || !img3 || !skip_mem) return dawn_set_error_msg(-238, "dawn_decoder_encode: NULL argument");
    CK(bad_size(dec, H, W, "dawn_decoder_encode"));
    if (skip_bytes < dawn_decoder_skip_bytes(dec, H, W))
        return dawn_set_error_msg(-232, "dawn_decoder_encode: skip memory too small (dawn_decoder_skip_bytes)");
    DawnArena dry;
    dry.reset(nullptr, 0, true);
    CK(encode(dec, dry, H, W, nullptr, nullptr, nullptr, true, nullptr));
    if (!workspace || workspace_bytes < dry.high)
        return dawn_set_error_msg(-232, "dawn_decoder_encode: workspace too small (dawn_decoder_workspace_bytes)");
    DawnArena A;
    A.reset(workspace, workspace_bytes, false);
    return encode(dec, A, H, W, img3, skip_mem, fea_out, false, stream);
}

extern "C" int dawn_decode_clip(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                                const float* latent, long latent_plane, int chunk, float* out_vid, float* warped_vid, long out_plane,
                                unsigned char* frames_u8, const double* mean3, int bgr, void* workspace, size_t workspace_bytes,
                                void* stream) {
    return decode_clip(dec, "dawn_decode_clip", H, W, T, h, w, img3, skip_mem, latent, latent_plane, nullptr,
                       latent ? latent + 2 * latent_plane : nullptr, chunk, out_vid, warped_vid, out_plane, frames_u8, mean3, bgr,
                       workspace, workspace_bytes, stream);
}

extern "C" int dawn_decode_clip_conf(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                                     const float* grid, long grid_plane, const float* conf, int chunk, float* out_vid,
                                     float* warped_vid, long out_plane, unsigned char* frames_u8, const double* mean3, int bgr,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    if (!conf) return dawn_set_error_msg(-238, "dawn_decode_clip_conf: NULL conf");
    return decode_clip(dec, "dawn_decode_clip_conf", H, W, T, h, w, img3, skip_mem, grid, grid_plane, conf, nullptr, chunk, out_vid,
                       warped_vid, out_plane, frames_u8, mean3, bgr, workspace, workspace_bytes, stream);
}

extern "C" int dawn_decode_clip_yuv420(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3, const void* skip_mem,
                                       const float* latent, long latent_plane, int chunk, unsigned char* frames_yuv420,
                                       const double* mean3, void* workspace, size_t workspace_bytes, void* stream) {
    return decode_clip(dec, "dawn_decode_clip_yuv420", H, W, T, h, w, img3, skip_mem, latent, latent_plane, nullptr,
                       latent ? latent + 2 * latent_plane : nullptr, chunk, nullptr, nullptr, 0, nullptr, mean3, 0, workspace,
                       workspace_bytes, stream, frames_yuv420, true);
}

extern "C" int dawn_decode_clip_conf_yuv420(dawn_decoder* dec, int H, int W, int T, int h, int w, const float* img3,
                                            const void* skip_mem, const float* grid, long grid_plane, const float* conf, int chunk,
                                            unsigned char* frames_yuv420, const double* mean3, void* workspace, size_t workspace_bytes,
                                            void* stream) {
    if (!conf) return dawn_set_error_msg(-238, "dawn_decode_clip_conf_yuv420: NULL conf");
    return decode_clip(dec, "dawn_decode_clip_conf_yuv420", H, W, T, h, w, img3, skip_mem, grid, grid_plane, conf, nullptr, chunk, nullptr,
                       nullptr, 0, nullptr, mean3, 0, workspace, workspace_bytes, stream, frames_yuv420, true);
}
