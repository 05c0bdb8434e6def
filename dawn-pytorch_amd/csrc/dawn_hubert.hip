// C-side HuBERT audio-feature stage (SURVEY 8f N3 as a whole path): dawn_hubert_*.  The launch sequence of
// dawn-pytorch_amd/hubert.py -- HubertFeatures.encode (transformers.HubertModel.forward on one segment) and
// get_hubert_from_16k_speech / interpolate_25fps (UVG:433-501, 229-247) -- issued through the per-op entry points of this library, so
// that a non-Python host turns 16 kHz samples into the audio rows of `cond` with nothing but this .so.  Two differences from the
// Python default path, both in the positional block: it is the one dawn_hubert_pos_conv launch (no padded copy, no per-group
// GEMMs, no add_act), and segments are encoded straight to their rows of the hidden block (no concatenation, no pad / cut copy).
//
// Conventions as in dawn_decoder.hip: no allocation on the device (the caller provides the workspace, sized by a dry pass of the same
// code), every launch on the caller's stream, no synchronisation, int return codes + dawn_last_error().  One kernel lives here: the
// interpolation positions (numpy's linspace).
#include "dawn_host.h"

#include <vector>

namespace {

const long SEG = 320000, SEG_CTX = 80, KERNEL = 400, STRIDE = 320;     // UVG:466-470: clip_length, kernel - stride, kernel, stride

// np.linspace(0, last, m): arange(m) * step, the last entry `last` exactly
__global__ __launch_bounds__(256) void linspace_kernel(double step, double last, long m, double* __restrict__ xi) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < m) xi[i] = i == m - 1 && m > 1 ? last : (double)i * step;
}

struct ConvL { const float *w, *b, *g, *be; };
struct Layer { const float *ln1g, *ln1b, *wqkv, *bqkv, *wo, *bo, *ln2g, *ln2b, *w1, *b1, *w2, *b2; };

}  // namespace

struct dawn_hubert {
    dawn_hubert_cfg cfg;
    std::vector<ConvL> conv;
    const float *fp_g = nullptr, *fp_b = nullptr, *fp_w = nullptr, *fp_bias = nullptr, *pos_w = nullptr, *pos_b = nullptr,
                *enc_g = nullptr, *enc_b = nullptr;
    std::vector<Layer> layers;
};                                // immutable after dawn_hubert_create: every call sub-allocates its workspace with an arena of its own

namespace {

// a Linear / 1-D conv over (time, channel) rows through dawn_conv_gemm, as HipOps.conv_gemm fills the descriptor
int gemm(const float* x, int Cin, long Ti, long To, int KW, int stride, const float* w, const float* bias, int N, const float* res,
         float* out, void* stream) {
    dawn_conv_desc d = {};
    d.in0 = x; d.C0 = Cin; d.ld0 = Cin;
    d.F = 1; d.Hi = 1; d.Wi = (int)Ti; d.Ho = 1; d.Wo = (int)To;
    d.KH = 1; d.KW = KW; d.stride = stride; d.pad = 0; d.mode = 0;
    d.w = w; d.bias = bias; d.N = N;
    d.res = res; d.ld_res = res ? N : 0;
    d.out = out; d.ld_out = N;
    return dawn_conv_gemm(&d, stream);
}

#define ALLOC(ptr, floats) DAWN_ALLOC(A, ptr, floats, -252, "dawn_hubert: workspace too small (dawn_hubert_workspace_bytes)")

long conv_frames(const dawn_hubert_cfg& c, long n) {
    long T = n;
    for (int i = 0; i < c.n_conv; ++i) {
        if (T < c.conv_k[i]) return 0;
        T = (T - c.conv_k[i]) / c.conv_stride[i] + 1;
    }
    return T;
}

// HubertFeatures.encode of n samples; the final LayerNorm writes the first `keep` rows only.  dry: sizes the workspace, launches nothing.
int encode(const dawn_hubert* h, DawnArena& A, const float* x, long n, float* out, long keep, bool dry, void* stream) {
    const dawn_hubert_cfg& c = h->cfg;
    const int D = c.conv_dim, E = c.hidden;
    long T = (n - c.conv_k[0]) / c.conv_stride[0] + 1;
    ALLOC(y, T * D);
    if (!dry) CK(dawn_hubert_conv0(x, n, h->conv[0].w, h->conv[0].b, D, c.conv_k[0], c.conv_stride[0], y, stream));
    ALLOC(cur, T * D);
    if (!dry) CK(dawn_ln_affine_act(y, T, D, h->conv[0].g, h->conv[0].be, c.eps, 2, cur, stream));
    A.free(y);
    for (int i = 1; i < c.n_conv; ++i) {
        const long To = (T - c.conv_k[i]) / c.conv_stride[i] + 1;
        ALLOC(z, To * D);
        if (!dry) CK(gemm(cur, D, T, To, c.conv_k[i], c.conv_stride[i], h->conv[i].w, h->conv[i].b, D, nullptr, z, stream));
        A.free(cur);
        ALLOC(nx, To * D);
        if (!dry) CK(dawn_ln_affine_act(z, To, D, h->conv[i].g, h->conv[i].be, c.eps, 2, nx, stream));
        A.free(z);
        cur = nx;
        T = To;
    }
    ALLOC(fl, T * D);
    if (!dry) CK(dawn_ln_affine_act(cur, T, D, h->fp_g, h->fp_b, c.eps, 0, fl, stream));
    A.free(cur);
    ALLOC(hid0, T * E);
    if (!dry) CK(gemm(fl, D, T, T, 1, 1, h->fp_w, h->fp_bias, E, nullptr, hid0, stream));
    A.free(fl);
    ALLOC(hid, T * E);
    if (!dry) CK(dawn_hubert_pos_conv(hid0, (int)T, E, c.pos_groups, c.pos_k, h->pos_w, h->pos_b, hid, stream));
    A.free(hid0);
    for (const Layer& ly : h->layers) {
        ALLOC(l1, T * E);
        if (!dry) CK(dawn_ln_affine_act(hid, T, E, ly.ln1g, ly.ln1b, c.eps, 0, l1, stream));
        ALLOC(qkv, T * 3 * E);
        if (!dry) CK(gemm(l1, E, T, T, 1, 1, ly.wqkv, ly.bqkv, 3 * E, nullptr, qkv, stream));
        A.free(l1);
        ALLOC(att, T * E);
        if (!dry) CK(dawn_attn64(qkv, (int)T, c.heads, att, stream));
        A.free(qkv);
        ALLOC(h2, T * E);
        if (!dry) CK(gemm(att, E, T, T, 1, 1, ly.wo, ly.bo, E, hid, h2, stream));
        A.free(att);
        A.free(hid);
        ALLOC(l2, T * E);
        if (!dry) CK(dawn_ln_affine_act(h2, T, E, ly.ln2g, ly.ln2b, c.eps, 0, l2, stream));
        ALLOC(f, T * c.intermediate);
        if (!dry) {
            CK(gemm(l2, E, T, T, 1, 1, ly.w1, ly.b1, c.intermediate, nullptr, f, stream));
            CK(dawn_add_act(nullptr, f, 2, T * c.intermediate, f, stream));
        }
        A.free(l2);
        ALLOC(h3, T * E);
        if (!dry) CK(gemm(f, c.intermediate, T, T, 1, 1, ly.w2, ly.b2, E, h2, h3, stream));
        A.free(f);
        A.free(h2);
        hid = h3;
    }
    if (!dry) CK(dawn_ln_affine_act(hid, keep < T ? keep : T, E, h->enc_g, h->enc_b, c.eps, 0, out, stream));
    A.free(hid);
    return 0;
}

size_t encode_bytes(const dawn_hubert* h, long n) {
    if (conv_frames(h->cfg, n) <= 0) return 0;
    DawnArena dry;
    dry.reset(nullptr, 0, true);
    if (encode(h, dry, nullptr, n, nullptr, 0, true, nullptr)) return 0;
    return dry.high;
}

struct Plan {
    std::vector<long> seg;            // (first sample, samples, rows) per segment
    long rows = 0, expected_T = 0, num_frames = 0;
};

int make_plan(const dawn_hubert* h, long n, Plan& p, const char* who) {
    char m[200];
    if (n < KERNEL) {
        snprintf(m, sizeof m, "%s: %ld samples, at least %ld needed", who, n, KERNEL);
        return dawn_set_error_msg(-253, m);
    }
    const long iters = n / SEG;
    p.expected_T = (n - SEG_CTX) / STRIDE;
    p.num_frames = (long)((double)n / 16000.0 * 25.0);
    for (long i = 0; i <= iters; ++i) {
        const long start = SEG * i;
        const long len = i < iters ? (n - start < SEG + SEG_CTX ? n - start : SEG + SEG_CTX) : n - start;
        if (i == iters && len < KERNEL) break;          // the remainder runs only if it holds one kernel
        const long rows = conv_frames(h->cfg, len);
        if (rows <= 0) {
            snprintf(m, sizeof m, "%s: a segment of %ld samples is shorter than the conv stack needs", who, len);
            return dawn_set_error_msg(-253, m);
        }
        p.seg.insert(p.seg.end(), {start, len, rows});
        p.rows += rows;
    }
    if (p.rows - p.expected_T > 1 || p.expected_T - p.rows > 1) {
        snprintf(m, sizeof m, "%s: %ld rows encoded, %ld expected (they may differ by one)", who, p.rows, p.expected_T);
        return dawn_set_error_msg(-254, m);
    }
    return 0;
}

// workspace of dawn_hubert_features: statistics, normalised samples, hidden block, positions, then the arena of one segment
struct FeatLayout { size_t stats, iv, hid, xi, arena, total; };

int feat_layout(const dawn_hubert* h, long n, const Plan& p, FeatLayout& L) {
    size_t enc = 0;
    for (size_t s = 0; s < p.seg.size(); s += 3) {
        const size_t b = encode_bytes(h, p.seg[s + 1]);
        if (b == 0) return dawn_set_error_msg(-252, "dawn_hubert: cannot size the workspace of a segment");
        if (b > enc) enc = b;
    }
    L.stats = 0;
    L.iv = 256;
    L.hid = L.iv + a256((size_t)n * 4);
    L.xi = L.hid + a256((size_t)(p.expected_T > 0 ? p.expected_T : 1) * h->cfg.hidden * 4);
    L.arena = L.xi + a256((size_t)(p.num_frames > 0 ? p.num_frames : 1) * 8);
    L.total = L.arena + enc;
    return 0;
}

}  // namespace

extern "C" int dawn_hubert_create(const dawn_hubert_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_hubert** out) {
    if (!cfg || !out || (!weights && n_weights > 0)) return dawn_set_error_msg(-251, "dawn_hubert_create: NULL argument");
    char m[200];
    if (cfg->n_conv < 1 || cfg->n_conv > 8 || cfg->n_layers < 0 || cfg->conv_dim <= 0 || cfg->conv_dim % 4 != 0 ||
        cfg->intermediate <= 0 || cfg->intermediate % 4 != 0 || cfg->pos_k < 1 || cfg->pos_groups < 1 || cfg->heads < 1)
        return dawn_set_error_msg(-251, "dawn_hubert_create: n_conv must be 1..8, conv_dim and intermediate positive multiples of 4, "
                                        "n_layers >= 0, heads, pos_k and pos_groups >= 1");
    for (int i = 0; i < cfg->n_conv; ++i)
        if (cfg->conv_k[i] < 1 || cfg->conv_stride[i] < 1) {
            snprintf(m, sizeof m, "dawn_hubert_create: conv_k[%d] = %d, conv_stride[%d] = %d must be positive", i, cfg->conv_k[i], i,
                     cfg->conv_stride[i]);
            return dawn_set_error_msg(-251, m);
        }
    if (cfg->hidden != 64 * cfg->heads) {
        snprintf(m, sizeof m, "dawn_hubert_create: hidden = %d is not 64 * heads = %d (the attention kernel has heads of 64)", cfg->hidden,
                 64 * cfg->heads);
        return dawn_set_error_msg(-251, m);
    }
    if (cfg->hidden % cfg->pos_groups != 0 || (cfg->hidden / cfg->pos_groups) % 16 != 0 ||
        (size_t)(63 + cfg->pos_k) * (cfg->hidden / cfg->pos_groups + 2) * 4 > 65536) {
        snprintf(m, sizeof m, "dawn_hubert_create: positional conv needs gw = hidden / pos_groups with gw %% 16 == 0 and (63 + pos_k) * "
                              "(gw + 2) floats within 64 KB (hidden = %d, pos_groups = %d, pos_k = %d)", cfg->hidden, cfg->pos_groups, cfg->pos_k);
        return dawn_set_error_msg(-251, m);
    }
    dawn_hubert* h = new dawn_hubert();
    h->cfg = *cfg;
    DawnWeights Wt(weights, n_weights, "dawn_hubert_create: missing packed weight", -250);
    auto F = [&](const std::string& n) { return Wt.getf(n); };
    h->conv.resize(cfg->n_conv);
    for (int i = 0; i < cfg->n_conv; ++i) {
        const std::string p = "conv." + std::to_string(i) + ".";
        h->conv[i] = {F(p + "w"), (const float*)Wt.opt(p + "b"), F(p + "g"), F(p + "be")};
    }
    h->fp_g = F("fp.g"); h->fp_b = F("fp.b"); h->fp_w = F("fp.w"); h->fp_bias = F("fp.bias");
    h->pos_w = F("pos.w"); h->pos_b = F("pos.b");
    h->layers.resize(cfg->n_layers);
    for (int i = 0; i < cfg->n_layers; ++i) {
        const std::string p = "layers." + std::to_string(i) + ".";
        h->layers[i] = {F(p + "ln1.g"), F(p + "ln1.b"), F(p + "wqkv"), F(p + "bqkv"), F(p + "wo"), F(p + "bo"),
                        F(p + "ln2.g"), F(p + "ln2.b"), F(p + "w1"), F(p + "b1"), F(p + "w2"), F(p + "b2")};
    }
    h->enc_g = F("enc_ln.g"); h->enc_b = F("enc_ln.b");
    if (!Wt.ok()) {
        delete h;
        return Wt.code();
    }
    *out = h;
    return 0;
}

extern "C" void dawn_hubert_destroy(dawn_hubert* hub) { delete hub; }

extern "C" long dawn_hubert_conv_frames(const dawn_hubert* hub, long n_samples) {
    return hub && n_samples > 0 ? conv_frames(hub->cfg, n_samples) : 0;
}

extern "C" int dawn_hubert_segments(const dawn_hubert* hub, long n_samples, long* start_len_rows, int max_segments, long* expected_T,
                                    long* num_frames) {
    if (!hub) return dawn_set_error_msg(-251, "dawn_hubert_segments: NULL handle");
    Plan p;
    CK(make_plan(hub, n_samples, p, "dawn_hubert_segments"));
    const int ns = (int)(p.seg.size() / 3);
    if (ns > max_segments || (ns > 0 && !start_len_rows)) {
        char m[120];
        snprintf(m, sizeof m, "dawn_hubert_segments: %d segments, room for %d", ns, start_len_rows ? max_segments : 0);
        return dawn_set_error_msg(-255, m);
    }
    for (size_t i = 0; i < p.seg.size(); ++i) start_len_rows[i] = p.seg[i];
    if (expected_T) *expected_T = p.expected_T;
    if (num_frames) *num_frames = p.num_frames;
    return ns;
}

extern "C" size_t dawn_hubert_workspace_bytes(const dawn_hubert* hub, long n_samples) {
    if (!hub) return 0;
    Plan p;
    FeatLayout L;
    if (make_plan(hub, n_samples, p, "dawn_hubert_workspace_bytes") || feat_layout(hub, n_samples, p, L)) return 0;
    const size_t enc = encode_bytes(hub, n_samples < SEG + SEG_CTX ? n_samples : SEG + SEG_CTX);
    return L.total > enc ? L.total : enc;
}

extern "C" int dawn_hubert_encode(dawn_hubert* hub, const float* input_values, long n, float* hidden_out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (!hub || !input_values || !hidden_out) return dawn_set_error_msg(-251, "dawn_hubert_encode: NULL argument");
    char m[200];
    if (n > SEG + SEG_CTX || conv_frames(hub->cfg, n) <= 0) {
        snprintf(m, sizeof m, "dawn_hubert_encode: %ld samples; one segment holds what the conv stack needs at least and %ld at most "
                              "(dawn_hubert_features splits longer audio)", n, SEG + SEG_CTX);
        return dawn_set_error_msg(-253, m);
    }
    const size_t need = encode_bytes(hub, n);
    if (!workspace || workspace_bytes < need || need == 0)
        return refuse_workspace(-252, "dawn_hubert_encode", workspace_bytes, need, "dawn_hubert_workspace_bytes");
    DawnArena A;
    A.reset(workspace, workspace_bytes, false);
    return encode(hub, A, input_values, n, hidden_out, conv_frames(hub->cfg, n), false, stream);
}

extern "C" int dawn_hubert_features(dawn_hubert* hub, const float* speech, long n, float* hidden_out, float* features_out,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!hub || !speech || !features_out) return dawn_set_error_msg(-251, "dawn_hubert_features: NULL argument");
    char m[200];
    Plan p;
    FeatLayout L;
    CK(make_plan(hub, n, p, "dawn_hubert_features"));
    if (p.num_frames < 1 || p.expected_T < 2) {
        snprintf(m, sizeof m, "dawn_hubert_features: %ld samples give %ld frames at 25 fps from %ld feature rows (at least 1 from 2 needed)",
                 n, p.num_frames, p.expected_T);
        return dawn_set_error_msg(-253, m);
    }
    CK(feat_layout(hub, n, p, L));
    if (!workspace || workspace_bytes < L.total)
        return refuse_workspace(-252, "dawn_hubert_features", workspace_bytes, L.total, "dawn_hubert_workspace_bytes");
    const hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const int E = hub->cfg.hidden;
    float* iv = (float*)(ws + L.iv);
    float* hid = hidden_out ? hidden_out : (float*)(ws + L.hid);
    double* xi = (double*)(ws + L.xi);
    CK(dawn_wave_normalize(speech, n, (double*)(ws + L.stats), iv, stream));
    long row = 0;
    for (size_t s = 0; s < p.seg.size(); s += 3) {
        DawnArena A;
        A.reset(ws + L.arena, workspace_bytes - L.arena, false);
        // the surplus row (at most one, the last) is never computed: the final LayerNorm stops at expected_T
        CK(encode(hub, A, iv + p.seg[s], p.seg[s + 1], hid + row * E, p.expected_T - row, false, stream));
        row += p.seg[s + 2];
    }
    if (row < p.expected_T && hipMemsetAsync(hid + row * E, 0, (size_t)(p.expected_T - row) * E * 4, st) != hipSuccess)
        return dawn_set_error(hipGetLastError(), __FILE__, __LINE__);
    const double last = (double)(p.expected_T - 1);
    const double step = p.num_frames > 1 ? last / (double)(p.num_frames - 1) : 0.0;
    hipLaunchKernelGGL(linspace_kernel, dim3(dawn_cdiv(p.num_frames, 256)), dim3(256), 0, st, step, last, p.num_frames, xi);
    DAWN_LAUNCH_CHECK();
    return dawn_interp_linear(hid, p.expected_T, E, xi, p.num_frames, features_out, stream);
}
