// C-side PBnet pose / blink stage (SURVEY 8f N4 as a whole path): dawn_pbnet_*, dawn_pose_blink_stage.  The launch sequence of
// dawn-pytorch_amd/pbnet.py -- PoseBlinkGenerator._decode_one (Decoder.forward for one sample, all frames valid) and pose_blink_stage
// (UVG:252-302) -- issued through the per-op entry points of this library, so that a non-Python host produces the pose and blink columns
// of `cond` with nothing but this .so.  Differences from the Python default path:
//   * attention is dawn_attn_win32: the eval-mode window is the kernel's key range, the relative-position bias one (heads, 2 win + 1)
//     table per generator.  No (heads, T, T) table exists, so memory and time are linear in T;
//   * the rotary tables are filled on the device;
//   * the decoder memory is projected to every layer's cross-attention K and V in one dawn_linear against the concatenated
//     weight image "mem_kv.w" (every output element of dawn_linear is one wave's own sum: the bits do not change);
//   * the audio embedding is written straight into its columns of the ztimelinear input.
//
// Conventions as in dawn_hubert.hip: no allocation on the device, every launch on the caller's stream, no synchronisation, int return
// codes + dawn_last_error().  The workspace is a fixed list of per-frame buffers, so its size is exactly linear in T.
#include "dawn_host.h"

#include <vector>

namespace {

// normalisation of the pose rows (UVG:95-98): yaw, pitch, roll in degrees, scale, tx, ty
const float POSE_MAX[6] = {90.f, 90.f, 90.f, 1.f, 720.f, 1080.f};
const float POSE_MIN[6] = {-90.f, -90.f, -90.f, 0.f, 0.f, 0.f};

struct Layer {
    const float *sa_qkv, *sa_out, *ln1w, *ln1b, *ca_q, *ca_out, *ln2w, *ln2b, *f1w, *f1b, *f2w, *f2b, *ln3w, *ln3b;
};

// cos / sin (T, nrot) of angle = t * freqs[p]: the product in fp32 like `arange(T)[:, None] * freqs`, cos / sin evaluated in fp64 and
// rounded once (dawn_rotary_tables does the same for the UNet's fixed 16 frequencies)
__global__ __launch_bounds__(256) void pb_rotary_kernel(const float* __restrict__ freqs, long T, int nrot, float* __restrict__ c,
                                                        float* __restrict__ s) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * nrot) return;
    const float ang = __fmul_rn((float)(i / nrot), freqs[i % nrot]);
    c[i] = (float)cos((double)ang);
    s[i] = (float)sin((double)ang);
}

// out[t][0:nr] = row[0:nr] and, where z is given, out[t][nr:nr + nz] = z[t][0:nz], for t < T: the [x_ref | z | .] columns of the
// ztimelinear input (the audio embedding writes the rest) and the broadcast of init_proj's bias
__global__ __launch_bounds__(256) void pb_rows_kernel(const float* __restrict__ row, int nr, const float* __restrict__ z, int nz, long T,
                                                      float* __restrict__ out, int ld) {
    const int w = nr + nz;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * w) return;
    const long t = i / w;
    const int c = (int)(i - t * w);
    out[t * ld + c] = c < nr ? row[c] : z[t * nz + (c - nr)];
}

struct X0 { float p[6], b[2]; };
__global__ void pb_x0_kernel(X0 v, float* __restrict__ x0p, float* __restrict__ x0b) {
    const int i = threadIdx.x;
    if (i < 6) x0p[i] = v.p[i];
    else if (i < 8) x0b[i - 6] = v.b[i - 6];
}

// in place: pose = (pose + ip) * (max - min) + min, blink = blink + ib, each operation rounded on its own (pose_blink_stage's order)
struct Fin { float ip[6], range[6], mn[6], ib[2]; };
__global__ __launch_bounds__(256) void pb_finish_kernel(Fin f, long T, float* __restrict__ pose, int ldp, float* __restrict__ blink,
                                                        int ldb) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= T * 8) return;
    const long t = i >> 3;
    const int c = (int)(i & 7);
    if (c < 6) pose[t * ldp + c] = __fadd_rn(__fmul_rn(__fadd_rn(pose[t * ldp + c], f.ip[c]), f.range[c]), f.mn[c]);
    else blink[t * ldb + c - 6] = __fadd_rn(blink[t * ldb + c - 6], f.ib[c - 6]);
}

}  // namespace

struct dawn_pbnet {
    dawn_pbnet_cfg cfg;
    const float *fpe_w = nullptr, *fpe_b = nullptr, *ae_w = nullptr, *ae_b = nullptr, *zt_w = nullptr, *zt_b = nullptr, *ip_b = nullptr,
                *in_g = nullptr, *in_be = nullptr, *in_qkv = nullptr, *in_out = nullptr, *fin_w = nullptr, *fin_b = nullptr,
                *bias_tgt = nullptr, *bias_mem = nullptr, *mem_kv = nullptr, *freqs = nullptr;
    std::vector<Layer> layers;
};                                // immutable after dawn_pbnet_create

namespace {

int up4(int n) { return (n + 3) & ~3; }

// The workspace: a header and one buffer per line below, each T rows of the given width (rounded up to 4 floats), one after the other.
struct Layout {
    size_t xref, cat, mem, memkv, a, b, c, qkv, qc, att, ff, rc, rs, total;     // byte offsets
    int ld_cat, ld_kv;
};

Layout layout(const dawn_pbnet_cfg& c, long T) {
    const int hd = c.heads * 32;
    Layout L;
    L.ld_cat = c.d + 2 * c.latent_dim;
    L.ld_kv = c.n_layers * 2 * hd;
    size_t off = ((size_t)c.d * 4 + 255) & ~(size_t)255;                        // header: x_ref (1, d)
    L.xref = 0;
    auto take = [&](int width) {
        const size_t o = off;
        off += (size_t)T * up4(width) * 4;
        return o;
    };
    L.cat = take(L.ld_cat);                 // [x_ref | z | audio embedding]
    L.mem = take(c.d);                      // ztimelinear's output: the decoder memory
    L.memkv = take(L.ld_kv);                // every layer's cross-attention [K | V] of the memory
    L.a = take(c.d);                        // three activations of the residual stream
    L.b = take(c.d);
    L.c = take(c.d);
    L.qkv = take(3 * hd);                   // self-attention [q | k | v]
    L.qc = take(hd);                        // cross-attention q
    L.att = take(hd);                       // attention output
    L.ff = take(c.ff);                      // FFN hidden
    L.rc = take(c.nrot);                    // rotary cos / sin
    L.rs = take(c.nrot);
    L.total = off;
    return L;
}

const size_t STAGE_HEADER = 256;            // dawn_pose_blink_stage: the two normalised first rows in front of the decoder's workspace

int attn(const dawn_pbnet* h, const float* q, int ldq, const float* k, const float* v, int ldkv, long T, const float* bias,
         const float* rc, const float* rs, float* out, void* stream) {
    const dawn_pbnet_cfg& c = h->cfg;
    return dawn_attn_win32(q, ldq, k, ldkv, v, ldkv, (int)T, (int)T, c.heads, c.win, bias, c.nrot ? rc : nullptr, c.nrot ? rs : nullptr,
                           c.nrot, 0.17677669529663687f /* 32^-1/2 */, out, c.heads * 32, stream);
}

int check_generate(const dawn_pbnet* h, const float* x0, const float* audio, int ld_audio, const float* z, long T, const float* out,
                   int ld_out, const void* ws, size_t bytes, const char* who) {
    char m[240];
    if (!h || !x0 || !audio || !z || !out) {
        snprintf(m, sizeof m, "%s: NULL argument (handle, x0, audio, z and out are required)", who);
        return dawn_set_error_msg(-261, m);
    }
    if (T < 1 || T > 0x7fffffffL / (h->cfg.ff > 1024 ? h->cfg.ff : 1024)) {
        snprintf(m, sizeof m, "%s: T = %ld frames, at least 1 needed (and rows * width must fit an int)", who, T);
        return dawn_set_error_msg(-263, m);
    }
    if (ld_audio < h->cfg.audio_dim || ld_out < h->cfg.in_dim) {
        snprintf(m, sizeof m, "%s: ld_audio = %d / ld_out = %d smaller than audio_dim = %d / in_dim = %d", who, ld_audio, ld_out,
                 h->cfg.audio_dim, h->cfg.in_dim);
        return dawn_set_error_msg(-263, m);
    }
    const size_t need = layout(h->cfg, T).total;
    if (!ws || bytes < need) return refuse_workspace(-262, who, ws ? bytes : 0, need, "dawn_pbnet_workspace_bytes");
    if (overlaps(out, ((size_t)(T - 1) * ld_out + h->cfg.in_dim) * 4, ws, bytes)) {
        snprintf(m, sizeof m, "%s: out overlaps the workspace", who);
        return dawn_set_error_msg(-264, m);
    }
    return 0;
}

// _decode_one; every argument has been checked
int generate(const dawn_pbnet* h, const float* x0, const float* audio, int ld_audio, const float* z, long T, float* out, int ld_out,
             void* workspace, void* stream) {
    const dawn_pbnet_cfg& c = h->cfg;
    const hipStream_t st = (hipStream_t)stream;
    const int d = c.d, hd = c.heads * 32, M = (int)T;
    const Layout L = layout(c, T);
    char* ws = (char*)workspace;
    auto F = [&](size_t off) { return (float*)(ws + off); };
    float *xref = F(L.xref), *cat = F(L.cat), *mem = F(L.mem), *memkv = F(L.memkv), *A = F(L.a), *B = F(L.b), *Cc = F(L.c),
          *qkv = F(L.qkv), *qc = F(L.qc), *att = F(L.att), *ff = F(L.ff), *rc = F(L.rc), *rs = F(L.rs);
    if (c.nrot > 0) {
        hipLaunchKernelGGL(pb_rotary_kernel, dim3(dawn_cdiv(T * c.nrot, 256)), dim3(256), 0, st, h->freqs, T, c.nrot, rc, rs);
        DAWN_LAUNCH_CHECK();
    }
    CK(dawn_linear(x0, 1, c.in_dim, c.in_dim, h->fpe_w, h->fpe_b, d, 0, xref, d, stream));             // identical for all frames
    CK(dawn_linear(audio, M, c.audio_dim, ld_audio, h->ae_w, h->ae_b, c.latent_dim, 0, cat + d + c.latent_dim, L.ld_cat, stream));
    hipLaunchKernelGGL(pb_rows_kernel, dim3(dawn_cdiv(T * (d + c.latent_dim), 256)), dim3(256), 0, st, xref, d, z, c.latent_dim, T, cat,
                       L.ld_cat);
    DAWN_LAUNCH_CHECK();
    CK(dawn_linear(cat, M, L.ld_cat, L.ld_cat, h->zt_w, h->zt_b, d, 0, mem, d, stream));
    if (c.n_layers > 0) CK(dawn_linear(mem, M, d, d, h->mem_kv, nullptr, L.ld_kv, 0, memkv, L.ld_kv, stream));
    hipLaunchKernelGGL(pb_rows_kernel, dim3(dawn_cdiv(T * d, 256)), dim3(256), 0, st, h->ip_b, d, (const float*)nullptr, 0, T, A, d);
    DAWN_LAUNCH_CHECK();                                                                               // init_proj(zeros) = its bias
    CK(dawn_ln_affine_act(A, T, d, h->in_g, h->in_be, c.eps, 0, Cc, stream));
    CK(dawn_linear(Cc, M, d, d, h->in_qkv, nullptr, 3 * hd, 0, qkv, 3 * hd, stream));
    CK(attn(h, qkv, 3 * hd, qkv + hd, qkv + 2 * hd, 3 * hd, T, h->bias_tgt, rc, rs, att, stream));
    CK(dawn_linear(att, M, hd, hd, h->in_out, nullptr, d, 0, B, d, stream));
    CK(dawn_add_act(A, B, 0, T * d, Cc, stream));
    float *x = Cc, *t1 = A, *t2 = B;                    // x: the residual stream; t1, t2: the two free activations
    for (int i = 0; i < c.n_layers; ++i) {
        const Layer& ly = h->layers[i];
        CK(dawn_linear(x, M, d, d, ly.sa_qkv, nullptr, 3 * hd, 0, qkv, 3 * hd, stream));
        CK(attn(h, qkv, 3 * hd, qkv + hd, qkv + 2 * hd, 3 * hd, T, h->bias_tgt, rc, rs, att, stream));
        CK(dawn_linear(att, M, hd, hd, ly.sa_out, nullptr, d, 0, t1, d, stream));
        CK(dawn_add_act(x, t1, 0, T * d, t2, stream));
        CK(dawn_ln_affine_act(t2, T, d, ly.ln1w, ly.ln1b, c.eps, 0, x, stream));
        CK(dawn_linear(x, M, d, d, ly.ca_q, nullptr, hd, 0, qc, hd, stream));
        CK(attn(h, qc, hd, memkv + (long)i * 2 * hd, memkv + (long)i * 2 * hd + hd, L.ld_kv, T, h->bias_mem, rc, rs, att, stream));
        CK(dawn_linear(att, M, hd, hd, ly.ca_out, nullptr, d, 0, t1, d, stream));
        CK(dawn_add_act(x, t1, 0, T * d, t2, stream));
        CK(dawn_ln_affine_act(t2, T, d, ly.ln2w, ly.ln2b, c.eps, 0, x, stream));
        CK(dawn_linear(x, M, d, d, ly.f1w, ly.f1b, c.ff, 0, ff, c.ff, stream));
        CK(dawn_linear(ff, M, c.ff, c.ff, ly.f2w, ly.f2b, d, 2, t1, d, stream));                       // exact GELU on linear2's input
        CK(dawn_add_act(x, t1, 0, T * d, t2, stream));
        CK(dawn_ln_affine_act(t2, T, d, ly.ln3w, ly.ln3b, c.eps, 0, x, stream));
    }
    return dawn_linear(x, M, d, d, h->fin_w, h->fin_b, c.in_dim, 0, out, ld_out, stream);
}

}  // namespace

extern "C" int dawn_pbnet_create(const dawn_pbnet_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_pbnet** out) {
    if (!cfg || !out || (!weights && n_weights > 0)) return dawn_set_error_msg(-261, "dawn_pbnet_create: NULL argument");
    char m[240];
    if (cfg->nrot < 0 || cfg->nrot > 16) {
        snprintf(m, sizeof m, "dawn_pbnet_create: nrot = %d rotary pairs, 0..16 fit a head of 32", cfg->nrot);
        return dawn_set_error_msg(-261, m);
    }
    if (cfg->in_dim < 1 || cfg->audio_dim < 1 || cfg->latent_dim < 1 || cfg->d < 1 || cfg->ff < 1 || cfg->heads < 1 || cfg->n_layers < 0 ||
        cfg->win < 0 || cfg->d > (1 << 20) || cfg->ff > (1 << 20) || cfg->audio_dim > (1 << 20) || cfg->latent_dim > (1 << 20) ||
        cfg->heads > 1024 || cfg->n_layers > 1024) {
        snprintf(m, sizeof m, "dawn_pbnet_create: in_dim = %d, audio_dim = %d, latent_dim = %d, d = %d, ff = %d, heads = %d must be "
                              "positive (widths up to 2^20), n_layers = %d and win = %d not negative",
                 cfg->in_dim, cfg->audio_dim, cfg->latent_dim, cfg->d, cfg->ff, cfg->heads, cfg->n_layers, cfg->win);
        return dawn_set_error_msg(-261, m);
    }
    dawn_pbnet* h = new dawn_pbnet();
    h->cfg = *cfg;
    DawnWeights Wt(weights, n_weights, "dawn_pbnet_create: missing weight", -260);
    auto F = [&](const std::string& n) { return Wt.getf(n); };
    h->fpe_w = F("firstposeEmbedding.weight"); h->fpe_b = F("firstposeEmbedding.bias");
    h->ae_w = F("audioEmbedding.weight"); h->ae_b = F("audioEmbedding.bias");
    h->zt_w = F("ztimelinear.weight"); h->zt_b = F("ztimelinear.bias");
    h->ip_b = F("init_proj.bias");
    h->in_g = F("init_temporal_attn.fn.norm.gamma"); h->in_be = F("init_temporal_attn.fn.norm.beta");
    h->in_qkv = F("init_temporal_attn.fn.fn.to_qkv.weight"); h->in_out = F("init_temporal_attn.fn.fn.to_out.weight");
    if (cfg->nrot > 0) h->freqs = F("init_temporal_attn.fn.fn.rotary_emb.freqs");
    h->bias_tgt = F("bias_tgt.rel"); h->bias_mem = F("bias_mem.rel");
    if (cfg->n_layers > 0) h->mem_kv = F("mem_kv.w");
    h->layers.resize(cfg->n_layers);
    for (int i = 0; i < cfg->n_layers; ++i) {
        const std::string p = "seqTransDecoder.decoder_layers." + std::to_string(i) + ".";
        h->layers[i] = {F(p + "self_attn.to_qkv.weight"), F(p + "self_attn.to_out.weight"), F(p + "layer_norm1.weight"),
                        F(p + "layer_norm1.bias"), F(p + "multihead_attn.to_q.weight"), F(p + "multihead_attn.to_out.weight"),
                        F(p + "layer_norm2.weight"), F(p + "layer_norm2.bias"), F(p + "ffn.linear1.weight"), F(p + "ffn.linear1.bias"),
                        F(p + "ffn.linear2.weight"), F(p + "ffn.linear2.bias"), F(p + "layer_norm3.weight"), F(p + "layer_norm3.bias")};
    }
    h->fin_w = F("finallayer.weight"); h->fin_b = F("finallayer.bias");
    if (!Wt.ok()) {
        delete h;
        return Wt.code();
    }
    *out = h;
    return 0;
}

extern "C" void dawn_pbnet_destroy(dawn_pbnet* pb) { delete pb; }

extern "C" size_t dawn_pbnet_workspace_bytes(const dawn_pbnet* pb, long T) {
    return pb && T >= 1 ? layout(pb->cfg, T).total : 0;
}

extern "C" size_t dawn_pose_blink_workspace_bytes(const dawn_pbnet* pose, const dawn_pbnet* blink, long T) {
    if (!pose || !blink || T < 1) return 0;
    const size_t a = layout(pose->cfg, T).total, b = layout(blink->cfg, T).total;
    return STAGE_HEADER + (a > b ? a : b);
}

extern "C" int dawn_pbnet_generate(dawn_pbnet* pb, const float* x0, const float* audio, int ld_audio, const float* z, long T, float* out,
                                   int ld_out, void* workspace, size_t workspace_bytes, void* stream) {
    CK(check_generate(pb, x0, audio, ld_audio, z, T, out, ld_out, workspace, workspace_bytes, "dawn_pbnet_generate"));
    return generate(pb, x0, audio, ld_audio, z, T, out, ld_out, workspace, stream);
}

extern "C" int dawn_pose_blink_stage(dawn_pbnet* pose, dawn_pbnet* blink, const float* audio, int ld_audio, long T,
                                     const float* init_pose6, const float* init_blink2, const float* z_pose, const float* z_blink,
                                     float* dri_pose, int ld_pose, float* dri_blink, int ld_blink, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const char* who = "dawn_pose_blink_stage";
    if (!pose || !blink || !init_pose6 || !init_blink2)
        return dawn_set_error_msg(-261, "dawn_pose_blink_stage: NULL argument (both handles and both initial rows are required)");
    if (pose->cfg.in_dim != 6 || blink->cfg.in_dim != 2 || pose->cfg.audio_dim != blink->cfg.audio_dim) {
        char m[200];
        snprintf(m, sizeof m, "%s: in_dim = %d / %d, expected 6 (pose) / 2 (blink) on one audio width (%d / %d)", who, pose->cfg.in_dim,
                 blink->cfg.in_dim, pose->cfg.audio_dim, blink->cfg.audio_dim);
        return dawn_set_error_msg(-263, m);
    }
    if (!workspace || workspace_bytes < STAGE_HEADER)
        return refuse_workspace(-262, who, workspace ? workspace_bytes : 0, dawn_pose_blink_workspace_bytes(pose, blink, T),
                                "dawn_pose_blink_workspace_bytes");
    char* ws = (char*)workspace;
    float *x0p = (float*)ws, *x0b = (float*)(ws + 64);
    void* gws = ws + STAGE_HEADER;
    const size_t gbytes = workspace_bytes - STAGE_HEADER;
    // both decoders are checked before the first launch; each output may not overlap the whole workspace (header included)
    CK(check_generate(pose, x0p, audio, ld_audio, z_pose, T, dri_pose, ld_pose, gws, gbytes, who));
    CK(check_generate(blink, x0b, audio, ld_audio, z_blink, T, dri_blink, ld_blink, gws, gbytes, who));
    if (overlaps(dri_pose, ((size_t)(T - 1) * ld_pose + 6) * 4, ws, STAGE_HEADER) ||
        overlaps(dri_blink, ((size_t)(T - 1) * ld_blink + 2) * 4, ws, STAGE_HEADER))
        return dawn_set_error_msg(-264, "dawn_pose_blink_stage: out overlaps the workspace");
    X0 v;
    Fin f;
    for (int c = 0; c < 6; ++c) {
        f.range[c] = POSE_MAX[c] - POSE_MIN[c];
        f.mn[c] = POSE_MIN[c];
        v.p[c] = f.ip[c] = (init_pose6[c] - POSE_MIN[c]) / f.range[c];                       // UVG:282
    }
    for (int c = 0; c < 2; ++c) v.b[c] = f.ib[c] = init_blink2[c];
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pb_x0_kernel, dim3(1), dim3(64), 0, st, v, x0p, x0b);
    DAWN_LAUNCH_CHECK();
    CK(generate(pose, x0p, audio, ld_audio, z_pose, T, dri_pose, ld_pose, gws, stream));   // UVG:287, 291
    CK(generate(blink, x0b, audio, ld_audio, z_blink, T, dri_blink, ld_blink, gws, stream));
    hipLaunchKernelGGL(pb_finish_kernel, dim3(dawn_cdiv(T * 8, 256)), dim3(256), 0, st, f, T, dri_pose, ld_pose, dri_blink, ld_blink);
    DAWN_LAUNCH_CHECK();                                                                    // UVG:294-296
    return 0;
}
