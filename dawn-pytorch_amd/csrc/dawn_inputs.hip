// C-side host of the clip-input stage (include/dawn_hip.h: dawn_inputs_*, dawn_clip_inputs) and of the one-call pipeline that
// chains the five stage hosts (dawn_generate_bytes, dawn_generate_clip; from decoded media, with the two conversions of
// media_ingest.hip in front: dawn_generate_media_bytes, dawn_generate_clip_media; with PCM at any sample rate, through the resampler of
// audio_resample.hip: dawn_generate_media_rate_bytes, dawn_generate_clip_media_rate).  Same contract as the other four: opaque handle, device
// pointers by name, every launch on the caller's stream, no allocation, no synchronisation, errors by return code + dawn_last_error
// with nothing launched.  The pipeline calls nothing but the public entry points of the stages.
#include "clip_inputs.h"
#include "media_ingest.h"
#include "audio_resample.h"

#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

// the layout dawn-pytorch_amd/ctx.py mirrors (GenerateArgs) and tests/test_clip_inputs_cpu.py states
static_assert(sizeof(dawn_generate_args) == 224 && offsetof(dawn_generate_args, samples) == 48 && offsetof(dawn_generate_args, H) == 72 &&
                  offsetof(dawn_generate_args, bbox6) == 80 && offsetof(dawn_generate_args, n_init) == 104 &&
                  offsetof(dawn_generate_args, init_pose6) == 112 && offsetof(dawn_generate_args, T) == 128 &&
                  offsetof(dawn_generate_args, S) == 136 && offsetof(dawn_generate_args, cond_scale) == 140 &&
                  offsetof(dawn_generate_args, ddim_steps) == 144 && offsetof(dawn_generate_args, seed) == 168 &&
                  offsetof(dawn_generate_args, format) == 176 && offsetof(dawn_generate_args, chunk) == 184 &&
                  offsetof(dawn_generate_args, mean3) == 192 && offsetof(dawn_generate_args, cond_out) == 216,
              "dawn_generate_args layout");

struct dawn_inputs {
    dawn_inputs_cfg cfg;
    const float *w1, *b1, *w2, *b2;
};

namespace {

// every refusal of dawn_clip_inputs, before its first launch
int check_clip_inputs(const dawn_inputs* in, const float* bbox6, int size, const float* fea272, int fea_ch, const float* audio,
                      int ld_audio, const float* pose, int n_pose, int ld_pose, const float* eye, int ld_eye, const float* init_pose,
                      int n_init, const float* init_eye, long T, const float* cond, int ld_cond, const char* who) {
    char m[200];
    if (!in || !fea272) {
        snprintf(m, sizeof m, "%s: NULL handle or fea272", who);
        return dawn_set_error_msg(-291, m);
    }
    if (fea_ch < 16) {
        snprintf(m, sizeof m, "%s: fea_ch = %d, the face-location channels are its last 16", who, fea_ch);
        return dawn_set_error_msg(-292, m);
    }
    const long plane = size >= 4 ? (long)(size / 4) * (size / 4) : 0;
    int bounds[4];
    CK(clip_face_loc_check(bbox6, size, in->w1, in->b1, in->w2, in->b2, fea272 + (long)(fea_ch - 16) * plane, plane, who, bounds));
    CK(clip_cond_rows_check(audio, in->cfg.n_aud, ld_audio, pose, n_pose, ld_pose, eye, ld_eye, init_pose, n_init, init_eye, T, cond,
                            ld_cond, who));
    const int P = init_pose ? n_init : n_pose;
    if (P != in->cfg.pose_dim) {
        snprintf(m, sizeof m, "%s: %d pose columns in cond, the handle was created for pose_dim = %d", who, P, in->cfg.pose_dim);
        return dawn_set_error_msg(-292, m);
    }
    return 0;
}

// ---- the pipeline
struct Plan {
    int h, cond_dim, ld_cond;
    long num_frames;
    bool guided;
    size_t frames_bytes;
    // offsets into the workspace
    size_t cond, zero, fea, audio, z_pose, z_blink, x_init, latent, skip, clip, null_clip, stage;
    size_t skip_bytes, clip_bytes, stage_bytes, total;
    size_t hub_ws, pb_ws, dec_ws, unet_ws;
};

int refuse(int code, const char* who, const char* what) {
    char m[240];
    snprintf(m, sizeof m, "%s: %s", who, what);
    return dawn_set_error_msg(code, m);
}

int make_plan(const dawn_generate_args* a, const char* who, Plan& p) {
    if (!a) return refuse(-301, who, "NULL args");
    if (!a->hubert || !a->pose || !a->blink || !a->decoder || !a->inputs || !a->unet)
        return refuse(-301, who, "NULL handle (hubert, pose, blink, decoder, inputs and unet are required)");
    if (!a->samples || !a->img3 || !a->bbox6 || !a->init_pose6 || !a->init_blink2)
        return refuse(-301, who, "NULL pointer (samples, img3, bbox6, init_pose6 and init_blink2 are required)");
    char m[200];
    if (a->H < 4 || a->H % 4 != 0 || a->T < 1 || a->T > (1 << 24) || a->S < 0 || a->chunk < 1) {
        snprintf(m, sizeof m, "H = %d (a multiple of 4), T = %ld (1 .. 2^24), S = %d (>= 0), chunk = %d (>= 1)", a->H, a->T, a->S, a->chunk);
        return refuse(-302, who, m);
    }
    if ((a->ddim_steps != nullptr) == (a->ancestral_steps != nullptr))
        return refuse(-302, who, "exactly one of ddim_steps / ancestral_steps");
    if (a->format != DAWN_FRAMES_RGB && a->format != DAWN_FRAMES_YUV420) return refuse(-302, who, "format is DAWN_FRAMES_RGB or DAWN_FRAMES_YUV420");
    if (a->format == DAWN_FRAMES_YUV420 && a->bgr) return refuse(-302, who, "yuv420p frames have no channel order: bgr must be 0");
    if (a->latent_dim < 4 || a->latent_dim % 4 != 0 || a->fea_ch < 17) {
        snprintf(m, sizeof m, "latent_dim = %d (a multiple of 4), fea_ch = %d (the decoder's features + 16)", a->latent_dim, a->fea_ch);
        return refuse(-302, who, m);
    }
    if (!isfinite(a->cond_scale)) return refuse(-302, who, "cond_scale is not finite");
    if (a->clip) {                                   // what the sampler entries would refuse, before anything is launched
        const int k = a->clip->kind;
        if (k != DAWN_CLIP_DYNAMIC && k != DAWN_CLIP_STATIC && k != DAWN_CLIP_NONE) return refuse(-302, who, "unknown dawn_clip_mode kind");
        if (k == DAWN_CLIP_DYNAMIC && !(a->clip->q >= 0.0 && a->clip->q <= 1.0)) return refuse(-302, who, "dawn_clip_mode q outside [0, 1]");
        if (k == DAWN_CLIP_NONE && a->ancestral_steps) return refuse(-302, who, "DAWN_CLIP_NONE does not exist for ancestral steps");
    }
    const dawn_inputs_cfg& ic = a->inputs->cfg;
    p.h = a->H / 4;
    if (((long)p.h * p.h) % 4 != 0) return refuse(-302, who, "(H / 4)^2 must be a multiple of 4 (the noise generator draws four values at a time)");
    p.cond_dim = p.ld_cond = ic.n_aud + ic.pose_dim + 2;
    p.guided = a->cond_scale != 1.0f;
    const long T = a->T;
    // the audio: what dawn_hubert_features yields
    std::vector<long> seg(3 * (size_t)(a->n_samples > 0 ? a->n_samples / 320000 + 2 : 2));
    long eT = 0;
    p.num_frames = 0;
    const int ns = dawn_hubert_segments(a->hubert, a->n_samples, seg.data(), (int)(seg.size() / 3), &eT, &p.num_frames);
    if (ns < 0) return ns;
    if (p.num_frames < 1 || eT < 2) return refuse(-303, who, "the audio is too short for one frame at 25 fps");
    if (T > p.num_frames) {
        snprintf(m, sizeof m, "T = %ld frames, the audio yields %ld (dawn_hubert_segments)", T, p.num_frames);
        return refuse(-303, who, m);
    }
    p.frames_bytes = a->format == DAWN_FRAMES_YUV420 ? (size_t)T * a->H * a->H * 3 / 2 : (size_t)T * a->H * a->H * 3;
    p.skip_bytes = dawn_decoder_skip_bytes(a->decoder, a->H, a->H);
    p.clip_bytes = dawn_clip_bytes(a->unet, (int)T, p.h, p.h);
    const int chunk = a->chunk < T ? a->chunk : (int)T;
    p.hub_ws = dawn_hubert_workspace_bytes(a->hubert, a->n_samples);
    p.pb_ws = dawn_pose_blink_workspace_bytes(a->pose, a->blink, T);
    p.dec_ws = dawn_decoder_workspace_bytes(a->decoder, a->H, a->H, chunk);
    p.unet_ws = p.guided ? dawn_workspace_bytes_guided(a->unet, (int)T, p.h, p.h, 0, 1) : dawn_workspace_bytes(a->unet, (int)T, p.h, p.h);
    if (!p.skip_bytes || !p.clip_bytes || !p.hub_ws || !p.pb_ws || !p.dec_ws || !p.unet_ws)
        return refuse(-304, who, "a stage has no size for this clip (image side, clip length or audio length outside what it takes)");
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += a256(bytes); return at; };
    const size_t lat = (size_t)3 * T * p.h * p.h * 4;
    p.cond = take(a->cond_out ? 0 : (size_t)T * p.ld_cond * 4);
    p.zero = take(p.guided ? (size_t)p.cond_dim * 4 : 0);
    p.fea = take((size_t)a->fea_ch * p.h * p.h * 4);
    p.audio = take((size_t)p.num_frames * ic.n_aud * 4);
    p.z_pose = take((size_t)T * a->latent_dim * 4);
    p.z_blink = take((size_t)T * a->latent_dim * 4);
    p.x_init = take(lat);
    p.latent = take(a->latent_out ? 0 : lat);
    p.skip = take(p.skip_bytes);
    p.clip = take(p.clip_bytes);
    p.null_clip = take(p.guided ? p.clip_bytes : 0);
    p.stage = o;
    p.stage_bytes = a256(std::max(std::max(p.hub_ws, p.pb_ws), std::max(p.dec_ws, p.unet_ws)));
    p.total = o + p.stage_bytes;
    return 0;
}

}  // namespace

extern "C" int dawn_inputs_create(const dawn_inputs_cfg* cfg, const dawn_named_ptr* weights, int n_weights, dawn_inputs** out) {
    if (!cfg || !out || (!weights && n_weights > 0)) return dawn_set_error_msg(-291, "dawn_inputs_create: NULL argument");
    if (cfg->n_aud < 1 || cfg->n_aud > (1 << 20) || cfg->pose_dim < 1 || cfg->pose_dim > DAWN_COND_MAX_INIT || cfg->eye_dim != 2) {
        char m[200];
        snprintf(m, sizeof m, "dawn_inputs_create: n_aud = %d (1 .. 2^20), pose_dim = %d (1 .. %d), eye_dim = %d (2)", cfg->n_aud,
                 cfg->pose_dim, DAWN_COND_MAX_INIT, cfg->eye_dim);
        return dawn_set_error_msg(-292, m);
    }
    dawn_inputs* h = new dawn_inputs();
    h->cfg = *cfg;
    DawnWeights Wt(weights, n_weights, "dawn_inputs_create: missing weight", -290);
    h->w1 = Wt.getf("face_loc_emb.conv1.weight"); h->b1 = Wt.getf("face_loc_emb.conv1.bias");
    h->w2 = Wt.getf("face_loc_emb.conv2.weight"); h->b2 = Wt.getf("face_loc_emb.conv2.bias");
    if (!Wt.ok()) {
        delete h;
        return Wt.code();
    }
    *out = h;
    return 0;
}

extern "C" void dawn_inputs_destroy(dawn_inputs* in) { delete in; }

extern "C" int dawn_clip_inputs(dawn_inputs* in, const float* bbox6, int size, float* fea272, int fea_ch, const float* audio,
                                int ld_audio, const float* pose, int n_pose, int ld_pose, const float* eye, int ld_eye,
                                const float* init_pose, int n_init, const float* init_eye, long T, float* cond, int ld_cond,
                                void* stream) {
    CK(check_clip_inputs(in, bbox6, size, fea272, fea_ch, audio, ld_audio, pose, n_pose, ld_pose, eye, ld_eye, init_pose, n_init,
                         init_eye, T, cond, ld_cond, "dawn_clip_inputs"));
    const long plane = (long)(size / 4) * (size / 4);
    CK(dawn_face_loc_embed(bbox6, size, in->w1, in->b1, in->w2, in->b2, fea272 + (long)(fea_ch - 16) * plane, plane, stream));
    return dawn_cond_rows(audio, in->cfg.n_aud, ld_audio, pose, n_pose, ld_pose, eye, ld_eye, init_pose, n_init, init_eye, T, cond,
                          ld_cond, stream);
}

extern "C" int dawn_generate_bytes(const dawn_generate_args* args, size_t* clip_bytes, size_t* workspace_bytes) {
    Plan p;
    CK(make_plan(args, "dawn_generate_bytes", p));
    if (clip_bytes) *clip_bytes = p.frames_bytes;
    if (workspace_bytes) *workspace_bytes = p.total;
    return 0;
}

namespace {

// The pipeline on a plan that make_plan accepted: its remaining checks, then `before_first_launch` (the conversions of
// dawn_generate_clip_media, which write a.img3 / a.samples; it launches, so it comes after the last refusal), then the stages.
// `workspace` is the pipeline's own part: p.total bytes.
template <class Pre>
int run_pipeline(const dawn_generate_args& a, const Plan& p, void* workspace, size_t workspace_bytes, void* stream, const char* who,
                 Pre&& before_first_launch) {
    const dawn_inputs_cfg& ic = a.inputs->cfg;
    const long T = a.T;
    const int h = p.h, H = a.H, ldc = p.ld_cond;
    char* ws = (char*)workspace;
    auto F = [&](size_t off) { return (float*)(ws + off); };
    float* cond = a.cond_out ? a.cond_out : F(p.cond);
    float* latent = a.latent_out ? a.latent_out : F(p.latent);
    float *fea = F(p.fea), *audio = F(p.audio), *zp = F(p.z_pose), *zb = F(p.z_blink), *x_init = F(p.x_init);
    float *pose = cond + ic.n_aud, *eye = cond + ic.n_aud + ic.pose_dim;
    const size_t lat = (size_t)3 * T * h * h * 4;
    if ((a.cond_out && overlaps(cond, (size_t)T * ldc * 4, ws, workspace_bytes)) ||
        (a.latent_out && overlaps(latent, lat, ws, workspace_bytes)) || overlaps(a.frames_out, p.frames_bytes, ws, workspace_bytes))
        return refuse(-306, who, "frames_out / latent_out / cond_out overlaps the workspace");
    // the pose stage writes 6 pose columns; a 7th comes from init_pose (FD:348-349)
    CK(check_clip_inputs(a.inputs, a.bbox6, H, fea, a.fea_ch, audio, ic.n_aud, pose, 6, ldc, eye, ldc, a.init_pose, a.n_init, a.init_eye, T,
                         cond, ldc, who));
    CK(before_first_launch());
    void* sws = ws + p.stage;
    const size_t sbytes = p.stage_bytes;
    const hipStream_t st = (hipStream_t)stream;
    // 1. UVG:202-250, 433-501: samples -> audio rows (num_frames of them; the clip takes the first T)
    CK(dawn_hubert_features(a.hubert, a.samples, a.n_samples, nullptr, audio, sws, sbytes, stream));
    // 2., 3. UVG:252-302: pose and blink columns, straight into cond
    CK(dawn_philox_normal(zp, 1, (int)T, 0, (int)T, a.latent_dim, a.seed, 0xFFFFFFFEu, stream));
    CK(dawn_philox_normal(zb, 1, (int)T, 0, (int)T, a.latent_dim, a.seed, 0xFFFFFFFFu, stream));
    CK(dawn_pose_blink_stage(a.pose, a.blink, audio, ic.n_aud, T, a.init_pose6, a.init_blink2, zp, zb, pose, ldc, eye, ldc, sws, sbytes,
                             stream));
    // 4. GEN:132-146: encoder skips, and the decoder's features as the first planes of fea272
    CK(dawn_decoder_encode(a.decoder, H, H, a.img3, ws + p.skip, p.skip_bytes, fea, sws, sbytes, stream));
    // 5. FD:327-350: the face-location planes and the condition rows, pose / eye in place
    CK(dawn_clip_inputs(a.inputs, a.bbox6, H, fea, a.fea_ch, audio, ic.n_aud, pose, 6, ldc, eye, ldc, a.init_pose, a.n_init, a.init_eye, T,
                        cond, ldc, stream));
    // 6. the per-clip tables (and those of the all-zero condition: one zero row read with stride 0)
    CK(dawn_clip_prepare(a.unet, (int)T, h, h, fea, cond, ldc, nullptr, nullptr, ws + p.clip, p.clip_bytes, sws, sbytes, stream));
    if (p.guided) {
        if (hipMemsetAsync(F(p.zero), 0, (size_t)p.cond_dim * 4, st) != hipSuccess) return dawn_set_error(hipGetLastError(), __FILE__, __LINE__);
        CK(dawn_clip_prepare(a.unet, (int)T, h, h, fea, F(p.zero), 0, nullptr, nullptr, ws + p.null_clip, p.clip_bytes, sws, sbytes, stream));
    }
    // 7., 8. MT:1156-1208 / MT:1124-1135
    CK(dawn_philox_normal(x_init, 3, (int)T, 0, (int)T, h * h, a.seed, 0u, stream));
    const void* null_clip = p.guided ? ws + p.null_clip : nullptr;
    if (a.ddim_steps)
        CK(dawn_sampler_run_clip(a.unet, (int)T, h, h, ws + p.clip, null_clip, a.cond_scale, x_init, a.S, a.ddim_steps, a.seed, nullptr, latent,
                                 nullptr, sws, sbytes, nullptr, a.clip, stream));
    else
        CK(dawn_sampler_run_ancestral_clip(a.unet, (int)T, h, h, ws + p.clip, null_clip, a.cond_scale, x_init, a.S, a.ancestral_steps, a.seed,
                                           nullptr, latent, nullptr, sws, sbytes, nullptr, a.clip, stream));
    // 9. FD:372-385 + UVG:383-397
    const long plane = (long)T * h * h;
    if (a.format == DAWN_FRAMES_YUV420)
        return dawn_decode_clip_yuv420(a.decoder, H, H, (int)T, h, h, a.img3, ws + p.skip, latent, plane, a.chunk, a.frames_out, a.mean3, sws,
                                       sbytes, stream);
    return dawn_decode_clip(a.decoder, H, H, (int)T, h, h, a.img3, ws + p.skip, latent, plane, a.chunk, nullptr, nullptr, 0, a.frames_out,
                            a.mean3, a.bgr, sws, sbytes, stream);
}

// ---- the same from decoded media: the front of the workspace holds what the two conversions make
struct MediaPlan {
    dawn_generate_args gen;                 // the caller's, with img3 / samples / n_samples replaced where media are given
    Plan plan;
    size_t img3, samples, ingest, ingest_bytes, table, table_bytes, front;      // offsets; front = where the pipeline's own workspace starts
    long n_out;                             // the 16 kHz samples the PCM yields (= n_frames at 16 kHz)
};

// pcm_rate = the sample rate of m->pcm; 16000: the PCM is converted as it is and the plan is dawn_generate_clip_media's, byte for byte
int make_media_plan(const dawn_media_args* m, int pcm_rate, const char* who, MediaPlan& q) {
    if (!m || !m->gen) return refuse(-321, who, "NULL args or NULL gen");
    if (!m->pcm && pcm_rate != 16000) {
        char e[160];
        snprintf(e, sizeof e, "pcm is NULL with pcm_rate = %d: gen->samples are 16 kHz samples, only PCM is resampled", pcm_rate);
        return refuse(-321, who, e);
    }
    q.gen = *m->gen;
    dawn_generate_args& g = q.gen;
    if (!m->image && !g.img3) return refuse(-321, who, "image is NULL and so is gen->img3: one of the two is the source image");
    if (!m->pcm && !g.samples) return refuse(-321, who, "pcm is NULL and so is gen->samples: one of the two is the audio");
    // placeholders that only have to be non-NULL until the workspace is known: no check below reads through them
    static const float dummy_f = 0.0f;
    q.n_out = 0;
    q.table_bytes = 0;
    if (m->pcm) {
        if (pcm_rate == 16000) {
            CK(media_pcm_check(m->pcm, m->n_frames, m->channels, &dummy_f, who));
            q.n_out = m->n_frames;
        } else {
            CK(resample_pcm_check(m->pcm, m->n_frames, m->channels, pcm_rate, &q.n_out, who));
            q.table_bytes = dawn_resample16k_workspace_bytes(pcm_rate);
        }
        g.samples = &dummy_f;
        g.n_samples = q.n_out;
    }
    if (m->image) g.img3 = &dummy_f;
    CK(make_plan(&g, who, q.plan));
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += a256(bytes); return at; };
    q.ingest_bytes = 0;
    if (m->image) {
        // out3 and the ingest workspace are this entry's own, carved below: only the source and the shapes can be wrong
        CK(media_image_check(m->image, m->Hs, m->Ws, m->row_bytes, m->pix_bytes, m->order, g.H, g.H, (long)g.H * g.H, who));
        q.ingest_bytes = dawn_image_ingest_workspace_bytes(m->Hs, m->Ws, g.H, g.H);
    }
    q.img3 = take(m->image ? (size_t)3 * g.H * g.H * 4 : 0);
    q.samples = take(m->pcm ? (size_t)q.n_out * 4 : 0);
    q.ingest = take(q.ingest_bytes);
    q.table = take(q.table_bytes);
    q.front = o;
    return 0;
}

}  // namespace

extern "C" int dawn_generate_clip(const dawn_generate_args* args, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "dawn_generate_clip";
    Plan p;
    CK(make_plan(args, who, p));
    if (!args->frames_out) return refuse(-301, who, "NULL frames_out");
    if (!workspace || workspace_bytes < p.total)
        return refuse_workspace(-305, who, workspace ? workspace_bytes : 0, p.total, "dawn_generate_bytes");
    return run_pipeline(*args, p, workspace, workspace_bytes, stream, who, [] { return 0; });
}

namespace {

int media_bytes(const dawn_media_args* args, int pcm_rate, size_t* clip_bytes, size_t* workspace_bytes, const char* who) {
    MediaPlan q;
    CK(make_media_plan(args, pcm_rate, who, q));
    if (clip_bytes) *clip_bytes = q.plan.frames_bytes;
    if (workspace_bytes) *workspace_bytes = q.front + q.plan.total;
    return 0;
}

int clip_media(const dawn_media_args* args, int pcm_rate, void* workspace, size_t workspace_bytes, void* stream, const char* who,
               const char* sizer) {
    MediaPlan q;
    CK(make_media_plan(args, pcm_rate, who, q));
    const dawn_media_args& m = *args;
    dawn_generate_args& g = q.gen;
    if (!g.frames_out) return refuse(-301, who, "NULL frames_out");
    const size_t total = q.front + q.plan.total;
    if (!workspace || workspace_bytes < total) return refuse_workspace(-305, who, workspace ? workspace_bytes : 0, total, sizer);
    char* ws = (char*)workspace;
    float* img3 = (float*)(ws + q.img3);
    float* samples = (float*)(ws + q.samples);
    if (m.image) g.img3 = img3;
    if (m.pcm) g.samples = samples;
    // the conversions' pieces are workspace too (run_pipeline checks the outputs against its own part)
    if (overlaps(g.frames_out, q.plan.frames_bytes, ws, q.front) ||
        (g.cond_out && overlaps(g.cond_out, (size_t)g.T * q.plan.ld_cond * 4, ws, q.front)) ||
        (g.latent_out && overlaps(g.latent_out, (size_t)3 * g.T * q.plan.h * q.plan.h * 4, ws, q.front)))
        return refuse(-306, who, "frames_out / latent_out / cond_out overlaps the workspace");
    const long HH = (long)g.H * g.H;
    return run_pipeline(g, q.plan, ws + q.front, workspace_bytes - q.front, stream, who, [&] {
        if (m.image)
            CK(dawn_image_ingest(m.image, m.Hs, m.Ws, m.row_bytes, m.pix_bytes, m.order, g.H, g.H, img3, HH, ws + q.ingest, q.ingest_bytes,
                                 stream));
        if (m.pcm && pcm_rate == 16000) CK(dawn_pcm16_to_samples(m.pcm, m.n_frames, m.channels, samples, stream));
        if (m.pcm && pcm_rate != 16000)
            CK(dawn_resample16k_pcm16(m.pcm, m.n_frames, m.channels, pcm_rate, samples, q.n_out, ws + q.table, q.table_bytes, stream));
        return 0;
    });
}

}  // namespace

extern "C" int dawn_generate_media_bytes(const dawn_media_args* args, size_t* clip_bytes, size_t* workspace_bytes) {
    return media_bytes(args, 16000, clip_bytes, workspace_bytes, "dawn_generate_media_bytes");
}

extern "C" int dawn_generate_clip_media(const dawn_media_args* args, void* workspace, size_t workspace_bytes, void* stream) {
    return clip_media(args, 16000, workspace, workspace_bytes, stream, "dawn_generate_clip_media", "dawn_generate_media_bytes");
}

extern "C" int dawn_generate_media_rate_bytes(const dawn_media_args* args, int pcm_rate, size_t* clip_bytes, size_t* workspace_bytes) {
    return media_bytes(args, pcm_rate, clip_bytes, workspace_bytes, "dawn_generate_media_rate_bytes");
}

extern "C" int dawn_generate_clip_media_rate(const dawn_media_args* args, int pcm_rate, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    return clip_media(args, pcm_rate, workspace, workspace_bytes, stream, "dawn_generate_clip_media_rate", "dawn_generate_media_rate_bytes");
}
