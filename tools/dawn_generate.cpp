// dawn_generate: a WAV and an image to a talking-head clip, without Python.  Plain C++ against include/dawn_hip.h and the HIP runtime
// API; no kernels of its own.
//
//   dawn_generate --bundle M.dawn --wav A.wav --image F.ppm --out clip.y4m
//                 [--frames T] [--steps ddim.20] [--seed N] [--cond-scale X] [--format y4m|rgb] [--chunk N]
//   dawn_generate --bundle M.dawn --driving D.y4m --image F.ppm --out clip.y4m [--frames T] [--format y4m|rgb] [--chunk N]
//
// With --driving (and no --wav) the clip is video-driven: the motion of the frames of D.y4m (8-bit 4:2:0, of the model's size; the
// parser and what it refuses: tools/media_files.h) is encoded against the image and decoded from it in one dawn_reenact_clip call --
// no audio, no sampler.  That needs a bundle with the motion stage; another one is refused with the loader's message.
// The model comes from a bundle file (dawn_pytorch_amd/bundle.py writes it; include/dawn_hip.h, "model bundle").  The WAV is 16-bit
// PCM, 1 .. 8 channels, at any rate the resampler takes; the image a binary PPM (P6) or PGM (P5) with maxval 255 (tools/media_files.h).
// T = min(max_n_frames, frames the audio yields) as the Python host forms it, unless --frames states it.
// y4m: "YUV4MPEG2 W<H> H<H> F25:1 Ip A1:1 C420jpeg" (centre-sited chroma: the siting of dawn_decode_clip_yuv420), then FRAME-prefixed
// I420 planes; rgb: the raw (T, H, H, 3) bytes.  Exit status: 0, 2 for a bad command line, 3 for any refusal (with the library's message).
//
// Build (host compiler; $ROCM = the ROCm root):
//   g++ -std=c++17 -O2 -D__HIP_PLATFORM_AMD__ -I include -I $ROCM/include tools/dawn_generate.cpp -L dawn-pytorch_amd -ldawn_hip
//       -L $ROCM/lib -lamdhip64 -Wl,-rpath,$PWD/dawn-pytorch_amd -Wl,-rpath,$ROCM/lib -o dawn_generate      (one command line)
#include <hip/hip_runtime_api.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dawn_hip.h"
#include "media_files.h"

namespace {

[[noreturn]] void die(const std::string& what) {
    fprintf(stderr, "dawn_generate: %s\n", what.c_str());
    exit(3);
}
void ck(int rc, const char* what) {
    if (rc != 0) die(std::string(what) + " failed with code " + std::to_string(rc) + ": " + dawn_last_error());
}
void hk(hipError_t e, const char* what) {
    if (e != hipSuccess) die(std::string(what) + ": " + hipGetErrorString(e));
}
size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

[[noreturn]] void usage() {
    fprintf(stderr, "usage: dawn_generate --bundle M.dawn --wav A.wav --image F.ppm --out clip.y4m [--frames T] [--steps ddim.20] [--seed N]\n"
                    "                     [--cond-scale X] [--format y4m|rgb] [--chunk N]\n"
                    "       dawn_generate --bundle M.dawn --driving D.y4m --image F.ppm --out clip.y4m [--frames T] [--format y4m|rgb] [--chunk N]\n");
    exit(2);
}

// the frames as a .y4m stream or as raw bytes
void write_clip(const std::string& out_path, const std::string& format, const std::vector<unsigned char>& out, int H, long T) {
    FILE* f = fopen(out_path.c_str(), "wb");
    if (!f) die("cannot write '" + out_path + "'");
    bool ok = true;
    if (format == "y4m") {
        const size_t frame = (size_t)H * H * 3 / 2;
        ok = fprintf(f, "YUV4MPEG2 W%d H%d F25:1 Ip A1:1 C420jpeg\n", H, H) > 0;
        for (long t = 0; ok && t < T; ++t) ok = fputs("FRAME\n", f) >= 0 && fwrite(out.data() + (size_t)t * frame, 1, frame, f) == frame;
    } else {
        ok = fwrite(out.data(), 1, out.size(), f) == out.size();
    }
    if (fclose(f) != 0 || !ok) die("short write to '" + out_path + "'");
}

// --driving: the frames of a .y4m file reenacted on the image, one dawn_reenact_clip call
int reenact(const std::string& bundle, const std::string& driving_path, const std::string& image_path, const std::string& out_path,
            const std::string& format, long frames, int chunk) {
    std::string err;
    std::vector<unsigned char> raw;
    media_files::Y4m drv;
    media_files::Image img;
    if (media_files::read_file(driving_path.c_str(), &raw, &err) != 0 || media_files::parse_y4m(raw.data(), raw.size(), &drv, &err) != 0) die(err);
    if (media_files::read_file(image_path.c_str(), &raw, &err) != 0 || media_files::parse_pnm(raw.data(), raw.size(), &img, &err) != 0) die(err);

    hipStream_t stream = nullptr;
    hk(hipStreamCreate(&stream), "hipStreamCreate");
    dawn_bundle* b = nullptr;
    ck(dawn_bundle_open(bundle.c_str(), &b), "dawn_bundle_open");
    const size_t model_bytes = std::max<size_t>(dawn_bundle_device_bytes(b), 256), verify_bytes = dawn_bundle_verify_workspace_bytes(b);
    void *model = nullptr, *verify_ws = nullptr;
    hk(hipMalloc(&model, model_bytes), "hipMalloc (model)");
    ck(dawn_bundle_upload(b, model, model_bytes, stream), "dawn_bundle_upload");
    hk(hipMalloc(&verify_ws, verify_bytes), "hipMalloc (verify workspace)");
    ck(dawn_bundle_verify(b, model, model_bytes, verify_ws, verify_bytes, stream), "dawn_bundle_verify");
    hk(hipFree(verify_ws), "hipFree");
    dawn_motion* motion = nullptr;
    ck(dawn_bundle_create_motion(b, model, &motion), "dawn_bundle_create_motion");
    dawn_generate_args g;
    memset(&g, 0, sizeof g);
    ck(dawn_bundle_create_handles(b, model, &g), "dawn_bundle_create_handles");
    const void* blob = nullptr;
    size_t blob_bytes = 0;
    ck(dawn_bundle_host(b, "defaults", &blob, &blob_bytes), "dawn_bundle_host");
    dawn_bundle_defaults def;
    memcpy(&def, blob, sizeof def);
    const int H = def.H;
    if (drv.width != H || drv.height != H)
        die("y4m: frames of " + std::to_string(drv.width) + " x " + std::to_string(drv.height) + ", the bundle's model takes " + std::to_string(H) + " x " + std::to_string(H));
    const long T = frames > 0 ? std::min<long>(frames, drv.n_frames) : std::min<long>(def.max_n_frames, drv.n_frames);
    const double mean3[3] = {def.mean[0] / 255.0, def.mean[1] / 255.0, def.mean[2] / 255.0};
    const size_t frame_in = (size_t)H * H * 3 / 2;

    // device memory: [image bytes | img3 | I420 frames | ingest workspace] in one allocation, then the frames and the stage workspace
    const size_t img_bytes = up256(img.pixels.size()), img3_bytes = up256((size_t)3 * H * H * 4), drv_bytes = up256((size_t)T * frame_in);
    const size_t ingest_bytes = up256(dawn_image_ingest_workspace_bytes(img.height, img.width, H, H));
    if (ingest_bytes == 0) die(std::string("dawn_image_ingest_workspace_bytes: ") + dawn_last_error());
    unsigned char* io = nullptr;
    hk(hipMalloc((void**)&io, img_bytes + img3_bytes + drv_bytes + ingest_bytes), "hipMalloc (media)");
    float* img3 = (float*)(io + img_bytes);
    unsigned char* drv_dev = io + img_bytes + img3_bytes;
    dawn_reenact_args a;
    memset(&a, 0, sizeof a);
    a.size = sizeof a;
    a.motion = motion; a.decoder = g.decoder;
    a.img3 = img3; a.H = H; a.W = H;
    a.drv = drv_dev; a.drv_kind = 2; a.T = (int)T; a.drv_frame_stride = (long)frame_in;
    a.motion_chunk = chunk; a.chunk = chunk;
    a.format = format == "y4m" ? DAWN_FRAMES_YUV420 : DAWN_FRAMES_RGB;
    a.mean3 = mean3;
    size_t clip_bytes = 0, ws_bytes = 0;
    ck(dawn_reenact_bytes(&a, &clip_bytes, &ws_bytes), "dawn_reenact_bytes");
    unsigned char* frames_dev = nullptr;
    void* ws = nullptr;
    hk(hipMalloc((void**)&frames_dev, clip_bytes), "hipMalloc (frames)");
    hk(hipMalloc(&ws, ws_bytes), "hipMalloc (workspace)");
    a.frames_out = frames_dev;
    hk(hipMemcpyAsync(io, img.pixels.data(), img.pixels.size(), hipMemcpyHostToDevice, stream), "hipMemcpyAsync (image)");
    hk(hipMemcpyAsync(drv_dev, drv.frames.data(), (size_t)T * frame_in, hipMemcpyHostToDevice, stream), "hipMemcpyAsync (driving)");
    ck(dawn_image_ingest(io, img.height, img.width, (long)img.width * img.channels, img.channels, DAWN_PIXELS_RGB, H, H, img3, (long)H * H,
                         io + img_bytes + img3_bytes + drv_bytes, ingest_bytes, stream), "dawn_image_ingest");
    ck(dawn_reenact_clip(&a, ws, ws_bytes, stream), "dawn_reenact_clip");
    std::vector<unsigned char> out(clip_bytes);
    hk(hipMemcpyAsync(out.data(), frames_dev, clip_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync (frames)");
    hk(hipStreamSynchronize(stream), "hipStreamSynchronize");
    write_clip(out_path, format, out, H, T);
    fprintf(stderr, "dawn_generate: %ld driving frames of %d x %d reenacted (%s) -> %s\n", T, H, H, format.c_str(), out_path.c_str());

    dawn_motion_destroy(motion);
    dawn_bundle_destroy_handles(&g);
    dawn_bundle_close(b);
    (void)hipFree(ws); (void)hipFree(frames_dev); (void)hipFree(io); (void)hipFree(model);
    (void)hipStreamDestroy(stream);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::string bundle, wav_path, driving_path, image_path, out_path, steps_name, format = "y4m";
    long frames = -1;
    int chunk = 16;
    bool have_seed = false, have_scale = false;
    unsigned long long seed = 0;
    float cond_scale = 1.0f;
    for (int i = 1; i < argc; ++i) {
        const std::string k = argv[i];
        if (i + 1 >= argc) usage();
        const char* v = argv[++i];
        if (k == "--bundle") bundle = v;
        else if (k == "--wav") wav_path = v;
        else if (k == "--driving") driving_path = v;
        else if (k == "--image") image_path = v;
        else if (k == "--out") out_path = v;
        else if (k == "--steps") steps_name = v;
        else if (k == "--format") format = v;
        else if (k == "--frames") frames = atol(v);
        else if (k == "--chunk") chunk = atoi(v);
        else if (k == "--seed") { seed = strtoull(v, nullptr, 10); have_seed = true; }
        else if (k == "--cond-scale") { cond_scale = strtof(v, nullptr); have_scale = true; }
        else usage();
    }
    if (bundle.empty() || wav_path.empty() == driving_path.empty() || image_path.empty() || out_path.empty() || (format != "y4m" && format != "rgb")) usage();
    if (!driving_path.empty()) return reenact(bundle, driving_path, image_path, out_path, format, frames, chunk);

    // the media, parsed on the host
    std::string err;
    std::vector<unsigned char> raw;
    media_files::Wav wav;
    media_files::Image img;
    if (media_files::read_file(wav_path.c_str(), &raw, &err) != 0 || media_files::parse_wav(raw.data(), raw.size(), &wav, &err) != 0) die(err);
    if (media_files::read_file(image_path.c_str(), &raw, &err) != 0 || media_files::parse_pnm(raw.data(), raw.size(), &img, &err) != 0) die(err);

    // the model: open, upload, verify, handles
    hipStream_t stream = nullptr;
    hk(hipStreamCreate(&stream), "hipStreamCreate");
    dawn_bundle* b = nullptr;
    ck(dawn_bundle_open(bundle.c_str(), &b), "dawn_bundle_open");
    const size_t model_bytes = std::max<size_t>(dawn_bundle_device_bytes(b), 256), verify_bytes = dawn_bundle_verify_workspace_bytes(b);
    void *model = nullptr, *verify_ws = nullptr;
    hk(hipMalloc(&model, model_bytes), "hipMalloc (model)");
    ck(dawn_bundle_upload(b, model, model_bytes, stream), "dawn_bundle_upload");
    hk(hipMalloc(&verify_ws, verify_bytes), "hipMalloc (verify workspace)");
    ck(dawn_bundle_verify(b, model, model_bytes, verify_ws, verify_bytes, stream), "dawn_bundle_verify");
    hk(hipFree(verify_ws), "hipFree");
    dawn_generate_args a;
    memset(&a, 0, sizeof a);
    ck(dawn_bundle_create_handles(b, model, &a), "dawn_bundle_create_handles");

    // defaults and the step table
    const void* blob = nullptr;
    size_t blob_bytes = 0;
    ck(dawn_bundle_host(b, "defaults", &blob, &blob_bytes), "dawn_bundle_host");
    dawn_bundle_defaults def;
    memcpy(&def, blob, sizeof def);
    if (steps_name.empty()) steps_name = std::string(def.ancestral ? "ancestral." : "ddim.") + std::to_string(def.sampling_step);
    ck(dawn_bundle_host(b, ("steps." + steps_name).c_str(), &blob, &blob_bytes), "dawn_bundle_host");
    const bool ancestral = steps_name.compare(0, 10, "ancestral.") == 0;
    if (ancestral) {
        a.ancestral_steps = (const dawn_ancestral_step*)blob;
        a.S = (int)(blob_bytes / sizeof(dawn_ancestral_step));
    } else {
        a.ddim_steps = (const dawn_ddim_step*)blob;
        a.S = (int)(blob_bytes / sizeof(dawn_ddim_step));
    }
    dawn_inputs_cfg in_cfg;
    ck(dawn_bundle_cfg(b, DAWN_STAGE_INPUTS, &in_cfg, sizeof in_cfg), "dawn_bundle_cfg");

    // T = min(max_n_frames, frames the audio yields), judged on the 16 kHz sample count as dawn_generate_clip_media_rate judges it
    const long n16 = wav.rate == 16000 ? wav.n_frames : dawn_resample16k_len(wav.n_frames, wav.rate);
    if (n16 < 1) die("wav: " + std::to_string(wav.n_frames) + " frames at " + std::to_string(wav.rate) + " Hz: a rate of 1000 .. 384000 Hz and at least one sample at 16 kHz");
    std::vector<long> seg(3 * (size_t)(n16 / 320000 + 2));
    long expected_T = 0, num_frames = 0;
    if (dawn_hubert_segments(a.hubert, n16, seg.data(), (int)(seg.size() / 3), &expected_T, &num_frames) < 0) die(std::string("dawn_hubert_segments: ") + dawn_last_error());
    const long T = frames > 0 ? frames : std::min<long>(def.max_n_frames, num_frames);

    const double mean3[3] = {def.mean[0] / 255.0, def.mean[1] / 255.0, def.mean[2] / 255.0};
    a.H = def.H;
    a.fea_ch = def.fea_ch;
    a.latent_dim = def.latent_dim;
    a.bbox6 = def.bbox6;
    a.init_pose6 = def.init_pose6;
    a.init_blink2 = def.init_blink2;
    if (in_cfg.pose_dim == 6) {                        // the condition subtracts the initial pose / blink, as the Python host passes them
        a.init_pose = def.init_pose6;
        a.n_init = 6;
        a.init_eye = def.init_blink2;
    }
    a.T = T;
    a.cond_scale = have_scale ? cond_scale : def.cond_scale;
    a.clip = &def.clip;
    a.seed = have_seed ? seed : def.random_seed;
    a.format = format == "y4m" ? DAWN_FRAMES_YUV420 : DAWN_FRAMES_RGB;
    a.chunk = chunk;
    a.mean3 = mean3;

    // device memory: [image bytes | PCM] in one allocation, then the frames and the workspace that the size query states
    dawn_media_args m;
    memset(&m, 0, sizeof m);
    m.gen = &a;
    m.Hs = img.height; m.Ws = img.width; m.pix_bytes = img.channels; m.row_bytes = (long)img.width * img.channels; m.order = DAWN_PIXELS_RGB;
    m.n_frames = wav.n_frames; m.channels = wav.channels;
    const size_t img_bytes = up256(img.pixels.size()), pcm_bytes = up256(wav.pcm.size() * 2);
    unsigned char* io = nullptr;
    hk(hipMalloc((void**)&io, img_bytes + pcm_bytes), "hipMalloc (media)");
    m.image = io;
    m.pcm = (const int16_t*)(io + img_bytes);
    size_t clip_bytes = 0, ws_bytes = 0;
    ck(dawn_generate_media_rate_bytes(&m, wav.rate, &clip_bytes, &ws_bytes), "dawn_generate_media_rate_bytes");
    unsigned char* frames_dev = nullptr;
    void* ws = nullptr;
    hk(hipMalloc((void**)&frames_dev, clip_bytes), "hipMalloc (frames)");
    hk(hipMalloc(&ws, ws_bytes), "hipMalloc (workspace)");
    a.frames_out = frames_dev;
    hk(hipMemcpyAsync(io, img.pixels.data(), img.pixels.size(), hipMemcpyHostToDevice, stream), "hipMemcpyAsync (image)");
    hk(hipMemcpyAsync(io + img_bytes, wav.pcm.data(), wav.pcm.size() * 2, hipMemcpyHostToDevice, stream), "hipMemcpyAsync (pcm)");
    ck(dawn_generate_clip_media_rate(&m, wav.rate, ws, ws_bytes, stream), "dawn_generate_clip_media_rate");
    std::vector<unsigned char> out(clip_bytes);
    hk(hipMemcpyAsync(out.data(), frames_dev, clip_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync (frames)");
    hk(hipStreamSynchronize(stream), "hipStreamSynchronize");

    write_clip(out_path, format, out, a.H, T);
    fprintf(stderr, "dawn_generate: %ld frames of %d x %d (%s, %d %s steps) -> %s\n", T, a.H, a.H, format.c_str(), a.S, ancestral ? "ancestral" : "DDIM",
            out_path.c_str());

    dawn_bundle_destroy_handles(&a);
    dawn_bundle_close(b);
    (void)hipFree(ws); (void)hipFree(frames_dev); (void)hipFree(io); (void)hipFree(model);
    (void)hipStreamDestroy(stream);
    return 0;
}
