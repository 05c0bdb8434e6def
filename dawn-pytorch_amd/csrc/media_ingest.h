// What csrc/media_ingest.hip shares with the pipeline that calls its two entry points (dawn_inputs.hip): the argument checks on their
// own, so that a host can refuse a whole call before its first launch.  Internal (C++ linkage, not part of the C ABI).
#pragma once
#include "dawn_host.h"

#define DAWN_INGEST_MAX_SIDE 65535          // every image side, source and result: JPEG's own limit; keeps every index inside int

// the refusals of dawn_image_ingest that concern the source and the shapes, under the caller's name (the output and the workspace are
// the caller's own there: dawn_image_ingest checks them itself)
int media_image_check(const unsigned char* src, int Hs, int Ws, long row_bytes, int pix_bytes, int order, int Ho, int Wo, long plane,
                      const char* who);
// every refusal of dawn_pcm16_to_samples under the caller's name
int media_pcm_check(const int16_t* pcm, long n_frames, int channels, const float* out, const char* who);
