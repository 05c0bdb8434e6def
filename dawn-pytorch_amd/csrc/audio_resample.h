// What csrc/audio_resample.hip shares with the pipeline that calls it (dawn_inputs.hip): the argument checks of dawn_resample16k_pcm16 that
// concern the source and the rate, on their own, so that a host can refuse a whole call before its first launch.  Internal (C++ linkage,
// not part of the C ABI).
#pragma once
#include "dawn_host.h"

#define DAWN_RESAMPLE_MIN_RATE 1000
#define DAWN_RESAMPLE_MAX_RATE 384000
#define DAWN_RESAMPLE_MAX_FRAMES (1L << 34)  // keeps n_frames * 16000, i * M and the grid inside their integer types

// the refusals of dawn_resample16k_pcm16 that concern pcm, n_frames, channels and rate, under the caller's name (out and the workspace are
// the caller's own there); *n_out = dawn_resample16k_len(n_frames, rate)
int resample_pcm_check(const int16_t* pcm, long n_frames, int channels, int rate, long* n_out, const char* who);
