// What csrc/clip_inputs.hip shares with the stage host that chains its two entry points (dawn_inputs.hip): the argument checks on
// their own, so that a host can refuse a whole call before its first launch.  Internal (C++ linkage, not part of the C ABI).
#pragma once
#include "dawn_host.h"

#define DAWN_COND_MAX_INIT 16               // values of a host init_pose that travel to the kernel by value

// every refusal of dawn_face_loc_embed under the caller's name; bounds4 receives lt_x, lt_y, rb_x, rb_y
int clip_face_loc_check(const float* bbox6, int size, const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* out, long plane, const char* who, int* bounds4);
// every refusal of dawn_cond_rows under the caller's name
int clip_cond_rows_check(const float* audio, int n_aud, int ld_audio, const float* pose, int n_pose, int ld_pose, const float* eye,
                         int ld_eye, const float* init_pose, int n_init, const float* init_eye, long T, const float* cond, int ld_cond,
                         const char* who);
