// What the resampler's entry points (ls_resample_api.cpp) take from its kernels (ls_resample.hip).  Plain structs of device pointers;
// every launch goes to the null stream.
#pragma once
#include <hip/hip_runtime.h>

#include "ls_hip.h"
#include "ls_resample_frame.h"

namespace ls {

// ---- one-shot: workgroup (x, b) computes outputs [256 x, 256 x + 256) of clip b; the output was zeroed ahead of the launch ----
struct ResampleArgs {
    ResampleRatio q;
    int dtype, C;                  // LS_RESAMPLE_F32 | LS_RESAMPLE_I16, interleaved channels
    float gain;                    // float(1 / C), int16: float(1 / (32768 C))
    const void* audio;             // [B, row_stride] elements
    long long row_stride;
    const long long* lengths;      // [B] frames of each clip
    const long long* out_lengths;  // [B] ceil(lengths up / down)
    float* out;                    // [B, out_stride]
    long long out_stride;
    const float* tab;              // [up, Tp]
};
void launch_resample(const ResampleArgs& a, int B, long long max_out);

// ---- stream: workgroup g computes one tile of the push's new outputs of one slot ----
struct ResampleSlotRow {           // one per slot and launch, uploaded ahead of it
    int tile_off;                  // prefix sum of the slots' tiles (row S: the total)
    int fresh;                     // new frames in the chunk
    int parity;                    // which of the two carries holds the old samples; the other receives the new ones
    int reserved;
    long long out_first, out_count;    // the plan's range
    long long before;              // samples the series held before this push
    long long carry_first;         // index in the series of the carry's first sample
    long long total;               // samples after this push
    long long next_first;          // index in the series of the new carry's first sample
};
struct ResampleStreamArgs {
    ResampleRatio q;
    int dtype, C, S, n_max;
    float gain;
    const ResampleSlotRow* rows;   // [S + 1]
    const void* chunk;             // [S, n_max, C]
    float* carry;                  // [S, 2, carry_len] mono
    long long carry_len;
    float* out;                    // [S, out_capacity]: slot s's new outputs from column 0 on
    long long out_capacity;
    const float* tab;
};
void launch_resample_stream(const ResampleStreamArgs& a, int total_tiles);      // total_tiles may be 0: nothing is launched
void launch_resample_carry(const ResampleStreamArgs& a);                        // old carry + chunk -> the other carry, per slot

}  // namespace ls
