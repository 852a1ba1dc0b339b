// One output of the polyphase resampler -- the arithmetic the one-shot kernel and the stream's kernel share, so a chunked series gives
// the bits of the whole one.  Included by ls_resample.hip only.
//   y[m] = sum_k h[m down - k up + half] x[k].  With t0 = m down + half, kmax = floor(t0 / up) and r = t0 mod up the taps of output m
//   are h[r + j up] at sample kmax - j, j = 0 .. T - 1: row r of the table `tab` [up][Tp] (the designed taps transposed; Tp = T rounded
//   up to 4, zero behind the last tap), which a lane walks front to back in float4 steps.  r is the phase (m down) mod up moved by the
//   constant half mod up.
//   THE ORDER: acc = 0, then acc = fma(tab[r][j], x(kmax - j), acc) for j = 0, 1, .. Tp - 1.  It depends on (up, down, half) alone.  A
//   sample that does not exist is read as 0, and fma(h, 0, acc) == acc for every acc this chain can hold (acc starts at +0), so such a
//   tap contributes nothing, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ls {

constexpr int kResampleTile = 256;        // outputs per workgroup
constexpr int kResampleStage = 4096;      // mono samples a workgroup stages in LDS, at most
constexpr int kResampleTapLds = 4096;     // floats of the tap table held in LDS when the whole table fits

struct ResampleRatio {
    long long up, down, half;
    int T, Tp;                 // taps per output, and the table's row stride
    int span;                  // samples a tile of kResampleTile outputs reads: ((tile - 1) down + up - 1) / up + Tp
    int staged;                // span <= kResampleStage: the tile's samples go through LDS
    int taps_in_lds;           // up * Tp <= kResampleTapLds
    int pass_through;          // in_sr == out_sr: the mixdown alone
};

// the mixdown of one frame of `C` interleaved channels: the float sum in channel order (int16: the exact int32 sum) times `gain`
template <class In>
__device__ __forceinline__ float mix_frame(const In* __restrict__ p, int C, float gain);

template <>
__device__ __forceinline__ float mix_frame<float>(const float* __restrict__ p, int C, float gain) {
    float s = p[0];
    for (int c = 1; c < C; ++c) s += p[c];
    return s * gain;
}

template <>
__device__ __forceinline__ float mix_frame<int16_t>(const int16_t* __restrict__ p, int C, float gain) {
    int s = p[0];
    for (int c = 1; c < C; ++c) s += p[c];
    return (float)s * gain;
}

// sample(k): the mono sample k of the series, 0 where there is none; tap(i): entry i of the row
template <class Sample, class Tap>
__device__ __forceinline__ float resample_output(Sample sample, Tap tap, long long kmax, int Tp) {
    float acc = 0.0f;
    for (int j = 0; j < Tp; j += 4) {
        const float4 h = tap(j);
        acc = __builtin_fmaf(h.x, sample(kmax - j), acc);
        acc = __builtin_fmaf(h.y, sample(kmax - j - 1), acc);
        acc = __builtin_fmaf(h.z, sample(kmax - j - 2), acc);
        acc = __builtin_fmaf(h.w, sample(kmax - j - 3), acc);
    }
    return acc;
}

}  // namespace ls
