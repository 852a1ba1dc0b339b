// What the post-processing stream's host side (ls_post_stream_api.cpp) and its kernels (ls_post_stream.hip) share: the carry sizes,
// the per-push slot table and the two launches.
#pragma once
#include <hip/hip_runtime.h>

#include "ls_hip.h"
#include "ls_post_frame.h"

namespace ls {

constexpr int kPsTile = LS_TIMELINE_TILE;                          // units (new frames or beat entries) per workgroup
constexpr int kPsSeries = 6;
constexpr int kPsTedCarry = 3;                                     // TED: raw frames n - 3 .. n - 1 of a slot, [S, J*3, 3]
constexpr int kPsBeatCarry = 2 * LS_POST_STREAM_MAX_ORDER + 1;     // BEAT: rows of six Euler triples, [S, 17, 18]; 2 order + 1 are live
constexpr int kPsBeatRow = kPsSeries * 3;
// most tiles a slot can have in one push: its units are max(new frames, beat entries) <= MAX_CHUNK + MAX_ORDER
constexpr int kPsSlotTiles = (LS_POST_STREAM_MAX_CHUNK + LS_POST_STREAM_MAX_ORDER + kPsTile - 1) / kPsTile;

// device arrays of one push: per slot the frames of its series before the push, its new frames and its finish flag; per workgroup
// the slot and the first unit of its tile
struct PostStreamTable {
    const long long* n;
    const int *k, *fin, *tile_slot, *tile_start;
};

struct TedStreamArgs {
    const float* frames;        // [S, J, 3, K]
    int K, Kb;
    PostStreamTable t;
    float* carry;
    float *aligned, *pose, *angle_diff;
    unsigned char* beat_mask;   // [S, Kb]
};

struct BeatStreamArgs {
    const float* frames;        // [S, J, 6, K]
    int K, Kb, J, order;
    int joint[kPsSeries];
    PostStreamTable t;
    float* carry;
    float *decoded, *euler;
    unsigned char* beat_mask;   // [S, 6, Kb]
};

// both return the launch's status; `tiles` >= 1
hipError_t launch_ted_post_stream(const PostParams& p, const TedStreamArgs& a, unsigned tiles, hipStream_t stream);
hipError_t launch_beat_post_stream(const BeatStreamArgs& a, unsigned tiles, hipStream_t stream);

}  // namespace ls
