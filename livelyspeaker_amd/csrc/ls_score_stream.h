// What the score stream's handle (ls_score_stream_api.cpp) takes from the kernels: the tiled pick of ls_onsets_long.hip and the
// stream's own launches (ls_score_stream.hip).  Plain structs of device pointers; every launch goes to the null stream.
#pragma once
#include <hip/hip_runtime.h>

#include "ls_hip.h"

namespace ls {

// the tiled pick over B clips of F frames each (row stride F); see ls_onsets_long.hip
struct LongPickParams {
    int F, nT;                 // frames per clip, tiles of LS_SCORE_TILE frames per clip
    int pre_max, post_max, pre_avg, post_avg, wait;
    float delta;
    const float* mel_db;       // [B, F, 128] or NULL (a given envelope)
    const float* env;          // [B, F]: the envelope (given, or written by k_long_flux)
    float* env_out;            // [B, F]: where k_long_flux writes; for a given envelope the copy the caller asked for, or NULL
    const float* rms;          // [B, F] or NULL
    float* part;               // [2, B, nT] tile partials
    float* stat;               // [B, 3]: maximum of mel_db, minimum and maximum of the envelope
    int* cand;                 // [B, F]: tile t's flagged frames from t * LS_SCORE_TILE on
    int* ncand;                // [B, nT]
    int *count, *onset_raw, *onset_bt, *onset_bt_rms;      // count and onset_raw are required
};
// onset_detect's default windows in frames of `hop` samples for sr_pick, cut to F; fills pre_max .. wait
void long_pick_windows(LongPickParams* p, double sr_pick);
void launch_long_pick(const LongPickParams& p, int B);

// ---- the stream's spectrum: one wave per newly decided (slot, frame) ----
struct ScoreSlotRow {          // one per slot and launch, uploaded ahead of it
    int frame_off;             // prefix sum of the slots' new frames (row S: the total)
    int frame_first;           // the slot's first new frame
    int before;                // samples the series held before this push
    int carry_first;           // index in the series of the carry's first sample
    int total;                 // samples after this push: the length the end padding uses (reached only at a finish)
    int fresh;                 // new samples in the chunk
    int parity;                // which of the two carries holds the old samples; the other receives the new ones
    int next_first;            // index in the series of the new carry's first sample
};
constexpr int kScoreCarry = 2048 + 512;        // floats per carry
struct ScoreSpectrumArgs {
    int S, n_max, pad_mode;
    long long max_frames;      // per slot: row stride of mel_db (x 128) and rms
    const ScoreSlotRow* rows;  // [S + 1]
    const float* chunk;        // [S, n_max] or NULL (a finish)
    float* carry;              // [S, 2, kScoreCarry]
    const float* window;
    const float2* twiddle;
    const int* mel_ptr;
    const int* mel_col;
    const float* mel_w;
    float* mel_db;             // [S, max_frames, 128]
    float* rms;                // [S, max_frames]
};
void launch_score_spectrum(const ScoreSpectrumArgs& a, int total_frames);      // total_frames may be 0: nothing is launched
void launch_score_carry(const ScoreSpectrumArgs& a);                           // old carry + chunk -> the other carry, per slot

// beats[s, :count[s]] -> dst[s * max_entries + first[s] ...]; rows: [S][2] ints (first, count)
void launch_score_beats(const unsigned char* beats, int S, int stride, const int* first_count, unsigned char* dst, long long max_entries);

// ---- the alignment sums of one slot ----
struct ScoreAlignArgs {
    const unsigned char* beats;        // [n_entries]
    int n_entries;
    int* list;                         // [n_entries]: the set entries, ascending
    int* n_list;                       // [1]
    const int* onset_frames;           // the slab the score reads
    const int* onset_count;            // [1]
    int hop;
    double fps, sigma, rate;           // TED: rate = sr; BEAT: rate = time_rate
    double* align_sum;                 // TED
    int* n_beats;                      // TED
    float* align;                      // BEAT
};
void launch_score_align(const ScoreAlignArgs& a, bool beat);

}  // namespace ls
