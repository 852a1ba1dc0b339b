// The host-only plan of the score stream (ls_score_stream_plan): the one definition of the audio frames a push decides.  It includes
// neither HIP nor the handle, so tests/score_plan_main.cpp links this unit alone under the host sanitizers.
//   frame f covers samples [512 f - 1024, 512 f + 1024): it is decided once the series holds 512 f + 1024 samples -- everything to
//   its right is there, so the end padding cannot reach it -- and, under reflect padding, 1025 (the start padding of frames 0 and 1
//   reads sample 1024).  A finish decides what is left below F = 1 + L / 512, with the end padding at the series' own last sample.
#include <cstdint>

#include "ls_hip.h"

namespace {

constexpr int64_t kHop = 512, kHalf = 1024, kMaxSamples = 0x7fffffffLL - 2047;       // 2^31 - 2048

// the frames decided by `n` samples of a series that goes on
int64_t decided(int32_t pad_mode, int64_t n) {
    if (n < kHalf + (pad_mode == LS_ONSETS_PAD_REFLECT ? 1 : 0)) return 0;
    return (n - kHalf) / kHop + 1;
}

}  // namespace

extern "C" int ls_score_stream_plan(int32_t pad_mode, int64_t samples_before, int64_t n_new, int32_t finishing, int64_t* frame_first,
                                    int32_t* frame_count) {
    if (!frame_first || !frame_count) return LS_EINVAL;
    if (pad_mode != LS_ONSETS_PAD_CONSTANT && pad_mode != LS_ONSETS_PAD_REFLECT) return LS_EINVAL;
    if (samples_before < 0 || n_new < 0 || samples_before > kMaxSamples || n_new > kMaxSamples) return LS_EINVAL;
    const int64_t L = samples_before + n_new;
    if (L > kMaxSamples) return LS_EINVAL;
    if (finishing && (L < 1 || (pad_mode == LS_ONSETS_PAD_REFLECT && L <= kHalf))) return LS_EINVAL;
    const int64_t first = decided(pad_mode, samples_before);
    const int64_t end = finishing ? 1 + L / kHop : decided(pad_mode, L);
    *frame_first = first;
    *frame_count = (int32_t)(end - first);
    return LS_OK;
}
