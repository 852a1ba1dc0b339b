// The host-only half of the post-processing stream: which beat entries a push decides (ls_post_stream_plan) and the check a push
// runs ahead of any launch (ls_post_stream_check).  Nothing here touches a device; tests/post_stream_plan_main.cpp links this unit alone.
#include "ls_hip.h"

namespace {

constexpr int64_t kMaxFrames = (int64_t)1 << 62;

// entries of a series of n frames that no later frame can change: TED's beat at f needs angle_diff[f + 1], BEAT's minimum at f the
// velocity v[f + order], which needs frame f + order + 1
inline int64_t decided(int32_t dataset, int32_t order, int64_t n) {
    const int64_t d = dataset == 0 ? n - 1 : n - order - 1;
    return d > 0 ? d : 0;
}

}  // namespace

extern "C" int ls_post_stream_plan(int32_t dataset, int32_t order, int64_t n_before, int64_t n_new, int32_t finishing, int64_t* beat_first,
                                   int32_t* beat_count) {
    if (!beat_first || !beat_count || (dataset != 0 && dataset != 1)) return LS_EINVAL;
    if (dataset == 1 && (order < 1 || order > LS_POST_STREAM_MAX_ORDER)) return LS_EINVAL;
    if (n_before < 0 || n_new < 0 || n_before > kMaxFrames || n_new > kMaxFrames) return LS_EINVAL;
    const int64_t N = n_before + n_new;
    if (finishing && N < 1) return LS_EINVAL;
    const int64_t first = decided(dataset, order, n_before);
    // at the finish: every frame (TED: N - 1 is never a beat), every velocity (BEAT: V = N - 1 of them)
    const int64_t end = finishing ? (dataset == 0 ? N : N - 1) : decided(dataset, order, N);
    if (end - first > 0x7fffffffLL) return LS_EINVAL;
    *beat_first = first;
    *beat_count = (int32_t)(end - first);
    return LS_OK;
}

extern "C" int ls_post_stream_check(int32_t dataset, int32_t order, int32_t capacity, const int64_t* frames_in, int32_t K,
                                    const int32_t* counts, const int32_t* finish, int32_t beat_capacity, int64_t* beat_first,
                                    int32_t* beat_count) {
    if (capacity < 1 || !frames_in || !counts || K < 0 || K > LS_POST_STREAM_MAX_CHUNK || beat_capacity < 0) return LS_EINVAL;
    for (int32_t s = 0; s < capacity; ++s)
        if (counts[s] < 0 || counts[s] > K) return LS_EINVAL;
    for (int32_t s = 0; s < capacity; ++s)
        if (finish && finish[s] && frames_in[s] >= 0 && frames_in[s] + counts[s] < 1) return LS_ESTATE;
    for (int32_t s = 0; s < capacity; ++s) {
        int64_t first = 0;
        int32_t count = 0;
        const int rc = ls_post_stream_plan(dataset, order, frames_in[s], counts[s], finish ? finish[s] != 0 : 0, &first, &count);
        if (rc != LS_OK) return rc;
        if (count > beat_capacity) return LS_EINVAL;
        if (beat_first) beat_first[s] = first;
        if (beat_count) beat_count[s] = count;
    }
    return LS_OK;
}
