// The plan of the dataset ingest (ls_ingest.hip): which raw frames every resampled frame is interpolated from, and where every
// window starts in its recording's frames and audio.  No HIP in here: the reference computes all of it in Python floats, so it is
// restated in double, operation by operation and in the same order, and ls_ingest_plan hands the tables out so that they can be
// checked against numpy and scipy without a GPU.
//   TED   scripts/data_loader/data_preprocessor.py:80-128, scripts/utils/data_utils.py:46-56
//   BEAT  scripts_beat/dataloaders/beat.py:364-372, 392-404
#include <cmath>
#include <cstdint>

#include "ls_hip.h"

namespace ls {
namespace {

// DataPreprocessor.get_words_in_time_range (data_preprocessor.py:174-188) on one recording's sorted (start, end) rows: a window
// needs at least two words
bool has_two_words(const double* words, int64_t first, int64_t last, double start_time, double end_time) {
    int found = 0;
    for (int64_t w = first; w < last; ++w) {
        if (words[2 * w] >= end_time) break;
        if (words[2 * w + 1] <= start_time) continue;
        if (++found >= 2) return true;
    }
    return false;
}

struct Tables {
    ls_ingest_plan_args* a;
    int64_t frames = 0, windows = 0;
    bool frame(int clip, int lo, double frac) {
        if (a->frame_clip || a->frame_lo || a->frame_hi || a->frame_frac) {
            if (frames >= a->frame_cap) return false;
            if (a->frame_clip) a->frame_clip[frames] = clip;
            if (a->frame_lo) a->frame_lo[frames] = lo;
            if (a->frame_hi) a->frame_hi[frames] = lo + 1;
            if (a->frame_frac) a->frame_frac[frames] = (float)frac;
        }
        ++frames;
        return frames <= INT32_MAX;
    }
    bool window(int clip, int64_t first, int64_t audio_start, int64_t n_pad, bool words) {
        if (a->win_clip || a->win_first || a->win_audio_start || a->win_n_pad || a->win_has_words) {
            if (windows >= a->window_cap) return false;
            if (a->win_clip) a->win_clip[windows] = clip;
            if (a->win_first) a->win_first[windows] = (int32_t)first;
            if (a->win_audio_start) a->win_audio_start[windows] = audio_start;
            if (a->win_n_pad) a->win_n_pad[windows] = (int32_t)n_pad;
            if (a->win_has_words) a->win_has_words[windows] = words ? 1 : 0;
        }
        ++windows;
        return windows <= INT32_MAX;
    }
};

}  // namespace
}  // namespace ls

extern "C" int ls_ingest_plan(ls_ingest_plan_args* a) {
    using namespace ls;
    if (!a || !a->n_raw || !a->start_time || !a->end_time || !a->audio_len || a->batch < 1) return LS_EINVAL;
    if (a->n_poses < 1 || a->n_poses > LS_INGEST_MAX_POSES || a->n_ext < a->n_poses || a->n_ext > LS_INGEST_MAX_EXT || a->stride < 1)
        return LS_EINVAL;
    if (!(a->fps > 0.0) || !(a->sr > 0.0) || a->frame_cap < 0 || a->window_cap < 0) return LS_EINVAL;
    if (a->word_offsets) {
        if (!a->word_times || a->word_offsets[0] != 0) return LS_EINVAL;
        for (int b = 0; b < a->batch; ++b)
            if (a->word_offsets[b + 1] < a->word_offsets[b]) return LS_EINVAL;
    }
    Tables t{a};
    const int64_t audio_window = (int64_t)((double)a->n_ext / a->fps * a->sr);      // int(n / fps * 16000), math.floor for BEAT: > 0 either way
    for (int b = 0; b < a->batch; ++b) {
        const int64_t n = a->n_raw[b], L = a->audio_len[b];
        const double s_t = a->start_time[b], e_t = a->end_time[b];
        if (n < 2 || L < 1 || (!a->beat && !(e_t > s_t))) return LS_EINVAL;      // BEAT: nothing left between the clean seconds, no window
        if (a->frame_offsets) a->frame_offsets[b] = (int32_t)t.frames;
        if (a->window_offsets) a->window_offsets[b] = (int32_t)t.windows;
        int64_t K, first0, audio0, audio_end_limit;
        if (!a->beat) {
            const double expected_n = (e_t - s_t) * a->fps;                          // resample_pose_seq
            const double step = (double)n / expected_n;
            const double count = std::ceil((double)n / step);                        // len(np.arange(0, n, step))
            if (!(count >= 1.0) || count > (double)INT32_MAX) return LS_EINVAL;
            K = (int64_t)count;
            for (int64_t i = 0; i < K; ++i) {
                const double x = (double)i * step;                                   // arange: start + i * delta
                int64_t idx = x > (double)(n - 1) ? n : (int64_t)std::ceil(x);       // searchsorted(arange(n), x), side left
                idx = idx < 1 ? 1 : (idx > n - 1 ? n - 1 : idx);
                if (!t.frame(b, (int)(idx - 1), x - (double)(idx - 1))) return LS_EINVAL;
            }
            first0 = 0; audio0 = 0; audio_end_limit = L;
        } else {                                                                     // whole seconds of an already 15 fps recording
            const int64_t s_f = std::llround(s_t * a->fps), e_f = std::llround(e_t * a->fps);
            audio0 = std::llround(s_t * a->sr);
            audio_end_limit = std::llround(e_t * a->sr);
            if (s_f < 0 || audio0 < 0 || e_f > n || audio_end_limit > L) return LS_EINVAL;
            K = e_f - s_f;
            first0 = s_f;
        }
        const int64_t n_sub = (int64_t)std::floor((double)(K - a->n_ext) / (double)a->stride) + 1;
        const int64_t w0 = a->word_offsets ? a->word_offsets[b] : 0, w1 = a->word_offsets ? a->word_offsets[b + 1] : 0;
        for (int64_t i = 0; i < n_sub; ++i) {
            const int64_t start_idx = i * a->stride;
            const int64_t audio_start = a->beat ? audio0 + (int64_t)std::floor((double)(start_idx * (int64_t)a->sr) / a->fps)
                                                : (int64_t)std::floor((double)start_idx / (double)K * (double)L);
            const int64_t audio_end = audio_start + audio_window;
            const int64_t n_pad = audio_end > audio_end_limit ? audio_end - audio_end_limit : 0;
            if (n_pad > L) return LS_EINVAL;                                         // np.pad would reflect more than once
            const double w_s = s_t + (double)start_idx / a->fps, w_e = s_t + (double)(start_idx + a->n_ext) / a->fps;
            const bool words = !a->word_offsets || has_two_words(a->word_times, w0, w1, w_s, w_e);
            if (!t.window(b, first0 + start_idx, audio_start, n_pad, words)) return LS_EINVAL;
        }
    }
    if (a->frame_offsets) a->frame_offsets[a->batch] = (int32_t)t.frames;
    if (a->window_offsets) a->window_offsets[a->batch] = (int32_t)t.windows;
    a->n_frames = (int32_t)t.frames;
    a->n_windows = (int32_t)t.windows;
    return LS_OK;
}
