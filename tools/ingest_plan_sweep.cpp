// Stand-alone host program for a sanitizer run of ls_ingest_plan (csrc/ls_ingest_plan.cpp; no GPU, no HIP): the sweep of
// tests/test_ingest_host.py -- n in 2..120, fps 10 / 15 / 25, durations on and beside whole frame counts, audio short enough to be
// padded, word lists -- with every output array allocated at exactly the size the counting call reported, so that a row written
// past its table is an AddressSanitizer error, and the refusals.  Build and run:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/ingest_plan_sweep.cpp \
//       livelyspeaker_amd/csrc/ls_ingest_plan.cpp -o build/ingest_plan_sweep && build/ingest_plan_sweep
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ls_hip.h"

namespace {

struct Batch {
    std::vector<int32_t> n_raw;
    std::vector<double> start, end;
    std::vector<int64_t> audio_len, word_off{0};
    std::vector<double> words;
};

long long g_frames = 0, g_windows = 0, g_padded = 0, g_tails = 0, g_calls = 0;

int run(Batch& b, int beat, int n_poses, int n_ext, double fps, bool with_words) {
    ls_ingest_plan_args a{};
    a.batch = (int32_t)b.n_raw.size();
    a.n_poses = n_poses; a.n_ext = n_ext; a.stride = 10; a.beat = beat; a.fps = fps; a.sr = 16000.0;
    a.n_raw = b.n_raw.data(); a.start_time = b.start.data(); a.end_time = b.end.data(); a.audio_len = b.audio_len.data();
    if (with_words) { a.word_offsets = b.word_off.data(); a.word_times = b.words.data(); }
    int rc = ls_ingest_plan(&a);
    if (rc != LS_OK) return rc;
    const size_t F = (size_t)a.n_frames, W = (size_t)a.n_windows, B = (size_t)a.batch;
    std::vector<int32_t> f_off(B + 1), f_clip(F), f_lo(F), f_hi(F), w_off(B + 1), w_clip(W), w_first(W), w_pad(W);
    std::vector<float> f_frac(F);
    std::vector<int64_t> w_audio(W);
    std::vector<unsigned char> w_words(W);
    a.frame_cap = a.n_frames; a.window_cap = a.n_windows;
    a.frame_offsets = f_off.data(); a.frame_clip = f_clip.data(); a.frame_lo = f_lo.data(); a.frame_hi = f_hi.data();
    a.frame_frac = f_frac.data(); a.window_offsets = w_off.data(); a.win_clip = w_clip.data(); a.win_first = w_first.data();
    a.win_audio_start = w_audio.data(); a.win_n_pad = w_pad.data(); a.win_has_words = w_words.data();
    rc = ls_ingest_plan(&a);
    if (rc != LS_OK) return rc;
    if ((size_t)a.n_frames != F || (size_t)a.n_windows != W || f_off[B] != a.n_frames || w_off[B] != a.n_windows) return 100;
    for (size_t i = 0; i < F; ++i) {
        const int32_t n = b.n_raw[(size_t)f_clip[i]];
        if (f_lo[i] < 0 || f_hi[i] != f_lo[i] + 1 || f_hi[i] >= n || !(f_frac[i] >= 0.f)) return 101;
        g_tails += f_frac[i] > 1.f;
    }
    for (size_t w = 0; w < W; ++w) {
        const int64_t L = b.audio_len[(size_t)w_clip[w]];
        if (w_audio[w] < 0 || w_pad[w] < 0 || w_pad[w] > L || w_first[w] < 0) return 102;
        g_padded += w_pad[w] > 0;
    }
    if (W) {                                       // one row short: refused, and nothing written past the shorter arrays
        a.window_cap = a.n_windows - 1;
        w_clip.resize(W - 1); w_clip.shrink_to_fit();
        a.win_clip = w_clip.data();
        if (ls_ingest_plan(&a) != LS_EINVAL) return 103;
    }
    g_frames += (long long)F; g_windows += (long long)W; ++g_calls;
    return LS_OK;
}

}  // namespace

int main() {
    for (double fps : {10.0, 15.0, 25.0}) {
        for (int n = 2; n <= 120; ++n) {
            Batch b;
            const int ms[] = {n, 2 * n, n / 2 > 2 ? n / 2 : 2, (int)std::lround(n * 0.6) > 2 ? (int)std::lround(n * 0.6) : 2, 41, 42, 43, 7, 63};
            int k = 0;
            for (int m : ms) {
                const double d = (double)m / fps;
                for (double dur : {d, std::nextafter(d, 0.0), std::nextafter(d, 1e9), d * (1 - 1e-9), d * (1 + 1e-9), d + 1 / (3 * fps)}) {
                    const double s = 0.37 * (k++ % 11);
                    b.n_raw.push_back(n);
                    b.start.push_back(s);
                    b.end.push_back(s + dur);
                    const int64_t window = (int64_t)(42.0 / fps * 16000.0);
                    const int64_t L = (int64_t)(dur * 16000.0 * (k % 3 == 0 ? 0.8 : 1.0));
                    b.audio_len.push_back(L > window ? L : window);
                    for (int w = 0; w < k % 9; ++w) { b.words.push_back(s + 0.41 * w); b.words.push_back(s + 0.41 * w + 0.2); }
                    b.word_off.push_back((int64_t)b.words.size() / 2);
                }
            }
            for (bool words : {false, true}) {
                const int rc = run(b, 0, 34, 42, fps, words);
                if (rc != LS_OK) { std::printf("FAIL: fps %g n %d words %d -> %d\n", fps, n, (int)words, rc); return 1; }
            }
        }
    }
    for (int n = 34; n <= 600; n += 7) {                                     // BEAT: whole seconds of a 15 fps recording
        Batch b;
        const int64_t L = (int64_t)n * 16000 / 15 + 77;
        const int64_t seconds = std::min<int64_t>(n / 15, L / 16000);
        b.n_raw = {n}; b.start = {0.0}; b.end = {(double)seconds}; b.audio_len = {L};
        const int rc = run(b, 1, 34, 34, 15.0, false);
        if (rc != LS_OK) { std::printf("FAIL: beat n %d -> %d\n", n, rc); return 1; }
    }
    {                                                                        // the refusals
        Batch b;
        b.n_raw = {100}; b.start = {0.0}; b.end = {4.0}; b.audio_len = {64000};
        int bad = 0;
        bad += run(b, 0, 34, 42, 15.0, false) != LS_OK;
        b.audio_len = {0};     bad += run(b, 0, 34, 42, 15.0, false) != LS_EINVAL;
        b.audio_len = {20000}; bad += run(b, 0, 34, 42, 15.0, false) != LS_EINVAL;
        b.audio_len = {64000}; b.n_raw = {1}; bad += run(b, 0, 34, 42, 15.0, false) != LS_EINVAL;
        b.n_raw = {100};       bad += run(b, 0, 43, 42, 15.0, false) != LS_EINVAL;
        bad += run(b, 0, 34, 129, 15.0, false) != LS_EINVAL;
        bad += run(b, 0, 34, 42, 0.0, false) != LS_EINVAL;
        bad += ls_ingest_plan(nullptr) != LS_EINVAL;
        if (bad) { std::printf("FAIL: %d refusals answered otherwise\n", bad); return 1; }
    }
    std::printf("ok: %lld calls, %lld frame rows (%lld extrapolated), %lld windows (%lld padded)\n", g_calls, g_frames, g_tails, g_windows,
                g_padded);
    return 0;
}
