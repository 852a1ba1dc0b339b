// The plans of the chained-window engine (ls_chain_api.cpp): which clips run which window of a ragged call, which windows a timeline
// edit runs (and which clips run each of them in its compact form), which windows a push of a stream runs, which rounds a push of a
// session pool runs, at which keys its rows draw and into which sampling calls pinned poses split them, which copies feed the slots' rings.  Every edit plan is made from PAIR FLAGS
// (edit_plan_of_flags): the range form and the element-mask form (ls_long_edit_plan_mask) differ only in how the flags come about.
// Integer arithmetic on host arrays, no HIP in here: each is the single definition for its entry and for Python (long_form.py), and
// tests/chain_plan_main.cpp, tests/pool_plan_main.cpp, tests/pool_keys_main.cpp, tests/pool_pin_plan_main.cpp, tests/edit_plan_main.cpp and
// tests/edit_mask_plan_main.cpp run them on their edges under the host sanitizers.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "ls_hip.h"

namespace ls {

// The plan of a ragged long-form call (ls_long_plan_drop): windows per clip from plan_windows' arithmetic (long_form.py), the clips
// stably sorted by them, longest first, and per window the clips that run it.  Declared in ls_handle.h for ls_long_prepare_ragged.
void long_plan_drop(int B, int AL, const int64_t* lengths, std::vector<int>& row, std::vector<int>& wins, std::vector<int>& bw) {
    std::vector<int> wb((size_t)B);
    int wmax = 1;
    for (int b = 0; b < B; ++b) {
        const long long over = (long long)lengths[b] - AL;
        wb[(size_t)b] = over <= 0 ? 1 : (int)((over + LS_LONG_AUDIO_STRIDE - 1) / LS_LONG_AUDIO_STRIDE) + 1;
        if (wb[(size_t)b] > wmax) wmax = wb[(size_t)b];
    }
    row.resize((size_t)B); wins.resize((size_t)B);
    for (int b = 0; b < B; ++b) row[(size_t)b] = b;
    std::stable_sort(row.begin(), row.end(), [&](int x, int y) { return wb[(size_t)x] > wb[(size_t)y]; });      // descending; ties keep the caller's order
    for (int s = 0; s < B; ++s) wins[(size_t)s] = wb[(size_t)row[(size_t)s]];
    bw.assign((size_t)wmax, 0);                     // B_w = clips with W_b > w: count the clips that END at each w, then a running sum from the back
    for (int b = 0; b < B; ++b) ++bw[(size_t)wb[(size_t)b] - 1];
    for (int w = wmax - 2; w >= 0; --w) bw[(size_t)w] += bw[(size_t)w + 1];
}

// The copies that feed a session's rings (ls_chain_api.cpp: feed): slot s takes take[s] new samples, from column from[s] of its row of
// the caller's chunk to position pos[s] of its ring of R samples.  Consecutive slots with the same (pos, from, take), take > 0, form
// a run, and a run is one strided copy -- two where it passes the ring's end.  Every run is maximal, so a stream (all slots alike) is
// one run whatever its batch.  Five ints per copy: first slot, slots, ring position, offset into the take, samples.  Declared in
// ls_handle.h.
void feed_copies(int S, int R, const int* pos, const long long* from, const int* take, std::vector<int>& copies) {
    copies.clear();
    for (int s = 0, n; s < S; s += n) {
        for (n = 1; take[s] > 0 && s + n < S && pos[s + n] == pos[s] && from[s + n] == from[s] && take[s + n] == take[s];) ++n;
        if (take[s] <= 0) continue;
        const int seg1 = take[s] < R - pos[s] ? take[s] : R - pos[s];
        copies.insert(copies.end(), {s, n, pos[s], 0, seg1});
        if (take[s] > seg1) copies.insert(copies.end(), {s, n, 0, seg1, take[s] - seg1});
    }
}

// ---- The plan of a timeline edit FROM PAIR FLAGS: flags [W][B], non-zero where clip b has an editable element in window w.  The one
// definition every edit entry shares -- a range, a host mask and a device mask (k_edit_mask_pairs) all reduce to flags first: the
// windows that run are those some clip flags, ascending; the rows of a window are its flagged clips, ascending; counts per window,
// n_pairs = sum.  Capacities as in ls_long_edit_plan_compact: null arrays with zero capacities count alone, LS_EINVAL where an
// array does not hold the plan.  Declared in ls_handle.h.
int edit_plan_of_flags(int B, int W, const unsigned char* flags, int32_t* windows, int32_t* counts, int32_t window_capacity, int32_t* rows,
                       int32_t row_capacity, int32_t* n_windows_run, int32_t* n_pairs) {
    long long nw = 0, np = 0;
    for (int w = 0; w < W; ++w) {
        const unsigned char* fw = flags + (size_t)w * B;
        int n = 0;
        for (int b = 0; b < B; ++b) {
            if (!fw[b]) continue;
            if (rows) { if (np + n >= row_capacity) return LS_EINVAL; rows[np + n] = b; }
            ++n;
        }
        if (n == 0) continue;
        if (windows) { if (nw >= window_capacity) return LS_EINVAL; windows[nw] = w; counts[nw] = n; }
        ++nw; np += n;
        if (np > INT32_MAX) return LS_EINVAL;
    }
    *n_windows_run = (int32_t)nw;
    *n_pairs = (int32_t)np;
    return LS_OK;
}

// the windows of each clip: all W, or with frames (a ragged batch) W_b = (frames[b] - T) / S + 1; false: a frames[b] that is no
// stitched length T + k S with 0 <= k < W
static bool clip_windows(int B, int W, int T, int n_pre, const int32_t* frames, std::vector<int>& wb) {
    const long long S = T - n_pre, Tt = T + (long long)(W - 1) * S;
    wb.assign((size_t)B, W);
    for (int b = 0; b < B && frames; ++b) {
        if (frames[b] < T || frames[b] > Tt || (frames[b] - T) % S) return false;
        wb[(size_t)b] = (int)((frames[b] - T) / S) + 1;
    }
    return true;
}

// The flags of the RANGE form: clip b, window w iff [lo_b, hi_b) meets the frames w owns, the clip has a selected channel (any[b]) and
// w < wb[b].  The ranges are the caller's to check.
static void range_flags(int B, int W, int T, int n_pre, const int32_t* lo, const int32_t* hi, const char* any, const int* wb, std::vector<unsigned char>& flags) {
    const long long S = T - n_pre;
    flags.assign((size_t)W * B, 0);
    for (int w = 0; w < W; ++w) {
        const long long own_lo = w ? w * S + n_pre : 0, own_hi = w * S + T;
        for (int b = 0; b < B; ++b)
            flags[(size_t)w * B + b] = (!any || any[b]) && w < wb[b] && (lo[b] > own_lo ? lo[b] : own_lo) < (hi[b] < own_hi ? hi[b] : own_hi);
    }
}

// The flags of a HOST element mask [B][JF][T + (W - 1) S]: the OR over the frames w owns and all channels -- what k_edit_mask_pairs
// computes for a mask on the device.  Every frame has one owner, so one pass over the mask's rows does it.  LS_EINVAL: a frames[b]
// that is no stitched length, or a set byte at or beyond frames[b].  Declared in ls_handle.h.
int edit_mask_flags(int B, int W, int T, int n_pre, int JF, const unsigned char* mask, const int32_t* frames, std::vector<unsigned char>& flags) {
    std::vector<int> wb;
    if (!clip_windows(B, W, T, n_pre, frames, wb)) return LS_EINVAL;
    const long long S = T - n_pre, Tt = T + (long long)(W - 1) * S;
    flags.assign((size_t)W * B, 0);
    for (int b = 0; b < B; ++b) {
        const long long most = T + (long long)(wb[(size_t)b] - 1) * S;
        for (int c = 0; c < JF; ++c) {
            const unsigned char* m = mask + ((size_t)b * JF + c) * (size_t)Tt;
            for (long long n = 0; n < Tt; ++n) {
                if (!m[n]) continue;
                if (n >= most) return LS_EINVAL;
                flags[(size_t)(n < T ? 0 : (n - n_pre) / S) * B + b] = 1;      // the owner of frame n
            }
        }
    }
    return LS_OK;
}

}  // namespace ls

extern "C" {

int ls_long_plan_drop(int32_t batch, int32_t audio_len, const int64_t* audio_lengths, int32_t* slot_row, int32_t* slot_windows,
                      int32_t* active, int32_t active_capacity, int32_t* n_windows) {
    if (batch < 1 || audio_len < 1 || !audio_lengths || !n_windows || active_capacity < 0 || (active_capacity > 0 && !active)) return LS_EINVAL;
    for (int b = 0; b < batch; ++b)
        if (audio_lengths[b] < 1 || (audio_lengths[b] - audio_len) / LS_LONG_AUDIO_STRIDE > (1 << 20)) return LS_EINVAL;
    std::vector<int> row, wins, bw;
    ls::long_plan_drop(batch, audio_len, audio_lengths, row, wins, bw);
    for (int s = 0; s < batch; ++s) {
        if (slot_row) slot_row[s] = row[(size_t)s];
        if (slot_windows) slot_windows[s] = wins[(size_t)s];
    }
    for (int w = 0; w < (int)bw.size() && w < active_capacity; ++w) active[w] = bw[(size_t)w];
    *n_windows = (int32_t)bw.size();
    return LS_OK;
}

// The windows a timeline edit runs (ls_long_edit_args in ls_hip.h): window w owns the frames [w S + n_pre, w S + T) ([0, T) for w = 0) and
// runs when the range of some clip meets them.
int ls_long_edit_plan(int32_t batch, int32_t n_windows, int32_t T, int32_t n_pre, const int32_t* lo, const int32_t* hi, int32_t* window_flags,
                      int32_t* n_out) {
    if (batch < 1 || n_windows < 1 || n_pre < 1 || T <= n_pre || !lo || !hi || !n_out) return LS_EINVAL;
    const long long Tt = T + (long long)(n_windows - 1) * (T - n_pre);
    for (int b = 0; b < batch; ++b)
        if (lo[b] < 0 || lo[b] > hi[b] || hi[b] > Tt) return LS_EINVAL;
    std::vector<unsigned char> flags;
    const std::vector<int> wb((size_t)batch, n_windows);
    ls::range_flags(batch, n_windows, T, n_pre, lo, hi, nullptr, wb.data(), flags);
    int n = 0;
    for (int w = 0; w < n_windows; ++w) {
        bool run = false;
        for (int b = 0; b < batch && !run; ++b) run = flags[(size_t)w * batch + b] != 0;
        if (window_flags) window_flags[w] = run ? 1 : 0;
        n += run ? 1 : 0;
    }
    *n_out = n;
    return LS_OK;
}

// The clip-windows a COMPACT timeline edit runs (ls_long_edit_compact_args in ls_hip.h).  The pair (b, w) is in the plan iff clip b has
// an editable element in window w by ls_long_edit_plan's rule -- its range meets the frames w owns, and one of its channels is
// selected -- and, with `frames`, w is one of the clip's own W_b = (frames[b] - T) / S + 1 windows.  Window w runs iff some pair names
// it; its rows are the clips of its pairs, ascending; the windows run ascending.  Property: without `frames` the windows that run
// are exactly ls_long_edit_plan's for the same ranges (a clip without a selected channel folded to lo == hi), since both test the
// same intersection clip by clip.
int ls_long_edit_plan_compact(int32_t batch, int32_t n_windows, int32_t T, int32_t n_pre, const int32_t* lo, const int32_t* hi,
                              const unsigned char* channels, int32_t n_channels, const int32_t* frames, int32_t* windows, int32_t* counts,
                              int32_t window_capacity, int32_t* rows, int32_t row_capacity, int32_t* n_windows_run, int32_t* n_pairs) {
    if (batch < 1 || n_windows < 1 || n_pre < 1 || T <= n_pre || !lo || !hi || !n_windows_run || !n_pairs) return LS_EINVAL;
    if ((channels && n_channels < 1) || window_capacity < 0 || row_capacity < 0) return LS_EINVAL;
    if ((window_capacity > 0 && (!windows || !counts)) || (row_capacity > 0 && !rows)) return LS_EINVAL;
    const long long Tt = T + (long long)(n_windows - 1) * (T - n_pre);
    std::vector<int> wb;
    if (!ls::clip_windows(batch, n_windows, T, n_pre, frames, wb)) return LS_EINVAL;
    std::vector<char> any((size_t)batch, 1);
    for (int b = 0; b < batch; ++b) {
        const long long most = frames ? frames[b] : Tt;
        if (lo[b] < 0 || lo[b] > hi[b] || hi[b] > most) return LS_EINVAL;
        if (channels) {
            any[(size_t)b] = 0;
            for (int c = 0; c < n_channels && !any[(size_t)b]; ++c) any[(size_t)b] = channels[(size_t)b * n_channels + c] != 0;
        }
    }
    std::vector<unsigned char> flags;
    ls::range_flags(batch, n_windows, T, n_pre, lo, hi, any.data(), wb.data(), flags);
    return ls::edit_plan_of_flags(batch, n_windows, flags.data(), windows, counts, window_capacity, rows, row_capacity, n_windows_run, n_pairs);
}

// The plan of a timeline edit by ELEMENT MASK (ls_long_edit_mask and its kin in ls_hip.h): mask bytes [batch][n_channels][T + (W - 1) S]
// on the HOST, non-zero = editable.  The pair (b, w) is in the plan iff the clip has a set byte on a frame w owns; the rest is
// ls_long_edit_plan_compact's, through the same flags.
int ls_long_edit_plan_mask(int32_t batch, int32_t n_windows, int32_t T, int32_t n_pre, const unsigned char* mask, int32_t n_channels,
                           const int32_t* frames, int32_t* windows, int32_t* counts, int32_t window_capacity, int32_t* rows, int32_t row_capacity,
                           int32_t* n_windows_run, int32_t* n_pairs) {
    if (batch < 1 || n_windows < 1 || n_pre < 1 || T <= n_pre || !mask || n_channels < 1 || !n_windows_run || !n_pairs) return LS_EINVAL;
    if (window_capacity < 0 || row_capacity < 0 || (window_capacity > 0 && (!windows || !counts)) || (row_capacity > 0 && !rows)) return LS_EINVAL;
    std::vector<unsigned char> flags;
    if (ls::edit_mask_flags(batch, n_windows, T, n_pre, n_channels, mask, frames, flags) != LS_OK) return LS_EINVAL;
    return ls::edit_plan_of_flags(batch, n_windows, flags.data(), windows, counts, window_capacity, rows, row_capacity, n_windows_run, n_pairs);
}

// The windows one call of a stream runs (ls_long_stream_push_args in ls_hip.h): window w is complete once audio_stride * w + audio_len
// samples have arrived; the closing call adds the windows plan_windows' arithmetic (long_form.py) still owes for the total.
int ls_long_stream_plan(int64_t samples_before, int64_t samples_new, int32_t audio_len, int32_t closing, int64_t* first_window, int64_t* n_windows) {
    if (samples_before < 0 || samples_new < 0 || audio_len < 1 || !first_window || !n_windows) return LS_EINVAL;
    if (samples_before > INT64_MAX - samples_new) return LS_EINVAL;
    const int64_t S = LS_LONG_AUDIO_STRIDE, AL = audio_len, total = samples_before + samples_new;
    auto complete = [&](int64_t n) { return n < AL ? (int64_t)0 : (n - AL) / S + 1; };
    int64_t last = complete(total);
    if (closing) {
        if (total < 1) return LS_EINVAL;        // a waveform without a sample has no windows (plan_windows)
        const int64_t cover = total > AL ? (total - AL - 1) / S + 2 : 1;      // ceil((total - AL) / S) + 1 without the sum that can pass INT64_MAX
        if (cover > last) last = cover;
    }
    *first_window = complete(samples_before);
    *n_windows = last - *first_window;
    return LS_OK;
}

// The rounds one push of a session pool runs (ls_long_pool_push_args in ls_hip.h).  Each open slot is a stream of its own, and its
// windows are ls_long_stream_plan's; round r holds the slots that run at least r + 1 windows, in ascending slot order.
int ls_long_pool_plan(int32_t n_slots, int32_t audio_len, const int64_t* samples_in, const int64_t* windows_run, const int64_t* samples_new,
                      const int32_t* closing, const int32_t* open, int32_t* n_windows, int32_t* frames, int32_t* round_slots,
                      int32_t round_capacity, int32_t* n_rounds, int32_t* n_entries) {
    if (n_slots < 1 || audio_len < 1 || !samples_in || !windows_run || !samples_new || !closing || !open || !n_windows || !n_rounds || !n_entries) return LS_EINVAL;
    if (round_capacity < 0 || (round_capacity > 0 && !round_slots)) return LS_EINVAL;
    const int64_t kMost = 1 << 20;              // windows of one slot in one call (ls_long_plan_drop's cap on a clip)
    int64_t rounds = 0, entries = 0;
    for (int s = 0; s < n_slots; ++s) {
        if (samples_in[s] < 0 || windows_run[s] < 0 || samples_new[s] < 0) return LS_EINVAL;
        int64_t first = 0, k = 0;
        if (!open[s]) {
            if (samples_new[s] > 0) return LS_EINVAL;           // samples for a slot that is not open
        } else {
            if (ls_long_stream_plan(samples_in[s], samples_new[s], audio_len, closing[s] ? 1 : 0, &first, &k) != LS_OK) return LS_EINVAL;
            if (first != windows_run[s] || k > kMost) return LS_EINVAL;
        }
        n_windows[s] = (int32_t)k;
        if (frames) frames[s] = (int32_t)(k == 0 ? 0 : 30 * k + (first == 0 ? 4 : 0));     // 34 for window 0, 30 for each later one
        if (k > rounds) rounds = k;
        entries += k;
        if (entries > INT32_MAX) return LS_EINVAL;
    }
    if (round_slots) {
        if (entries > round_capacity) return LS_EINVAL;
        int64_t p = 0;
        for (int64_t r = 0; r < rounds; ++r)
            for (int s = 0; s < n_slots; ++s)
                if (n_windows[s] > r) round_slots[p++] = s;
    }
    *n_rounds = (int32_t)rounds;
    *n_entries = (int32_t)entries;
    return LS_OK;
}

// The key table of a keyed pool's push (ls_long_pool_keyed in ls_hip.h), in ls_long_pool_plan's order: round r holds the slots with
// n_windows[s] > r, ascending, and the row of slot s there draws at keys[s] + ((windows_run[s] + r) << 48) -- the slot's key and the
// slot's OWN window, whatever runs beside it and however many rounds the pool has run.  Only slots that run a window are looked at.
int ls_long_pool_keys(int32_t n_slots, const uint64_t* keys, const int64_t* windows_run, const int32_t* n_windows, uint64_t* row_keys,
                      int32_t row_capacity, int32_t* n_entries) {
    if (n_slots < 1 || !keys || !windows_run || !n_windows || !n_entries || row_capacity < 0 || (row_capacity > 0 && !row_keys)) return LS_EINVAL;
    int64_t rounds = 0, entries = 0;
    for (int s = 0; s < n_slots; ++s) {
        if (n_windows[s] < 0 || windows_run[s] < 0) return LS_EINVAL;
        if (n_windows[s] == 0) continue;
        if (keys[s] >> 48) return LS_EINVAL;                                    // the window index sits above bit 47
        if (windows_run[s] > (1 << 16) - (int64_t)n_windows[s]) return LS_ESTATE;       // a clip's windows stay below 2^16
        if (n_windows[s] > rounds) rounds = n_windows[s];
        entries += n_windows[s];
        if (entries > INT32_MAX) return LS_EINVAL;
    }
    if (row_keys) {
        if (entries > row_capacity) return LS_EINVAL;
        int64_t p = 0;
        for (int64_t r = 0; r < rounds; ++r)
            for (int s = 0; s < n_slots; ++s)
                if (n_windows[s] > r) row_keys[p++] = keys[s] + ((uint64_t)(windows_run[s] + r) << 48);
    }
    *n_entries = (int32_t)entries;
    return LS_OK;
}

// The sampling calls of a push of a session with pinned poses (ls_long_pool_pins in ls_hip.h), in ls_long_pool_plan's round order:
// in round r slot s (n_windows[s] > r) runs its window w = windows_run[s] + r, which owns the series frames [0, T) for w = 0 and
// [w S + n_pre, w S + T) otherwise (S = T - n_pre); its row is PINNED iff one of the slot's pending pinned frames is among them.
// The round becomes its unpinned rows, ascending, as one call, then its pinned rows, ascending, as another; an empty half is no
// call.  Without a pending frame the calls are the rounds.
int ls_long_pool_pin_plan(int32_t n_slots, int32_t T, int32_t n_pre, const int64_t* windows_run, const int32_t* n_windows,
                          const int32_t* pin_first, const int64_t* pin_frames, int32_t* call_rows, int32_t row_capacity,
                          int32_t* call_counts, int32_t* call_pinned, int32_t* call_rounds, int32_t call_capacity, int32_t* n_calls,
                          int32_t* n_entries) {
    if (n_slots < 1 || n_pre < 1 || T <= n_pre || !windows_run || !n_windows || !n_calls || !n_entries) return LS_EINVAL;
    if (row_capacity < 0 || call_capacity < 0 || (row_capacity > 0 && !call_rows)) return LS_EINVAL;
    if (!pin_first && pin_frames) return LS_EINVAL;
    if (pin_first && !pin_frames && pin_first[n_slots] != pin_first[0]) return LS_EINVAL;
    const int64_t S = T - n_pre;
    int64_t rounds = 0, entries = 0;
    for (int s = 0; s < n_slots; ++s) {
        if (n_windows[s] < 0 || n_windows[s] > (1 << 20) || windows_run[s] < 0 || windows_run[s] > (INT64_MAX - T) / S - n_windows[s]) return LS_EINVAL;
        if (n_windows[s] > rounds) rounds = n_windows[s];
        entries += n_windows[s];
        if (entries > INT32_MAX) return LS_EINVAL;
        if (pin_first) {
            if ((s == 0 && pin_first[0] != 0) || pin_first[s + 1] < pin_first[s]) return LS_EINVAL;
            for (int32_t i = pin_first[s]; i < pin_first[s + 1]; ++i)
                if (pin_frames[i] < 0) return LS_EINVAL;
        }
    }
    int64_t calls = 0, p = 0;
    for (int64_t r = 0; r < rounds; ++r)
        for (int half = 0; half < 2; ++half) {          // the unpinned rows, then the pinned ones
            int32_t n = 0;
            for (int s = 0; s < n_slots; ++s) {
                if (n_windows[s] <= r) continue;
                const int64_t w = windows_run[s] + r, lo = w ? w * S + n_pre : 0, hi = w * S + T;
                bool pinned = false;
                for (int32_t i = pin_first ? pin_first[s] : 0; pin_first && i < pin_first[s + 1] && !pinned; ++i)
                    pinned = pin_frames[i] >= lo && pin_frames[i] < hi;
                if (pinned != (half == 1)) continue;
                if (call_rows) { if (p + n >= row_capacity) return LS_EINVAL; call_rows[p + n] = s; }
                ++n;
            }
            if (n == 0) continue;
            if (call_counts || call_pinned || call_rounds) {
                if (calls >= call_capacity) return LS_EINVAL;
                if (call_counts) call_counts[calls] = n;
                if (call_pinned) call_pinned[calls] = half;
                if (call_rounds) call_rounds[calls] = (int32_t)r;
            }
            ++calls; p += n;
        }
    *n_calls = (int32_t)calls;
    *n_entries = (int32_t)entries;
    return LS_OK;
}

}  // extern "C"
