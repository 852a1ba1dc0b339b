// Host-only half of the entry points that take no handle (ls_ted_post, ls_beat_post, ls_beat_metrics, ls_beat_ldiv, ls_onsets[_ragged],
// the ls_*_timeline[_ragged] entries, ls_ted_beat_align): the host <-> device staging of one call, and the argument check the two
// BEAT metrics entries share.  (The TED configuration check both post entries share is post_params, next to PostParams.)
#pragma once
#include <deque>

#include "ls_hip.h"
#include "ls_host.h"

namespace ls {

// host <-> device staging of one call: with on_device the caller's pointers pass through (an output the kernels need although the
// caller left it out becomes a temporary); otherwise inputs are uploaded and outputs come back in finish().  The first HIP error
// is kept and no HIP call follows it; a caller launches only while `e == hipSuccess`.  Temporaries are freed with the object.
struct Staging {
    const bool on_device;
    hipError_t e = hipSuccess;
    std::deque<DevBuf> bufs;
    struct Down { void* dst; const void* src; size_t bytes; };
    std::vector<Down> downs;
    explicit Staging(bool dev) : on_device(dev) {}
    void chk(hipError_t x) { if (e == hipSuccess) e = x; }
    void* temp(size_t bytes) {                     // an empty table (a filterbank above fmax) still gets a pointer
        bufs.emplace_back();
        if (e == hipSuccess) chk(bufs.back().ensure(bytes ? bytes : 1));
        return bufs.back().p;
    }
    template <class T>
    const T* upload(const T* src, size_t count) {  // host data in both modes: tables, lengths, offsets
        void* d = temp(count * sizeof(T));
        if (count && e == hipSuccess) chk(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
        return static_cast<const T*>(d);
    }
    template <class T>
    const T* in(const T* src, size_t count) { return !src || on_device ? src : upload(src, count); }
    template <class T>
    T* out(T* dst, size_t count, bool needed = false) {
        if (on_device) return dst || !needed ? dst : static_cast<T*>(temp(count * sizeof(T)));
        if (!dst && !needed) return nullptr;
        T* d = static_cast<T*>(temp(count * sizeof(T)));
        if (dst) downs.push_back({dst, d, count * sizeof(T)});
        return d;
    }
    void fill(void* d, int byte, size_t bytes) {   // the padding value of a ragged call's output, ahead of the launch
        if (d && bytes && e == hipSuccess) chk(hipMemset(d, byte, bytes));
    }
    void sync() {
        chk(hipGetLastError());
        chk(hipDeviceSynchronize());
    }
    int copy_back() {                              // in registration order
        for (const Down& d : downs)
            if (e == hipSuccess) chk(hipMemcpy(d.dst, d.src, d.bytes, hipMemcpyDeviceToHost));
        return e == hipSuccess ? LS_OK : LS_EHIP;
    }
    int finish() {
        sync();
        return copy_back();
    }
};

// what ls_beat_metrics and the timeline metrics entries refuse alike (LS_EINVAL, ahead of any HIP call); `motion`: a velocity series
// is read, `n_onsets`: the length of onset_times.  Frame-count and grid bounds belong to the entry.
inline bool beat_metrics_args_ok(const ls_beat_metrics_args* a, bool* motion, long long* n_onsets) {
    constexpr int kSeries = 6;
    if (!a || !a->pred || a->batch < 1 || a->njoints < 1 || a->order < 1) return false;
    if (!a->target && (a->success || a->srgr_sum)) return false;              // SRGR needs the target planes
    if (a->align && (!a->onset_times || !a->onset_offsets)) return false;
    if (a->align_series < 0 || a->align_series >= kSeries) return false;
    *motion = a->vel || a->beat_mask || a->align;
    for (int s = 0; s < kSeries; ++s)
        if (*motion && (a->series_joint[s] < 0 || a->series_joint[s] >= a->njoints)) return false;
    *n_onsets = 0;
    if (a->align) {                                                            // offsets are host data in both modes
        if (a->onset_offsets[0] != 0) return false;
        for (int b = 0; b < a->batch; ++b)
            if (a->onset_offsets[b + 1] <= a->onset_offsets[b]) return false;         // a clip without an onset has no score (0 / 0)
        *n_onsets = a->onset_offsets[a->batch];
        if (!(a->sigma > 0.f) || !(a->fps > 0.f)) return false;
    }
    return true;
}

}  // namespace ls
