// The score stream's own kernels (the handle is ls_score_stream_api.cpp, the tiled pick ls_onsets_long.hip):
//   k_score_spectrum   one wave per newly decided (slot, frame): ls_onsets_frame.h's frame body over a fetch that reads the slot's
//                      carry and the push's chunk, so a frame's mel_db and rms are those of k_onset_spectrum on the whole series
//   k_score_carry      the samples a pending frame still needs, from the old carry and the chunk into the slot's other carry
//   k_score_beats      the push's motion-beat bytes appended to the slot's entries
//   k_score_compact    a slot's set entries as an ascending list (ballot and a running offset, 256 entries at a time)
//   k_score_ted_align  k_ted_align's float64 sum and k_score_beat_align k_beat_reduce_timeline's float32 align (ls_timeline.hip) with
//                      the beats read from that list: onset i on thread i % 256, added in index order, the wave butterfly, then
//                      ((p0 + p1) + p2) + p3.  The nearest beat is found by binary search; the square (the absolute value) of a
//                      difference grows with the distance, so the two neighbours hold the minimum over all beats -- the same value.
#include "ls_hip.h"
#include "ls_onsets_frame.h"
#include "ls_score_stream.h"

namespace ls {
namespace {

// (a name of its own: an overload declared here would hide the header's float wave_sum)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// Every wave of a workgroup runs the same sequence of barriers: a wave without a frame computes on zeros and stores nothing.
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_score_spectrum(const ScoreSpectrumArgs p, int total) {
    __shared__ float2 sbuf[kWavesPerBlock][kFrameSlots];
    const int wave = threadIdx.x >> 6;
    const int g = blockIdx.x * kWavesPerBlock + wave;
    const bool live = g < total;
    int s = 0;
    if (live) {                                      // the last slot whose first unit is at or before g (wave-uniform)
        int lo = 0, hi = p.S - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.rows[mid].frame_off <= g) lo = mid; else hi = mid - 1;
        }
        s = lo;
    }
    const ScoreSlotRow r = p.rows[s];
    const int t = r.frame_first + (g - r.frame_off);
    const size_t row = (size_t)s * p.max_frames + t;
    const float* carry = p.carry + ((size_t)s * 2 + r.parity) * kScoreCarry;
    const float* chunk = p.chunk ? p.chunk + (size_t)s * p.n_max : nullptr;
    const long long base = (long long)t * kHop - kHalf, L = r.total;
    const int pad_mode = p.pad_mode;
    auto sample_at = [=](int n) -> float {
        long long i = base + n;
        if (pad_mode == LS_ONSETS_PAD_REFLECT) {     // numpy's 'reflect': the edge sample is not repeated
            if (i < 0) i = -i;
            else if (i >= L) i = 2 * (L - 1) - i;
        }
        if (!live || i < r.carry_first || i >= L) return 0.0f;         // below the carry: never, by the plan (a frame's samples are kept)
        return i < r.before ? carry[i - r.carry_first] : chunk[i - r.before];
    };
    onset_frame(sample_at, live, sbuf[wave], p.window, p.twiddle, p.mel_ptr, p.mel_col, p.mel_w, p.mel_db + row * kMels, p.rms + row);
}

__global__ __launch_bounds__(256) void k_score_carry(const ScoreSpectrumArgs p) {
    const int s = blockIdx.x;
    const ScoreSlotRow r = p.rows[s];
    if (r.fresh == 0 && r.next_first == r.carry_first) return;         // nothing moves: the parity stays too (the host knows)
    const float* old = p.carry + ((size_t)s * 2 + r.parity) * kScoreCarry;
    float* next = p.carry + ((size_t)s * 2 + (r.parity ^ 1)) * kScoreCarry;
    const float* chunk = p.chunk ? p.chunk + (size_t)s * p.n_max : nullptr;
    const int n = r.total - r.next_first;                                // < kScoreCarry, by the plan
    for (int j = threadIdx.x; j < n; j += 256) {
        const int i = r.next_first + j;
        next[j] = i < r.before ? old[i - r.carry_first] : chunk[i - r.before];
    }
}

__global__ __launch_bounds__(256) void k_score_beats(const unsigned char* __restrict__ beats, int stride, const int* __restrict__ first_count,
                                                     unsigned char* __restrict__ dst, long long max_entries) {
    const int s = blockIdx.x, first = first_count[2 * s], n = first_count[2 * s + 1];
    for (int i = threadIdx.x; i < n; i += 256) dst[(size_t)s * max_entries + first + i] = beats[(size_t)s * stride + i] ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_score_compact(const ScoreAlignArgs p) {
    __shared__ int wave_n[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int off = 0;
    for (int i0 = 0; i0 < p.n_entries; i0 += 256) {
        const int i = i0 + threadIdx.x;
        const bool set = i < p.n_entries && p.beats[i] != 0;
        const unsigned long long mask = __ballot(set);
        __syncthreads();                                                 // the previous round's reads of wave_n
        if (lane == 0) wave_n[wave] = __popcll(mask);
        __syncthreads();
        int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += wave_n[w];
            total += wave_n[w];
        }
        if (set) p.list[off + before] = i;
        off += total;
    }
    if (threadIdx.x == 0) *p.n_list = off;
}

// the largest j with key(list[j]) <= a, or -1
template <class T, class Key>
__device__ __forceinline__ int last_at_or_before(const int* list, int n, T a, Key key) {
    int lo = -1, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (key(list[mid]) <= a) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_score_ted_align(const ScoreAlignArgs p) {
#pragma clang fp contract(off)
    __shared__ double dpart[4];
    const int tid = threadIdx.x, wave = tid >> 6, beats = *p.n_list;
    if (tid == 0 && p.n_beats) *p.n_beats = beats;
    if (!p.align_sum) return;
    if (beats == 0) {
        if (tid == 0) *p.align_sum = 0.0;
        return;
    }
    const int cnt = *p.onset_count;
    const double fps = p.fps, two_var = (2.0 * p.sigma) * p.sigma;
    auto time_of = [=](int entry) { return (double)entry / fps; };
    double s = 0.0;
    for (int i = tid; i < cnt; i += 256) {
        const double a = (double)((long long)p.onset_frames[i] * (long long)p.hop) / p.rate;
        const int j = last_at_or_before(p.list, beats, a, time_of);
        double dmin = INFINITY;
        if (j >= 0) { const double d = a - time_of(p.list[j]); dmin = fmin(dmin, d * d); }
        if (j + 1 < beats) { const double d = a - time_of(p.list[j + 1]); dmin = fmin(dmin, d * d); }
        s += exp(-dmin / two_var);
    }
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) dpart[wave] = s;
    __syncthreads();
    if (tid == 0) *p.align_sum = ((dpart[0] + dpart[1]) + dpart[2]) + dpart[3];
}

__global__ __launch_bounds__(256) void k_score_beat_align(const ScoreAlignArgs p) {
#pragma clang fp contract(off)
    __shared__ float part[4];
    const int tid = threadIdx.x, wave = tid >> 6, beats = *p.n_list, cnt = *p.onset_count;
    const float fps = (float)p.fps, sigma = (float)p.sigma;
    const float two_var = 2.0f * (sigma * sigma);
    auto time_of = [=](int entry) { return (float)entry / fps; };
    float s = 0.f;
    for (int i = tid; i < cnt; i += 256) {
        const float t = (float)((double)((long long)p.onset_frames[i] * (long long)p.hop) / p.rate);      // the host's float64 time, rounded
        const int j = last_at_or_before(p.list, beats, t, time_of);
        float dmin = INFINITY;
        if (j >= 0) dmin = fminf(dmin, fabsf(time_of(p.list[j]) - t));
        if (j + 1 < beats) dmin = fminf(dmin, fabsf(time_of(p.list[j + 1]) - t));
        s += expf(-(dmin * dmin) / two_var);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) *p.align = (((part[0] + part[1]) + part[2]) + part[3]) / (float)cnt;
}

}  // namespace

void launch_score_spectrum(const ScoreSpectrumArgs& a, int total_frames) {
    if (total_frames < 1) return;
    const unsigned blocks = (unsigned)((total_frames + kWavesPerBlock - 1) / kWavesPerBlock);
    hipLaunchKernelGGL(k_score_spectrum, dim3(blocks), dim3(64 * kWavesPerBlock), 0, 0, a, total_frames);
}

void launch_score_carry(const ScoreSpectrumArgs& a) { hipLaunchKernelGGL(k_score_carry, dim3((unsigned)a.S), dim3(256), 0, 0, a); }

void launch_score_beats(const unsigned char* beats, int S, int stride, const int* first_count, unsigned char* dst, long long max_entries) {
    hipLaunchKernelGGL(k_score_beats, dim3((unsigned)S), dim3(256), 0, 0, beats, stride, first_count, dst, max_entries);
}

void launch_score_align(const ScoreAlignArgs& a, bool beat) {
    hipLaunchKernelGGL(k_score_compact, dim3(1), dim3(256), 0, 0, a);
    if (beat) hipLaunchKernelGGL(k_score_beat_align, dim3(1), dim3(256), 0, 0, a);
    else hipLaunchKernelGGL(k_score_ted_align, dim3(1), dim3(256), 0, 0, a);
}

}  // namespace ls
