// The resampler's kernels (the entry points are ls_resample_api.cpp, the plan and the taps ls_resample_plan.cpp):
//   k_resample          one-shot, ragged over (clip, tile of 256 outputs): a workgroup whose tile lies behind its clip's outputs leaves
//   k_resample_stream   the push's new outputs, over the (slot, tile) table: the fetch reads the slot's carry below n_before and the
//                       chunk from there on
//   k_resample_carry    the last carry_len mono samples of the series, from the old carry and the chunk into the slot's other carry
// One body, resample_tile, serves both forms; an output's arithmetic is ls_resample_frame.h's.  The mixdown sits in the fetch.  A tile
// stages the mono samples it reads once in LDS (at 48 kHz -> 16 kHz, 32 zeros: 3 * 255 + 196 samples for 256 outputs, against 193
// each) when they fit kResampleStage, and the tap table beside them when all of it fits kResampleTapLds; otherwise the taps come
// from global memory, one contiguous row per lane.  Nothing in LDS is sized by up, the tap count or the clip.  Plain fp32 FMAs.
#include "ls_hip.h"
#include "ls_resample.h"

namespace ls {
namespace {

template <class Fetch>
__device__ __forceinline__ void resample_tile(Fetch fetch, const ResampleRatio& q, const float* __restrict__ tab, long long m0, int count,
                                              float* __restrict__ out) {
    __shared__ __align__(16) float stage[kResampleStage];
    __shared__ __align__(16) float tap_lds[kResampleTapLds];
    const int tid = threadIdx.x;
    const bool live = tid < count;
    if (q.pass_through) {
        if (live) out[tid] = fetch(m0 + tid);
        return;
    }
    const long long k_lo = (m0 * q.down + q.half) / q.up - (q.Tp - 1);       // the oldest sample output m0's row reaches
    if (q.staged) {                                                             // uniform over the launch
        for (int i = tid; i < q.span; i += kResampleTile) stage[i] = fetch(k_lo + i);
        if (q.taps_in_lds)
            for (int i = tid; i < (int)q.up * q.Tp; i += kResampleTile) tap_lds[i] = tab[i];
        __syncthreads();
    }
    if (!live) return;
    const long long t0 = (m0 + tid) * q.down + q.half, kmax = t0 / q.up;
    const int r = (int)(t0 - kmax * q.up);
    const float4* grow = reinterpret_cast<const float4*>(tab + (size_t)r * q.Tp);
    const float4* lrow = reinterpret_cast<const float4*>(tap_lds + (size_t)r * q.Tp);
    const int base = (int)(kmax - k_lo);                                        // in [Tp - 1, span)
    float y;
    if (q.staged && q.taps_in_lds)
        y = resample_output([&](long long k) { return stage[base - (int)(kmax - k)]; }, [&](int j) { return lrow[j >> 2]; }, kmax, q.Tp);
    else if (q.staged)
        y = resample_output([&](long long k) { return stage[base - (int)(kmax - k)]; }, [&](int j) { return grow[j >> 2]; }, kmax, q.Tp);
    else
        y = resample_output(fetch, [&](int j) { return grow[j >> 2]; }, kmax, q.Tp);
    out[tid] = y;
}

template <class In>
__global__ __launch_bounds__(kResampleTile) void k_resample(const ResampleArgs p) {
    const int b = blockIdx.y;
    const long long n_out = p.out_lengths[b], m0 = (long long)blockIdx.x * kResampleTile;
    if (m0 >= n_out) return;                                                    // the whole workgroup
    const long long len = p.lengths[b];
    const In* row = static_cast<const In*>(p.audio) + (size_t)b * p.row_stride;
    const int C = p.C;
    const float gain = p.gain;
    auto fetch = [=](long long k) -> float { return k < 0 || k >= len ? 0.0f : mix_frame<In>(row + (size_t)k * C, C, gain); };
    const long long left = n_out - m0;
    resample_tile(fetch, p.q, p.tab, m0, left < kResampleTile ? (int)left : kResampleTile, p.out + (size_t)b * p.out_stride + m0);
}

template <class In>
__global__ __launch_bounds__(kResampleTile) void k_resample_stream(const ResampleStreamArgs p) {
    const int g = blockIdx.x;
    int lo = 0, hi = p.S - 1;                                                   // the last slot whose first tile is at or before g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.rows[mid].tile_off <= g) lo = mid; else hi = mid - 1;
    }
    const int s = lo;
    const ResampleSlotRow r = p.rows[s];
    const long long done = (long long)(g - r.tile_off) * kResampleTile;        // outputs of this push in the slot's earlier tiles
    if (done >= r.out_count) return;                                            // never, by the table
    const float* carry = p.carry + ((size_t)s * 2 + r.parity) * p.carry_len;
    const In* chunk = static_cast<const In*>(p.chunk) + (size_t)s * p.n_max * p.C;
    const int C = p.C;
    const float gain = p.gain;
    auto fetch = [=](long long k) -> float {                                    // below the carry: never, the carry holds 3 samples past what a padded row reaches
        if (k < r.carry_first || k >= r.total) return 0.0f;
        return k < r.before ? carry[k - r.carry_first] : mix_frame<In>(chunk + (size_t)(k - r.before) * C, C, gain);
    };
    const long long left = r.out_count - done;
    resample_tile(fetch, p.q, p.tab, r.out_first + done, left < kResampleTile ? (int)left : kResampleTile, p.out + (size_t)s * p.out_capacity + done);
}

template <class In>
__global__ __launch_bounds__(256) void k_resample_carry(const ResampleStreamArgs p) {
    const int s = blockIdx.x;
    const ResampleSlotRow r = p.rows[s];
    if (r.fresh == 0) return;                                                   // nothing moves: the parity stays too (the host knows)
    const float* old = p.carry + ((size_t)s * 2 + r.parity) * p.carry_len;
    float* next = p.carry + ((size_t)s * 2 + (r.parity ^ 1)) * p.carry_len;
    const In* chunk = static_cast<const In*>(p.chunk) + (size_t)s * p.n_max * p.C;
    const long long n = r.total - r.next_first;                                 // <= carry_len, by the host
    for (long long j = threadIdx.x; j < n; j += 256) {
        const long long i = r.next_first + j;
        next[j] = i < r.before ? old[i - r.carry_first] : mix_frame<In>(chunk + (size_t)(i - r.before) * p.C, p.C, p.gain);
    }
}

}  // namespace

void launch_resample(const ResampleArgs& a, int B, long long max_out) {
    if (B < 1 || max_out < 1) return;
    const dim3 grid((unsigned)((max_out + kResampleTile - 1) / kResampleTile), (unsigned)B);
    if (a.dtype == LS_RESAMPLE_I16) hipLaunchKernelGGL(k_resample<int16_t>, grid, dim3(kResampleTile), 0, 0, a);
    else hipLaunchKernelGGL(k_resample<float>, grid, dim3(kResampleTile), 0, 0, a);
}

void launch_resample_stream(const ResampleStreamArgs& a, int total_tiles) {
    if (total_tiles < 1) return;
    if (a.dtype == LS_RESAMPLE_I16) hipLaunchKernelGGL(k_resample_stream<int16_t>, dim3((unsigned)total_tiles), dim3(kResampleTile), 0, 0, a);
    else hipLaunchKernelGGL(k_resample_stream<float>, dim3((unsigned)total_tiles), dim3(kResampleTile), 0, 0, a);
}

void launch_resample_carry(const ResampleStreamArgs& a) {
    if (a.dtype == LS_RESAMPLE_I16) hipLaunchKernelGGL(k_resample_carry<int16_t>, dim3((unsigned)a.S), dim3(256), 0, 0, a);
    else hipLaunchKernelGGL(k_resample_carry<float>, dim3((unsigned)a.S), dim3(256), 0, 0, a);
}

}  // namespace ls
