// ls_onsets_long: the audio-onset chain of ls_onsets.hip for clips of any length.  The spectrum is the same kernel
// (k_onset_spectrum, ls_onsets_frame.h); what follows it is k_onset_pick's steps with nothing in LDS sized by the clip, over
// (clip, tile of LS_SCORE_TILE frames), one frame per thread:
//   k_long_db_max      tile maximum of mel_db                               -> part[b, tile]
//   k_long_combine     clip maximum of the tile partials (max and min are exact in any order)
//   k_long_flux        the envelope of the tile's frames (k_onset_pick's expression and wave butterfly) -> global memory
//   k_long_env_range   tile minimum and maximum of the envelope; k_long_combine again -> lo, hi
//   k_long_detect      x = (e - lo) / denom over the two windows read from global memory, the detection flag, and the tile's
//                      flagged frames compacted in frame order (ballot, prefix over the four waves)
//   k_long_greedy      n > last + wait is sequential: one wave per clip walks the CANDIDATES tile by tile (64 at a time through
//                      lane reads), not the frames
//   k_long_backtrack   one thread per slab entry: an onset searches left for its nearest minimum (envelope and rms), every other
//                      entry becomes -1
// Every float is a per-frame expression or an exact reduction, so for F <= LS_ONSETS_MAX_FRAMES the outputs are those of ls_onsets
// bit for bit (tests/test_gpu_onsets_long.py).
#include <cmath>

#include "ls_hip.h"
#include "ls_onsets.h"
#include "ls_onsets_frame.h"
#include "ls_score_stream.h"
#include "ls_staging.h"

namespace ls {
namespace {

constexpr int kTile = LS_SCORE_TILE;
static_assert(kTile == 256, "one frame per thread of a 256-thread workgroup");

struct Max { __device__ float operator()(float a, float c) const { return fmaxf(a, c); } };
struct Min { __device__ float operator()(float a, float c) const { return fminf(a, c); } };

__global__ __launch_bounds__(256) void k_long_db_max(const LongPickParams p) {
    __shared__ float part[4];
    const int b = blockIdx.x / p.nT, tile = blockIdx.x - b * p.nT;
    const int f0 = tile * kTile, nf = min(kTile, p.F - f0);
    const float* S = p.mel_db + ((size_t)b * p.F + f0) * kMels;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < nf * kMels; i += 256) mx = fmaxf(mx, S[i]);
    mx = block_combine(wave_max(mx), part, Max());
    if (threadIdx.x == 0) p.part[blockIdx.x] = mx;
}

// stat[b, which] = max (kMax) or min over the clip's nT partials of plane `plane`
template <bool kMax>
__global__ __launch_bounds__(256) void k_long_combine(const LongPickParams p, int plane, int which) {
    __shared__ float part[4];
    const int b = blockIdx.x;
    const float* src = p.part + ((size_t)plane * gridDim.x + b) * p.nT;
    float v = kMax ? -INFINITY : INFINITY;
    for (int i = threadIdx.x; i < p.nT; i += 256) v = kMax ? fmaxf(v, src[i]) : fminf(v, src[i]);
    v = kMax ? block_combine(wave_max(v), part, Max()) : block_combine(wave_min(v), part, Min());
    if (threadIdx.x == 0) p.stat[b * 3 + which] = v;
}

// S = max(S, clip max - 80); d[t] = mean over the mels of max(0, S[t + 1] - S[t]); the envelope is d shifted by kLagShift
__global__ __launch_bounds__(256) void k_long_flux(const LongPickParams p) {
    const int b = blockIdx.x / p.nT, tile = blockIdx.x - b * p.nT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* S = p.mel_db + (size_t)b * p.F * kMels;
    float* env = p.env_out + (size_t)b * p.F;
    const float floor_db = p.stat[b * 3] - 80.0f;
    const int n1 = min(p.F, (tile + 1) * kTile);
    for (int n = tile * kTile + wave; n < n1; n += 4) {          // one wave per frame pair: two mels per lane, then the butterfly
        float d = 0.0f;
        if (n >= kLagShift) {                                     // wave-uniform
            const float* s0 = S + (size_t)(n - kLagShift) * kMels;
            const float* s1 = s0 + kMels;
            const float d0 = fmaxf(0.0f, fmaxf(s1[lane], floor_db) - fmaxf(s0[lane], floor_db));
            const float d1 = fmaxf(0.0f, fmaxf(s1[lane + 64], floor_db) - fmaxf(s0[lane + 64], floor_db));
            d = wave_sum(d0 + d1) / (float)kMels;
        }
        if (lane == 0) env[n] = d;
    }
}

__global__ __launch_bounds__(256) void k_long_env_range(const LongPickParams p) {
    __shared__ float part[4];
    const int b = blockIdx.x / p.nT, tile = blockIdx.x - b * p.nT;
    const int n = tile * kTile + threadIdx.x;
    const size_t planes = (size_t)gridDim.x;
    float lo = INFINITY, hi = -INFINITY;
    if (n < p.F) {
        lo = hi = p.env[(size_t)b * p.F + n];
        if (p.env_out && p.env_out != p.env) p.env_out[(size_t)b * p.F + n] = lo;          // a given envelope, handed back
    }
    lo = block_combine(wave_min(lo), part, Min());
    hi = block_combine(wave_max(hi), part, Max());
    if (threadIdx.x == 0) {
        p.part[blockIdx.x] = lo;
        p.part[planes + blockIdx.x] = hi;
    }
}

// x[n] == max(x[n - pre_max : n + post_max]), x[n] != 0, x[n] >= mean(x[n - pre_avg : n + post_avg]) + delta; both windows are cut
// at the ends of the clip, the mean is added left to right; an envelope without a non-zero entry has no onsets
__global__ __launch_bounds__(256) void k_long_detect(const LongPickParams p) {
    __shared__ int wave_n[4];
    const int b = blockIdx.x / p.nT, tile = blockIdx.x - b * p.nT, F = p.F;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = tile * kTile + threadIdx.x;
    const float* e = p.env + (size_t)b * F;
    const float lo = p.stat[b * 3 + 1], hi = p.stat[b * 3 + 2];
    const bool any = lo != 0.0f || hi != 0.0f;
    const float denom = (hi - lo) + 1.17549435e-38f;
    bool det = false;
    if (n < F) {
        const float x = (e[n] - lo) / denom;
        float mx = x, sum = 0.0f;
        for (int i = max(0, n - p.pre_max); i < (int)min((long long)F, (long long)n + p.post_max); ++i) mx = fmaxf(mx, (e[i] - lo) / denom);
        const int a0 = max(0, n - p.pre_avg), a1 = (int)min((long long)F, (long long)n + p.post_avg);
        for (int i = a0; i < a1; ++i) sum += (e[i] - lo) / denom;
        det = any && x == mx && x != 0.0f && x >= sum / (float)(a1 - a0) + p.delta;
    }
    const unsigned long long mask = __ballot(det);
    if (lane == 0) wave_n[wave] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1ull)), total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) before += wave_n[w];
        total += wave_n[w];
    }
    if (det) p.cand[(size_t)b * F + tile * kTile + before] = n;      // before < the tile's frames: inside the clip's row
    if (threadIdx.x == 0) p.ncand[blockIdx.x] = total;
}

// greedy left to right: keep n when n > last + wait.  One wave per clip; 64 tile counts, then 64 candidates, are loaded at once
// and handed round by lane reads, so every lane takes the same decisions and lane 0 stores them.
__global__ __launch_bounds__(64) void k_long_greedy(const LongPickParams p) {
    const int b = blockIdx.x, lane = threadIdx.x, F = p.F;
    const int* cand = p.cand + (size_t)b * F;
    const int* ncand = p.ncand + (size_t)b * p.nT;
    int* raw = p.onset_raw + (size_t)b * F;
    int c = 0;
    long long last = -(long long)p.wait - 1;                         // the first candidate is always kept
    for (int t0 = 0; t0 < p.nT; t0 += 64) {
        const int mine = t0 + lane < p.nT ? ncand[t0 + lane] : 0;
        for (int j = 0; j < 64 && t0 + j < p.nT; ++j) {
            const int nc = __shfl(mine, j);
            for (int k0 = 0; k0 < nc; k0 += 64) {
                const int v = k0 + lane < nc ? cand[(size_t)(t0 + j) * kTile + k0 + lane] : 0;
                const int m = min(64, nc - k0);
                for (int k = 0; k < m; ++k) {
                    const int n = __shfl(v, k);
                    if (n > last + p.wait) {
                        if (lane == 0) raw[c] = n;
                        ++c;
                        last = n;
                    }
                }
            }
        }
    }
    if (lane == 0) p.count[b] = c;
}

// the nearest minimum at or before each onset; frame 0 is one, so the search ends
__device__ __forceinline__ int nearest_minimum(const float* e, int n, int F) {
    while (!is_minimum(e, n, F)) --n;
    return n;
}

__global__ __launch_bounds__(256) void k_long_backtrack(const LongPickParams p) {
    const int b = blockIdx.x / p.nT, tile = blockIdx.x - b * p.nT, F = p.F;
    const int i = tile * kTile + threadIdx.x;
    if (i >= F) return;
    const size_t at = (size_t)b * F + i;
    if (i < p.count[b]) {
        const int n = p.onset_raw[at];
        if (p.onset_bt) p.onset_bt[at] = nearest_minimum(p.env + (size_t)b * F, n, F);
        if (p.onset_bt_rms) p.onset_bt_rms[at] = nearest_minimum(p.rms + (size_t)b * F, n, F);
    } else {
        p.onset_raw[at] = -1;
        if (p.onset_bt) p.onset_bt[at] = -1;
        if (p.onset_bt_rms) p.onset_bt_rms[at] = -1;
    }
}

}  // namespace

// onset_detect's defaults in frames of 512 samples: 0.03 s and 0.10 s before, one frame and pre_avg + 1 after (a window longer than
// the clip is cut to the clip anyway: F stands for it, and the kernels' arithmetic stays in range)
void long_pick_windows(LongPickParams* p, double sr_pick) {
    p->pre_max = (int)std::fmin(std::floor(0.03 * sr_pick / kHop), (double)p->F);
    p->post_max = 1;
    p->pre_avg = (int)std::fmin(std::floor(0.10 * sr_pick / kHop), (double)p->F);
    p->post_avg = p->pre_avg + 1;
    p->wait = p->pre_max;
}

// the tiled pick on the null stream: B clips of p.F frames
void launch_long_pick(const LongPickParams& p, int B) {
    const dim3 tiles((unsigned)((long long)B * p.nT)), clips((unsigned)B), block(256);
    if (p.mel_db) {
        hipLaunchKernelGGL(k_long_db_max, tiles, block, 0, 0, p);
        hipLaunchKernelGGL(k_long_combine<true>, clips, block, 0, 0, p, 0, 0);
        hipLaunchKernelGGL(k_long_flux, tiles, block, 0, 0, p);
    }
    hipLaunchKernelGGL(k_long_env_range, tiles, block, 0, 0, p);
    hipLaunchKernelGGL(k_long_combine<false>, clips, block, 0, 0, p, 0, 1);
    hipLaunchKernelGGL(k_long_combine<true>, clips, block, 0, 0, p, 1, 2);
    hipLaunchKernelGGL(k_long_detect, tiles, block, 0, 0, p);
    hipLaunchKernelGGL(k_long_greedy, clips, dim3(64), 0, 0, p);
    hipLaunchKernelGGL(k_long_backtrack, tiles, block, 0, 0, p);
}

}  // namespace ls

extern "C" int ls_onsets_long(int device, const ls_onsets_args* a) {
    using namespace ls;
    if (!a || a->batch < 1 || a->length < 1) return LS_EINVAL;
    if ((a->audio == nullptr) == (a->envelope == nullptr)) return LS_EINVAL;          // exactly one input
    const bool given = a->envelope != nullptr;
    if (!(a->sr_pick > 0.f)) return LS_EINVAL;
    if (!given) {
        if (a->pad_mode != LS_ONSETS_PAD_CONSTANT && a->pad_mode != LS_ONSETS_PAD_REFLECT) return LS_EINVAL;
        if (a->pad_mode == LS_ONSETS_PAD_REFLECT && a->length <= kHalf) return LS_EINVAL;
        if (!(a->sr > 0.f) || !(a->fmax > 0.f)) return LS_EINVAL;
    } else if (a->mel_db || a->rms || a->onset_bt_rms) {
        return LS_EINVAL;
    }
    if (a->length > 0x7fffffff - (kNfft - 1)) return LS_EINVAL;                       // a frame's last sample, a tile's last thread: ints
    const int B = a->batch, L = a->length, F = given ? L : 1 + L / kHop, nT = (F + kTile - 1) / kTile;
    const size_t n_bf = (size_t)B * F;
    if ((n_bf + kWavesPerBlock - 1) / kWavesPerBlock > 0x7fffffffull) return LS_EINVAL;        // one wave per frame; B * nT is smaller
    const bool want_pick = given || a->oenv || a->count || a->onset_raw || a->onset_bt || a->onset_bt_rms;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;

    Staging st(a->on_device != 0);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (a->kernel_ms)
        for (auto& v : ev) st.chk(hipEventCreate(&v));

    SpectrumParams sp{};
    LongPickParams pp{};
    pp.F = F; pp.nT = nT; pp.delta = a->delta;
    long_pick_windows(&pp, (double)a->sr_pick);
    if (given) {
        pp.env = st.in(a->envelope, n_bf);
        pp.env_out = st.out(a->oenv, n_bf);
    } else {
        const OnsetTables tab = make_onset_tables(a->sr, kNfft, kMels, 0.0, a->fmax);
        sp.B = B; sp.L = L; sp.F = F; sp.pad_mode = a->pad_mode;
        sp.audio = st.in(a->audio, (size_t)B * L);
        sp.window = st.upload(tab.window.data(), tab.window.size());
        sp.twiddle = reinterpret_cast<const float2*>(st.upload(tab.twiddle.data(), tab.twiddle.size()));
        sp.mel_ptr = st.upload(tab.mel_ptr.data(), tab.mel_ptr.size());
        sp.mel_col = st.upload(tab.mel_col.data(), tab.mel_col.size());      // a filterbank may be empty (fmax below the first bin)
        sp.mel_w = st.upload(tab.mel_w.data(), tab.mel_w.size());
        sp.mel_db = st.out(a->mel_db, n_bf * kMels, /*needed=*/true);         // the pick reads it
        sp.rms = st.out(a->rms, n_bf, /*needed=*/a->onset_bt_rms != nullptr);
        if (want_pick) {
            pp.mel_db = sp.mel_db;
            pp.rms = a->onset_bt_rms ? sp.rms : nullptr;
            pp.env = pp.env_out = st.out(a->oenv, n_bf, /*needed=*/true);
        }
    }
    if (want_pick) {
        pp.count = st.out(a->count, (size_t)B, /*needed=*/true);
        pp.onset_raw = st.out(a->onset_raw, n_bf, /*needed=*/true);           // the backtracks read it
        pp.onset_bt = st.out(a->onset_bt, n_bf);
        pp.onset_bt_rms = st.out(a->onset_bt_rms, n_bf);
        pp.part = static_cast<float*>(st.temp((size_t)2 * B * nT * sizeof(float)));
        pp.stat = static_cast<float*>(st.temp((size_t)3 * B * sizeof(float)));
        pp.cand = static_cast<int*>(st.temp(n_bf * sizeof(int)));
        pp.ncand = static_cast<int*>(st.temp((size_t)B * nT * sizeof(int)));
    }
    if (st.e == hipSuccess) {
        if (!given) {
            if (ev[0]) st.chk(hipEventRecord(ev[0], 0));
            launch_onset_spectrum(sp);
            if (ev[1]) st.chk(hipEventRecord(ev[1], 0));
        }
        if (want_pick) {
            if (ev[2]) st.chk(hipEventRecord(ev[2], 0));
            launch_long_pick(pp, B);
            if (ev[3]) st.chk(hipEventRecord(ev[3], 0));
        }
        st.sync();
    }
    if (a->kernel_ms) {                              // events destroyed, then the copy-backs
        a->kernel_ms[0] = a->kernel_ms[1] = 0.0f;
        if (st.e == hipSuccess && !given) st.chk(hipEventElapsedTime(&a->kernel_ms[0], ev[0], ev[1]));
        if (st.e == hipSuccess && want_pick) st.chk(hipEventElapsedTime(&a->kernel_ms[1], ev[2], ev[3]));
        for (auto& v : ev)
            if (v) (void)hipEventDestroy(v);
    }
    return st.copy_back();
}
