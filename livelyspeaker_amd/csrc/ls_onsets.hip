// Audio onsets for the beat-alignment scores: what the reference's scripts take from librosa 0.9.2 (onset_detect of
// scripts/test_RAG_ted.py:113, alignment.load_audio of scripts_beat/utils/metric.py:60-74), on the device.
//   k_onset_spectrum  one wave per frame, four frames per workgroup: gather 2048 samples (the centre padding is index arithmetic),
//                     window, a 2048-point real FFT as a 1024-point complex Stockham radix-4 FFT in LDS plus the real-FFT post-pass,
//                     power, rms, and the 128 mel sums gathered per filter from a CSR table in a fixed order -> dB
//   k_onset_pick      one workgroup per clip: clip-wide clamp, spectral flux, normalisation, peak picking, both backtracks
// Every sum is a fixed tree (per-lane order, wave butterfly) and a frame never looks at another clip, so a clip's numbers do not
// depend on the batch it travels in.  The tables come from the host-only unit ls_onsets_tables.cpp.  The spectrum's per-frame work is
// ls_onsets_frame.h's onset_frame over a sample fetch; ls_onsets_long.hip launches the same kernel for clips of any length, and the
// score stream (ls_score_stream.hip) runs the same body over its carries.
// Ragged batches (ls_onsets_ragged): clip b holds lens[b] valid samples (frames, with a given envelope) in a row of stride L; the same
// kernel bodies are instantiated with kRagged.  The spectrum runs one wave per VALID frame: wave g finds its clip by a binary search
// in the prefix sums of the clips' frame counts.  Padding, reflection, the clip-wide maximum, the windows and the backtracks use the
// clip's own L_b / F_b; only the addresses use the strides L and F.  What lies beyond a clip is never read; its outputs are set by a
// memset ahead of the launch (0, and 0xFF bytes for the -1 of the onset slabs).
#include "ls_hip.h"
#include "ls_onsets.h"
#include "ls_onsets_frame.h"
#include "ls_staging.h"

namespace ls {
namespace {

constexpr int kMaxF = LS_ONSETS_MAX_FRAMES;

}  // namespace

// Every wave of a workgroup runs the same sequence of barriers: a wave whose frame lies past the end computes on zeros and
// stores nothing.
template <bool kRagged>
__global__ __launch_bounds__(64 * kWavesPerBlock) void k_onset_spectrum(const SpectrumParams p) {
    __shared__ float2 sbuf[kWavesPerBlock][kFrameSlots];
    const int wave = threadIdx.x >> 6;
    const long long g = (long long)blockIdx.x * kWavesPerBlock + wave, total = kRagged ? (long long)p.frame_off[p.B] : (long long)p.B * p.F;
    const bool live = g < total;
    int b = 0, t = 0, L = p.L;                       // L: the clip's own samples; p.L and p.F are the row strides
    if (kRagged) {
        if (live) {                                  // the last clip whose first frame is at or before g (wave-uniform)
            int lo = 0, hi = p.B - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if ((long long)p.frame_off[mid] <= g) lo = mid; else hi = mid - 1;
            }
            b = lo;
            t = (int)(g - p.frame_off[b]);
        }
        L = p.lens[b];
    } else if (live) {
        b = (int)(g / p.F);
        t = (int)(g - (long long)b * p.F);
    }
    const size_t row = kRagged ? (size_t)b * p.F + t : (size_t)g;      // the frame's place in the [B, F] outputs
    const float* y = p.audio + (size_t)b * p.L;
    const long long base = (long long)t * kHop - kHalf;               // the frame's first sample; 64-bit: 2 (L - 1) passes 2^31
    const int pad_mode = p.pad_mode;
    auto sample_at = [=](int n) -> float {
        long long i = base + n;
        if (pad_mode == LS_ONSETS_PAD_REFLECT) {                       // numpy's 'reflect': the edge sample is not repeated
            if (i < 0) i = -i;
            else if (i >= L) i = 2 * ((long long)L - 1) - i;
        }
        return (live && i >= 0 && i < L) ? y[i] : 0.0f;
    };
    onset_frame(sample_at, live, sbuf[wave], p.window, p.twiddle, p.mel_ptr, p.mel_col, p.mel_w, p.mel_db + row * kMels,
                p.rms ? p.rms + row : nullptr);
}

void launch_onset_spectrum(const SpectrumParams& p) {
    const long long blocks = ((long long)p.B * p.F + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(k_onset_spectrum<false>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, 0, p);
}

namespace {

struct PickParams {
    int F, pre_max, post_max, pre_avg, post_avg, wait, given;
    float delta;
    const float* mel_db;       // [B, F, 128] (given == 0)
    const float* envelope;     // [B, F]      (given == 1)
    const float* rms;          // [B, F] or NULL
    float* oenv;
    int *count, *onset_raw, *onset_bt, *onset_bt_rms;
    const int* frame_off;      // ragged: [B + 1] prefix sums of the clips' frame counts; F is the row stride
};

}  // namespace

template <bool kRagged>
__global__ __launch_bounds__(256) void k_onset_pick(const PickParams p) {
    __shared__ float senv[kMaxF];            // the envelope
    __shared__ float sx[kMaxF];              // normalised; once the detections are marked, the picked frames (sraw)
    __shared__ float srms[kMaxF];
    __shared__ unsigned char sdet[kMaxF];    // passes the maximum and the threshold test
    __shared__ float part[4];
    __shared__ int scount;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, FS = p.F;
    const int F = kRagged ? p.frame_off[b + 1] - p.frame_off[b] : FS;          // the clip's own frames

    if (p.given) {
        for (int n = tid; n < F; n += 256) senv[n] = p.envelope[(size_t)b * FS + n];
    } else {
        // ---- S = max(S, clip max - 80); d[t] = mean over the mels of max(0, S[t + 1] - S[t]); the envelope is d shifted by 3 ----
        const float* S = p.mel_db + (size_t)b * FS * kMels;
        float mx = -INFINITY;
        for (int i = tid; i < F * kMels; i += 256) mx = fmaxf(mx, S[i]);
        mx = block_combine(wave_max(mx), part, [](float a, float c) { return fmaxf(a, c); });
        const float floor_db = mx - 80.0f;
        for (int n = tid; n < kLagShift && n < F; n += 256) senv[n] = 0.0f;
        for (int t = wave; t + kLagShift < F; t += 4) {         // one wave per frame pair: two mels per lane, then the butterfly
            const float* s0 = S + (size_t)t * kMels;
            const float* s1 = s0 + kMels;
            const float d0 = fmaxf(0.0f, fmaxf(s1[lane], floor_db) - fmaxf(s0[lane], floor_db));
            const float d1 = fmaxf(0.0f, fmaxf(s1[lane + 64], floor_db) - fmaxf(s0[lane + 64], floor_db));
            const float d = wave_sum(d0 + d1) / (float)kMels;
            if (lane == 0) senv[t + kLagShift] = d;
        }
    }
    if (p.rms)
        for (int n = tid; n < F; n += 256) srms[n] = p.rms[(size_t)b * FS + n];
    __syncthreads();

    // ---- x = (oenv - min) / (max(oenv - min) + tiny); an envelope without a non-zero entry has no onsets ----
    float lo = INFINITY, hi = -INFINITY;
    for (int n = tid; n < F; n += 256) {
        lo = fminf(lo, senv[n]);
        hi = fmaxf(hi, senv[n]);
        if (p.oenv) p.oenv[(size_t)b * FS + n] = senv[n];
    }
    lo = block_combine(wave_min(lo), part, [](float a, float c) { return fminf(a, c); });
    hi = block_combine(wave_max(hi), part, [](float a, float c) { return fmaxf(a, c); });
    const bool any = lo != 0.0f || hi != 0.0f;
    const float denom = (hi - lo) + 1.17549435e-38f;
    for (int n = tid; n < F; n += 256) sx[n] = (senv[n] - lo) / denom;
    __syncthreads();

    // ---- x[n] == max(x[n - pre_max : n + post_max]), x[n] != 0, x[n] >= mean(x[n - pre_avg : n + post_avg]) + delta; both
    //      windows are cut at the ends of the clip, the mean is added left to right ----
    for (int n = tid; n < F; n += 256) {
        const float x = sx[n];
        float mx = x, sum = 0.0f;
        for (int i = max(0, n - p.pre_max); i < min(F, n + p.post_max); ++i) mx = fmaxf(mx, sx[i]);
        const int a0 = max(0, n - p.pre_avg), a1 = min(F, n + p.post_avg);
        for (int i = a0; i < a1; ++i) sum += sx[i];
        sdet[n] = any && x == mx && x != 0.0f && x >= sum / (float)(a1 - a0) + p.delta;
    }
    __syncthreads();

    // ---- greedy left to right: keep n when n > last + wait ----
    int* sraw = reinterpret_cast<int*>(sx);
    if (tid == 0) {
        int c = 0;
        long long last = -(long long)kMaxF - 2;
        for (int n = 0; n < F; ++n)
            if (sdet[n] && n > last + p.wait) {
                sraw[c++] = n;
                last = n;
            }
        scount = c;
        if (p.count) p.count[b] = c;
    }
    __syncthreads();
    const int c = scount;
    for (int n = tid; n < F; n += 256)
        if (p.onset_raw) p.onset_raw[(size_t)b * FS + n] = n < c ? sraw[n] : -1;

    // ---- backtracks: the nearest minimum at or before each onset, one serial walk per energy (wave 0: oenv, wave 1: rms) ----
    if (lane == 0 && wave < 2) {
        const float* e = wave == 0 ? senv : srms;
        int* out = wave == 0 ? p.onset_bt : p.onset_bt_rms;
        if (out) {
            int cur = 0, i = 0;
            for (int n = 0; n < F && i < c; ++n) {
                if (is_minimum(e, n, F)) cur = n;
                while (i < c && sraw[i] == n) out[(size_t)b * FS + i++] = cur;
            }
            for (; i < F; ++i) out[(size_t)b * FS + i] = -1;
        }
    }
}

namespace {

// both entry points: `lengths` [B] (HOST) is read by the ragged one alone
int onsets(int device, const ls_onsets_args* a, const int32_t* lengths, bool ragged) {
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
    const long long F64 = given ? a->length : 1 + a->length / kHop;
    if (F64 > kMaxF) return LS_EINVAL;
    const int B = a->batch, L = a->length, F = (int)F64;
    std::vector<int32_t> frame_off;                  // ragged: prefix sums of the clips' frame counts
    if (ragged) {
        if (!lengths) return LS_EINVAL;
        frame_off.assign((size_t)B + 1, 0);
        for (int b = 0; b < B; ++b) {
            if (lengths[b] < 1 || lengths[b] > L) return LS_EINVAL;
            if (!given && a->pad_mode == LS_ONSETS_PAD_REFLECT && lengths[b] <= kHalf) return LS_EINVAL;
            const long long next = (long long)frame_off[b] + (given ? lengths[b] : 1 + lengths[b] / kHop);
            if (next > 0x7fffffffLL) return LS_EINVAL;
            frame_off[b + 1] = (int32_t)next;
        }
    }
    const bool want_pick = given || a->oenv || a->count || a->onset_raw || a->onset_bt || a->onset_bt_rms;
    const size_t n_bf = (size_t)B * F;
    if ((n_bf + kWavesPerBlock - 1) / kWavesPerBlock > 0x7fffffffull) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;

    Staging st(a->on_device != 0);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (a->kernel_ms)
        for (auto& v : ev) st.chk(hipEventCreate(&v));

    SpectrumParams sp{};
    PickParams pp{};
    pp.F = F; pp.given = given ? 1 : 0; pp.delta = a->delta;
    // onset_detect's defaults in frames of 512 samples: 0.03 s and 0.10 s before, one frame and pre_avg + 1 after
    pp.pre_max = (int)std::floor(0.03 * (double)a->sr_pick / kHop);
    pp.post_max = 1;
    pp.pre_avg = (int)std::floor(0.10 * (double)a->sr_pick / kHop);
    pp.post_avg = pp.pre_avg + 1;
    pp.wait = pp.pre_max;
    if (given) {
        pp.envelope = st.in(a->envelope, n_bf);
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
        pp.mel_db = sp.mel_db;
        pp.rms = a->onset_bt_rms ? sp.rms : nullptr;
    }
    pp.oenv = st.out(a->oenv, n_bf);
    pp.count = st.out(a->count, (size_t)B);
    pp.onset_raw = st.out(a->onset_raw, n_bf);
    pp.onset_bt = st.out(a->onset_bt, n_bf);
    pp.onset_bt_rms = st.out(a->onset_bt_rms, n_bf);
    if (ragged) {                                    // the lengths are host data in both modes; the padding values go in ahead of the launch
        pp.frame_off = sp.frame_off = st.upload(frame_off.data(), frame_off.size());
        if (!given) sp.lens = st.upload(lengths, (size_t)B);
        if (a->mel_db) st.fill(sp.mel_db, 0, n_bf * kMels * 4);
        if (a->rms) st.fill(sp.rms, 0, n_bf * 4);
        st.fill(pp.oenv, 0, n_bf * 4);
        st.fill(pp.onset_raw, 0xFF, n_bf * 4);
        st.fill(pp.onset_bt, 0xFF, n_bf * 4);
        st.fill(pp.onset_bt_rms, 0xFF, n_bf * 4);
    }
    if (st.e == hipSuccess) {
        if (!given) {
            const long long waves = ragged ? (long long)frame_off[B] : (long long)n_bf;
            const long long blocks = (waves + kWavesPerBlock - 1) / kWavesPerBlock;
            if (ev[0]) st.chk(hipEventRecord(ev[0], 0));
            if (ragged) hipLaunchKernelGGL(k_onset_spectrum<true>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, 0, sp);
            else hipLaunchKernelGGL(k_onset_spectrum<false>, dim3((unsigned)blocks), dim3(64 * kWavesPerBlock), 0, 0, sp);
            if (ev[1]) st.chk(hipEventRecord(ev[1], 0));
        }
        if (want_pick) {
            if (ev[2]) st.chk(hipEventRecord(ev[2], 0));
            if (ragged) hipLaunchKernelGGL(k_onset_pick<true>, dim3(B), dim3(256), 0, 0, pp);
            else hipLaunchKernelGGL(k_onset_pick<false>, dim3(B), dim3(256), 0, 0, pp);
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

}  // namespace
}  // namespace ls

extern "C" int ls_onsets(int device, const ls_onsets_args* a) { return ls::onsets(device, a, nullptr, false); }

extern "C" int ls_onsets_ragged(int device, const ls_onsets_args* a, const int32_t* lengths) { return ls::onsets(device, a, lengths, true); }
