// The per-frame arithmetic of the audio-onset spectrum, stated once: k_onset_spectrum (ls_onsets.hip) calls it for the capped, the
// ragged and the any-length entry (ls_onsets_long.hip launches the same kernel), so a frame's mel_db and rms do not depend on which
// entry computed them.  onset_frame takes the frame's samples through a fetch, `float sample_at(int i)` with i counted from the
// frame's first sample: the caller's index rule applies the centre padding (zeros or reflection) and returns 0 outside the signal.
// Loads of the signal, the frame table and the stores belong to the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "ls_hip.h"

namespace ls {

constexpr int kNfft = 2048, kHop = 512, kHalf = kNfft / 2, kQuarter = kHalf / 4, kMels = 128;
constexpr int kWavesPerBlock = 4;
constexpr int kLagShift = 1 + kNfft / (2 * kHop);
// One padding slot after every 16 complex numbers: the pass with output stride 4 writes 32-byte groups 128 bytes apart, which
// without the padding all land on the same 8 of the 32 banks a ds_write sees; with it every pass spreads evenly over the banks.
constexpr int kFrameSlots = kHalf + kHalf / 16;

struct SpectrumParams {
    int B, L, F, pad_mode;
    const float* audio;        // [B, L]
    const float* window;       // [2048]
    const float2* twiddle;     // [2048] exp(-2 pi i n / 2048)
    const int* mel_ptr;        // [129]
    const int* mel_col;
    const float* mel_w;
    float* mel_db;             // [B, F, 128]
    float* rms;                // [B, F] or NULL
    const int* lens;           // ragged: [B] valid samples of a clip
    const int* frame_off;      // ragged: [B + 1] prefix sums of the clips' frame counts
};

// k_onset_spectrum<false> over the B * F frames of an equal-length batch on the null stream (defined in ls_onsets.hip)
void launch_onset_spectrum(const SpectrumParams& p);

__device__ __forceinline__ int slot(int i) { return i + (i >> 4); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}

// the four wave partials of a 256-thread block combined in wave order; every thread receives the result
template <class Op>
__device__ __forceinline__ float block_combine(float v, float* part, Op op) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return op(op(op(part[0], part[1]), part[2]), part[3]);
}

// minima of onset_backtrack: frame 0, and i + 1 where e[i + 1] <= e[i] and e[i + 1] < e[i + 2]
__device__ __forceinline__ bool is_minimum(const float* e, int n, int F) {
    return n == 0 || (n + 1 < F && e[n] <= e[n - 1] && e[n] < e[n + 1]);
}

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// One Stockham radix-4 pass over the 1024 complex numbers of this wave's frame; v holds the lane's 16 inputs x[j + 256 t] for its
// four butterflies j = lane + 64 q.  Output t of butterfly j goes to expand(j) + t * Ns, with twiddles exp(-2 pi i k t / (4 Ns)).
template <int Ns>
__device__ __forceinline__ void radix4_pass(const float2 (&v)[16], float2* buf, const float2* __restrict__ tw, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = lane + 64 * q, k = j & (Ns - 1);
        float2 a0 = v[4 * q], a1 = v[4 * q + 1], a2 = v[4 * q + 2], a3 = v[4 * q + 3];
        if (Ns > 1) {
            const int m = 2 * k * (kQuarter / Ns);        // index into the 2048-entry table; 3 m < 1536
            a1 = cmul(a1, tw[m]);
            a2 = cmul(a2, tw[2 * m]);
            a3 = cmul(a3, tw[3 * m]);
        }
        const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
        const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
        const int j0 = ((j - k) << 2) + k;
        buf[slot(j0)] = make_float2(s02.x + s13.x, s02.y + s13.y);
        buf[slot(j0 + Ns)] = make_float2(d02.x + d13.y, d02.y - d13.x);            // d02 - i d13
        buf[slot(j0 + 2 * Ns)] = make_float2(s02.x - s13.x, s02.y - s13.y);
        buf[slot(j0 + 3 * Ns)] = make_float2(d02.x - d13.y, d02.y + d13.x);        // d02 + i d13
    }
}

__device__ __forceinline__ void load_pass_inputs(float2 (&v)[16], const float2* buf, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) v[4 * q + t] = buf[slot(lane + 64 * q + kQuarter * t)];
}

// sample * window as a rounded product of its own: it must not contract into the first pass's additions (the frame's bits are
// those of a product that is stored before the butterfly reads it)
__device__ __forceinline__ float windowed(float s, float w) {
#pragma clang fp contract(off)
    return s * w;
}

// One frame on one wave: `buf` is the wave's kFrameSlots complex numbers of LDS.  Every wave of the workgroup must call it (the
// passes are separated by workgroup barriers); a wave without a frame passes live = false, computes on what its fetch returns and
// stores nothing.  mel_row: the frame's 128 dB values; rms_out: the frame's rms, or NULL.
template <class Fetch>
__device__ __forceinline__ void onset_frame(Fetch sample_at, bool live, float2* buf, const float* __restrict__ window,
                                            const float2* __restrict__ twiddle, const int* __restrict__ mel_ptr,
                                            const int* __restrict__ mel_col, const float* __restrict__ mel_w, float* mel_row,
                                            float* rms_out) {
    const int lane = threadIdx.x & 63;

    // ---- gather and window: complex point n is (y[2n], y[2n + 1]); the lane loads exactly the inputs of its first pass ----
    float2 v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = lane + 64 * q + kQuarter * r;
            v[4 * q + r] = make_float2(windowed(sample_at(2 * n), window[2 * n]), windowed(sample_at(2 * n + 1), window[2 * n + 1]));
        }

    // ---- 1024-point complex FFT: five radix-4 passes, each reading everything into registers before it writes ----
    radix4_pass<1>(v, buf, twiddle, lane);
    __syncthreads();
    load_pass_inputs(v, buf, lane);
    __syncthreads();
    radix4_pass<4>(v, buf, twiddle, lane);
    __syncthreads();
    load_pass_inputs(v, buf, lane);
    __syncthreads();
    radix4_pass<16>(v, buf, twiddle, lane);
    __syncthreads();
    load_pass_inputs(v, buf, lane);
    __syncthreads();
    radix4_pass<64>(v, buf, twiddle, lane);
    __syncthreads();
    load_pass_inputs(v, buf, lane);
    __syncthreads();
    radix4_pass<256>(v, buf, twiddle, lane);
    __syncthreads();

    // ---- real-FFT post-pass: X[k] = E + W^k O and X[1024 - k] = conj(E - W^k O), E = (Z[k] + conj Z[1024 - k]) / 2,
    //      O = -i (Z[k] - conj Z[1024 - k]) / 2; the lane takes k = lane + 64 i, lane 0 also k = 512 ----
    float pk[9], pn[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int k = i < 8 ? lane + 64 * i : kHalf / 2;
        const float2 zk = buf[slot(k)], zn = buf[slot((kHalf - k) & (kHalf - 1))];
        const float2 e = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
        const float2 o = make_float2(0.5f * (zk.y + zn.y), -0.5f * (zk.x - zn.x));
        const float2 wo = cmul(twiddle[k], o);
        const float ar = e.x + wo.x, ai = e.y + wo.y, br = e.x - wo.x, bi = e.y - wo.y;
        pk[i] = ar * ar + ai * ai;
        pn[i] = br * br + bi * bi;
    }
    __syncthreads();
    float* P = reinterpret_cast<float*>(buf);       // 1025 powers over the frame's FFT buffer
    float s = 0.0f;                                  // rms: rows 0 and 1024 halved, lane order then the wave butterfly
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = lane + 64 * i;
        P[k] = pk[i];
        P[kHalf - k] = pn[i];
        s += (k == 0) ? (0.5f * pk[i] + 0.5f * pn[i]) : (pk[i] + pn[i]);
    }
    if (lane == 0) {
        P[kHalf / 2] = pk[8];
        s += pk[8];
    }
    s = wave_sum(s);
    if (live && rms_out && lane == 0) *rms_out = sqrtf(2.0f * s / ((float)kNfft * (float)kNfft));
    __syncthreads();

    // ---- mel: the lane owns filters lane and 127 - lane (a narrow and a wide one) and adds each one's bins in table order ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int f = h == 0 ? lane : kMels - 1 - lane;
        const int i0 = mel_ptr[f], i1 = mel_ptr[f + 1];
        float m = 0.0f;
        int i = i0;
        for (; i + 4 <= i1; i += 4) {          // four table entries in flight, added in table order
            const float w0 = mel_w[i], w1 = mel_w[i + 1], w2 = mel_w[i + 2], w3 = mel_w[i + 3];
            const int c0 = mel_col[i], c1 = mel_col[i + 1], c2 = mel_col[i + 2], c3 = mel_col[i + 3];
            m += w0 * P[c0];
            m += w1 * P[c1];
            m += w2 * P[c2];
            m += w3 * P[c3];
        }
        for (; i < i1; ++i) m += mel_w[i] * P[mel_col[i]];
        if (live) mel_row[f] = 10.0f * log10f(fmaxf(1e-10f, m));
    }
}

}  // namespace ls
