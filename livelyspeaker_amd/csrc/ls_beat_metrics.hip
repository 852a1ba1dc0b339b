// The BEAT evaluation metrics of a sampled batch (scripts_beat/utils/metric.py), on the Euler planes ls_beat_post writes:
//   SRGR.run                      :27-51    success[frame, joint] = sum_k |pred - target| < threshold, weighted by semantic[frame]
//   alignment.load_pose           :76-98    six joint-velocity series and their strict local minima (scipy argrelextrema, mode='clip')
//   alignment.GAHR/calculate_align :162-193 mean over the audio onsets of exp(-min_m (onset - beat_m / fps)^2 / (2 sigma^2))
//   L1div.run                     :12-24    sum |x - column mean| over rows
// One workgroup per clip for the first three (1598 (frame, joint) entries and 6 x 33 velocities per clip: latency-bound, it exists so
// that only per-clip scalars leave the GPU); the L1 diversity takes three small launches over row blocks.  Every sum is a fixed tree
// (per-thread stride order, wave butterfly, four wave partials added in order), so a clip's numbers do not depend on the batch size.
#include "ls_hip.h"
#include "ls_internal.h"
#include "ls_staging.h"

namespace ls {
namespace {

constexpr int kSeries = 6, kV = kT - 1;      // velocity series per clip, frames per series
constexpr int kL1Rows = 64;                  // rows per block of the L1-diversity launches

struct BeatMetricsParams {
    int J, order, align_series;
    int joint[kSeries];
    float threshold, scale, sigma, fps;
    const float *pred, *target, *semantic, *onset_times;
    const long long* onset_offsets;
    unsigned char *success, *beat_mask;
    float *srgr_sum, *vel, *align;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_beat_metrics(const BeatMetricsParams p) {
#pragma clang fp contract(off)
    __shared__ float sang[kSeries][kT][3];      // the six joints' Euler angles
    __shared__ float svel[kSeries][kV];
    __shared__ unsigned char sbeat[kV];         // beats of the series the alignment uses
    __shared__ float part[4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int JC = p.J * 3;
    const float* pred = p.pred + (size_t)b * kT * JC;

    // ---- SRGR: per (frame, joint) success, and the clip's weighted sum ----
    if (p.target) {
        const float* tar = p.target + (size_t)b * kT * JC;
        float s = 0.f;
        for (int e = tid; e < kT * p.J; e += 256) {
            const int f = e / p.J;
            const float* a = pred + (size_t)e * 3;
            const float* t = tar + (size_t)e * 3;
            const float diff = (fabsf(a[0] - t[0]) + fabsf(a[1] - t[1])) + fabsf(a[2] - t[2]);
            const bool ok = diff < p.threshold;
            if (p.success) p.success[(size_t)b * kT * p.J + e] = ok ? 1 : 0;
            if (ok) s += (p.semantic ? p.semantic[(size_t)b * kT + f] : 1.0f) * p.scale;
        }
        s = wave_sum(s);
        if ((tid & 63) == 0) part[wave] = s;
        __syncthreads();
        if (tid == 0 && p.srgr_sum) p.srgr_sum[b] = ((part[0] + part[1]) + part[2]) + part[3];
        __syncthreads();
    }
    if (!p.vel && !p.beat_mask && !p.align) return;

    // ---- motion beats: norm of the frame-to-frame difference of each joint's three angles, raw degrees (no wrapping) ----
    for (int i = tid; i < kSeries * kT * 3; i += 256) {
        const int s = i / (kT * 3), r = i - s * (kT * 3), f = r / 3, k = r - f * 3;
        sang[s][f][k] = pred[(size_t)f * JC + p.joint[s] * 3 + k];
    }
    __syncthreads();
    for (int i = tid; i < kSeries * kV; i += 256) {
        const int s = i / kV, f = i - s * kV;
        const float dx = sang[s][f + 1][0] - sang[s][f][0], dy = sang[s][f + 1][1] - sang[s][f][1], dz = sang[s][f + 1][2] - sang[s][f][2];
        const float v = sqrtf((dx * dx + dy * dy) + dz * dz);
        svel[s][f] = v;
        if (p.vel) p.vel[((size_t)b * kSeries + s) * kV + f] = v;
    }
    __syncthreads();
    // argrelextrema(x, np.less, order) in mode='clip': x[i] < x[clip(i - k)] and x[i] < x[clip(i + k)] for k = 1..order; an end
    // frame is compared with itself, so it is never a beat
    for (int i = tid; i < kSeries * kV; i += 256) {
        const int s = i / kV, f = i - s * kV;
        const float x = svel[s][f];
        bool beat = true;
        for (int k = 1; k <= p.order && beat; ++k) {
            const int lo = f - k < 0 ? 0 : f - k, hi = f + k > kV - 1 ? kV - 1 : f + k;
            beat = x < svel[s][lo] && x < svel[s][hi];
        }
        if (p.beat_mask) p.beat_mask[((size_t)b * kSeries + s) * kV + f] = beat ? 1 : 0;
        if (s == p.align_series) sbeat[f] = beat ? 1 : 0;
    }
    if (!p.align) return;
    __syncthreads();

    // ---- BeatAlign: every audio onset against its nearest motion beat; no beat leaves the distance infinite and the clip at 0 ----
    const long long o0 = p.onset_offsets[b], o1 = p.onset_offsets[b + 1];
    const float two_var = 2.0f * (p.sigma * p.sigma);
    float s = 0.f;
    for (long long i = o0 + tid; i < o1; i += 256) {
        const float t = p.onset_times[i];
        float dmin = INFINITY;
        for (int m = 0; m < kV; ++m)
            if (sbeat[m]) dmin = fminf(dmin, fabsf((float)m / p.fps - t));
        s += expf(-(dmin * dmin) / two_var);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) p.align[b] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)(o1 - o0);
}

// ---- L1 diversity: column sums per row block, the column means, then per-block sums of |x - mean| ----------------------------------
// block (r, c) of k_l1div_colsum: rows [r * 64, r * 64 + 64) of columns c * 256 + tid, added in row order
__global__ __launch_bounds__(256) void k_l1div_colsum(const float* __restrict__ x, long long rows, int dim, double* __restrict__ colsum) {
    const int d = blockIdx.y * 256 + threadIdx.x;
    if (d >= dim) return;
    const long long r0 = (long long)blockIdx.x * kL1Rows, r1 = r0 + kL1Rows < rows ? r0 + kL1Rows : rows;
    double s = 0.0;
    for (long long r = r0; r < r1; ++r) s += (double)x[(size_t)r * dim + d];
    colsum[(size_t)blockIdx.x * dim + d] = s;
}

// the block partials added in block order; the mean is rounded to fp32, which is what np.mean of an fp32 array returns
__global__ __launch_bounds__(256) void k_l1div_mean(const double* __restrict__ colsum, long long n_blocks, long long rows, int dim,
                                                    float* __restrict__ mean) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= dim) return;
    double s = 0.0;
    for (long long r = 0; r < n_blocks; ++r) s += colsum[(size_t)r * dim + d];
    mean[d] = (float)(s / (double)rows);
}

// one block per 64 rows: |x - mean| in fp32 as the reference forms it, summed in float64; the caller's rows are only read
__global__ __launch_bounds__(256) void k_l1div_abs(const float* __restrict__ x, const float* __restrict__ mean, long long rows, int dim,
                                                   double* __restrict__ partial) {
    __shared__ double part[4];
    const long long r0 = (long long)blockIdx.x * kL1Rows, r1 = r0 + kL1Rows < rows ? r0 + kL1Rows : rows;
    double s = 0.0;
    for (int d = threadIdx.x; d < dim; d += 256) {
        const float m = mean[d];
        for (long long r = r0; r < r1; ++r) s += (double)fabsf(x[(size_t)r * dim + d] - m);
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

}  // namespace ls

extern "C" int ls_beat_metrics(int device, const ls_beat_metrics_args* a) {
    using namespace ls;
    bool motion;
    long long n_onsets;
    if (!beat_metrics_args_ok(a, &motion, &n_onsets)) return LS_EINVAL;       // any order >= 1: the kernel clamps at the clip's ends
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    const int B = a->batch;
    const size_t n_eu = (size_t)B * kT * a->njoints * 3, n_tj = (size_t)B * kT * a->njoints, n_v = (size_t)B * kSeries * kV;
    BeatMetricsParams p{};
    p.J = a->njoints; p.order = a->order; p.align_series = a->align_series;
    for (int s = 0; s < kSeries; ++s) p.joint[s] = motion ? a->series_joint[s] : 0;
    p.threshold = a->threshold; p.scale = a->scale; p.sigma = a->sigma; p.fps = a->fps;
    Staging st(a->on_device != 0);
    if (a->align) {
        p.onset_offsets = reinterpret_cast<const long long*>(st.upload(a->onset_offsets, (size_t)B + 1));       // host data in both modes
        p.onset_times = st.in(a->onset_times, (size_t)n_onsets);
    }
    p.pred = st.in(a->pred, n_eu);
    p.target = st.in(a->target, n_eu);
    p.semantic = a->target ? st.in(a->semantic, (size_t)B * kT) : nullptr;
    p.success = st.out(a->success, n_tj);
    p.srgr_sum = st.out(a->srgr_sum, (size_t)B);
    p.vel = st.out(a->vel, n_v);
    p.beat_mask = st.out(a->beat_mask, n_v);
    p.align = st.out(a->align, (size_t)B);
    if (st.e == hipSuccess) hipLaunchKernelGGL(k_beat_metrics, dim3(B), dim3(256), 0, 0, p);
    return st.finish();
}

extern "C" int ls_beat_ldiv(int device, int on_device, int64_t rows, int dim, const float* x, double* sum_out) {
    using namespace ls;
    if (!x || !sum_out || rows < 1 || dim < 1) return LS_EINVAL;
    const long long n_blocks = (rows + kL1Rows - 1) / kL1Rows;
    if (n_blocks > 0x7fffffffLL) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    Staging st(on_device != 0);
    const float* d_x = st.in(x, (size_t)rows * dim);
    double* colsum = static_cast<double*>(st.temp((size_t)n_blocks * dim * sizeof(double)));
    float* mean = static_cast<float*>(st.temp((size_t)dim * 4));
    double* d_part = static_cast<double*>(st.temp((size_t)n_blocks * sizeof(double)));
    std::vector<double> partial((size_t)n_blocks);
    if (st.e == hipSuccess) {
        const unsigned cb = (unsigned)((dim + 255) / 256);
        hipLaunchKernelGGL(k_l1div_colsum, dim3((unsigned)n_blocks, cb), dim3(256), 0, 0, d_x, (long long)rows, dim, colsum);
        hipLaunchKernelGGL(k_l1div_mean, dim3(cb), dim3(256), 0, 0, colsum, n_blocks, (long long)rows, dim, mean);
        hipLaunchKernelGGL(k_l1div_abs, dim3((unsigned)n_blocks), dim3(256), 0, 0, d_x, mean, (long long)rows, dim, d_part);
        st.chk(hipGetLastError());
        st.chk(hipMemcpy(partial.data(), d_part, (size_t)n_blocks * sizeof(double), hipMemcpyDeviceToHost));      // the one wait
    }
    if (st.e != hipSuccess) return LS_EHIP;
    double s = 0.0;
    for (double v : partial) s += v;        // block order, float64
    *sum_out = s;
    return LS_OK;
}
