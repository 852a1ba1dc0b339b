// Variational-bound terms for gfx950: one column of calc_bpd_loop (scripts/diffusion/gaussian_diffusion.py:1591-1646) behind a denoiser
// launch that left the CFG-combined model output in memory -- _vb_terms_bpd's KL / decoder NLL (:1213-1246, losses.py:12-77), the x_0
// MSE (:1630) and the eps MSE (:1631-1632), each reduced to one number per sample.
// Mapping: one workgroup of 256 lanes per sample (918 or 9588 elements: 4 or 38 per lane), lanes stride the sample's plane so every
// wave reads whole 256-byte rows (a sample's plane starts on an 8-byte boundary only, so no 16-byte loads); three fp32 partial sums per
// lane, a 64-lane xor-shuffle tree, then the four waves' sums through LDS in wave order.  The tree is fixed and there is no atomic, so
// the same inputs give the same bits on every launch, captured or not.
#include "ls_internal.h"
#include "ls_philox.h"

namespace ls {

namespace {

// approx_standard_normal_cdf (losses.py:42-47); th.pow(x, 3) is x * x * x on the CPU, the constant is the fp32 cast of sqrt(2 / pi)
__device__ __forceinline__ float approx_cdf(float x) {
#pragma clang fp contract(off)
    return 0.5f * (1.0f + tanhf(0.7978845608028654f * (x + 0.044715f * (x * x * x))));
}

// -discretized_gaussian_log_likelihood (losses.py:50-77) of one element, fp32 in the reference's operation order
__device__ __forceinline__ float decoder_nll(float x, float mean, float inv_stdv) {
#pragma clang fp contract(off)
    const float centered = x - mean;
    const float cdf_plus = approx_cdf(inv_stdv * (centered + (float)(1.0 / 255.0)));
    const float cdf_min = approx_cdf(inv_stdv * (centered - (float)(1.0 / 255.0)));
    float q;
    if (x < -0.999f) q = cdf_plus;
    else if (x > 0.999f) q = 1.0f - cdf_min;
    else q = cdf_plus - cdf_min;
    return -logf(fmaxf(q, 1e-12f));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

}  // namespace

__global__ __launch_bounds__(256) void k_vb_terms(const VbArgs a) {
#pragma clang fp contract(off)
    __shared__ float part[4][3];
    const int b = blockIdx.x;
    long long i = a.indices ? (long long)a.indices[b] : (long long)a.index;
    i = i < 0 ? 0 : (i >= a.n_steps ? a.n_steps - 1 : i);
    const float* coef = a.table + (size_t)i * 8;
    const float c1 = coef[0], c2 = coef[1], lv = coef[2], srac = coef[3], srm1ac = coef[4];
    const bool t0 = i == 0;
    // normal_kl (losses.py:33-39) with logvar1 == logvar2 == lv: the terms that do not depend on the element, in the reference's order
    const float kl_head = ((-1.0f + lv) - lv) + expf(lv - lv);
    const float inv_var = expf(-lv);
    const float inv_stdv = expf(-(0.5f * lv));                          // log_scales = 0.5 * log_variance (:1238)
    const size_t base = (size_t)b * a.n;
    float s_vb = 0.f, s_x0 = 0.f, s_eps = 0.f;
    for (int e = threadIdx.x; e < a.n; e += 256) {
        const float x0 = a.x_start[base + e], xt = a.x_t[base + e];
        float px = a.pred[base + e];
        if (a.clip) {                                                   // process_xstart (:365-371)
            px = fminf(fmaxf(px, -1.0f), 1.0f);
            a.pred[base + e] = px;
        }
        if (a.pred_copy) a.pred_copy[base + e] = px;
        const float mean = c1 * px + c2 * xt;                           // q_posterior_mean_variance(pred_xstart, x_t, t) (:385-387)
        if (t0) {
            s_vb += decoder_nll(x0, mean, inv_stdv);
        } else {
            const float true_mean = c1 * x0 + c2 * xt;                  // (:1226-1228)
            const float d = true_mean - mean;
            s_vb += 0.5f * (kl_head + (d * d) * inv_var);
        }
        const float dx = px - x0;
        s_x0 += dx * dx;
        if (a.noise) {
            const float eps = (srac * xt - px) / srm1ac;                // _predict_eps_from_xstart (:418-422)
            const float de = eps - a.noise[base + e];
            s_eps += de * de;
        }
    }
    s_vb = wave_sum(s_vb); s_x0 = wave_sum(s_x0); s_eps = wave_sum(s_eps);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { part[wave][0] = s_vb; part[wave][1] = s_x0; part[wave][2] = s_eps; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float r[3];
        for (int j = 0; j < 3; ++j) r[j] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
        const float n = (float)a.n;
        const size_t o = (size_t)b * a.out_stride + a.out_col;
        a.vb[o] = (r[0] / n) / 0.6931471805599453f;                    // mean_flat(.) / np.log(2.0) (:1235 / :1241)
        a.xstart_mse[o] = r[1] / n;
        if (a.noise) a.mse[o] = r[2] / n;
    }
}

hipError_t launch_vb_terms(const VbArgs& a, int B, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (!a.x_start || !a.x_t || !a.pred || !a.table || !a.vb || !a.xstart_mse || (a.noise && !a.mse)) return hipErrorInvalidValue;
    if (a.n <= 0 || a.n_steps <= 0 || a.out_stride <= 0 || a.out_col < 0 || a.out_col >= a.out_stride) return hipErrorInvalidValue;
    if (!a.indices && (a.index < 0 || a.index >= a.n_steps)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_vb_terms, dim3(B), dim3(256), 0, st, a);
    return hipGetLastError();
}

// PHILOX mode of a column: the column's noise plane from the step-noise stream (3) of step_id -- element index in the reference
// layout (c * T + f), as in the step kernels' own step noise -- and q_sample on it (k_q_sample's expression) in the same pass
__global__ void k_q_sample_philox(const float* __restrict__ x0, float* __restrict__ noise_out, float* __restrict__ xt_out, int JF, int T,
                                  const CallParams* __restrict__ call, unsigned step_id, float a, float b) {
    const int s = blockIdx.x;
    const unsigned long long gidx = call->sample_offset + (unsigned long long)s;
    for (int i = threadIdx.x; i < T * JF; i += blockDim.x) {
        const int f = i / JF, c = i - f * JF;
        const size_t o = (size_t)s * T * JF + i;
        const float nz = philox_normal(call, gidx, step_id, 3u, (unsigned)(c * T + f));
        noise_out[o] = nz;
        xt_out[o] = a * x0[o] + b * nz;
    }
}
hipError_t launch_q_sample_philox(const float* x0, float* noise_out, float* xt_out, int B, int JF, int T, const CallParams* call,
                                  unsigned step_id, float a, float b, hipStream_t st) {
    if (B <= 0) return hipSuccess;
    if (!x0 || !noise_out || !xt_out || !call) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_q_sample_philox, dim3(B), dim3(256), 0, st, x0, noise_out, xt_out, JF, T, call, step_id, a, b);
    return hipGetLastError();
}

}  // namespace ls
