// PLMS (pseudo linear multistep) sampler update for gfx950: the arithmetic of plms_sample
// (scripts/diffusion/gaussian_diffusion.py:1016-1098) behind a denoiser launch that left the CFG-combined model output in memory.
// Pure streaming work: up to six planes read and three written per element, four elements per lane (global_load_dwordx4), no LDS.
#include "ls_internal.h"

namespace ls {

typedef float f4 __attribute__((ext_vector_type(4)));

namespace {

struct PlmsOut { float out, eps, x0; };

// One element.  Every product and sum is written as the reference writes it (fp32, left to right); the divisions are true divisions.
__device__ __forceinline__ PlmsOut plms_element(const PlmsArgs& a, float xt, float x0, float xm, float h0, float h1, float h2) {
    PlmsOut r;
    if (a.clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);                  // process_xstart, before eps is derived (:365-371)
    r.x0 = x0;
    if (a.mode == kPlmsEulerA) {
        const float eps = (a.c0 * xt - x0) / a.c1;                   // _predict_eps_from_xstart (:418-422)
        r.eps = eps;
        r.out = x0 * a.c2 + a.c3 * eps;                              // mean_pred (:1069)
        return r;
    }
    float ep;
    if (a.mode == kPlmsEulerB) {
        const float eps2 = (a.d0 * xm - x0) / a.d1;                  // eps of the evaluation at (mean_pred, t - 1)
        r.eps = eps2;
        ep = (h0 + eps2) / 2.0f;                                     // (:1071)
    } else {
        const float eps = (a.c0 * xt - x0) / a.c1;
        r.eps = eps;
        switch (a.nh) {                                              // (:1078-1086)
        case 0: ep = eps; break;
        case 1: ep = (3.0f * eps - h0) / 2.0f; break;
        case 2: ep = (23.0f * eps - 16.0f * h0 + 5.0f * h1) / 12.0f; break;
        default: ep = (55.0f * eps - 59.0f * h0 + 37.0f * h1 - 9.0f * h2) / 24.0f; break;
        }
    }
    const float pred = a.c0 * xt - a.c1 * ep;                        // _predict_xstart_from_eps (:411-416)
    const float mean = pred * a.c2 + a.c3 * ep;                      // (:1073 / :1090)
    r.out = a.t_nonzero ? mean : x0;                                 // nonzero_mask (:1095-1096)
    return r;
}

}  // namespace

__global__ __launch_bounds__(256) void k_plms_update(const PlmsArgs a) {
    const size_t n4 = a.n >> 2;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool multi = a.mode == kPlmsMulti;
    for (size_t i = tid; i < n4; i += stride) {
        const f4 xt = reinterpret_cast<const f4*>(a.x_t)[i];
        const f4 x0 = reinterpret_cast<const f4*>(a.x0)[i];
        f4 xm = {0.f, 0.f, 0.f, 0.f}, h0 = xm, h1 = xm, h2 = xm;
        if (a.mode == kPlmsEulerB) xm = reinterpret_cast<const f4*>(a.x_mid)[i];
        if (a.mode == kPlmsEulerB || (multi && a.nh >= 1)) h0 = reinterpret_cast<const f4*>(a.hist[0])[i];
        if (multi && a.nh >= 2) h1 = reinterpret_cast<const f4*>(a.hist[1])[i];
        if (multi && a.nh >= 3) h2 = reinterpret_cast<const f4*>(a.hist[2])[i];
        f4 o, e, p;
        for (int j = 0; j < 4; ++j) {
            const PlmsOut r = plms_element(a, xt[j], x0[j], xm[j], h0[j], h1[j], h2[j]);
            o[j] = r.out; e[j] = r.eps; p[j] = r.x0;
        }
        reinterpret_cast<f4*>(a.out)[i] = o;
        if (a.eps_out) reinterpret_cast<f4*>(a.eps_out)[i] = e;
        if (a.pred_out) reinterpret_cast<f4*>(a.pred_out)[i] = p;
    }
    for (size_t i = (n4 << 2) + tid; i < a.n; i += stride) {          // at most three tail elements
        const float xm = a.mode == kPlmsEulerB ? a.x_mid[i] : 0.f;
        const float h0 = (a.mode == kPlmsEulerB || (multi && a.nh >= 1)) ? a.hist[0][i] : 0.f;
        const float h1 = (multi && a.nh >= 2) ? a.hist[1][i] : 0.f;
        const float h2 = (multi && a.nh >= 3) ? a.hist[2][i] : 0.f;
        const PlmsOut r = plms_element(a, a.x_t[i], a.x0[i], xm, h0, h1, h2);
        a.out[i] = r.out;
        if (a.eps_out) a.eps_out[i] = r.eps;
        if (a.pred_out) a.pred_out[i] = r.x0;
    }
}

hipError_t launch_plms_update(const PlmsArgs& a, hipStream_t st) {
    if (a.n == 0) return hipSuccess;
    if (!a.x_t || !a.x0 || !a.out || a.nh < 0 || a.nh > 3) return hipErrorInvalidValue;
    if (a.mode == kPlmsEulerB && (!a.x_mid || !a.hist[0])) return hipErrorInvalidValue;
    if (a.mode == kPlmsMulti)
        for (int j = 0; j < a.nh; ++j) if (!a.hist[j]) return hipErrorInvalidValue;
    const void* ptrs[9] = {a.x_t, a.x0, a.x_mid, a.hist[0], a.hist[1], a.hist[2], a.out, a.eps_out, a.pred_out};
    for (const void* p : ptrs) if (reinterpret_cast<uintptr_t>(p) & 15u) return hipErrorInvalidValue;     // the 16-byte accesses above
    const size_t work = (a.n + 3) / 4;
    const size_t blocks = (work + 255) / 256;
    hipLaunchKernelGGL(k_plms_update, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace ls
