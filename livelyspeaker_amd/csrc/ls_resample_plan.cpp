// The host-only half of the resampler (ls_resample_ratio, ls_resample_plan, ls_resample_taps): the ratio of two rates, the one
// definition of the outputs a push decides, and the taps.  It includes neither HIP nor a handle, so tests/resample_plan_main.cpp
// links this unit alone under the host sanitizers.
//   up / down = out_sr / in_sr in lowest terms, q = max(up, down), half = zeros * q;
//   h[i] = up * (rolloff / q) * sinc(rolloff * (i - half) / q) * kaiser(2 half + 1, beta)[i],  i = 0 .. 2 half;
//   y[m] = sum_k h[m down - k up + half] x[k]: output m reads samples up to floor((m down + half) / up), so with n samples of a series
//   that goes on the outputs below D(n) = max(0, floor((n up - 1 - half) / down) + 1) are decided; a finish decides ceil(n up / down).
#include <cmath>
#include <cstdint>

#include "ls_hip.h"

namespace {

constexpr int64_t kMost = 1LL << 62;              // counts and products stay at or below this
constexpr int64_t kMaxTaps = 1LL << 22;

int64_t gcd64(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

int64_t floor_div(int64_t a, int64_t b) {         // b > 0
    const int64_t d = a / b;
    return d * b > a ? d - 1 : d;
}

// I0 by its own series, sum ((x / 2)^k / k!)^2: every term is positive, so nothing cancels
double bessel_i0(double x) {
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}

}  // namespace

extern "C" int ls_resample_ratio(int32_t in_sr, int32_t out_sr, int32_t zeros, int64_t* up, int64_t* down, int64_t* half, int64_t* taps_per_output,
                                 int64_t* carry_len, int64_t* n_taps) {
    if (!up || !down || !half || !taps_per_output || !carry_len || !n_taps) return LS_EINVAL;
    if (in_sr < 1 || out_sr < 1 || zeros < 1) return LS_EINVAL;
    const int64_t g = gcd64(in_sr, out_sr), u = out_sr / g, d = in_sr / g, q = u > d ? u : d;
    const int64_t hf = (int64_t)zeros * q;        // below 2^62: both factors are below 2^31
    if (2 * hf + 1 > kMaxTaps) return LS_EUNSUPPORTED;
    *up = u;
    *down = d;
    *half = hf;
    *n_taps = 2 * hf + 1;
    *taps_per_output = 2 * hf / u + 1;            // the samples k with |m down - k up| <= half, at most
    *carry_len = (2 * hf + d + u - 1) / u + 1;    // ceil((2 half + down) / up) + 1
    return LS_OK;
}

extern "C" int ls_resample_plan(int64_t up, int64_t down, int64_t half, int64_t n_before, int64_t n_new, int32_t finishing, int64_t* out_first,
                                int64_t* out_count) {
    if (!out_first || !out_count) return LS_EINVAL;
    if (up < 1 || down < 1 || half < 0 || n_before < 0 || n_new < 0) return LS_EINVAL;
    if (up > kMost || down > kMost || half > kMost || n_before > kMost || n_new > kMost - n_before) return LS_EINVAL;
    const int64_t N = n_before + n_new;
    if (N > kMost / up) return LS_EINVAL;         // N * up stays below 2^62 (and so does every sum with half and down below)
    if (finishing && N < 1) return LS_EINVAL;
    auto decided = [&](int64_t n) -> int64_t {
        const int64_t d = floor_div(n * up - 1 - half, down) + 1;
        return d > 0 ? d : 0;
    };
    const int64_t first = decided(n_before);
    const int64_t end = finishing ? (N * up) / down + ((N * up) % down != 0) : decided(N);       // ceil(N up / down), without a sum that could pass 2^63
    *out_first = first;
    *out_count = end - first;
    return LS_OK;
}

extern "C" int ls_resample_taps(int64_t up, int64_t down, int32_t zeros, double beta, double rolloff, double* h64, float* h32) {
    if (!h64 && !h32) return LS_EINVAL;
    if (up < 1 || down < 1 || zeros < 1 || !(beta >= 0.0) || !(rolloff > 0.0) || !(rolloff <= 1.0) || !std::isfinite(beta)) return LS_EINVAL;
    const int64_t q = up > down ? up : down;
    if (q > kMaxTaps || 2 * (int64_t)zeros * q + 1 > kMaxTaps) return LS_EUNSUPPORTED;
    const int64_t half = (int64_t)zeros * q;
    const double pi = 3.14159265358979323846, i0_beta = bessel_i0(beta), scale = (double)up * (rolloff / (double)q);
    for (int64_t i = 0; i <= 2 * half; ++i) {
        const double t = (double)(i - half);
        const double x = rolloff * t / (double)q;
        const double y = pi * (x == 0.0 ? 1e-20 : x);     // np.sinc's own guard
        const double r = t / (double)half;
        const double w = bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0_beta;
        const double h = scale * (std::sin(y) / y) * w;
        if (h64) h64[i] = h;
        if (h32) h32[i] = (float)h;
    }
    return LS_OK;
}
