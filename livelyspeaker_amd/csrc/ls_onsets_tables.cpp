// The constant tables of the audio-onset chain (ls_onsets.hip): the periodic Hann window, the FFT twiddles and the Slaney mel
// filterbank as librosa.filters.mel(htk=False, norm='slaney') builds it, in CSR form.  No HIP in here: everything is computed in
// double on the host and rounded to float32 once, and ls_onsets_tables hands the result out so that it can be checked without a GPU.
#include <cmath>
#include <cstdint>
#include <vector>

#include "ls_hip.h"
#include "ls_onsets.h"

namespace ls {
namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr double kFsp = 200.0 / 3.0, kMinLogHz = 1000.0, kMinLogMel = kMinLogHz / kFsp;

double hz_to_mel(double f) {
    const double logstep = std::log(6.4) / 27.0;
    return f >= kMinLogHz ? kMinLogMel + std::log(f / kMinLogHz) / logstep : f / kFsp;
}

double mel_to_hz(double m) {
    const double logstep = std::log(6.4) / 27.0;
    return m >= kMinLogMel ? kMinLogHz * std::exp(logstep * (m - kMinLogMel)) : kFsp * m;
}

// numpy.linspace: start + i * step, the last point set to stop
std::vector<double> linspace(double start, double stop, int n) {
    std::vector<double> v((size_t)n);
    const double step = n > 1 ? (stop - start) / (n - 1) : 0.0;
    for (int i = 0; i < n; ++i) v[(size_t)i] = (double)i * step + start;
    if (n > 1) v[(size_t)n - 1] = stop;
    return v;
}

}  // namespace

bool onset_tables_valid(double sr, int n_fft, int n_mels, double fmin, double fmax) {
    return sr > 0 && n_fft >= 4 && (n_fft & (n_fft - 1)) == 0 && n_mels >= 1 && fmin >= 0 && fmax > fmin;
}

OnsetTables make_onset_tables(double sr, int n_fft, int n_mels, double fmin, double fmax) {
    OnsetTables t;
    t.window.resize((size_t)n_fft);
    t.twiddle.resize((size_t)n_fft * 2);
    for (int n = 0; n < n_fft; ++n) {
        const double a = 2.0 * kPi * (double)n / (double)n_fft;
        t.window[(size_t)n] = (float)(0.5 - 0.5 * std::cos(a));
        t.twiddle[(size_t)2 * n] = (float)std::cos(a);            // exp(-2 pi i n / n_fft)
        t.twiddle[(size_t)2 * n + 1] = (float)(-std::sin(a));
    }
    const int bins = 1 + n_fft / 2;
    const std::vector<double> fftfreqs = linspace(0.0, sr / 2.0, bins);
    std::vector<double> mel_f = linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2);
    for (double& m : mel_f) m = mel_to_hz(m);
    t.mel_ptr.assign((size_t)n_mels + 1, 0);
    for (int i = 0; i < n_mels; ++i) {
        const double fd0 = mel_f[(size_t)i + 1] - mel_f[(size_t)i], fd1 = mel_f[(size_t)i + 2] - mel_f[(size_t)i + 1];
        const double enorm = 2.0 / (mel_f[(size_t)i + 2] - mel_f[(size_t)i]);
        for (int k = 0; k < bins; ++k) {
            const double lower = -(mel_f[(size_t)i] - fftfreqs[(size_t)k]) / fd0;
            const double upper = (mel_f[(size_t)i + 2] - fftfreqs[(size_t)k]) / fd1;
            // librosa writes the triangle into a float32 array and scales that array in place by the float64 norm: two roundings
            const float tri = (float)std::fmax(0.0, std::fmin(lower, upper));
            const float w = (float)((double)tri * enorm);
            if (w != 0.0f) {
                t.mel_col.push_back(k);
                t.mel_w.push_back(w);
            }
        }
        t.mel_ptr[(size_t)i + 1] = (int32_t)t.mel_col.size();
    }
    return t;
}

}  // namespace ls

extern "C" int ls_onsets_tables(float sr, int n_fft, int n_mels, float fmin, float fmax, float* window, float* twiddle,
                                int32_t* mel_ptr, int32_t* mel_col, float* mel_w, int32_t nnz_cap, int32_t* nnz_out) {
    if (!ls::onset_tables_valid(sr, n_fft, n_mels, fmin, fmax) || nnz_cap < 0) return LS_EINVAL;
    const ls::OnsetTables t = ls::make_onset_tables(sr, n_fft, n_mels, fmin, fmax);
    const int32_t nnz = (int32_t)t.mel_w.size();
    if (nnz_out) *nnz_out = nnz;
    if (window) for (int n = 0; n < n_fft; ++n) window[n] = t.window[(size_t)n];
    if (twiddle) for (int n = 0; n < 2 * n_fft; ++n) twiddle[n] = t.twiddle[(size_t)n];
    if (mel_ptr) for (int i = 0; i <= n_mels; ++i) mel_ptr[i] = t.mel_ptr[(size_t)i];
    if (mel_col || mel_w) {
        if (nnz_cap < nnz) return LS_EINVAL;
        for (int32_t i = 0; i < nnz; ++i) {
            if (mel_col) mel_col[i] = t.mel_col[(size_t)i];
            if (mel_w) mel_w[i] = t.mel_w[(size_t)i];
        }
    }
    return LS_OK;
}
