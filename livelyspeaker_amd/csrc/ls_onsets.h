// What ls_onsets.hip takes from the host-only table unit (ls_onsets_tables.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace ls {

struct OnsetTables {
    std::vector<float> window;      // [n_fft] periodic Hann
    std::vector<float> twiddle;     // [n_fft][2] exp(-2 pi i n / n_fft) as (re, im)
    std::vector<int32_t> mel_ptr;   // [n_mels + 1] CSR row starts
    std::vector<int32_t> mel_col;   // [nnz] FFT bin of each weight, ascending inside a row
    std::vector<float> mel_w;       // [nnz]
};

bool onset_tables_valid(double sr, int n_fft, int n_mels, double fmin, double fmax);
OnsetTables make_onset_tables(double sr, int n_fft, int n_mels, double fmin, double fmax);

}  // namespace ls
