// Double-precision references, derived per-element bounds and deliberately wrong ("perturbed") references for the transformer towers'
// non-GEMM kernels (ls_sag.hip, ls_sag_enc.hip, ls_clip_text.hip).  Plain C++, no HIP: tools/xfmr_check.cpp uses it for the GPU
// comparison and for its --host mode (tests/test_xfmr_ref_host.py checks these references against torch in float64 and the bounds
// against the perturbed references).
//
// Error model, u = 2^-24 (half an ulp of fp32, relative): one rounding costs u |result|; a sum of n terms in ANY order costs at most
// (n + 8) u sum|terms| (n - 1 additions, each at most u of a partial sum that is at most sum|terms|; the + 8 leaves room for the FMA /
// MFMA forms and the scalings around the sum).  Every bound below is computed from the operands alone, never from a kernel's output.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace xfmr {

constexpr double kU = 1.0 / 16777216.0;      // 2^-24
// The device's expf, reciprocal and the normalisation of the probabilities, in units of u of sum_j p_j |v_jd|.  Measured on the MI355X
// with the probe case clip_probe (integer q and k and scale 1/8: exact scores; positive v, so sum p |v| is the result itself): the
// worst distance of the kernel's P.V from fp64 is 7.83 ulp of the result (profiles/r30_xfmr_check.md; it contains the rounding of the
// row sum and of the P.V sum over up to 80 keys as well); times 4 = 31.3, rounded up to a power of two.
constexpr double kCexp = 32.0;

// ---------------------------------------------------------------- inputs: an integer hash turned into uniform or normal values
inline uint32_t hash3(uint32_t t, uint32_t i, uint32_t j) {
    uint32_t h = t * 0x9e3779b9u + i * 0x85ebca6bu + j * 0xc2b2ae35u + 0x27d4eb2fu;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return h;
}
inline float unif(uint32_t t, uint32_t i, uint32_t j) { return (float)(hash3(t, i, j) >> 8) * (1.0f / 16777216.0f) - 0.5f; }      // [-0.5, 0.5)
// N(0, 1) as the sum of twelve 24-bit uniforms minus 6 (Irwin-Hall): integer arithmetic and one exact conversion, the same bits everywhere
inline float normal(uint32_t t, uint32_t i, uint32_t j) {
    uint64_t s = 0;
    for (uint32_t n = 0; n < 12; ++n) s += hash3(t + 0x01000193u * (n + 1), i, j) >> 8;
    return (float)(((double)s - 6.0 * 16777216.0) * (1.0 / 16777216.0));
}
inline float sign_of(uint32_t t, uint32_t i, uint32_t j) { return (hash3(t, i, j) & 0x100u) ? 1.0f : -1.0f; }

inline double ulp32(double v) {
    v = std::fabs(v);
    if (v < 1.17549435e-38) return std::ldexp(1.0, -149);
    return std::ldexp(1.0, std::ilogb(v) - 23);
}

// ---------------------------------------------------------------- attention
// out[a][d] = sum_j p_j v[j][d], p = softmax_j(scale q_a . k_j) over the valid keys of row a.
//   scores   : s_j carries E_s(a, j) = (HD + 8) u scale sum_d |q_d k_d|                       (a sum of HD products, then the scale)
//   softmax  : an error e of every score changes every p_j by at most the factor exp(2 e): the numerator moves by exp(+-e), the
//              normaliser by exp(-+e); to first order 2 max_j E_s relative to p_j.  expf, the reciprocal of the row sum and the
//              product e_j * (1 / sum) are kCexp u relative (measured, see kCexp).
//   P.V      : a sum over the S_keys valid keys (the padded keys enter as exact zeros): (S_keys + 8) u sum_j p_j |v_jd|.
// |err(a, d)| <= sum_j p_j |v_jd| (2 max_j E_s(a, j) + kCexp u + (S_keys + 8) u)
struct AttnData {
    int B = 0, heads = 0, HD = 0;
    std::vector<int> len, row0;              // tokens of sample b and its first row in qkv (dense: len = S, row0 = b S)
    std::vector<double> qkv;                 // [rows][3 D]: q | k | v
    std::vector<uint8_t> mask;               // [B][S] key-padding mask, 1 = valid; empty: none
    bool causal = false;
    int D() const { return heads * HD; }
    int rows() const { return row0.back() + len.back(); }
};
enum Drop { kDropNone, kDropLast, kDropLeast };
// A variant of the operation: the true one (all defaults) or one of the known-wrong ones of the sensitivity check.
struct AttnVar {
    int scale_mode = 0;          // 0: 1 / sqrt(HD); 1: q unscaled; 2: 1 / HD
    Drop drop = kDropNone;       // the last valid key, or the least probable valid key, of every row with two or more valid keys
    int mask_shift = 0;          // the key mask rotated by one key
    int causal_off = 0;          // -1: key a excluded (rows a >= 1); +1: key a + 1 included (rows a + 1 < len)
    int v_head = 0;              // head h reads head (h + v_head) % heads' V
    bool only_row0 = false;      // query row 0 of every sample only; out is [B][D]
};
inline void attn_ref(const AttnData& t, const AttnVar& var, std::vector<double>& out, std::vector<double>* bound) {
    const int D = t.D(), HD = t.HD, ld = 3 * D;
    const double scale = var.scale_mode == 1 ? 1.0 : var.scale_mode == 2 ? 1.0 / HD : 1.0 / std::sqrt((double)HD);
    const size_t nout = (size_t)(var.only_row0 ? t.B : t.rows()) * D;
    out.assign(nout, 0.0);
    if (bound) bound->assign(nout, 0.0);
    for (int b = 0; b < t.B; ++b) {
        const int S = t.len[b];
        std::vector<double> s(S), p(S);
        std::vector<char> ok(S);
        for (int h = 0; h < t.heads; ++h)
            for (int a = 0; a < (var.only_row0 ? 1 : S); ++a) {
                const double* q = &t.qkv[(size_t)(t.row0[b] + a) * ld + h * HD];
                int nvalid = 0, last = -1;
                double emax = 0, m = -INFINITY;
                for (int j = 0; j < S; ++j) {
                    bool v = t.mask.empty() || t.mask[(size_t)b * S + (j + S - var.mask_shift) % S] != 0;
                    if (t.causal) v = v && (var.causal_off < 0 && a > 0 ? j < a : j <= a + std::max(var.causal_off, 0));
                    ok[j] = v;
                    if (!v) continue;
                    const double* k = &t.qkv[(size_t)(t.row0[b] + j) * ld + D + h * HD];
                    double dot = 0, ad = 0;
                    for (int d = 0; d < HD; ++d) { dot += q[d] * k[d]; ad += std::fabs(q[d] * k[d]); }
                    s[j] = scale * dot;
                    emax = std::max(emax, (HD + 8) * kU * scale * ad);
                    m = std::max(m, s[j]);
                    ++nvalid; last = j;
                }
                if (var.drop != kDropNone && nvalid >= 2) {
                    int gone = last;
                    if (var.drop == kDropLeast)
                        for (int j = 0; j < S; ++j) if (ok[j] && s[j] < s[gone]) gone = j;
                    ok[gone] = 0; --nvalid;
                    m = -INFINITY;
                    for (int j = 0; j < S; ++j) if (ok[j]) m = std::max(m, s[j]);
                }
                double sum = 0;
                for (int j = 0; j < S; ++j) { p[j] = ok[j] ? std::exp(s[j] - m) : 0.0; sum += p[j]; }
                const double rel = 2 * emax + kCexp * kU + (nvalid + 8) * kU;
                const int hv = (h + var.v_head) % t.heads;
                const size_t o = (size_t)(var.only_row0 ? b : t.row0[b] + a) * D + h * HD;
                for (int d = 0; d < HD; ++d) {
                    double acc = 0, aacc = 0;
                    for (int j = 0; j < S; ++j) {
                        if (!ok[j]) continue;
                        const double pv = p[j] / sum * t.qkv[(size_t)(t.row0[b] + j) * ld + 2 * D + hv * HD + d];
                        acc += pv; aacc += std::fabs(pv);
                    }
                    out[o + d] = acc;
                    if (bound) (*bound)[o + d] = aacc * rel;
                }
            }
    }
}

// ---------------------------------------------------------------- LayerNorm over 512 features
// y_i = (x_i - mean) rstd w_i + beta_i, rstd = 1 / sqrt(var + eps), biased variance; x_i = x0_i + bc_i when a per-sample vector is added.
// With n = 512, e_i the error x_i arrives with (u |x_i| for the rounded sum x0 + bc; the first stage's whole bound in the two-stage form)
// and a_i = x_i - mean, three errors are carried through:
//   mean : dm = (n + 8) u mean|x| + mean(e)               -- on a row of 1000 + 0.01 N(0,1) this is 0.03, three times the row's sigma,
//                                                            and it is the term that decides the bound there: nothing hides it
//   a_i  : da_i = dm + e_i + u |a_i|
//   var  : the common shift dm moves mean(a^2) by dm^2 + 2 dm mean(g) only (sum a_i = 0), the element-wise part g_i = e_i + u |a_i| by
//          mean(2 |a_i| g_i + g_i^2), the sum itself by (n + 12) u var:  dvar = dm^2 + 2 dm mean(g) + mean(2 |a| g + g^2) + (n + 12) u var'
//   rstd : |d rstd / rstd| <= dvar / (2 (var + eps - dvar_minus)) + 4 u                     (scaling by 1/n, + eps, sqrt, reciprocal)
//          dvar_minus = the part of dvar that can lower the variance (all of it but dm^2)
//   y    : |w_i| rstd da_i + |a_i rstd w_i| (rel_rstd + 4 u) + 2 u (|a_i rstd w_i| + |beta_i|)
struct LnVar {
    bool unbiased = false;
    double eps = 1e-5;
    int bc_div = 34;
};
// x [rows][512] (double), bc [..][bc_ld] or null, e_in [rows][512] or null; y and bound [rows][512]
inline void ln_ref(const double* x0, const double* e_in, const double* bc, int bc_ld, const float* w, const float* beta, int rows, const LnVar& var,
                   double* y, double* bound) {
    constexpr int n = 512;
    std::vector<double> x(n), e(n);
    for (int r = 0; r < rows; ++r) {
        double s = 0, sa = 0, se = 0;
        for (int i = 0; i < n; ++i) {
            x[i] = x0[(size_t)r * n + i] + (bc ? bc[(size_t)(r / var.bc_div) * bc_ld + i] : 0.0);
            e[i] = (e_in ? e_in[(size_t)r * n + i] : 0.0) + (bc ? kU * std::fabs(x[i]) : 0.0);
            s += x[i]; sa += std::fabs(x[i]); se += e[i];
        }
        const double mean = s / n, dm = (n + 8) * kU * (sa / n) + se / n;
        double q = 0, g1 = 0, g2 = 0;
        for (int i = 0; i < n; ++i) {
            const double a = x[i] - mean, g = e[i] + kU * std::fabs(a);
            q += a * a; g1 += g; g2 += 2 * std::fabs(a) * g + g * g;
        }
        const double vb = q / n, v = var.unbiased ? q / (n - 1) : vb;
        const double rstd = 1.0 / std::sqrt(v + var.eps);
        const double minus0 = 2 * dm * (g1 / n) + g2 / n;
        const double minus = minus0 + (n + 12) * kU * (vb + dm * dm + minus0), dvar = dm * dm + minus;
        const double rel = dvar / (2 * std::max(vb + var.eps - minus, 0.5 * (vb + var.eps))) + 4 * kU;
        for (int i = 0; i < n; ++i) {
            const double a = x[i] - mean, t = a * rstd * w[i];
            y[(size_t)r * n + i] = t + beta[i];
            if (bound)
                bound[(size_t)r * n + i] = std::fabs(w[i]) * rstd * (dm + e[i] + kU * std::fabs(a)) + std::fabs(t) * (rel + 4 * kU) +
                                           2 * kU * (std::fabs(t) + std::fabs(beta[i]));
        }
    }
}

// ---------------------------------------------------------------- k_sag_final: out[b][c][f] = [mask[b][f]] (sum_d W[c][d] x[b, f, d] + bias[c])
// The GEMM form: |err| <= 2 (K + 8) u (sum_d |W x| + |bias|), K = 512 (four partial sums of 128, summed, then the bias); 0 where masked.
struct FinalVar {
    bool no_bias = false;
    int mask_shift = 0;          // frame f reads mask[f - 1] (cyclic)
};
inline void final_ref(const float* xh, const float* wf, const float* bf, const uint8_t* mask, int B, int JF, int T, int D, const FinalVar& var,
                      std::vector<double>& out, std::vector<double>* bound) {
    out.assign((size_t)B * JF * T, 0.0);
    if (bound) bound->assign(out.size(), 0.0);
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < JF; ++c)
            for (int f = 0; f < T; ++f) {
                if (mask && mask[b * T + (f + T - var.mask_shift) % T] == 0) continue;
                double dot = 0, ad = 0;
                for (int d = 0; d < D; ++d) {
                    const double pr = (double)wf[(size_t)c * D + d] * xh[((size_t)b * T + f) * D + d];
                    dot += pr; ad += std::fabs(pr);
                }
                const double bv = var.no_bias ? 0.0 : bf[c];
                out[((size_t)b * JF + c) * T + f] = dot + bv;
                if (bound) (*bound)[((size_t)b * JF + c) * T + f] = 2.0 * (D + 8) * kU * (ad + std::fabs(bv));
            }
}

// ---------------------------------------------------------------- k_sag_queries
// q[b T + f][d] = bmap[d] + [f < n_pre] (sum_c W[d][c] x[b][c][f] + W[d][JF]) + pe[f][d]
// The GEMM form with K = JF: |err| <= 2 (K + 8) u (sum_c |W x| + |W[d][JF]| + |bmap| + |pe|).  pe holds T + 1 rows here (the device gets T).
struct QueriesVar {
    bool no_bit = false;
    int pe_shift = 0;
};
inline void queries_ref(const float* x, const float* wmap, const float* bmap, const float* pe, int B, int JF, int T, int D, int n_pre,
                        const QueriesVar& var, std::vector<double>& out, std::vector<double>* bound) {
    out.assign((size_t)B * T * D, 0.0);
    if (bound) bound->assign(out.size(), 0.0);
    for (int b = 0; b < B; ++b)
        for (int f = 0; f < T; ++f)
            for (int d = 0; d < D; ++d) {
                double v = bmap[d], av = std::fabs(bmap[d]);
                if (f < n_pre) {
                    const float* w = wmap + (size_t)d * (JF + 1);
                    for (int c = 0; c < JF; ++c) {
                        const double pr = (double)w[c] * x[((size_t)b * JF + c) * T + f];
                        v += pr; av += std::fabs(pr);
                    }
                    if (!var.no_bit) { v += w[JF]; av += std::fabs(w[JF]); }
                }
                const double p = pe[(size_t)(f + var.pe_shift) * D + d];
                out[((size_t)b * T + f) * D + d] = v + p;
                if (bound) (*bound)[((size_t)b * T + f) * D + d] = 2.0 * (JF + 8) * kU * (av + std::fabs(p));
            }
}

// worst |wrong - true| / bound over the elements with a bound above zero (a zero bound with a difference counts as detected)
inline double sensitivity(const std::vector<double>& wrong, const std::vector<double>& truth, const std::vector<double>& bound) {
    double worst = 0;
    for (size_t i = 0; i < truth.size(); ++i) {
        const double d = std::fabs(wrong[i] - truth[i]);
        if (!(d == d)) return INFINITY;          // the wrong form is not even finite here (eps omitted on a constant row)
        if (d == 0) continue;
        worst = std::max(worst, bound[i] > 0 ? d / bound[i] : INFINITY);
    }
    return worst;
}

}  // namespace xfmr
