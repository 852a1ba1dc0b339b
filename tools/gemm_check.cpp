// Stand-alone check of launch_gemm_tr (csrc/ls_gemm.hip) against fp64 on every dispatch path -- tests/test_gpu_gemm.py builds and runs it:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -I include -I livelyspeaker_amd/csrc -I tools tools/gemm_check.cpp livelyspeaker_amd/csrc/ls_gemm.hip -o gemm_check
//   gemm_check <general | fulltile | dma | dma_ln | splitk>
// For every case of the group (tools/gemm_cases.h): operands from an integer hash, every buffer embedded in a larger one whose rest is
// NaN (pad columns, gaps of two-level strides, guard blocks), outputs pre-filled with a NaN sentinel; the plan's kind is printed, the
// product is launched twice, and EVERY output element is compared with a double-precision evaluation under a derived bound
//     |err| <= 2 (K + 8) 2^-24 (sum_k |a_k b_k| + |bias| + |R| + |C_old|)       (fp32 FMA accumulation in any order)
// carried through the activation's Lipschitz constant plus kActUlp ulp of the result; the LayerNorm form adds the error of the
// reconstructed rstd (kRstdRel).  One line per case:
//     case=<name> kind=<...> ratio=<worst err / bound> nonfinite=<n> guard=<ok|bad> repeat=<ok|bad> ...
// The program stops with a non-zero exit at the first HIP error and starts nothing after it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>
#include "ls_gemm_plan.h"
#include "gemm_cases.h"

using namespace gemm_cases;

// Measured on the MI355X (profiles/r23_gemm_check.md).  kActUlp: worst distance of C from act64 of the kernel's OWN stored
// pre-activation over the K = 32 cases, 7.13 ulp (exact GELU; SiLU 2.35, exp 0.77, QuickGELU 2.82), times 4, rounded up to a power
// of two.  (Against act64 of the REFERENCE pre-activation the distance is 1.4e4 ulp: where the pre-activation crosses zero its own
// 1e-8 of product error is thousands of ulp of a result near zero.  That part is the Lipschitz term's, not the activation's.)
// kRstdRel: worst relative error of the epilogue's rstd against fp64, 2.29e-7 (case ln_rstd_probe), times 4.
constexpr double kActUlp = 32.0;
constexpr double kRstdRel = 9.2e-7;

constexpr double kU = 1.0 / 16777216.0;       // 2^-24
constexpr size_t kGuard = 256;                // floats before and after every buffer (keeps the 256-byte alignment of the base)
constexpr uint32_t kNanIn = 0x7fc00000u;      // quiet NaN around the inputs
constexpr uint32_t kNanOut = 0x7fc0beefu;     // sentinel in the outputs

#define HIP_OK(x)                                                                                            \
    do {                                                                                                     \
        hipError_t e_ = (x);                                                                                 \
        if (e_ != hipSuccess) {                                                                              \
            std::printf("HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, __LINE__, #x);     \
            std::fflush(stdout);                                                                             \
            std::exit(3);                                                                                    \
        }                                                                                                    \
    } while (0)

static float bits_f(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t f_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

// value in [-0.5, 0.5) from (tensor, row, column): a fixed integer hash, the same on every machine
static float hval(uint32_t t, uint32_t i, uint32_t j) {
    uint32_t h = t * 0x9e3779b9u + i * 0x85ebca6bu + j * 0xc2b2ae35u + 0x27d4eb2fu;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    return (float)(h >> 8) * (1.0f / 16777216.0f) - 0.5f;
}
enum { tA = 1, tB, tBias, tR, tC, tAddn, tMean };

// a host buffer [guard | body | guard] with a mask of the body's logical elements, and its device twin
struct Buf {
    std::vector<float> h;
    std::vector<uint8_t> used;
    float* d = nullptr;
    size_t off = 0;                                   // logical base inside the body, in floats
    void init(size_t body, size_t off_, uint32_t fill) {
        off = off_;
        h.assign(kGuard + off + body + kGuard, bits_f(fill));
        used.assign(h.size(), 0);
        HIP_OK(hipMalloc(&d, h.size() * 4));
    }
    float& at(long long i) { used[kGuard + off + i] = 1; return h[kGuard + off + i]; }
    float get(long long i) const { return h[kGuard + off + i]; }
    float* base() const { return d + kGuard + off; }
    void up() const { HIP_OK(hipMemcpy(d, h.data(), h.size() * 4, hipMemcpyHostToDevice)); }
    std::vector<float> down() const {
        std::vector<float> o(h.size());
        HIP_OK(hipMemcpy(o.data(), d, o.size() * 4, hipMemcpyDeviceToHost));
        return o;
    }
    void release() { if (d) HIP_OK(hipFree(d)); d = nullptr; }
};

static double act64(double v, int act) {
    if (act == 1) return v / (1.0 + std::exp(-v));
    if (act == 2) return std::exp(0.5 * v);
    if (act == 3) return 0.5 * v * (1.0 + std::erf(v * 0.70710678118654752440));
    if (act == 4) return v / (1.0 + std::exp(-1.702 * v));
    return v;
}
// Lipschitz constant on [v - e, v + e]: sup |SiLU'| = sup |QuickGELU'| = 1.0998, sup |GELU'| = 1.1290; exp(y / 2) by its own derivative
static double act_lip(double v, double e, int act) {
    if (act == 1 || act == 4) return 1.1;
    if (act == 2) return 0.5 * std::exp(0.5 * (v + e));
    if (act == 3) return 1.13;
    return 1.0;
}
static double ulp32(double v) {
    v = std::fabs(v);
    if (v < 1.17549435e-38) return std::ldexp(1.0, -149);
    return std::ldexp(1.0, std::ilogb(v) - 23);
}

struct Worst {
    double ratio = 0, actulp = 0, actulp_own = 0, rstd_rel = 0;
    long long nonfinite = 0;
    void merge(const Worst& o) {
        ratio = std::max(ratio, o.ratio); actulp = std::max(actulp, o.actulp); actulp_own = std::max(actulp_own, o.actulp_own);
        rstd_rel = std::max(rstd_rel, o.rstd_rel); nonfinite += o.nonfinite;
    }
    void see(double err, double bound) {
        if (!(err == err) || std::isinf(err)) { ++nonfinite; return; }
        const double r = bound > 0 ? err / bound : (err > 0 ? 1e30 : 0.0);
        if (r > ratio) ratio = r;
    }
};

template <class F>
static void parallel_rows(int rows, F f) {            // f(thread, row0, row1)
    const int nt = std::max(1, std::min(16, std::min(rows, (int)std::thread::hardware_concurrency())));
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([=] { f(t, (int)((long long)rows * t / nt), (int)((long long)rows * (t + 1) / nt)); });
    for (auto& x : th) x.join();
}

static std::map<std::string, std::vector<float>> g_kept;      // logical C [M][N] of the cases that a later case refers to

static bool run_case(const Case& c, bool keep) {
    const auto t0 = std::chrono::steady_clock::now();
    const int M = c.M, N = c.N, K = c.K, nb = c.nbatch;
    const ls::GemmOperand oa = op_make(c.A, nullptr, M, K), ob = op_make(c.B, nullptr, N, K);
    const long long extA = op_extent(c.A, M, K), extB = op_extent(c.B, N, K), extC = c_extent(c);
    const long long bsA = nb > 1 ? batch_stride(extA) : 0, bsB = nb > 1 && !c.shared_b ? batch_stride(extB) : 0, bsC = nb > 1 ? batch_stride(extC) : 0;
    const bool has_r = c.r || (c.ln && !c.probe);

    // ---- inputs: NaN everywhere, data at the addressed elements ----
    Buf A, B, bias, R, C, Cpre, ws, lnp, wsum, addn, pout;
    A.init((size_t)(bsA * (nb - 1) + extA), c.A.off, kNanIn);
    B.init((size_t)(bsB * (nb - 1) + extB), c.B.off, kNanIn);
    std::vector<double> Ad((size_t)nb * M * K), Bd((size_t)(c.shared_b ? 1 : nb) * N * K);      // dense double copies for the reference
    for (int b = 0; b < nb; ++b)
        for (int m = 0; m < M; ++m)
            for (int k = 0; k < K; ++k) {
                float v = hval(tA, (uint32_t)(b * 65536 + c.row0 + m), (uint32_t)k);
                if (c.ln) v = 0.6f * hval(tMean, (uint32_t)(c.row0 + m), 0) + 3.4641016f * v;       // row mean in [-0.3, 0.3), std 1
                A.at(b * bsA + op_at(oa, m, k)) = v;
                Ad[((size_t)b * M + m) * K + k] = v;
            }
    for (int b = 0; b < (c.shared_b ? 1 : nb); ++b)
        for (int n = 0; n < N; ++n)
            for (int k = 0; k < K; ++k) {
                const float v = c.probe ? (n == k ? 1.0f : 0.0f) : hval(tB, (uint32_t)(b * 65536 + n), (uint32_t)k);
                B.at(b * bsB + op_at(ob, n, k)) = v;
                Bd[((size_t)b * N + n) * K + k] = v;
            }
    bias.init((size_t)N, (size_t)c.bias_off, kNanIn);
    for (int n = 0; n < N; ++n) bias.at(n) = hval(tBias, 0, (uint32_t)n);
    addn.init((size_t)N, 0, kNanIn);
    for (int n = 0; n < N; ++n) addn.at(n) = hval(tAddn, 0, (uint32_t)n);
    const size_t cbody = (size_t)(bsC * (nb - 1) + extC);
    R.init(cbody, (size_t)c.offc, kNanIn);
    C.init(cbody, (size_t)c.offc, kNanOut);
    Cpre.init(cbody, (size_t)c.offc, kNanOut);
    const bool c_data = c.acc || c.r_inplace;                                // the logical extent of C holds data before the launch
    for (int b = 0; b < nb; ++b)
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) {
                const long long o = b * bsC + c_at(c, m, n);
                R.at(o) = hval(tR, (uint32_t)(b * 65536 + c.row0 + m), (uint32_t)n);
                float& cv = C.at(o);
                if (c_data) cv = hval(c.r_inplace ? tR : tC, (uint32_t)(b * 65536 + c.row0 + m), (uint32_t)n);
                Cpre.at(o) = bits_f(kNanOut);
            }
    // LayerNorm inputs, computed in double and rounded once: (mean, M2) of the eight 64-column groups of every A row, wsum[n] = sum_k W'[n][k]
    std::vector<double> rmean, rrstd, wsum64;
    if (c.ln) {
        lnp.init((size_t)M * 16, 0, kNanIn);
        wsum.init((size_t)N, 0, kNanIn);
        pout.init((size_t)M * (N / 64) * 2, 0, kNanOut);
        rmean.resize(M); rrstd.resize(M); wsum64.resize(N);
        for (int m = 0; m < M; ++m) {
            double s = 0;
            for (int k = 0; k < K; ++k) s += Ad[(size_t)m * K + k];
            const double mean = s / K;
            double q = 0;
            for (int k = 0; k < K; ++k) q += (Ad[(size_t)m * K + k] - mean) * (Ad[(size_t)m * K + k] - mean);
            rmean[m] = mean;
            rrstd[m] = 1.0 / std::sqrt(q / K + 1e-5);
            for (int gq = 0; gq < 8; ++gq) {
                double gs = 0, gm2 = 0;
                for (int k = 0; k < 64; ++k) gs += Ad[(size_t)m * K + 64 * gq + k];
                gs /= 64;
                for (int k = 0; k < 64; ++k) gm2 += (Ad[(size_t)m * K + 64 * gq + k] - gs) * (Ad[(size_t)m * K + 64 * gq + k] - gs);
                lnp.at((size_t)m * 16 + 2 * gq) = (float)gs;
                lnp.at((size_t)m * 16 + 2 * gq + 1) = (float)gm2;
            }
        }
        for (int n = 0; n < N; ++n) {
            double s = 0;
            for (int k = 0; k < K; ++k) s += Bd[(size_t)n * K + k];
            wsum64[n] = s;
            wsum.at(n) = (float)s;
        }
        for (size_t i = 0; i < (size_t)M * (N / 64) * 2; ++i) pout.at((long long)i) = bits_f(kNanOut);
    }

    // ---- plan ----
    Ptrs p{};
    p.A = A.base(); p.B = B.base(); p.C = C.base(); p.Cpre = Cpre.base(); p.R = R.base(); p.bias = bias.base();
    p.ln_part = c.ln ? lnp.base() : nullptr; p.wsum = c.ln ? wsum.base() : nullptr; p.addn = addn.base(); p.part_out = c.ln ? pout.base() : nullptr;
    ls::GemmArgs a = make_args(c, p);
    const ls::GemmPlan first = ls::gemm_plan(a, c.A.kc, c.B.kc, c.splits);
    const size_t need = ws_need(c, first.splits);                           // a workspace exactly large enough, in a buffer with a tail
    if (need) {
        ws.init(need + 1024, 0, kNanOut);
        a.ws = ws.base();
        a.ws_floats = need - (size_t)c.ws_short;
    }
    const ls::GemmPlan plan = ls::gemm_plan(a, c.A.kc, c.B.kc, c.splits);

    // ---- launch, twice ----
    A.up(); B.up(); bias.up(); addn.up(); R.up();
    if (c.ln) { lnp.up(); wsum.up(); }
    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));
    std::vector<float> outC[2], outP[2], outO[2], outW[2];
    bool rejected = false;
    for (int rep = 0; rep < 2; ++rep) {
        C.up(); Cpre.up();
        if (need) ws.up();
        if (c.ln) pout.up();
        const hipError_t e = ls::launch_gemm_tr(a, c.A.kc, c.B.kc, c.splits, st);
        if (c.reject) {
            if (e != hipErrorInvalidValue) { std::printf("case=%s: expected hipErrorInvalidValue, got %s\n", c.name.c_str(), hipGetErrorString(e)); return false; }
            rejected = true;
        } else HIP_OK(e);
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(st));
        outC[rep] = C.down(); outP[rep] = Cpre.down();
        if (need) outW[rep] = ws.down();
        if (c.ln) outO[rep] = pout.down();
    }
    HIP_OK(hipStreamDestroy(st));
    auto same = [](const std::vector<float>& x, const std::vector<float>& y) { return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * 4) == 0); };
    const bool repeat_ok = same(outC[0], outC[1]) && same(outP[0], outP[1]) && same(outO[0], outO[1]);

    // ---- guards: outside the logical extent every output still holds its sentinel, bit for bit ----
    bool guard_ok = true;
    auto untouched = [&](const Buf& b, const std::vector<float>& o, bool all) {
        for (size_t i = 0; i < o.size(); ++i)
            if ((all || !b.used[i]) && f_bits(o[i]) != f_bits(b.h[i])) return false;
        return true;
    };
    guard_ok = guard_ok && untouched(C, outC[0], c.reject);
    guard_ok = guard_ok && untouched(Cpre, outP[0], c.reject || !c.cpre);
    if (c.ln) guard_ok = guard_ok && untouched(pout, outO[0], false);
    if (need) {
        for (size_t i = 0; i < outW[0].size(); ++i) {
            const bool inside = i >= kGuard && i < kGuard + need && !c.reject;
            if (!inside && f_bits(outW[0][i]) != kNanOut) guard_ok = false;
        }
    }

    // ---- reference: every element, in double ----
    Worst w;
    if (!c.reject) {
        const double kb = 2.0 * (K + 8) * kU;
        const std::vector<float>& gc = outC[0];
        const std::vector<float>& gp = outP[0];
        const size_t cbase = kGuard + (size_t)c.offc;
        std::vector<Worst> tw(16);
        for (int b = 0; b < nb; ++b) {
            const double* Ab = Ad.data() + (size_t)b * M * K;
            const double* Bb = Bd.data() + (size_t)(c.shared_b ? 0 : b) * N * K;
            parallel_rows(M, [&, b](int t, int m0, int m1) {
                Worst& ww = tw[t];
                for (int m = m0; m < m1; ++m)
                    for (int n = 0; n < N; ++n) {
                        const double* x = Ab + (size_t)m * K;
                        const double* y = Bb + (size_t)n * K;
                        double d0 = 0, d1 = 0, s0 = 0, s1 = 0;
                        int k = 0;
                        for (; k + 1 < K; k += 2) {
                            const double p0 = x[k] * y[k], p1 = x[k + 1] * y[k + 1];
                            d0 += p0; d1 += p1; s0 += std::fabs(p0); s1 += std::fabs(p1);
                        }
                        if (k < K) { const double p0 = x[k] * y[k]; d0 += p0; s0 += std::fabs(p0); }
                        const double dot = d0 + d1, S = s0 + s1;
                        const long long o = b * bsC + c_at(c, m, n);
                        const double bv = c.bias ? (double)bias.get(n) : 0.0;
                        double pre, epre;
                        if (c.ln) {
                            const double t2 = dot - rmean[m] * wsum64[n];
                            pre = rrstd[m] * t2 + bv;
                            epre = rrstd[m] * (kb * S + 8 * kU * std::fabs(rmean[m]) * std::fabs(wsum64[n])) + kRstdRel * std::fabs(rrstd[m] * t2) + kb * std::fabs(bv);
                        } else {
                            pre = dot + bv;
                            epre = kb * (S + std::fabs(bv));
                        }
                        if (c.cpre) {
                            const double g = gp[cbase + o];
                            ww.see(std::fabs(g - pre), epre);
                        }
                        const double av = act64(pre, c.act);
                        const double rv = has_r ? (c.ln ? x[n] : (double)R.get(o)) : 0.0;          // ln: R = A, same addressing as C
                        const double cold = c.acc ? (double)C.get(o) : 0.0;
                        const double an = c.ln && c.addn ? (double)addn.get(n) : 0.0;
                        const bool added = has_r || c.acc || an != 0.0;
                        double bound = act_lip(pre, epre, c.act) * epre + kb * (std::fabs(rv) + std::fabs(cold) + std::fabs(an));
                        if (c.act) bound += kActUlp * ulp32(av) + (added ? kb * std::fabs(av) : 0.0);
                        const double ref = av + rv + cold + an;
                        const double g = gc[cbase + o];
                        // The probe (W' = identity, an exact product) is a measurement: the bound's `8 u |mean| |wsum|` models the error of the
                        // reconstructed mean relative to |mean|, which holds beside a product bound over 512 terms but not beside none, so it is
                        // held to the bound where the measurement is taken, |x - mean| >= 1 (and must be finite everywhere).
                        const bool measured = !c.probe || std::fabs(x[n] - rmean[m]) >= 1.0;
                        if (measured) ww.see(std::fabs(g - ref), bound);
                        else if (!std::isfinite(g)) ++ww.nonfinite;
                        if (c.act && !added) {
                            if (g == g) ww.actulp = std::max(ww.actulp, std::fabs(g - av) / ulp32(av));
                            if (c.cpre) {
                                const double own = act64((double)gp[cbase + o], c.act);
                                if (g == g && own == own) ww.actulp_own = std::max(ww.actulp_own, std::fabs(g - own) / ulp32(own));
                            }
                        }
                        if (c.probe && std::fabs(x[n] - rmean[m]) >= 1.0) {
                            const double want = (x[n] - rmean[m]) * rrstd[m];
                            ww.rstd_rel = std::max(ww.rstd_rel, std::fabs(g / want - 1.0));
                        }
                    }
            });
        }
        for (auto& x : tw) w.merge(x);
        // part_out: the (mean, M2) of every 64-column group of the STORED rows -- what the next kernel's LayerNorm reads
        if (c.ln) {
            const std::vector<float>& po = outO[0];
            for (int m = 0; m < M; ++m)
                for (int gq = 0; gq < N / 64; ++gq) {
                    double s = 0, s2 = 0;
                    for (int j = 0; j < 64; ++j) { const double v = gc[cbase + c_at(c, m, 64 * gq + j)]; s += v; s2 += v * v; }
                    const double mean = s / 64;
                    double m2 = 0;
                    for (int j = 0; j < 64; ++j) { const double v = gc[cbase + c_at(c, m, 64 * gq + j)]; m2 += (v - mean) * (v - mean); }
                    const double gm = po[kGuard + ((size_t)m * (N / 64) + gq) * 2], gq2 = po[kGuard + ((size_t)m * (N / 64) + gq) * 2 + 1];
                    w.see(std::fabs(gm - mean), 64 * kU * (std::fabs(mean) + std::sqrt(s2 / 64)));
                    w.see(std::fabs(gq2 - m2), 64 * kU * m2);
                }
        }
    }

    // ---- schedule independence: the same rows inside a taller product, bit for bit ----
    std::string same_field;
    std::vector<float> logical;
    if (keep || !c.same_as.empty()) {
        logical.resize((size_t)M * N);
        for (int m = 0; m < M; ++m)
            for (int n = 0; n < N; ++n) logical[(size_t)m * N + n] = outC[0][kGuard + c.offc + c_at(c, m, n)];
    }
    if (!c.same_as.empty()) {
        const auto it = g_kept.find(c.same_as);
        const bool ok = it != g_kept.end() && it->second.size() >= (size_t)(c.row0 + M) * N &&
                        std::memcmp(it->second.data() + (size_t)c.row0 * N, logical.data(), logical.size() * 4) == 0;
        same_field = std::string(" same=") + (ok ? "ok" : "bad");
    }
    if (keep) g_kept[c.name] = std::move(logical);

    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("case=%s kind=%s ratio=%.4g nonfinite=%lld guard=%s repeat=%s", c.name.c_str(), ls::gemm_kind_name(plan.kind), w.ratio, w.nonfinite,
                guard_ok ? "ok" : "bad", repeat_ok ? "ok" : "bad");
    if (c.reject) std::printf(" rejected=%s", rejected ? "yes" : "no");
    if (plan.splits > 1 || c.splits > 1) std::printf(" splits=%d kchunk=%d", plan.splits, plan.kchunk);
    if (c.act && w.actulp > 0) std::printf(" actulp=%.3g", w.actulp);
    if (c.act && c.cpre && w.actulp_own > 0) std::printf(" actulp_own=%.3g", w.actulp_own);
    if (c.probe) std::printf(" rstd_rel=%.3g", w.rstd_rel);
    std::printf("%s ms=%.0f\n", same_field.c_str(), ms);
    std::fflush(stdout);
    for (Buf* b : {&A, &B, &bias, &R, &C, &Cpre, &ws, &lnp, &wsum, &addn, &pout}) b->release();
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: gemm_check <general | fulltile | dma | dma_ln | splitk>\n"); return 2; }
    const std::vector<Case> all = all_cases();
    int ran = 0;
    for (const Case& c : all) {
        if (c.group != argv[1]) continue;
        bool keep = false;
        for (const Case& o : all) keep = keep || o.same_as == c.name;
        if (!run_case(c, keep)) return 4;
        ++ran;
    }
    if (!ran) { std::fprintf(stderr, "no such group: %s\n", argv[1]); return 2; }
    return 0;
}
