// Stand-alone check of the transformer towers' non-GEMM kernels (ls_sag.hip, ls_sag_enc.hip, ls_clip_text.hip) against fp64 --
// tests/test_gpu_xfmr.py and tests/test_xfmr_ref_host.py build and run it:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fno-slp-vectorize -I include -I livelyspeaker_amd/csrc -I tools tools/xfmr_check.cpp
//         livelyspeaker_amd/csrc/ls_sag.hip livelyspeaker_amd/csrc/ls_sag_enc.hip livelyspeaker_amd/csrc/ls_clip_text.hip -o xfmr_check
//   xfmr_check <dec | enc | clip | ln | final | queries | prepare>
//       every case of the group (tools/xfmr_cases.h) on the GPU through the launch_* functions of ls_internal.h: operands embedded in NaN
//       guards, outputs pre-filled with a NaN sentinel, two launches, EVERY logical output element against the double-precision
//       reference under the derived bound of tools/xfmr_ref.h.  One line per case:
//           case=<name> ratio=<worst err / bound> nonfinite=<n> guard=<ok|bad> repeat=<ok|bad> [same=<ok|bad>] ...
//       The program stops with a non-zero exit at the first HIP error and launches nothing after it.
//   xfmr_check --host <group> <dir>
//       no HIP call: writes every case's inputs and fp64 references as raw little-endian files <dir>/<case>.<tensor>.<f32|f64|u8|i32>,
//       prints their shapes (`host case=... `) and, for every known-wrong reference that applies to the case, how far it lies from the
//       true one in units of the bound (`sens case=... pert=... ratio=...`).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>
#include "ls_internal.h"
#include "xfmr_cases.h"
#include "xfmr_ref.h"

using namespace xfmr;
using namespace xfmr_cases;

constexpr size_t kGuard = 256;                // elements before and after every buffer (keeps the 256-byte alignment of the base)
constexpr uint32_t kNanIn = 0x7fc00000u;      // quiet NaN around the inputs
constexpr uint32_t kNanOut = 0x7fc0beefu;     // sentinel in the outputs
constexpr int kT = ls::kT, kS = ls::kSagEncS, kD = ls::kD;

#define HIP_OK(x)                                                                                            \
    do {                                                                                                     \
        hipError_t e_ = (x);                                                                                 \
        if (e_ != hipSuccess) {                                                                              \
            std::printf("HIP error %s at %s:%d (%s)\n", hipGetErrorString(e_), __FILE__, __LINE__, #x);     \
            std::fflush(stdout);                                                                             \
            std::exit(3);                                                                                    \
        }                                                                                                    \
    } while (0)

static bool g_host = false;
static std::string g_dir;
static hipStream_t g_st = nullptr;

static float bits_f(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t f_bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
enum { tQKV = 1, tAlt, tX, tW, tBeta, tBc, tW2, tBeta2, tBias, tPe, tMu, tSigma };

// a host buffer [guard | body | guard] with a mask of the body's logical elements, and its device twin (allocated on first use)
template <class T>
struct BufT {
    std::vector<T> h;
    std::vector<uint8_t> used;
    T* d = nullptr;
    void init(size_t body, T fill) { h.assign(kGuard + body + kGuard, fill); used.assign(h.size(), 0); }
    T& at(size_t i) { used[kGuard + i] = 1; return h[kGuard + i]; }
    T get(size_t i) const { return h[kGuard + i]; }
    T* base() {
        if (!d) HIP_OK(hipMalloc(&d, h.size() * sizeof(T)));
        return d + kGuard;
    }
    void up() { base(); HIP_OK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
    std::vector<T> down() {
        std::vector<T> o(h.size());
        HIP_OK(hipMemcpy(o.data(), d, o.size() * sizeof(T), hipMemcpyDeviceToHost));
        return o;
    }
    std::vector<T> logical() const {                      // the logical elements in buffer order
        std::vector<T> o;
        for (size_t i = 0; i < h.size(); ++i) if (used[i]) o.push_back(h[i]);
        return o;
    }
    ~BufT() { if (d) (void)hipFree(d); }
};
using Buf = BufT<float>;
using Bytes = BufT<unsigned char>;
static void init_in(Buf& b, size_t body) { b.init(body, bits_f(kNanIn)); }
static void init_out(Buf& b, size_t body) { b.init(body, bits_f(kNanOut)); }

struct IntBuf {                                           // row0 / len of the CLIP launch
    int* d = nullptr;
    void set(const std::vector<int>& v) {
        if (!d) HIP_OK(hipMalloc(&d, 64 * sizeof(int)));
        HIP_OK(hipMemcpy(d, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    ~IntBuf() { if (d) (void)hipFree(d); }
};

struct Verdict {
    double ratio = 0;
    long long nonfinite = 0;
    bool guard = true, repeat = true;
    std::string extra;                                    // further " key=value" fields
    void see(double got, double ref, double bound) {
        const double err = std::fabs(got - ref);
        if (!std::isfinite(got)) { ++nonfinite; return; }
        const double r = bound > 0 ? err / bound : (err > 0 ? 1e30 : 0.0);
        if (r > ratio) ratio = r;
    }
    void field(const std::string& k, const std::string& v) { extra += " " + k + "=" + v; }
    void field(const std::string& k, double v) { char s[64]; std::snprintf(s, sizeof s, "%.4g", v); field(k, std::string(s)); }
    void ok(const std::string& k, bool v) { field(k, v ? "ok" : "bad"); }
};

template <class T>
static bool same_bits(const std::vector<T>& x, const std::vector<T>& y) {
    return x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(T)) == 0);
}
// outside the logical extent an output still holds what it was filled with, bit for bit
template <class T>
static bool untouched(const BufT<T>& b, const std::vector<T>& o) {
    for (size_t i = 0; i < o.size(); ++i)
        if (!b.used[i] && std::memcmp(&o[i], &b.h[i], sizeof(T)) != 0) return false;
    return true;
}
// refill the output with its sentinel, launch, wait, read back; twice; keeps the first result
template <class T, class F>
static std::vector<T> run2(BufT<T>& out, Verdict& v, F launch) {
    std::vector<T> o[2];
    for (int rep = 0; rep < 2; ++rep) {
        out.up();
        HIP_OK(launch());
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(g_st));
        o[rep] = out.down();
    }
    v.repeat = v.repeat && same_bits(o[0], o[1]);
    v.guard = v.guard && untouched(out, o[0]);
    return o[0];
}
template <class T, class F>
static std::vector<T> run1(BufT<T>& out, F launch) {
    out.up();
    HIP_OK(launch());
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g_st));
    return out.down();
}
// every logical element (buffer order) against ref / bound (logical order)
static void compare(const Buf& b, const std::vector<float>& got, const std::vector<double>& ref, const std::vector<double>& bound, Verdict& v) {
    size_t n = 0;
    for (size_t i = 0; i < got.size(); ++i)
        if (b.used[i]) { v.see(got[i], ref[n], bound[n]); ++n; }
    if (n != ref.size()) v.ratio = 1e30;
}

static void dump(const std::string& cs, const std::string& name, const void* p, size_t bytes) {
    const std::string path = g_dir + "/" + cs + "." + name;
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, 1, bytes, f) != bytes) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(5); }
    std::fclose(f);
}
template <class T>
static void dump(const std::string& cs, const std::string& name, const std::vector<T>& v) { dump(cs, name, v.data(), v.size() * sizeof(T)); }
static void sens(const Case& c, const char* pert, double r) { std::printf("sens case=%s pert=%s ratio=%.4g\n", c.name.c_str(), pert, r); }
static void report(const Case& c, const Verdict& v, double ms) {
    std::printf("case=%s ratio=%.4g nonfinite=%lld guard=%s repeat=%s%s ms=%.0f\n", c.name.c_str(), v.ratio, v.nonfinite, v.guard ? "ok" : "bad",
                v.repeat ? "ok" : "bad", v.extra.c_str(), ms);
    std::fflush(stdout);
}

// ================================================================ attention
// the sensitivity of the attention bound: every wrong form that applies to the case
static void attn_sens(const Case& c, const AttnData& t, const std::vector<double>& ref, const std::vector<double>& bound, bool scale, bool drops, bool shift,
                      bool causal) {
    std::vector<double> w;
    auto one = [&](const char* name, const AttnVar& var) { attn_ref(t, var, w, nullptr); sens(c, name, sensitivity(w, ref, bound)); };
    AttnVar v;
    if (scale) { v = AttnVar(); v.scale_mode = 1; one("q_unscaled", v); v.scale_mode = 2; one("scale_1_hd", v); }
    if (drops) { v = AttnVar(); v.drop = kDropLast; one("drop_last", v); v.drop = kDropLeast; one("drop_least", v); }
    if (shift) { v = AttnVar(); v.mask_shift = 1; one("mask_shift", v); }
    if (causal) { v = AttnVar(); v.causal_off = -1; one("causal_excl", v); v.causal_off = 1; one("causal_incl", v); }
    v = AttnVar(); v.v_head = 1; one("v_next_head", v);
}
static void to_double(const Buf& b, std::vector<double>& d) {
    const std::vector<float> l = b.logical();
    d.assign(l.begin(), l.end());
}

// ---- decoder: k_sag_attention<128, 34, false>, dense and compact
static void run_dec(const Case& c) {
    const int B = c.B, npc = c.n, D = kD, W = 3 * D, heads = 4;
    auto val = [&](int b, int t, int col) {       // the compact layout's shared rows hold the same values for every sample
        const float v = normal(tQKV, (uint32_t)((npc > 0 && t >= npc ? 1000 : b) * 128 + t), (uint32_t)col);
        return c.big && col < 2 * D ? 5.0f * v : v;   // q, k ~ N(0, 25): scores scale q.k ~ N(0, 25^2), the largest of 34 x 34 x 4 about 80
    };
    Buf dense, compact, out, outc;
    init_in(dense, (size_t)B * kT * W);
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < kT; ++t)
            for (int col = 0; col < W; ++col) dense.at(((size_t)b * kT + t) * W + col) = val(b, t, col);
    const int crows = B * npc + (kT - npc);
    if (npc > 0) {
        init_in(compact, (size_t)crows * W);
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < kT; ++t)
                for (int col = 0; col < W; ++col) compact.at((size_t)(t < npc ? b * npc + t : B * npc + (t - npc)) * W + col) = val(b, t, col);
    }
    AttnData t;
    t.B = B; t.heads = heads; t.HD = 128;
    for (int b = 0; b < B; ++b) { t.len.push_back(kT); t.row0.push_back(b * kT); }
    to_double(dense, t.qkv);
    std::vector<double> ref, bound;
    attn_ref(t, AttnVar(), ref, &bound);
    if (g_host) {
        std::printf("host case=%s group=dec B=%d S=%d heads=%d D=%d\n", c.name.c_str(), B, kT, heads, D);
        dump(c.name, "qkv.f32", dense.logical());
        dump(c.name, "ref.f64", ref);
        attn_sens(c, t, ref, bound, true, !c.big, false, false);
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    Verdict v;
    init_out(out, (size_t)B * kT * D);
    for (size_t i = 0; i < (size_t)B * kT * D; ++i) out.at(i) = bits_f(kNanOut);
    dense.up();
    const std::vector<float> got = run2(out, v, [&] { return ls::launch_sag_attention(dense.base(), out.base(), B, heads, D, 0, g_st); });
    compare(out, got, ref, bound, v);
    if (npc > 0) {                                // the compact launch: within the bound on its own, and the dense launch's bits
        outc.h = out.h; outc.used = out.used;
        compact.up();
        const std::vector<float> gc = run2(outc, v, [&] { return ls::launch_sag_attention(compact.base(), outc.base(), B, heads, D, npc, g_st); });
        compare(outc, gc, ref, bound, v);
        v.ok("same", same_bits(gc, got));
    }
    report(c, v, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// ---- encoder: k_sag_attention<128, 36, true> and k_sag_enc_attention_row0<128>
static void run_enc(const Case& c) {
    const int B = c.B, D = kD, W = 3 * D, heads = 4;
    Bytes mask;
    mask.init((size_t)B * kS, 0xff);
    static const int tails[3] = {17, 5, 33};
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < kS; ++j) {
            bool valid = true;
            if (c.mask == kMaskTail) valid = j < 2 + (b == 0 ? c.at : tails[b % 3]);
            else if (b == 0 && c.mask == kMaskOnly01) valid = j < 2;
            else if (b == 0 && c.mask == kMaskOne) valid = j != c.at;
            mask.at((size_t)b * kS + j) = valid ? (unsigned char)(1 + j % 2) : 0;       // any non-zero byte is a valid key
        }
    // masked keys hold +-7 in K and V (finite, of moderate size: what the reference model's padded frames can produce); `alt` rewrites them
    Buf qkv, alt, q0, kv, out, out0;
    init_in(qkv, (size_t)B * kS * W); init_in(alt, (size_t)B * kS * W);
    init_in(q0, (size_t)B * D); init_in(kv, (size_t)B * kS * 2 * D);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < kS; ++j)
            for (int col = 0; col < W; ++col) {
                const bool masked = mask.get((size_t)b * kS + j) == 0 && col >= D;
                const float v = masked ? 7.0f * sign_of(tQKV, (uint32_t)(b * 128 + j), (uint32_t)col) : normal(tQKV, (uint32_t)(b * 128 + j), (uint32_t)col);
                qkv.at(((size_t)b * kS + j) * W + col) = v;
                alt.at(((size_t)b * kS + j) * W + col) = masked ? 3.0f * normal(tAlt, (uint32_t)(b * 128 + j), (uint32_t)col) : v;
                if (col >= D) kv.at(((size_t)b * kS + j) * 2 * D + col - D) = v;
                else if (j == 0) q0.at((size_t)b * D + col) = v;
            }
    AttnData t;
    t.B = B; t.heads = heads; t.HD = 128;
    for (int b = 0; b < B; ++b) { t.len.push_back(kS); t.row0.push_back(b * kS); }
    to_double(qkv, t.qkv);
    for (unsigned char m : mask.logical()) t.mask.push_back(m != 0);
    std::vector<double> ref, bound, ref0, bound0;
    attn_ref(t, AttnVar(), ref, &bound);
    AttnVar r0; r0.only_row0 = true;
    attn_ref(t, r0, ref0, &bound0);
    if (g_host) {
        std::printf("host case=%s group=enc B=%d S=%d heads=%d D=%d\n", c.name.c_str(), B, kS, heads, D);
        dump(c.name, "qkv.f32", qkv.logical());
        dump(c.name, "mask.u8", mask.logical());
        dump(c.name, "ref.f64", ref);
        dump(c.name, "ref0.f64", ref0);
        attn_sens(c, t, ref, bound, true, true, c.mask != kMaskOnes, false);
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    Verdict v;
    init_out(out, (size_t)B * kS * D);
    for (size_t i = 0; i < (size_t)B * kS * D; ++i) out.at(i) = bits_f(kNanOut);
    init_out(out0, (size_t)B * D);
    for (size_t i = 0; i < (size_t)B * D; ++i) out0.at(i) = bits_f(kNanOut);
    qkv.up(); alt.up(); mask.up(); q0.up(); kv.up();
    const std::vector<float> got = run2(out, v, [&] { return ls::launch_sag_enc_attention(qkv.base(), mask.base(), out.base(), B, heads, D, g_st); });
    compare(out, got, ref, bound, v);
    const std::vector<float> ga = run1(out, [&] { return ls::launch_sag_enc_attention(alt.base(), mask.base(), out.base(), B, heads, D, g_st); });
    v.ok("same", same_bits(ga, got));             // what a masked key holds cannot reach the output
    Verdict v0;
    const std::vector<float> g0 = run2(out0, v0, [&] { return ls::launch_sag_enc_attention_row0(q0.base(), kv.base(), mask.base(), out0.base(), B, heads, D, g_st); });
    compare(out0, g0, ref0, bound0, v0);
    v.guard = v.guard && v0.guard; v.repeat = v.repeat && v0.repeat; v.nonfinite += v0.nonfinite;
    Verdict vx;                                   // the one-query kernel against row 0 of the full kernel: within the sum of the two bounds
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < D; ++d)
            vx.see(g0[kGuard + (size_t)b * D + d], got[kGuard + (size_t)b * kS * D + d], bound0[(size_t)b * D + d] + bound[(size_t)b * kS * D + d]);
    v.field("ratio0", v0.ratio);
    v.field("ratiox", vx.ratio);
    report(c, v, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// ---- CLIP: k_clip_attention<64>
static std::map<int, std::vector<float>> g_alone;         // the output rows [len][512] of the sample of every length, run alone
static void run_clip(const Case& c) {
    const int B = (int)c.lens.size(), D = kD, W = 3 * D, heads = 8, gap = 3;
    // sample data is keyed by the sample's length and the token; three NaN rows lie before every sample and behind the last
    auto val = [&](uint32_t tensor, int key, int tkn, int col) -> float {
        if (c.probe) {                            // exact scores: q, k in {-1, 0, 1} (a quarter non-zero), scale 1/8; v in [0.5, 1.5)
            if (col >= 2 * D) return 1.0f + unif(tensor, (uint32_t)(key * 128 + tkn), (uint32_t)col);
            const uint32_t h = hash3(tensor, (uint32_t)(key * 128 + tkn), (uint32_t)col);
            return (h & 3u) ? 0.0f : ((h & 4u) ? 1.0f : -1.0f);
        }
        const float v = normal(tensor, (uint32_t)(key * 128 + tkn), (uint32_t)col);
        return c.big && col < 2 * D ? 5.0f * v : v;
    };
    std::vector<int> row0(B), prow0(B), len = c.lens;
    int rows = gap, prows = 0, max_len = 0;
    for (int b = 0; b < B; ++b) { row0[b] = rows; prow0[b] = prows; rows += len[b] + gap; prows += len[b]; max_len = std::max(max_len, len[b]); }
    Buf qkv, out;
    init_in(qkv, (size_t)rows * W);
    for (int b = 0; b < B; ++b)
        for (int tk = 0; tk < len[b]; ++tk)
            for (int col = 0; col < W; ++col) qkv.at((size_t)(row0[b] + tk) * W + col) = val(tQKV, len[b], tk, col);
    AttnData t;
    t.B = B; t.heads = heads; t.HD = 64; t.causal = true;
    t.len = len; t.row0 = prow0;
    to_double(qkv, t.qkv);
    std::vector<double> ref, bound;
    attn_ref(t, AttnVar(), ref, &bound);
    if (g_host) {
        std::printf("host case=%s group=clip B=%d heads=%d D=%d lens=", c.name.c_str(), B, heads, D);
        for (int b = 0; b < B; ++b) std::printf("%s%d", b ? "," : "", len[b]);
        std::printf("\n");
        dump(c.name, "qkv.f32", qkv.logical());
        dump(c.name, "ref.f64", ref);
        const bool plain = !c.big && !c.probe, multi = max_len >= 2;
        attn_sens(c, t, ref, bound, plain ? multi : c.big, plain && multi, false, plain && multi);
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    Verdict v;
    init_out(out, (size_t)rows * D);
    for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < (size_t)len[b] * D; ++i) out.at((size_t)row0[b] * D + i) = bits_f(kNanOut);
    IntBuf drow0, dlen;
    drow0.set(row0); dlen.set(len);
    qkv.up();
    const std::vector<float> got = run2(out, v, [&] { return ls::launch_clip_attention(qkv.base(), out.base(), drow0.d, dlen.d, B, heads, D, max_len, g_st); });
    compare(out, got, ref, bound, v);
    if (c.probe) {                                // the measurement behind kCexp: distance in ulp of the result, scores being exact
        double worst = 0;
        size_t n = 0;
        for (size_t i = 0; i < got.size(); ++i)
            if (out.used[i]) { worst = std::max(worst, std::fabs(got[i] - ref[n]) / ulp32(ref[n])); ++n; }
        v.field("expulp", worst);
    }
    auto rows_of = [&](const std::vector<float>& o, int b, int nrows) {
        return std::vector<float>(o.begin() + kGuard + (size_t)row0[b] * D, o.begin() + kGuard + (size_t)(row0[b] + nrows) * D);
    };
    if (c.mode == kClipPlain && !c.big && !c.probe) {
        if (B == 1) g_alone[len[0]] = rows_of(got, 0, len[0]);
        else {                                    // every sample of the batch against the same sample run alone, at another row0
            bool same = true;
            for (int b = 0; b < B; ++b) same = same && g_alone.count(len[b]) && same_bits(g_alone[len[b]], rows_of(got, b, len[b]));
            v.ok("same", same);
        }
    }
    if (c.mode == kClipTruncate) {                // the same rows with len = L: rows below L keep their bits, rows from L on are not written
        bool same = true;
        for (int L : {1, 17, 64}) {
            dlen.set({L});
            const std::vector<float> g = run1(out, [&] { return ls::launch_clip_attention(qkv.base(), out.base(), drow0.d, dlen.d, 1, heads, D, L, g_st); });
            same = same && same_bits(rows_of(g, 0, L), rows_of(got, 0, L));
            for (size_t i = kGuard + (size_t)(row0[0] + L) * D; i < g.size(); ++i) v.guard = v.guard && f_bits(g[i]) == kNanOut;
            for (size_t i = 0; i < kGuard + (size_t)row0[0] * D; ++i) v.guard = v.guard && f_bits(g[i]) == kNanOut;
        }
        v.ok("same", same);
    }
    if (c.mode == kClipKvAbove) {                 // K and V of the rows above a rewritten: row a keeps its bits
        bool same = true;
        const std::vector<float> keep = qkv.h;
        for (int a : {0, 15, 16, 40, 63}) {
            qkv.h = keep;
            for (int tk = a + 1; tk < len[0]; ++tk)
                for (int col = D; col < W; ++col) qkv.h[kGuard + (size_t)(row0[0] + tk) * W + col] = 2.0f * val(tAlt, len[0], tk, col);
            qkv.up();
            const std::vector<float> g = run1(out, [&] { return ls::launch_clip_attention(qkv.base(), out.base(), drow0.d, dlen.d, 1, heads, D, max_len, g_st); });
            const std::vector<float> x = rows_of(g, 0, a + 1), y = rows_of(got, 0, a + 1);
            same = same && std::memcmp(x.data() + (size_t)a * D, y.data() + (size_t)a * D, D * sizeof(float)) == 0;
        }
        v.ok("same", same);
    }
    report(c, v, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// ================================================================ LayerNorm: k_layernorm512, k_layernorm512x2
static float ln_value(int kind, int r, int i) {
    const float n = normal(tX, (uint32_t)r, (uint32_t)i);
    switch (kind == kRowMixed ? r % 6 : kind) {
        case kRowBigMean: return 1000.0f + 0.01f * n;     // the mean dwarfs the variance
        case kRowConst: return 0.5f * (float)(r % 7 + 1); // variance 0
        case kRowLowVar: return 0.01f * n;                // variance 1e-4: eps = 1e-5 is a tenth of it
        case kRowTimes1e4: return 1e4f * n;
        case kRowTimes1em4: return 1e-4f * n;
        default: return n;
    }
}
static void run_ln(const Case& c) {
    const int rows = c.n, nb = (rows + kT - 1) / kT, ld = c.bc_stride;
    Buf x, bc, w1, b1, w2, b2, y, y1, y2;
    init_in(x, (size_t)rows * kD);
    for (int r = 0; r < rows; ++r)
        for (int i = 0; i < kD; ++i) x.at((size_t)r * kD + i) = ln_value(c.kind, r, i);
    for (Buf* b : {&w1, &b1, &w2, &b2}) init_in(*b, kD);
    for (int i = 0; i < kD; ++i) {
        w1.at(i) = 1.0f + 0.5f * unif(tW, 0, (uint32_t)i);  b1.at(i) = unif(tBeta, 0, (uint32_t)i);
        w2.at(i) = 1.0f + 0.5f * unif(tW2, 0, (uint32_t)i); b2.at(i) = unif(tBeta2, 0, (uint32_t)i);
    }
    std::vector<double> bcd;                      // [nb][512] dense
    if (ld) {
        init_in(bc, (size_t)(nb - 1) * ld + kD);  // vectors ld floats apart, NaN between them
        for (int s = 0; s < nb; ++s)
            for (int i = 0; i < kD; ++i) { bc.at((size_t)s * ld + i) = 0.5f * normal(tBc, (uint32_t)s, (uint32_t)i); bcd.push_back(bc.get((size_t)s * ld + i)); }
    }
    std::vector<double> xd, ref((size_t)rows * kD), bound(ref.size()), mid, midb;
    to_double(x, xd);
    const std::vector<float> fw1 = w1.logical(), fb1 = b1.logical(), fw2 = w2.logical(), fb2 = b2.logical();
    auto reference = [&](const LnVar& var, std::vector<double>& out, double* bnd) {
        out.resize((size_t)rows * kD);
        if (!c.x2) { ln_ref(xd.data(), nullptr, ld ? bcd.data() : nullptr, kD, fw1.data(), fb1.data(), rows, var, out.data(), bnd); return; }
        mid.resize(out.size()); midb.resize(out.size());
        ln_ref(xd.data(), nullptr, nullptr, 0, fw1.data(), fb1.data(), rows, var, mid.data(), midb.data());
        ln_ref(mid.data(), midb.data(), bcd.data(), kD, fw2.data(), fb2.data(), rows, var, out.data(), bnd);
    };
    reference(LnVar(), ref, bound.data());
    if (g_host) {
        std::printf("host case=%s group=ln rows=%d bc=%d x2=%d\n", c.name.c_str(), rows, ld ? nb : 0, c.x2 ? 1 : 0);
        dump(c.name, "x.f32", x.logical());
        dump(c.name, "w1.f32", fw1); dump(c.name, "b1.f32", fb1);
        dump(c.name, "w2.f32", fw2); dump(c.name, "b2.f32", fb2);
        if (ld) dump(c.name, "bc.f32", bc.logical());
        dump(c.name, "ref.f64", ref);
        std::vector<double> wr;
        LnVar var;
        const bool varied = c.kind == kRowNormal || c.kind == kRowLowVar || c.kind == kRowTimes1e4 || c.kind == kRowMixed;
        if (varied) { var = LnVar(); var.unbiased = true; reference(var, wr, nullptr); sens(c, "unbiased_var", sensitivity(wr, ref, bound)); }
        if (c.kind == kRowLowVar) {
            var = LnVar(); var.eps = 1e-6; reference(var, wr, nullptr); sens(c, "eps_1e-6", sensitivity(wr, ref, bound));
            var.eps = 0; reference(var, wr, nullptr); sens(c, "eps_omitted", sensitivity(wr, ref, bound));
        }
        if (ld && rows > 36) { var = LnVar(); var.bc_div = 36; reference(var, wr, nullptr); sens(c, "bc_div_36", sensitivity(wr, ref, bound)); }
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    Verdict v;
    for (Buf* b : {&y, &y1, &y2}) {
        init_out(*b, (size_t)rows * kD);
        for (size_t i = 0; i < (size_t)rows * kD; ++i) b->at(i) = bits_f(kNanOut);
    }
    x.up(); w1.up(); b1.up(); w2.up(); b2.up();
    if (ld) bc.up();
    std::vector<float> got;
    if (!c.x2) {
        got = run2(y, v, [&] { return ls::launch_layernorm512(x.base(), ld ? bc.base() : nullptr, ld, w1.base(), b1.base(), y.base(), rows, g_st); });
    } else {
        got = run2(y, v, [&] { return ls::launch_layernorm512x2(x.base(), w1.base(), b1.base(), bc.base(), ld, w2.base(), b2.base(), y.base(), rows, g_st); });
        // the kernel's claim: the same arithmetic, in the same order, as two k_layernorm512 launches
        (void)run2(y1, v, [&] { return ls::launch_layernorm512(x.base(), nullptr, 0, w1.base(), b1.base(), y1.base(), rows, g_st); });
        const std::vector<float> two = run2(y2, v, [&] { return ls::launch_layernorm512(y1.base(), bc.base(), ld, w2.base(), b2.base(), y2.base(), rows, g_st); });
        v.ok("same", same_bits(two, got));
    }
    compare(y, got, ref, bound, v);
    report(c, v, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// ================================================================ k_sag_final
// frames 0, 15, 16 and 33 cleared, rotated by the sample index; a valid frame holds 1 or 2 (any non-zero byte is valid)
static unsigned char frame_mask(int kind, int b, int f) {
    if (kind == kMaskCleared)
        for (int z : {0, 15, 16, 33}) if (f == (z + b) % kT) return 0;
    return (unsigned char)(1 + f % 2);
}
static void run_final(const Case& c) {
    const int B = c.B, JF = c.JF;
    Buf xh, wf, bf, out;
    Bytes mask;
    init_in(xh, (size_t)B * kT * kD); init_in(wf, (size_t)JF * kD); init_in(bf, (size_t)JF);
    mask.init((size_t)B * kT, 0xff);
    for (size_t i = 0; i < (size_t)B * kT; ++i)
        for (int d = 0; d < kD; ++d) xh.at(i * kD + d) = normal(tX, (uint32_t)i, (uint32_t)d);
    for (int j = 0; j < JF; ++j) {
        for (int d = 0; d < kD; ++d) wf.at((size_t)j * kD + d) = unif(tW, (uint32_t)j, (uint32_t)d);
        bf.at(j) = sign_of(tBias, 1, (uint32_t)j) * (0.5f + 0.5f * unif(tBias, 0, (uint32_t)j));          // |bias| in [0.25, 0.75)
    }
    for (int b = 0; b < B; ++b)
        for (int f = 0; f < kT; ++f) mask.at((size_t)b * kT + f) = frame_mask(c.mask, b, f);
    const std::vector<float> fx = xh.logical(), fw = wf.logical(), fb = bf.logical();
    const std::vector<unsigned char> fm = mask.logical();
    const unsigned char* pm = c.mask == kMaskNull ? nullptr : fm.data();
    std::vector<double> ref, bound, wr;
    final_ref(fx.data(), fw.data(), fb.data(), pm, B, JF, kT, kD, FinalVar(), ref, &bound);
    if (g_host) {
        std::printf("host case=%s group=final B=%d JF=%d mask=%d\n", c.name.c_str(), B, JF, pm ? 1 : 0);
        dump(c.name, "xh.f32", fx); dump(c.name, "wf.f32", fw); dump(c.name, "bf.f32", fb);
        if (pm) dump(c.name, "mask.u8", fm);
        dump(c.name, "ref.f64", ref);
        FinalVar var;
        var.no_bias = true;
        final_ref(fx.data(), fw.data(), fb.data(), pm, B, JF, kT, kD, var, wr, nullptr);
        sens(c, "no_bias", sensitivity(wr, ref, bound));
        if (c.mask == kMaskCleared) {
            var = FinalVar(); var.mask_shift = 1;
            final_ref(fx.data(), fw.data(), fb.data(), pm, B, JF, kT, kD, var, wr, nullptr);
            sens(c, "mask_shift", sensitivity(wr, ref, bound));
        }
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    Verdict v;
    init_out(out, (size_t)B * JF * kT);
    for (size_t i = 0; i < (size_t)B * JF * kT; ++i) out.at(i) = bits_f(kNanOut);
    xh.up(); wf.up(); bf.up(); mask.up();
    const std::vector<float> got = run2(out, v, [&] { return ls::launch_sag_final(xh.base(), wf.base(), bf.base(), pm ? mask.base() : nullptr, out.base(), B, JF, kD, g_st); });
    compare(out, got, ref, bound, v);
    if (pm) {                                     // a masked output is exactly +0
        bool zero = true;
        for (int b = 0; b < B; ++b)
            for (int j = 0; j < JF; ++j)
                for (int f = 0; f < kT; ++f)
                    if (fm[b * kT + f] == 0) zero = zero && f_bits(got[kGuard + ((size_t)b * JF + j) * kT + f]) == 0u;
        v.ok("zero", zero);
    }
    report(c, v, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// ================================================================ k_sag_queries
static void run_queries(const Case& c) {
    const int B = c.B, JF = c.JF, np = c.n;
    Buf x, wmap, bmap, pe, q, qc;
    init_in(x, (size_t)B * JF * kT); init_in(wmap, (size_t)kD * (JF + 1)); init_in(bmap, kD); init_in(pe, (size_t)kT * kD);
    for (size_t i = 0; i < (size_t)B * JF; ++i)
        for (int f = 0; f < kT; ++f) x.at(i * kT + f) = normal(tX, (uint32_t)i, (uint32_t)f);
    for (int d = 0; d < kD; ++d) {
        for (int j = 0; j < JF; ++j) wmap.at((size_t)d * (JF + 1) + j) = unif(tW, (uint32_t)d, (uint32_t)j);
        wmap.at((size_t)d * (JF + 1) + JF) = sign_of(tW2, 1, (uint32_t)d) * (0.5f + 0.5f * unif(tW2, 0, (uint32_t)d));      // the bit's column
        bmap.at(d) = unif(tBias, 0, (uint32_t)d);
    }
    std::vector<float> fpe((size_t)(kT + 1) * kD);                // one row more than the device gets: the wrong form reads pe[f + 1]
    for (int f = 0; f <= kT; ++f)
        for (int d = 0; d < kD; ++d) {
            fpe[(size_t)f * kD + d] = normal(tPe, (uint32_t)f, (uint32_t)d);
            if (f < kT) pe.at((size_t)f * kD + d) = fpe[(size_t)f * kD + d];
        }
    const std::vector<float> fx = x.logical(), fw = wmap.logical(), fb = bmap.logical();
    std::vector<double> ref, bound, wr;
    queries_ref(fx.data(), fw.data(), fb.data(), fpe.data(), B, JF, kT, kD, np, QueriesVar(), ref, &bound);
    if (g_host) {
        std::printf("host case=%s group=queries B=%d JF=%d n_pre=%d\n", c.name.c_str(), B, JF, np);
        dump(c.name, "x.f32", fx); dump(c.name, "wmap.f32", fw); dump(c.name, "bmap.f32", fb); dump(c.name, "pe.f32", pe.logical());
        dump(c.name, "ref.f64", ref);
        QueriesVar var;
        if (np > 0) {
            var.no_bit = true;
            queries_ref(fx.data(), fw.data(), fb.data(), fpe.data(), B, JF, kT, kD, np, var, wr, nullptr);
            sens(c, "no_bit", sensitivity(wr, ref, bound));
        }
        var = QueriesVar(); var.pe_shift = 1;
        queries_ref(fx.data(), fw.data(), fb.data(), fpe.data(), B, JF, kT, kD, np, var, wr, nullptr);
        sens(c, "pe_next_row", sensitivity(wr, ref, bound));
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    Verdict v;
    const size_t crows = (size_t)B * np + (kT - np);
    init_out(q, (size_t)B * kT * kD);
    for (size_t i = 0; i < (size_t)B * kT * kD; ++i) q.at(i) = bits_f(kNanOut);
    init_out(qc, crows * kD);
    if (c.qc) for (size_t i = 0; i < crows * kD; ++i) qc.at(i) = bits_f(kNanOut);
    x.up(); wmap.up(); bmap.up(); pe.up(); qc.up();
    const std::vector<float> got = run2(q, v, [&] { return ls::launch_sag_queries(x.base(), wmap.base(), bmap.base(), pe.base(), q.base(), c.qc ? qc.base() : nullptr, B, JF, np, kD, g_st); });
    compare(q, got, ref, bound, v);
    const std::vector<float> gc = qc.down();
    v.guard = v.guard && untouched(qc, gc);       // with qc null nothing of it is logical: all of it must be untouched
    if (c.qc) {                                   // prefix rows per sample, then the shared rows once; each the bits of the q row it copies
        bool same = true;
        for (int b = 0; b < B; ++b)
            for (int f = 0; f < kT; ++f) {
                if (f >= np && b != 0) continue;
                const size_t cr = f < np ? (size_t)b * np + f : (size_t)B * np + (f - np);
                same = same && std::memcmp(&gc[kGuard + cr * kD], &got[kGuard + ((size_t)b * kT + f) * kD], kD * sizeof(float)) == 0;
            }
        v.ok("same", same);
    }
    report(c, v, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// ================================================================ k_sag_enc_prepare: copies and single fp32 additions, compared exactly
static void run_prepare(const Case& c) {
    const int B = c.B, JF = c.JF, KP = c.KP;
    Buf x, mu, sigma, pe, tok, xt;
    Bytes mask, kmask;
    init_in(x, (size_t)B * JF * kT); init_in(mu, kD); init_in(sigma, kD); init_in(pe, (size_t)kS * kD);
    mask.init((size_t)B * kT, 0xff);
    for (size_t i = 0; i < (size_t)B * JF; ++i)
        for (int f = 0; f < kT; ++f) x.at(i * kT + f) = normal(tX, (uint32_t)i, (uint32_t)f);
    for (int d = 0; d < kD; ++d) { mu.at(d) = normal(tMu, 0, (uint32_t)d); sigma.at(d) = normal(tSigma, 0, (uint32_t)d); }
    for (int s = 0; s < kS; ++s)
        for (int d = 0; d < kD; ++d) pe.at((size_t)s * kD + d) = normal(tPe, (uint32_t)s, (uint32_t)d);
    for (int b = 0; b < B; ++b)
        for (int f = 0; f < kT; ++f) mask.at((size_t)b * kT + f) = frame_mask(c.mask, b, f);
    const bool masked = c.mask != kMaskNull;
    // the fp32 statement of the same copies and single additions
    std::vector<float> rtok((size_t)B * kS * kD), rxt((size_t)B * kT * KP, 0.0f);
    std::vector<unsigned char> rk((size_t)B * kS);
    for (int b = 0; b < B; ++b) {
        for (int s = 0; s < kS; ++s)
            for (int d = 0; d < kD; ++d) {
                float t = pe.get((size_t)s * kD + d);
                if (s == 0) t = t + mu.get(d);
                if (s == 1) t = t + sigma.get(d);
                rtok[((size_t)b * kS + s) * kD + d] = t;
            }
        for (int f = 0; f < kT; ++f)
            for (int j = 0; j < JF; ++j) rxt[((size_t)b * kT + f) * KP + j] = x.get(((size_t)b * JF + j) * kT + f);
        for (int s = 0; s < kS; ++s) rk[(size_t)b * kS + s] = s < 2 ? 1 : (masked ? mask.get((size_t)b * kT + s - 2) != 0 : 1);
    }
    if (g_host) {
        std::printf("host case=%s group=prepare B=%d JF=%d KP=%d mask=%d\n", c.name.c_str(), B, JF, KP, masked ? 1 : 0);
        dump(c.name, "x.f32", x.logical()); dump(c.name, "mu.f32", mu.logical()); dump(c.name, "sigma.f32", sigma.logical());
        dump(c.name, "pe.f32", pe.logical());
        if (masked) dump(c.name, "mask.u8", mask.logical());
        dump(c.name, "tok.f32", rtok); dump(c.name, "xt.f32", rxt); dump(c.name, "kmask.u8", rk);
        return;
    }
    const auto t0 = std::chrono::steady_clock::now();
    Verdict v;
    init_out(tok, rtok.size()); init_out(xt, rxt.size());
    for (size_t i = 0; i < rtok.size(); ++i) tok.at(i) = bits_f(kNanOut);
    for (size_t i = 0; i < rxt.size(); ++i) xt.at(i) = bits_f(kNanOut);
    kmask.init(rk.size(), 0xa5);
    for (size_t i = 0; i < rk.size(); ++i) kmask.at(i) = 0xa5;
    x.up(); mu.up(); sigma.up(); pe.up(); mask.up();
    std::vector<float> gtok[2], gxt[2];
    std::vector<unsigned char> gk[2];
    for (int rep = 0; rep < 2; ++rep) {
        tok.up(); xt.up(); kmask.up();
        HIP_OK(ls::launch_sag_enc_prepare(x.base(), masked ? mask.base() : nullptr, mu.base(), sigma.base(), pe.base(), tok.base(), xt.base(), kmask.base(),
                                          B, JF, KP, g_st));
        HIP_OK(hipGetLastError());
        HIP_OK(hipStreamSynchronize(g_st));
        gtok[rep] = tok.down(); gxt[rep] = xt.down(); gk[rep] = kmask.down();
    }
    v.repeat = same_bits(gtok[0], gtok[1]) && same_bits(gxt[0], gxt[1]) && same_bits(gk[0], gk[1]);
    v.guard = untouched(tok, gtok[0]) && untouched(xt, gxt[0]) && untouched(kmask, gk[0]);
    bool exact = std::memcmp(&gk[0][kGuard], rk.data(), rk.size()) == 0;
    for (size_t i = 0; i < rtok.size(); ++i) { v.see(gtok[0][kGuard + i], rtok[i], 0.0); exact = exact && f_bits(gtok[0][kGuard + i]) == f_bits(rtok[i]); }
    for (size_t i = 0; i < rxt.size(); ++i) { v.see(gxt[0][kGuard + i], rxt[i], 0.0); exact = exact && f_bits(gxt[0][kGuard + i]) == f_bits(rxt[i]); }
    v.ok("same", exact);                          // bit for bit, the zero padding of xt as +0
    report(c, v, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

int main(int argc, char** argv) {
    g_host = argc == 4 && std::string(argv[1]) == "--host";
    if (!g_host && argc != 2) {
        std::fprintf(stderr, "usage: xfmr_check <dec | enc | clip | ln | final | queries | prepare>\n       xfmr_check --host <group> <dir>\n");
        return 2;
    }
    const std::string group = g_host ? argv[2] : argv[1];
    if (g_host) g_dir = argv[3];
    else HIP_OK(hipStreamCreate(&g_st));
    const std::map<std::string, void (*)(const Case&)> run = {{"dec", run_dec}, {"enc", run_enc}, {"clip", run_clip}, {"ln", run_ln},
                                                              {"final", run_final}, {"queries", run_queries}, {"prepare", run_prepare}};
    if (!run.count(group)) { std::fprintf(stderr, "no such group: %s\n", group.c_str()); return 2; }
    for (const Case& c : all_cases())
        if (c.group == group) run.at(group)(c);
    if (!g_host) HIP_OK(hipStreamDestroy(g_st));
    return 0;
}
