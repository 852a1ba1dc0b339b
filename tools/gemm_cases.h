// The cases of tools/gemm_check.cpp (GPU: launch_gemm_tr against fp64 on every dispatch path) and of tests/gemm_plan_main.cpp
// (CPU: the plan each of them gets).  One list, so the plan test covers every shape the checker runs; the kind each case was written
// for is tests/gemm_cases.py.  Host-only: no pointer is dereferenced here.
#pragma once
#include <climits>
#include <string>
#include <vector>
#include "ls_internal.h"
#include "ls_train.h"

namespace gemm_cases {

// One operand: a stored row-major matrix [..][ld] read along its rows (kc, op_rows) or down its columns (op_cols).
struct Op {
    bool kc = true;
    int ld = 0;              // 0: tight (K for kc, the operand's rows otherwise)
    int off = 0;             // pointer offset in floats from a 256-byte aligned base
    int ri = 0, ro_mul = 0;  // kc only: two-level row index, ro = ro_mul * ld ("frames inside a token sequence")
    int ki = 0, ko_mul = 0;  // !kc only: two-level reduction index, ko = ko_mul * ld (the poseFinal weight gradient)
};

struct Case {
    std::string name, group;
    int M = 0, N = 0, K = 0;
    Op A, B;
    int ldc = 0, offc = 0;   // 0: tight (N, or M when transposed)
    bool ct = false;         // output transposed: crs = 1, cns = ldc
    int cri = 0, cro_mul = 0;        // two-level output rows, cro = cro_mul * ldc
    bool bias = false;
    int bias_off = 0;        // 1: misaligned bias (scalar epilogue)
    bool cpre = false, r = false, r_inplace = false, acc = false;
    int act = 0;
    int splits = 1, nbatch = 1;
    bool shared_b = false;   // bsB = 0
    int ws_short = 0;        // workspace this many floats too small: the call must be rejected
    bool reject = false;     // the call must return hipErrorInvalidValue before any launch
    bool ln = false;         // ln_part + wsum + part_out, R = A (as launch_step_long sets them)
    bool addn = false;
    bool probe = false;      // B = identity: C = (x - mean) rstd, the measurement of the reconstructed rstd
    int row0 = 0;            // the data of rows row0 .. row0 + M - 1 of a taller problem ...
    std::string same_as;     // ... whose output rows this case must reproduce bit for bit

    Case& lda(int v) { A.ld = v; return *this; }
    Case& ldb(int v) { B.ld = v; return *this; }
    Case& offa(int v) { A.off = v; return *this; }
    Case& offb(int v) { B.off = v; return *this; }
    Case& c_ld(int v) { ldc = v; return *this; }
    Case& c_off(int v) { offc = v; return *this; }
    Case& c_t() { ct = true; return *this; }
    Case& c_rows2(int i, int mul) { cri = i; cro_mul = mul; return *this; }
    Case& a_rows2(int i, int mul) { A.ri = i; A.ro_mul = mul; return *this; }
    Case& a_k2(int i, int mul) { A.ki = i; A.ko_mul = mul; return *this; }
    Case& b_k2(int i, int mul) { B.ki = i; B.ko_mul = mul; return *this; }
    Case& with_bias(int o = 0) { bias = true; bias_off = o; return *this; }
    Case& with_cpre() { cpre = true; return *this; }
    Case& with_r() { r = true; return *this; }
    Case& in_place() { r = true; r_inplace = true; return *this; }
    Case& with_acc() { acc = true; return *this; }
    Case& with_act(int v) { act = v; return *this; }
    Case& split(int v) { splits = v; return *this; }
    Case& batch(int v, bool shared = false) { nbatch = v; shared_b = shared; return *this; }
    Case& rejected(int ws_short_by = 0) { reject = true; ws_short = ws_short_by; return *this; }
    Case& with_ln(bool add) { ln = true; addn = add; return *this; }
    Case& rows_of(const std::string& parent, int r0) { same_as = parent; row0 = r0; return *this; }
};

inline Case mk(const std::string& group, const std::string& name, int M, int N, int K, bool ak, bool bk) {
    Case c;
    c.group = group; c.name = name; c.M = M; c.N = N; c.K = K; c.A.kc = ak; c.B.kc = bk;
    return c;
}

inline int op_ld(const Op& o, int rows, int K) { return o.ld ? o.ld : (o.kc ? K : rows); }

// strides of an operand, written out; gemm_operand() decides whether float4 loads are legal, as for every caller of the kernel
inline ls::GemmOperand op_make(const Op& o, const float* p, int rows, int K) {
    const long long ld = op_ld(o, rows, K);
    const long long rs = o.kc ? ld : 1, ks = o.kc ? 1 : ld;
    return ls::gemm_operand(p, o.ri ? o.ri : INT_MAX, o.ri ? o.ro_mul * ld : 0, rs, o.ki ? o.ki : INT_MAX, o.ki ? o.ko_mul * ld : 0, ks, o.kc, rows, K);
}

// offset of element (r, k) -- plain arithmetic, independent of the kernel's lvl()
inline long long op_at(const ls::GemmOperand& o, int r, int k) {
    const long long r1 = o.ri == INT_MAX ? 0 : r / o.ri, r2 = o.ri == INT_MAX ? r : r % o.ri;
    const long long k1 = o.ki == INT_MAX ? 0 : k / o.ki, k2 = o.ki == INT_MAX ? k : k % o.ki;
    return r1 * o.ro + r2 * o.rs + k1 * o.ko + k2 * o.ks;
}
inline long long op_extent(const Op& o, int rows, int K) { return op_at(op_make(o, nullptr, rows, K), rows - 1, K - 1) + 1; }

inline int c_ldc(const Case& c) { return c.ldc ? c.ldc : (c.ct ? c.M : c.N); }
inline long long c_at(const Case& c, int m, int n) {
    const long long ld = c_ldc(c), crs = c.ct ? 1 : ld, cns = c.ct ? ld : 1;
    const long long m1 = c.cri ? m / c.cri : 0, m2 = c.cri ? m % c.cri : m;
    return m1 * c.cro_mul * ld + m2 * crs + (long long)n * cns;
}
inline long long c_extent(const Case& c) { return c_at(c, c.M - 1, c.N - 1) + 1; }

// stride between the problems of a batch: the extent, a gap that nobody may touch, rounded so that alignment is kept
inline long long batch_stride(long long extent) { return (extent + 4 + 3) / 4 * 4; }

inline size_t ws_need(const Case& c, int plan_splits) { return plan_splits > 1 ? (size_t)c.nbatch * plan_splits * c.M * c.N : 0; }

struct Ptrs {
    const float* A; const float* B; float* C; float* Cpre; const float* R; const float* bias;
    float* ws; size_t ws_floats;
    const float* ln_part; const float* wsum; const float* addn; float* part_out;
};

// pointers are the logical bases (the case's offsets already applied)
inline ls::GemmArgs make_args(const Case& c, const Ptrs& p) {
    ls::GemmArgs a{};
    a.A = op_make(c.A, p.A, c.M, c.K);
    a.B = op_make(c.B, p.B, c.N, c.K);
    const long long ld = c_ldc(c);
    a.C = p.C;
    a.cri = c.cri ? c.cri : INT_MAX; a.cro = c.cri ? c.cro_mul * ld : 0; a.crs = c.ct ? 1 : ld; a.cns = c.ct ? ld : 1;
    a.bias = c.bias ? p.bias : nullptr;
    a.Cpre = c.cpre ? p.Cpre : nullptr;
    a.R = c.r ? (c.r_inplace ? p.C : p.R) : nullptr;
    a.act = c.act; a.accumulate = c.acc ? 1 : 0;
    a.M = c.M; a.N = c.N; a.K = c.K;
    a.ws = p.ws; a.ws_floats = p.ws_floats;
    a.nbatch = c.nbatch;
    a.bsA = c.nbatch > 1 ? batch_stride(op_extent(c.A, c.M, c.K)) : 0;
    a.bsB = c.nbatch > 1 && !c.shared_b ? batch_stride(op_extent(c.B, c.N, c.K)) : 0;
    a.bsC = c.nbatch > 1 ? batch_stride(c_extent(c)) : 0;
    if (c.ln) {
        if (!c.probe) a.R = p.A;                     // the residual is the product's own input rows
        a.ln_part = p.ln_part; a.wsum = p.wsum; a.part_out = p.part_out;
        a.addn = c.addn ? p.addn : nullptr;
    }
    return a;
}

inline std::vector<Case> all_cases() {
    std::vector<Case> v;
    auto lay = [](bool ak, bool bk) { return std::string(ak ? "r" : "c") + (bk ? "r" : "c"); };     // r: op_rows, c: op_cols
    auto up4 = [](int x) { return (x + 3) / 4 * 4; };
    auto odd4 = [](int x) { return (x + 1) % 4 ? x + 1 : x + 2; };                                  // > x, never a multiple of 4

    // ---- general: bounds-checked staging, every layout, alignment and epilogue ----
    const int shapes[5][3] = {{131, 67, 45}, {129, 129, 33}, {1, 1, 1}, {3, 512, 512}, {200, 130, 7}};
    for (const auto& s : shapes)
        for (int ak = 1; ak >= 0; --ak)
            for (int bk = 1; bk >= 0; --bk) {
                const int M = s[0], N = s[1], K = s[2];
                const std::string base = "g_" + std::to_string(M) + "x" + std::to_string(N) + "x" + std::to_string(K) + "_" + lay(ak, bk);
                const int ea = ak ? K : M, eb = bk ? K : N;            // extent along the contiguous index
                v.push_back(mk("general", base + "_vec", M, N, K, ak, bk).lda(up4(ea)).ldb(up4(eb)).with_bias());
                v.push_back(mk("general", base + "_ld", M, N, K, ak, bk).lda(odd4(ea)).ldb(odd4(eb)).with_bias());
                v.push_back(mk("general", base + "_off", M, N, K, ak, bk).lda(up4(ea)).ldb(up4(eb)).offa(1).offb(1).with_bias());
            }
    // float4 output rows with a scalar tail (N % 4 = 3 and 1, ldc a multiple of 4)
    v.push_back(mk("general", "g_cvec_tail3", 131, 67, 45, true, true).c_ld(68).with_bias());
    v.push_back(mk("general", "g_cvec_tail1", 129, 129, 33, true, false).c_ld(132).with_bias());
    v.push_back(mk("general", "g_c_off1", 131, 67, 45, true, true).c_ld(68).c_off(1).with_bias());
    // two-level indices
    v.push_back(mk("general", "g_a_rows2", 131, 67, 45, true, true).a_rows2(34, 37).with_bias());
    v.push_back(mk("general", "g_a_rows2_vec", 131, 68, 48, true, false).a_rows2(34, 37).with_bias());
    v.push_back(mk("general", "g_b_k2", 131, 67, 45, false, false).lda(512).ldb(512).b_k2(34, 37));
    v.push_back(mk("general", "g_ab_k2", 131, 67, 45, false, false).lda(512).ldb(512).a_k2(34, 37).b_k2(34, 37).with_acc());
    v.push_back(mk("general", "g_a_k2", 200, 130, 70, false, true).lda(512).a_k2(34, 37).with_bias());
    v.push_back(mk("general", "g_c_rows2", 131, 67, 45, true, true).c_rows2(34, 37).with_bias());
    v.push_back(mk("general", "g_c_rows2_vec", 131, 68, 45, true, true).c_rows2(34, 37).with_bias().with_r());
    v.push_back(mk("general", "g_c_t", 131, 67, 45, true, true).c_t().with_bias());
    v.push_back(mk("general", "g_c_t_ld", 129, 129, 33, false, true).c_t().c_ld(140).with_bias().with_r().with_act(1));
    // epilogues, on the scalar (ldc = 67) and the float4 (ldc = 68) store path
    for (int ld : {67, 68}) {
        const std::string e = "g_ep" + std::to_string(ld) + "_";
        auto base = [&](const std::string& n) { return mk("general", e + n, 131, 67, 45, true, true).c_ld(ld); };
        v.push_back(base("none"));
        v.push_back(base("bias").with_bias());
        v.push_back(base("cpre").with_cpre());
        v.push_back(base("r").with_r());
        v.push_back(base("acc").with_acc());
        v.push_back(base("inplace").in_place());
        v.push_back(base("all").with_bias().with_cpre().with_r().with_acc().with_act(1));
        for (int act = 1; act <= 4; ++act) v.push_back(base("act" + std::to_string(act)).with_bias().with_cpre().with_act(act));
    }
    // the activations alone at K = 32: the measurement of their ulp error
    for (int act = 1; act <= 4; ++act) v.push_back(mk("general", "g_k32_act" + std::to_string(act), 131, 67, 32, true, true).with_bias().with_cpre().with_act(act));

    // ---- fulltile: the register-staged full-tile kernel ----
    for (int l = 0; l < 3; ++l) {
        const bool ak = l == 0, bk = l == 1;                            // (r, c), (c, r), (c, c)
        v.push_back(mk("fulltile", "f_256x128x64_" + lay(ak, bk), 256, 128, 64, ak, bk).with_bias().with_cpre().with_act(1 + l));
        v.push_back(mk("fulltile", "f_128x256x96_" + lay(ak, bk), 128, 256, 96, ak, bk).with_bias().with_r().with_acc());
    }
    v.push_back(mk("fulltile", "f_plain", 256, 128, 64, true, false));
    v.push_back(mk("fulltile", "f_inplace", 128, 256, 96, false, true).with_bias().in_place().with_act(4));
    v.push_back(mk("fulltile", "f_bias_off", 256, 128, 64, true, false).with_bias(1).with_cpre().with_r().with_act(1));
    v.push_back(mk("fulltile", "f_c_t", 256, 128, 64, false, false).c_t().with_bias().with_act(3));
    v.push_back(mk("fulltile", "f_64row", 640, 512, 64, true, true).a_rows2(32, 35).with_bias().with_cpre().with_r().with_act(1));
    v.push_back(mk("fulltile", "f_64row_acc", 640, 512, 64, true, true).a_rows2(32, 35).with_acc());
    v.push_back(mk("fulltile", "f_64row_bias_off", 640, 512, 64, true, true).a_rows2(32, 35).with_bias(1).with_act(3));

    // ---- dma: the LDS-DMA kernel and its three schedules ----
    // The kernel needs whole 128-row tiles (the long path pads its row count to one, ls_long.hip: mrows), so 64, 14400 and 20288 rows
    // stay on the general kernel; they run on it here, and the DMA schedules run at the same row counts padded to 128.
    {
        auto d = [&](const std::string& n) { return mk("dma", "d_128_" + n, 128, 128, 32, true, true); };
        v.push_back(d("none"));
        v.push_back(d("bias").with_bias());
        v.push_back(d("cpre").with_cpre());
        v.push_back(d("r").with_r());
        v.push_back(d("inplace").in_place());
        v.push_back(d("acc").with_acc());
        v.push_back(d("bias_off").with_bias(1).with_cpre().with_r().with_act(1));
        v.push_back(d("all").with_bias().with_cpre().with_r().with_acc().with_act(1));
        for (int act = 1; act <= 4; ++act) v.push_back(d("act" + std::to_string(act)).with_bias().with_cpre().with_act(act));
    }
    v.push_back(mk("dma", "d_64x128x32", 64, 128, 32, true, true).with_bias().with_r().with_act(1));
    v.push_back(mk("dma", "d_384x512x512", 384, 512, 512, true, true).with_bias().in_place().with_act(1));
    v.push_back(mk("dma", "d_384_lda", 384, 512, 512, true, true).lda(516).ldb(520).c_ld(524).with_bias().with_acc());
    v.push_back(mk("dma", "d_14400", 14400, 512, 32, true, true).with_bias().with_r().with_act(1));
    v.push_back(mk("dma", "d_14464", 14464, 512, 32, true, true).with_bias().with_r().with_act(1));     // 904 tiles: 768 whole + 272 halves
    // schedule independence: rows 12288 .. 12351 run as half tiles there, rows 0 .. 63 as a whole tile; alone they run on the general
    // kernel (64 rows) or as the halves of a two-tile grid (128 rows)
    v.push_back(mk("dma", "d_rows12288_64", 64, 512, 32, true, true).with_bias().with_r().with_act(1).rows_of("d_14464", 12288));
    v.push_back(mk("dma", "d_rows12288_128", 128, 512, 32, true, true).with_bias().with_r().with_act(1).rows_of("d_14464", 12288));
    v.push_back(mk("dma", "d_rows0_64", 64, 512, 32, true, true).with_bias().with_r().with_act(1).rows_of("d_14464", 0));
    v.push_back(mk("dma", "d_rows0_128", 128, 512, 32, true, true).with_bias().with_r().with_act(1).rows_of("d_14464", 0));
    v.push_back(mk("dma", "d_20288", 20288, 512, 32, true, true).with_bias());
    v.push_back(mk("dma", "d_20352", 20352, 512, 32, true, true).with_bias());                           // 1272 tiles: the last round is 504, whole
    v.push_back(mk("dma", "d_batch3", 128, 128, 64, true, true).batch(3).with_bias().with_cpre().with_r().with_act(1));
    v.push_back(mk("dma", "d_batch3_acc", 128, 128, 64, true, true).batch(3, true).with_acc());
    v.push_back(mk("dma", "d_split2", 128, 128, 128, true, true).split(2).with_bias());

    // ---- dma_ln: the long path's fused LayerNorm around the product (14464 = 14400 rows padded as launch_step_long pads them) ----
    v.push_back(mk("dma_ln", "ln_rstd_probe", 256, 512, 512, true, true).with_ln(false));
    v.back().probe = true;
    v.push_back(mk("dma_ln", "ln_256", 256, 512, 512, true, true).with_bias().with_act(1).with_ln(true));
    v.push_back(mk("dma_ln", "ln_256_last", 256, 512, 512, true, true).with_bias().with_act(1).with_ln(false));
    v.push_back(mk("dma_ln", "ln_14464", 14464, 512, 512, true, true).with_bias().with_act(1).with_ln(true));

    // ---- splitk: partial tiles in a workspace, summed in a fixed order ----
    v.push_back(mk("splitk", "s_131x67x200_rr", 131, 67, 200, true, true).split(3).with_bias());
    v.push_back(mk("splitk", "s_131x67x200_cc", 131, 67, 200, false, false).split(3).with_bias().with_acc());
    v.push_back(mk("splitk", "s_131x67x200_rc", 131, 67, 200, true, false).split(3).with_acc());
    v.push_back(mk("splitk", "s_131x67x200_cr", 131, 67, 200, false, true).split(3));
    v.push_back(mk("splitk", "s_128_dma", 128, 128, 256, true, true).split(4).with_bias().with_acc());
    v.push_back(mk("splitk", "s_128_full_rc", 128, 128, 256, true, false).split(4).with_bias());
    v.push_back(mk("splitk", "s_128_full_cc", 128, 128, 256, false, false).split(4).with_acc());
    v.push_back(mk("splitk", "s_128_full_t", 128, 128, 256, false, true).split(4).c_t().with_bias());
    v.push_back(mk("splitk", "s_512x37x300", 512, 37, 300, true, true).split(2).with_bias());
    v.push_back(mk("splitk", "s_512x37x300_cc", 512, 37, 300, false, false).split(2).with_acc());
    v.push_back(mk("splitk", "s_req5_k96", 131, 67, 96, true, true).split(5).with_bias());
    // the long path's token mixing: batched, shared B, A read down its columns, output transposed
    v.push_back(mk("splitk", "s_tokmix", 512, 37, 37, false, true).lda(512).batch(4, true).c_t().c_ld(512).with_bias().in_place().with_act(1));
    v.push_back(mk("splitk", "s_tokmix_split", 512, 37, 37, false, true).lda(512).batch(4, true).c_t().c_ld(512).split(2).with_bias().with_acc());
    // batched weight gradient: both operands read down their columns, the reduction over 256 rows
    v.push_back(mk("splitk", "s_wgrad_batch", 67, 45, 256, false, false).batch(3).split(2).with_acc());
    // the two rejected calls
    v.push_back(mk("splitk", "s_reject_act", 131, 67, 200, true, true).split(3).with_act(1).rejected());
    v.push_back(mk("splitk", "s_reject_cpre", 131, 67, 200, true, true).split(3).with_cpre().rejected());
    v.push_back(mk("splitk", "s_reject_r", 131, 67, 200, true, true).split(3).with_r().rejected());
    v.push_back(mk("splitk", "s_reject_ws", 131, 67, 200, true, true).split(3).with_bias().rejected(1));
    return v;
}

}  // namespace gemm_cases
