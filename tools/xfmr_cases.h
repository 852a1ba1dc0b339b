// The cases of tools/xfmr_check.cpp: name, group and parameters.  tests/xfmr_cases.py lists the same names per group (both tests compare
// against it, so a case that vanishes from this table fails them).  Host-only.
#pragma once
#include <string>
#include <vector>

namespace xfmr_cases {

enum MaskKind { kMaskNull, kMaskOnes, kMaskOnly01, kMaskOne, kMaskTail, kMaskCleared };
enum RowKind { kRowNormal, kRowBigMean, kRowConst, kRowLowVar, kRowTimes1e4, kRowTimes1em4, kRowMixed };
enum ClipMode { kClipPlain, kClipTruncate, kClipKvAbove };

struct Case {
    std::string name, group;     // group: dec | enc | clip | ln | final | queries | prepare
    int B = 1;
    int n = 0;                   // dec: n_pre_c; queries: n_pre; ln: rows
    int JF = 0, KP = 0;
    int mask = kMaskNull, at = 0;        // at: the masked key (kMaskOne) or the first masked frame of sample 0 (kMaskTail)
    int kind = kRowNormal;       // ln: what the rows hold
    int bc_stride = 0;           // ln: 0 = no bc
    bool x2 = false, qc = false, big = false, probe = false;
    std::vector<int> lens;       // clip: the samples; sample data is keyed by its length, so "alone" and "in a batch" hold the same rows
    int mode = kClipPlain;
};

inline std::vector<Case> all_cases() {
    std::vector<Case> v;
    auto add = [&](const std::string& group, const std::string& name) -> Case& {
        v.emplace_back();
        v.back().group = group; v.back().name = name;
        return v.back();
    };
    // ---- decoder attention, S = 34, 4 heads of 128; compact cases are launched in both layouts
    add("dec", "dec_b1").B = 1;
    add("dec", "dec_b3").B = 3;
    { Case& c = add("dec", "dec_c4_b3"); c.B = 3; c.n = 4; }
    { Case& c = add("dec", "dec_c1_b3"); c.B = 3; c.n = 1; }
    { Case& c = add("dec", "dec_c4_b1"); c.B = 1; c.n = 4; }
    { Case& c = add("dec", "dec_big_b2"); c.B = 2; c.big = true; }
    // ---- encoder attention, S = 36, key mask; sample 0 carries the named mask, the others are all ones (ragged tails: every sample its own)
    { Case& c = add("enc", "enc_ones"); c.B = 2; c.mask = kMaskOnes; }
    { Case& c = add("enc", "enc_only01"); c.B = 2; c.mask = kMaskOnly01; }
    for (int k : {2, 15, 16, 17, 31, 32, 33, 35}) { Case& c = add("enc", "enc_m" + std::to_string(k)); c.B = 2; c.mask = kMaskOne; c.at = k; }
    { Case& c = add("enc", "enc_tail17"); c.B = 3; c.mask = kMaskTail; c.at = 17; }
    // ---- CLIP attention, 8 heads of 64, ragged packed rows with NaN rows between the samples
    for (int l : {1, 2, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 77, 80}) add("clip", "clip_l" + std::to_string(l)).lens = {l};
    add("clip", "clip_mix64").lens = {64, 1, 17, 33, 48};
    add("clip", "clip_mix80").lens = {80, 2, 65, 16, 49};
    { Case& c = add("clip", "clip_trunc80"); c.lens = {80}; c.mode = kClipTruncate; }
    { Case& c = add("clip", "clip_kv_above"); c.lens = {80}; c.mode = kClipKvAbove; }
    { Case& c = add("clip", "clip_big"); c.lens = {77, 33}; c.big = true; }
    { Case& c = add("clip", "clip_probe"); c.lens = {80, 49}; c.probe = true; }
    // ---- LayerNorm
    for (int r : {1, 3, 4, 5, 103}) add("ln", "ln_r" + std::to_string(r)).n = r;
    { Case& c = add("ln", "ln_bigmean_r5"); c.n = 5; c.kind = kRowBigMean; }
    { Case& c = add("ln", "ln_const_r5"); c.n = 5; c.kind = kRowConst; }
    { Case& c = add("ln", "ln_lowvar_r5"); c.n = 5; c.kind = kRowLowVar; }
    { Case& c = add("ln", "ln_times1e4_r5"); c.n = 5; c.kind = kRowTimes1e4; }
    { Case& c = add("ln", "ln_times1em4_r5"); c.n = 5; c.kind = kRowTimes1em4; }
    { Case& c = add("ln", "ln_mixed_r103"); c.n = 103; c.kind = kRowMixed; }
    { Case& c = add("ln", "ln_bc512_r103"); c.n = 103; c.bc_stride = 512; }
    { Case& c = add("ln", "ln_bc1536_r103"); c.n = 103; c.bc_stride = 1536; }
    { Case& c = add("ln", "ln_x2_bc512_r103"); c.n = 103; c.bc_stride = 512; c.x2 = true; }
    { Case& c = add("ln", "ln_x2_bc1536_r5"); c.n = 5; c.bc_stride = 1536; c.x2 = true; }
    { Case& c = add("ln", "ln_x2_bc512_r4"); c.n = 4; c.bc_stride = 512; c.x2 = true; }
    { Case& c = add("ln", "ln_x2_mixed_r103"); c.n = 103; c.bc_stride = 512; c.x2 = true; c.kind = kRowMixed; }
    // ---- k_sag_final
    for (int jf : {1, 16, 17, 27, 32, 33, 282})
        for (int b : {1, 3})
            for (int m : {(int)kMaskNull, (int)kMaskOnes, (int)kMaskCleared}) {
                Case& c = add("final", "fin_jf" + std::to_string(jf) + "_b" + std::to_string(b) + (m == kMaskNull ? "_null" : m == kMaskOnes ? "_ones" : "_clr"));
                c.JF = jf; c.B = b; c.mask = m;
            }
    // ---- k_sag_queries
    for (int np : {0, 4, 34})
        for (int b : {1, 3})
            for (int qc : {0, 1}) {
                Case& c = add("queries", "qry_n" + std::to_string(np) + "_b" + std::to_string(b) + (qc ? "_qc" : ""));
                c.JF = 27; c.B = b; c.n = np; c.qc = qc != 0;
            }
    { Case& c = add("queries", "qry_jf282_n4_b3_qc"); c.JF = 282; c.B = 3; c.n = 4; c.qc = true; }
    // ---- k_sag_enc_prepare
    for (int m : {(int)kMaskNull, (int)kMaskCleared}) {
        { Case& c = add("prepare", std::string("prep_jf27") + (m ? "_mask" : "_null")); c.JF = 27; c.KP = 32; c.B = 3; c.mask = m; }
        { Case& c = add("prepare", std::string("prep_jf282") + (m ? "_mask" : "_null")); c.JF = 282; c.KP = 288; c.B = 3; c.mask = m; }
    }
    return v;
}

}  // namespace xfmr_cases
