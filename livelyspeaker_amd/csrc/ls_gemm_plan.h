// The dispatch decision of launch_gemm_tr (ls_gemm.hip) as a host function: which kernel variant a product runs on, its grid and its
// split-K chunking.  launch_gemm_tr calls gemm_plan() and only launches; tests/test_gemm_plan_host.py and tools/gemm_check.cpp call it
// to pin the variant a shape reaches, so that a change of the heuristics cannot silently stop a variant from being tested.
#pragma once
#include "ls_internal.h"
#include "ls_train.h"

namespace ls {

constexpr int kGemmTileM = 128;     // output tile of k_gemm_tr: 128 x 128 (64 x 128 and 32 x 128 in the 64-row / LDS-DMA variants)
#ifndef LS_GEMM_HALF_MAX
#define LS_GEMM_HALF_MAX 768      // LDS-DMA grids of at most this many 64-row tiles run as 32-row half tiles (see gemm_plan)
#endif

enum GemmKind {
    kGemmGeneral = 0,         // k_gemm_tr<AK, BK, false>: bounds-checked staging, any strides
    kGemmFull128,             // k_gemm_tr<AK, BK, true>: full 128-row tiles, register-staged
    kGemmFull64,              // k_gemm_tr<true, true, true, 2>: the 64-row variant (`half`)
    kGemmDmaHalves,           // k_gemm_dma, every 64-row tile as two 32-row halves
    kGemmDmaWholeHalves,      // k_gemm_dma, nbig whole tiles + the last round as halves
    kGemmDmaWhole,            // k_gemm_dma, whole tiles only (1-D grid)
    kGemmDma3D,               // k_gemm_dma on the 3-D grid (batched / split-K)
};

inline const char* gemm_kind_name(GemmKind k) {
    switch (k) {
        case kGemmGeneral: return "general";
        case kGemmFull128: return "full128";
        case kGemmFull64: return "full64";
        case kGemmDmaHalves: return "dma_halves";
        case kGemmDmaWholeHalves: return "dma_whole_halves";
        case kGemmDmaWhole: return "dma_whole";
        case kGemmDma3D: return "dma_3d";
    }
    return "?";
}

struct GemmPlan {
    GemmKind kind;
    dim3 grid;                // the launch grid of the product kernel
    int gx, nbig;             // k_gemm_dma's arguments (tile columns of the 1-D schedule; whole tiles before the halves)
    int splits, kchunk;       // re-derived: every split starts on a K tile boundary
    int nbatch;               // at least 1
    bool fast;                // full tiles, whole K tiles, float4-legal operands, single-level reduction index
    bool ws_too_small;        // splits > 1 without a workspace of nbatch * splits * M * N floats  -> hipErrorInvalidValue
    bool split_epilogue;      // splits > 1 with Cpre, R or an activation                          -> hipErrorInvalidValue
    bool invalid() const { return ws_too_small || split_epilogue; }
};

inline GemmPlan gemm_plan(const GemmArgs& a, bool a_kcontig, bool b_kcontig, int splits) {
    constexpr int kTM = kGemmTileM, kTK = kGemmTileK;
    GemmPlan p{};
    if (splits < 1) splits = 1;
    // chunk is a multiple of the K tile so that every split starts on a tile boundary
    const int kchunk = ((a.K + splits - 1) / splits + kTK - 1) / kTK * kTK;
    splits = (a.K + kchunk - 1) / kchunk;
    p.kchunk = kchunk;
    p.splits = splits;
    p.nbatch = a.nbatch < 1 ? 1 : a.nbatch;
    p.ws_too_small = splits > 1 && (!a.ws || (size_t)p.nbatch * splits * a.M * a.N > a.ws_floats);
    p.split_epilogue = splits > 1 && (a.Cpre || a.R || a.act);
    dim3 grid((a.N + kTM - 1) / kTM, (a.M + kTM - 1) / kTM, p.nbatch * splits);
    // fast staging path: full tiles, whole K tiles in every split, float4-legal operands with a single-level reduction index
    const bool fast = a.M % kTM == 0 && a.N % kTM == 0 && a.K % kTK == 0 && a.A.vec && a.B.vec && a.A.ki == INT_MAX && a.B.ki == INT_MAX;
    p.fast = fast;
    // 64-row tiles when they balance the 256 CUs better: every CU works through ceil(workgroups / 256) tiles (co-resident ones share
    // its matrix pipes), so the efficiency of a grid is (workgroups / 256) / ceil(workgroups / 256) -- 544 tiles: 0.71, 1088 half tiles: 0.85
    auto balance = [](long long wgs) { const double per = (double)wgs / 256.0; return per / (double)((wgs + 255) / 256); };
    const long long t128 = (long long)grid.x * grid.y * grid.z;
    const bool half = fast && a_kcontig && b_kcontig && balance(2 * t128) > balance(t128) + 0.05;
    // LDS-DMA staging: single-level rows and every byte offset of an operand inside 31 bits (buffer addressing)
    const bool dma = fast && a_kcontig && b_kcontig && a.A.ri == INT_MAX && a.B.ri == INT_MAX &&
                     (long long)a.M * a.A.rs < (1ll << 29) && (long long)a.N * a.B.rs < (1ll << 29);
    if (dma) {
        // always 64-row tiles: 48 KB of double buffer lets three workgroups share a CU (the 128-row form: 64 KB, two); measured over the
        // sampler's shapes (tools/gemm_bench.cpp) the 128-row DMA tile lost to this one and, at some, to the register-staged kernel
        grid.y *= 2;
        if (grid.z == 1 && (long long)grid.x * grid.y <= LS_GEMM_HALF_MAX) {
            // a grid of at most one 64-row tile per slot: every tile as two 32-row halves -- twice the workgroups, half the MFMAs per wave and
            // K tile.  A lone workgroup's K tile costs 1.3 us (64 MFMAs per wave + issue + barrier), so what shortens a small product is
            // fewer MFMAs per wave, not a deeper prefetch (a three-buffer form with tiles k+1 and k+2 in flight measured SLOWER, 29.5 vs
            // 26.0 us at 384 x 512 x 512; removed).  Measured: 384 x 512 x 512 (a 4-clip batch's channel mixing) 26 -> 13 us, 4608 rows
            // 43 -> 32 us, 9728 rows 62 -> 55 us; above 768 tiles whole tiles win by 2-3 %.
            p.kind = kGemmDmaHalves;
            p.gx = (int)grid.x;
            p.nbig = 0;
            p.grid = dim3((unsigned)(2 * grid.x * grid.y));
        } else if (grid.z == 1) {
            // a last round that fills less than ~60 % of the 768 slots runs as half tiles (a half tile takes ~0.6 of a whole one)
            const long long tiles = (long long)grid.x * grid.y, slots = 768;
            const long long rem = tiles % slots;
            const int nbig = (rem > 0 && rem * 10 < slots * 6 && tiles > slots / 2) ? (int)(tiles - rem) : (int)tiles;
            p.kind = nbig < tiles ? kGemmDmaWholeHalves : kGemmDmaWhole;
            p.gx = (int)grid.x;
            p.nbig = nbig;
            p.grid = dim3((unsigned)(nbig + 2 * (tiles - nbig)));
        } else {
            p.kind = kGemmDma3D;
            p.gx = 0;
            p.nbig = 0;
            p.grid = grid;
        }
    } else if (half) {
        grid.y *= 2;
        p.kind = kGemmFull64;
        p.grid = grid;
    } else {
        p.kind = fast ? kGemmFull128 : kGemmGeneral;
        p.grid = grid;
    }
    return p;
}

}  // namespace ls
