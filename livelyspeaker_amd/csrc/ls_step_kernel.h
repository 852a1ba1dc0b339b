// Fused diffusion-step kernel for gfx950 (MI355X): ONE launch = one p_sample / ddim_sample step of the
// CFG-wrapped RAG denoiser for the whole batch.  Replaces, per step, the ~230 eager aten ops of
//   ClassifierFreeSampleModel.forward   scripts/model/cfg_sampler.py:24-31
//   RAG.forward                         scripts/model/RAG.py:98-133
//   TransMLP / MLPblock / LN_spatial    scripts/model/mlp_module.py:21-91
//   OutputProcess                       scripts/model/RAG.py:205-211
//   p_mean_variance / p_sample / ddim_sample   scripts/diffusion/gaussian_diffusion.py:284-399, 507-558, 745-798
//
// Mapping:
//   * one workgroup (8 waves, 512 threads) owns ONE sample: the cond and uncond passes are packed as
//     R = 2*S rows (70 TED / 72 BEAT) -> 5 token tiles of 16, so the CFG lerp and the sampler update fuse
//     into the same launch and nothing but x_t (3.7 KB) round-trips through HBM between steps.
//   * every contraction runs on v_mfma_f32_16x16x4_f32 (exact fp32; bf16/fp16 inputs fail the 1e-3
//     parity budget) -- except the channel mixing of PREC 2, the fp32 default, which runs on
//     v_mfma_f32_16x16x32_bf16 with both operands split exactly into three bf16 parts -- in the TRANSPOSED form D[channel][token]: channels on the
//     MFMA M axis, tokens on N.  The MFMA C/D layout (lane&15 = token, 4*(lane>>4)+reg = channel) is then
//     ALSO the layout of the residual stream, which therefore lives in registers for the whole forward:
//     wave w owns channels [64w, 64w+64) of all 80 rows = 80 VGPRs.
//   * the normalised operand (LN1(x) for token mixing, LN2(x) for channel mixing) is staged in LDS as
//     U[row][k] with row stride 520 floats: lane (token, g) fetches k = 16q+4g..+3 with one conflict-free
//     ds_read_b128 and feeds 4 consecutive MFMAs; the weight operand uses the same k permutation and is
//     pre-swizzled on the host so each wave-instruction reads 1 KiB contiguous from L2.
//     PREC 2 stages LN2(x) differently: the wave that owns a channel splits it into its three bf16 parts ONCE while writing it, and
//     the parts lie in LDS as three planes [48][520] of bf16 -- one 48-row chunk (token tiles 0-2, then tiles 3-4) at a time, because
//     the planes of all R rows would not fit.  The consumers read ready bf16 fragments (ds_read_b128 at row * 520 + 8g + 32q, the
//     PREC 1 address) and do no conversion work; each wave streams its weight slice once per chunk, i.e. twice per layer.
//   * token mixing (Conv1d(S,S,1) over the token axis) is a second small MFMA GEMM against a
//     block-diagonal [R x R] operand; its output lands directly in the residual layout.
#pragma once
#include "ls_step_common.h"
#include "ls_lanes.h"

namespace ls {

// PAIR = 1: single-pass sampling for guidance scale 1 (out_u + 1 * (out_c - out_u) = out_c, cfg_sampler.py:31, and the callers
// run guidance_param = 1: test_RAG_ted.py:183): the 2S rows hold the COND pass of TWO samples (2b, 2b+1) instead of the cond and
// uncond passes of one -- the same block-diagonal token mixing, half the work per sample.
// The training forward's activation stores (1.17 GB per launch at B = 512, read back only by the backward) are non-temporal: 2.06 -> 2.00 ms
// of forward at B = 512 (round 5; with no stores at all, LS_TRAIN_ABL: 1.91).  The same on the backward's dA stores changed nothing.
#define LS_TRAIN_ST(p, v) __builtin_nontemporal_store((v), (p))
#ifndef LS_TRAIN_ABL
#define LS_TRAIN_ABL 0          // timing-only A/B (tools): 1 = the training forward keeps no activations (its stores are skipped)
#endif
template <int S, int NPRE, int JF, int PREC, int TRAIN = 0, int PAIR = 0>
__global__ __launch_bounds__(512) void k_step(const StepArgs a) {
    static_assert(!TRAIN || PREC == 0, "the training forward is fp32");
    static_assert(!(TRAIN && PAIR), "PAIR is a sampling variant");
    constexpr int R = 2 * S;                 // packed rows: [cond tokens | uncond tokens]  (PAIR: [sample 2b | sample 2b+1])
    constexpr int KXQ = (JF + 15) / 16;      // 16-wide k groups of the x_t part of input_mapping
    constexpr int KXP = KXQ * 16;
    constexpr int NOB = (JF + 15) / 16;      // 16-wide output blocks of poseFinal
    constexpr int OSTR = NOB * 16 + 4;
    constexpr int MK = (R + 3) / 4;          // k steps of the token-mix GEMM
    constexpr int NU = NOB * kNT;            // output-projection work units
    constexpr int MAXU = (NU + kWaves - 1) / kWaves;
    constexpr int kFullTiles = 4;            // token tiles whose 16 rows are all real
    constexpr int NREM = R - 16 * kFullTiles;  // rows of the ragged last tile (6 TED / 8 BEAT)
    // Ragged rows: scalar FMAs (TED, 6 rows) or v_mfma_f32_4x4x1_16b row groups (BEAT, 8 rows = 2 full groups).
    // Measured on MI355X: the 4x4x1 MFMA issues in 16 cycles = 16 MAC/cycle, the same rate as a wave64 v_fma_f32,
    // so it only pays when no group is padded (BEAT 0.898 -> 0.867 ms/step: fewer LDS reads; TED 1.494 -> 1.518).
    constexpr bool kRemMfma = (NREM % 4 == 0);
    constexpr int NRG = kRemMfma ? NREM / 4 : 1;   // 4-row groups (MFMA path)
    constexpr int NRV = kRemMfma ? 1 : NREM;       // rows (VALU path)
    constexpr int NG = (R + 7) / 8;            // 8-row groups of the transposed bf16 operand of token mixing
    constexpr int KS = (R + 31) / 32;          // k steps (32 source rows) of the bf16 token-mix MFMA
    // bf16x3 token mixing: the operand stays ROW-major (the two [R][520] bf16 planes the channel mixing uses, 8-byte stores) and the MFMA
    // A fragment -- 8 consecutive source rows of one channel per lane -- is gathered by gfx950's transposing LDS read
    // (ds_read_b64_tr_b16: lane i of a 16-lane group supplies row k0 + i / 4, columns 4 (i % 4) .. + 3, and receives column i of rows
    // k0 .. k0 + 3); 0: the operand is written transposed with 160 ds_write_b16 per wave and layer (rounds 1-3).
#ifndef LS_TOK_TR
#define LS_TOK_TR 1
#endif
    constexpr bool kTokTr = LS_TOK_TR != 0;
    // Split-fp32 channel mixing (PREC 2): 1 = the LayerNorm-2 operand is split into its three bf16 parts once, by the wave that owns the
    // channel, and staged as three bf16 planes per 48-row chunk; 0 = it is staged as fp32 and every wave splits every fragment it reads
    // (the earlier form, kept for same-tree A/B: tools/ab_variants.py build old=LS_SPLIT_SHARED=0 new=).  Both give the same bits.
#ifndef LS_SPLIT_SHARED
#define LS_SPLIT_SHARED 1
#endif
    constexpr bool kSplitShared = PREC == 2 && LS_SPLIT_SHARED != 0;
    // Weight stream of that channel mixing: how many k blocks of weight fragments (6 x bf8 = 24 VGPRs each) are in flight ahead of the one
    // being multiplied -- LS_WRING0 in chunk 0 (tiles 0-2), LS_WRING1 in chunk 1 (tiles 3-4).  1 / 1 is the earlier loop (one block ahead,
    // handed over through copies, every pass fetching its first block after the previous pass's epilogue), kept for same-tree A/B like
    // LS_SPLIT_SHARED=0.  Anything deeper runs chmix_ring_pass: a register ring of depth + 1 statically addressed slots that keeps
    // running across the pass boundaries of a layer.  Every form gives the same bits.  Measured (profiles/r20_weight_ring.md): 2 / 2 is
    // 3.7 % faster than 1 / 1 at TED B = 512; 2 / 3 (255 - 256 VGPRs) and 1 / 2 are within the spread of it.  Carrying the ring across the
    // layer boundary as well, through LayerNorm 1, token mixing and LayerNorm 2, put 8 - 52 bytes per lane into scratch: not built.
#ifndef LS_WRING0
#define LS_WRING0 2
#endif
#ifndef LS_WRING1
#define LS_WRING1 2
#endif
    constexpr int kRing0 = LS_WRING0, kRing1 = LS_WRING1;
    static_assert(kRing0 >= 1 && kRing0 <= 3 && kRing1 >= 1 && kRing1 <= 3, "ring depth: 1, 2 or 3 k blocks");
    constexpr bool kRing = kSplitShared && (kRing0 > 1 || kRing1 > 1);
    constexpr int kRingSlots = (kRing0 > kRing1 ? kRing0 : kRing1) + 1;
    // Where the ring passes do their non-MFMA work (profiles/r21_layer_overlap.md).  Each switch is its own A/B on one tree
    // (tools/ab_variants.py build old=LS_EPI_BESIDE=0,... new=) and every combination gives the same bits: no term and no order changes.
    // Measured at TED B = 512, per launch: the parent 1.0124 ms, the default 0.9909.
    //   LS_EPI_BESIDE   1 = tile t's SiLU epilogue is issued among the MFMAs of the tile after it in k block 15 and pinned there; only
    //                   a pass's last tile applies its own after its MFMAs, so no accumulator outlives its pass or crosses a barrier.
    //                   0 = every epilogue after its pass; the compiler then carries chunk 0's across the mid-layer barriers.  Alone 0.9983.
    //   LS_PRIO_FLIP    1 = waves 4 - 7 run a chunk's first pass at s_setprio 1.  At equal priority the older wave w wins the issue
    //                   arbitration and finishes a chunk ~14 k clocks before its SIMD partner w + 4, which then runs on alone.  Alone 1.0046.
#ifndef LS_EPI_BESIDE
#define LS_EPI_BESIDE 1
#endif
#ifndef LS_PRIO_FLIP
#define LS_PRIO_FLIP 1
#endif
    constexpr bool kEpiBeside = LS_EPI_BESIDE != 0, kPrioFlip = LS_PRIO_FLIP != 0;
    constexpr int kChunkTiles = 3;             // token tiles of chunk 0 (rows 0..47); chunk 1 = tiles 3..4 (rows 48..R-1)
    constexpr int kChunkRows = 16 * kChunkTiles;
    constexpr int kPlane = kChunkRows * kUStride;      // bf16 per plane
    static_assert(!kSplitShared || 3 * kPlane * 2 <= (R * kUStride + kWaves * 2 * NREM * 16) * 4, "three bf16 planes of a chunk must fit U + REM");
    static_assert(R > kChunkRows && R - kChunkRows <= kChunkRows, "two chunks cover the rows");
    constexpr int kGrpStride = kD * 8 + 16;    // bf16 per 8-row group (+32 B so the two row halves of a tile miss each other's banks)
    static_assert(2 * NG * kGrpStride * 2 <= (R * kUStride + kWaves * 2 * NREM * 16) * 4, "bf16 token-mix planes must fit U + REM");
    static_assert(NREM > 0 && NREM <= 16, "ragged tile");
    static_assert(R <= 16 * kNT, "rows must fit the token tiles");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* psum = smem;                      // [8][80] (mean, M2) pairs of the LayerNorm merge
    float* U = smem + 2 * kWaves * 16 * kNT; // [R][520] fp32 operand / two bf16 planes (bf16x3 mode)
    float* REM = U + R * kUStride;           // [8 waves][2][NREM][16] remainder-row patch (fp32 mode)

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int s16 = lane & 15;
    int g = lane >> 4;
    int chw = 64 * w + 4 * g;                // + 16*cb + j  = this lane's channels
    // Register-pressure control: the residual stream (80 VGPRs) must stay in registers for the whole forward.
    // Left alone, LICM hoists every per-lane address of every phase out of the layer loop and keeps ~100 of them
    // live across the MFMA loops, which pushes X into scratch (each LayerNorm then reloads it with ~50 serialized
    // scratch_load + s_waitcnt pairs).  Laundering the lane id at phase boundaries makes those addresses
    // phase-local: 3 VALU ops to recompute instead of a register held for the whole kernel.
    auto fresh = [&]() {
        asm volatile("" : "+v"(lane));
        s16 = lane & 15;
        g = lane >> 4;
        chw = 64 * w + 4 * g;
    };

    // Row metadata is recomputed where needed (tiles 0..3 are always fully valid; only tile 4 is ragged).
    auto row_of = [&](int t) { return 16 * t + s16; };
    auto valid_of = [&](int t) { return (16 * t + 15 < R) ? true : (16 * t + s16 < R); };
    auto rowc_of = [&](int t) { const int r = 16 * t + s16; return (16 * t + 15 < R || r < R) ? r : R - 1; };

    f4 X[kCB][kNT];

    // TRAIN: global row (sample * S + token) of this lane's row of tile t, or -1 when the row is padding / past the batch
    auto grow_of = [&](int t) -> int {
        const int r = 16 * t + s16;
        if (r >= R) return -1;
        const int sq = r >= S ? 1 : 0;
        const int sample = 2 * b + sq;
        return sample < a.tr_B ? sample * S + (r - sq * S) : -1;
    };
    auto store_rows = [&](float* base, int l) {                 // X (residual layout) -> [L][tr_B*S][512]
        float* dst = base + (size_t)l * a.tr_B * S * kD;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int gr = grow_of(t);
            if (gr >= 0)
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb) *reinterpret_cast<f4*>(dst + (size_t)gr * kD + chw + 16 * cb) = X[cb][t];
        }
    };

    // phase stamps, -DLS_DEBUG builds only (tools/phase_profile.py): lane 0 of every wave of one workgroup records s_memtime
    auto stamp = [&](int idx) {
#ifdef LS_DEBUG
        if (a.prof && b == a.prof_wg && lane == 0 && idx < kProfPoints) a.prof[w * kProfPoints + idx] = __builtin_amdgcn_s_memtime();
        if (a.wgt && tid == 0 && (idx == 0 || idx == 4 + 8 * a.layers)) a.wgt[2 * b + (idx ? 1 : 0)] = __builtin_amdgcn_s_memtime();
#else
        (void)idx;
#endif
    };
    stamp(0);

    // ================= embedding: InputProcess + input_mapping (RAG.py:110-114, 184-192) ==========
    if constexpr (TRAIN) {
        // training forward: the token sequences were assembled by the batch-level kernels (input_mapping GEMM, style /
        // emotion tokens); load this workgroup's two samples into the residual layout
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int gr = grow_of(t);
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb)
                X[cb][t] = gr >= 0 ? *reinterpret_cast<const f4*>(a.tr_x0 + (size_t)gr * kD + chw + 16 * cb) : (f4){0.f, 0.f, 0.f, 0.f};
        }
    } else {
        // Base value of every row first (its loads overlap the x_t staging below): frame tokens start from the
        // per-call static projection, prefix tokens from the style sample / emotion embedding.  The x_t columns of
        // input_mapping are then accumulated ONTO these by using them as the MFMA C operand.
        // sm(sq): the sample whose pass occupies row half sq.  CFG: both halves are sample b (cond | uncond).  PAIR: samples
        // 2b and 2b+1, cond pass both; with an odd batch the last workgroup computes its last sample twice and stores it once.
        auto sm = [&](int sq) -> int { return PAIR ? min(2 * b + sq, a.batch - 1) : b; };
        const unsigned long long goff = a.call ? a.call->sample_offset : 0ull;
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            const int rc = rowc_of(t);
            const int sq = rc >= S ? 1 : 0;
            const int tk = rc - sq * S;
            const int smp = sm(sq);
            const bool unc = !PAIR && sq;
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb) {
                const int ch = chw + 16 * cb;
                f4 v = (f4){0.f, 0.f, 0.f, 0.f};
                if (valid_of(t)) {
                    if (tk >= NPRE) {
                        const float* st = (unc ? a.static_u : a.static_c) + ((size_t)smp * kT + (tk - NPRE)) * kD + ch;
                        v = *reinterpret_cast<const f4*>(st);
                    } else if (tk == 0) {
                        // style token: reparameterize(mu, logvar)  (RAG.py:10-13, 116-120)
                        const f4 mu = *reinterpret_cast<const f4*>(a.z_mu + (size_t)smp * kD + ch);
                        const f4 sd = *reinterpret_cast<const f4*>(a.z_std + (size_t)smp * kD + ch);
                        f4 e;
                        const float* ep = unc ? a.eps_u : a.eps_c;
                        if (ep) {
                            e = *reinterpret_cast<const f4*>(ep + (size_t)smp * kD + ch);
                        } else {
                            float z[4];            // this lane's 4 consecutive channels = one Philox block
                            philox_normal4(a.call, goff + (unsigned long long)smp, a.step_id, unc ? 2u : 1u, (unsigned)(ch >> 2), z);
                            e = (f4){z[0], z[1], z[2], z[3]};
                        }
                        v = mu + e * sd;
                    } else {
                        // BEAT emotion token (scripts_beat/model/RAG.py:125-126)
                        v = *reinterpret_cast<const f4*>(a.emo_tok + (size_t)smp * kD + ch);
                    }
                }
                X[cb][t] = v;
            }
        }
        constexpr int NIT = (R * KXP + 511) / 512;                   // x_t values per thread: 5 (TED) | 41 (BEAT)
        {
            // The thread's loads first (clamped address + select: branch-free, in flight together), then the LDS writes, in blocks of 14
            // so the registers stay bounded -- as a load -> write loop every iteration paid its own L2 round trip (41 in a row for
            // BEAT's 282-wide vectors, 5 for TED).  Same-box A/B (tools/ab_variants.py, 5 rounds): BEAT 0.8508 -> 0.8477 ms/step; TED
            // 1.3682 -> 1.3653 on the final build (1.4334 -> 1.4373 earlier in the round, under a different register allocation).
            constexpr int CH = 14;
#pragma unroll
            for (int it0 = 0; it0 < NIT; it0 += CH) {
                float xv[CH];
#pragma unroll
                for (int itl = 0; itl < CH; ++itl) {
                    if (it0 + itl >= NIT) break;
                    const int idx = min(tid + 512 * (it0 + itl), R * KXP - 1);
                    const int r = idx / KXP, k = idx - r * KXP;
                    const int sq = r >= S ? 1 : 0;
                    const int tk = r - sq * S;
                    const bool live = tk >= NPRE && k < JF;
                    xv[itl] = a.x_in[(size_t)sm(sq) * kT * JF + (live ? (tk - NPRE) * JF + k : 0)];
                    if (!live) xv[itl] = 0.f;
                }
#pragma unroll
                for (int itl = 0; itl < CH; ++itl) {
                    if (it0 + itl >= NIT) break;
                    const int idx = tid + 512 * (it0 + itl);
                    if (idx < R * KXP) {
                        const int r = idx / KXP;
                        U[r * kUStride + (idx - r * KXP)] = xv[itl];
                    }
                }
            }
        }
        __syncthreads();
        fresh();
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            f4 acc[2][kNT];
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                for (int t = 0; t < kNT; ++t) acc[c2][t] = X[2 * p + c2][t];
            const wrsrc_t wrs = wrsrc(a.W->winx_img);
            const int wsb = (w * 2 + p) * KXQ * 2 * 1024;
            f4 An[2];                                   // next k block's weight fragments in flight while this one is multiplied
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) An[c2] = wload4(wrs, lane * 16, wsb + c2 * 1024);
#pragma unroll 2
            for (int q = 0; q < KXQ; ++q) {
                f4 A[2], Bv[kNT];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) A[c2] = An[c2];
                const int qn = q + 1 < KXQ ? q + 1 : KXQ - 1;
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) An[c2] = wload4(wrs, lane * 16, wsb + (qn * 2 + c2) * 1024);
#pragma unroll
                for (int t = 0; t < kNT; ++t)
                    Bv[t] = *reinterpret_cast<const f4*>(&U[rowc_of(t) * kUStride + 16 * q + 4 * g]);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                        for (int t = 0; t < kNT; ++t) acc[c2][t] = MFMA(A[c2][j], Bv[t][j], acc[c2][t]);
            }
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                for (int t = 0; t < kNT; ++t)
                    X[2 * p + c2][t] = valid_of(t) ? acc[c2][t] : (f4){0.f, 0.f, 0.f, 0.f};   // pad rows stay zero
        }
    }

    auto dump_trace = [&](int stage) {
        if (!a.trace) return;
        float* tr = a.trace + ((size_t)b * (a.layers + 1) + stage) * R * kD;
#pragma unroll
        for (int t = 0; t < kNT; ++t)
            if (valid_of(t))
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb)
                    *reinterpret_cast<f4*>(tr + (size_t)row_of(t) * kD + chw + 16 * cb) = X[cb][t];
    };
    dump_trace(0);
    stamp(1);

    // LN_spatial statistics over the 512 channels of each row (mlp_module.py:29-33).  The reference is two-pass
    // (mean, then centred biased variance).  Here every lane does the two passes over its own 16 channels and the
    // (mean, M2) pairs are merged pairwise with Chan's parallel-variance update -- across the 4 lane groups with two
    // cross-lane exchanges, across the 8 waves through LDS -- which is as cancellation-free as two-pass but needs
    // ONE workgroup barrier per LayerNorm instead of two.
    float mean[kNT], rstd[kNT];
    auto ln_stats = [&](float* gstats) {
        (void)gstats;
        if (LS_ABLATED(a, 4)) {
#pragma unroll
            for (int t = 0; t < kNT; ++t) { mean[t] = 0.f; rstd[t] = 1.f; }
            return;
        }
        f2* pst = reinterpret_cast<f2*>(psum);            // [8 waves][80 rows] (mean, M2) of 64 channels
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            // both passes as float4 arithmetic (packed f32: two elements per issue); four interleaved partial sums per pass
            f4 sv = X[0][t];
#pragma unroll
            for (int cb = 1; cb < kCB; ++cb) sv += X[cb][t];
            const float s = (sv[0] + sv[1]) + (sv[2] + sv[3]);
            float m = s * (1.0f / 16.0f);
            const f4 mv = (f4){m, m, m, m};
            f4 qv = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb) {
                const f4 d = X[cb][t] - mv;
                qv = __builtin_elementwise_fma(d, d, qv);
            }
            float m2 = (qv[0] + qv[1]) + (qv[2] + qv[3]);
            {   // merge with the lane group 16 lanes away (16 + 16 values), then 32 lanes away (32 + 32); the update is symmetric
                // in the pair, so both members of the v_permlane swap are used as they come (no select, no LDS round trip)
                float ma, mb, qa, qb;
                xor16_pair(m, ma, mb);
                xor16_pair(m2, qa, qb);
                const float d = mb - ma;
                m2 = (qa + qb) + d * d * 8.0f;
                m = 0.5f * (ma + mb);
            }
            {
                float ma, mb, qa, qb;
                xor32_pair(m, ma, mb);
                xor32_pair(m2, qa, qb);
                const float d = mb - ma;
                m2 = (qa + qb) + d * d * 16.0f;
                m = 0.5f * (ma + mb);
            }
            if (g == 0) pst[w * 80 + 16 * t + s16] = (f2){m, m2};
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
            f2 pw[kWaves];
            f2 acc2 = (f2){0.f, 0.f};                     // (sum of means, sum of M2): packed f32 adds
#pragma unroll
            for (int ww = 0; ww < kWaves; ++ww) {
                pw[ww] = pst[ww * 80 + 16 * t + s16];
                acc2 += pw[ww];
            }
            const float ms = acc2.x, m2s = acc2.y;
            const float mt = ms * (1.0f / kWaves);
            const f2 mt2 = (f2){mt, mt};
            f2 dd2 = (f2){0.f, 0.f};                      // squared mean deviations, two waves per packed FMA
#pragma unroll
            for (int ww = 0; ww < kWaves; ww += 2) {
                const f2 d = (f2){pw[ww].x, pw[ww + 1].x} - mt2;
                dd2 = __builtin_elementwise_fma(d, d, dd2);
            }
            const float dd = dd2.x + dd2.y;
            mean[t] = mt;
            rstd[t] = rsqrtf((m2s + 64.0f * dd) * (1.0f / kD) + 1e-5f);
            if constexpr (TRAIN) {                        // (mean, rstd) of every row, kept for the LayerNorm backward
                const int gr = grow_of(t);
                if (w == 0 && g == 0 && gr >= 0) *reinterpret_cast<f2*>(gstats + (size_t)gr * 2) = (f2){mean[t], rstd[t]};
            }
        }
    };
    // write the normalised operand of this lane's channels into the LDS buffer: LN1 applies alpha/beta here
    // (2 FMAs per element); LN2's alpha/beta are folded into the channel-mix weights/bias on the host
    // (W' = W.diag(alpha), b' = b + W.beta), so its operand is just (x - mean) * rstd: 1 FMA per element.
    // alv/bev: LN1's alpha/beta of this lane's channels, loaded by the caller BEFORE the statistics (a load per channel block
    // here cost four serialised L2 round trips per layer); affine = false: LN2 when sampling, affine folded into the weights
    // `affine` is a compile-time tag (std::true_type: LN1, and LN2 while training): as a run-time `alpha != nullptr` the compiler could
    // not prove LN1's pointer non-null and computed BOTH forms of every element, selecting with four v_cndmask_b32 per float4
    // (160 per layer and wave) -- and, in bf16x3 mode, branched on it.
    auto ln_store = [&](auto affine, const f4 (&alv)[kCB], const f4 (&bev)[kCB], float* gout) {
        (void)gout;
        constexpr bool alpha = decltype(affine)::value;
        float nmr[kNT];
#pragma unroll
        for (int t = 0; t < kNT; ++t) nmr[t] = -mean[t] * rstd[t];
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            f4 al, be;
            if (alpha) {
                al = alv[cb];
                be = bev[cb];
            }
#pragma unroll
            for (int t = 0; t < kNT; ++t)
                if (PREC == 1 && alpha && !kTokTr && !valid_of(t) && row_of(t) < 8 * NG) {
                    __bf16* Th = reinterpret_cast<__bf16*>(U);
                    __bf16* Tl = Th + NG * kGrpStride;
                    const int r = row_of(t);
                    const int o = (r >> 3) * kGrpStride + (64 * w + 16 * cb + g) * 8 + (r & 7);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { Th[o + 32 * j] = (__bf16)0.f; Tl[o + 32 * j] = (__bf16)0.f; }
                } else if (valid_of(t)) {
                    const f4 rs = (f4){rstd[t], rstd[t], rstd[t], rstd[t]}, nm = (f4){nmr[t], nmr[t], nmr[t], nmr[t]};
                    f4 u = __builtin_elementwise_fma(X[cb][t], rs, nm);          // packed f32
                    if constexpr (TRAIN) {                // x-hat is what the backward needs (LayerNorm backward directly; the
                        const int gr = grow_of(t);        // weight gradients rebuild U = alpha * x-hat + beta from it)
                        if (gr >= 0 && !LS_TRAIN_ABL) LS_TRAIN_ST(reinterpret_cast<f4*>(gout + (size_t)gr * kD + chw + 16 * cb), u);
                    }
                    if (alpha) u = __builtin_elementwise_fma(u, al, be);
                    if (PREC == 1 && alpha && !kTokTr) {
                        // token-mix operand, bf16x3: the contraction runs over ROWS, so the MFMA A operand needs 8
                        // consecutive source rows of one channel in 16 contiguous bytes: UT[row/8][channel][row%8]
                        // slot of channel (g, j) inside its 16-channel block is 4*j + g (bit-fields swapped), so the four lane
                        // groups of one ds_write_b16 hit four different 16-byte slots instead of two
                        __bf16* Th = reinterpret_cast<__bf16*>(U);
                        __bf16* Tl = Th + NG * kGrpStride;
                        const int r = row_of(t);
                        const int o = (r >> 3) * kGrpStride + (64 * w + 16 * cb + g) * 8 + (r & 7);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const __bf16 hi = (__bf16)u[j];
                            Th[o + 32 * j] = hi;
                            Tl[o + 32 * j] = (__bf16)(u[j] - (float)hi);
                        }
                    } else if (PREC == 1 && (!alpha || kTokTr)) {
                        // bf16x3 operand: u = hi + lo (+ O(2^-17 |u|)), hi = bf16_rne(u), lo = bf16_rne(u - hi);
                        // two bf16 planes [R][520] in the space of the fp32 buffer
                        __bf16* Uh = reinterpret_cast<__bf16*>(U);
                        __bf16* Ul = Uh + R * kUStride;
                        bf4 hi, lo;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            hi[j] = (__bf16)u[j];
                            lo[j] = (__bf16)(u[j] - (float)hi[j]);
                        }
                        *reinterpret_cast<bf4*>(&Uh[row_of(t) * kUStride + chw + 16 * cb]) = hi;
                        *reinterpret_cast<bf4*>(&Ul[row_of(t) * kUStride + chw + 16 * cb]) = lo;
                    } else {
                        *reinterpret_cast<f4*>(&U[row_of(t) * kUStride + chw + 16 * cb]) = u;
                    }
                }
        }
    };

    // PREC 2 form of LN2's store (kSplitShared): token tiles [t0, t1) of one 48-row chunk, u = (x - mean) * rstd as above, split by its
    // owner into hi / mid / lo (split3_f4: the arithmetic of split3_bf16) and written as three 8-byte stores into the bf16 planes
    // P[part][row - first row of the chunk][520] that overlay U (+ REM).  Padding rows are not written: their lanes read the clamped last row.
    auto ln_store_split = [&](auto t0c, auto t1c) {
        constexpr int t0 = decltype(t0c)::value, t1 = decltype(t1c)::value;
        __bf16* P = reinterpret_cast<__bf16*>(U);
#pragma unroll
        for (int t = t0; t < t1; ++t)
            if (valid_of(t)) {
                const float nmr = -mean[t] * rstd[t];
                const f4 rs = (f4){rstd[t], rstd[t], rstd[t], rstd[t]}, nm = (f4){nmr, nmr, nmr, nmr};
                __bf16* dst = P + (row_of(t) - 16 * t0) * kUStride + chw;
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb) {
                    const f4 u = __builtin_elementwise_fma(X[cb][t], rs, nm);          // packed f32
                    bf4 hi, mid, lo;
                    split3_f4(u, hi, mid, lo);
                    *reinterpret_cast<bf4*>(dst + 16 * cb) = hi;
                    *reinterpret_cast<bf4*>(dst + kPlane + 16 * cb) = mid;
                    *reinterpret_cast<bf4*>(dst + 2 * kPlane + 16 * cb) = lo;
                }
            }
    };
    // the channel mixing of tiles [t0, t1) of the chunk that ln_store_split has staged, for both channel halves p of this wave; the six
    // terms of every (q, t) in the order of kSplitA / kSplitB (smallest first, c2 innermost), q ascending: each accumulator adds the same
    // sequence as in the in-register form.  The weight slice is prefetched one k block ahead.  (LS_WRING0 = LS_WRING1 = 1 only: the
    // default build runs chmix_ring_pass below.)
    auto chmix_split_chunk = [&](int l, auto t0c, auto t1c) {
        constexpr int t0 = decltype(t0c)::value, t1 = decltype(t1c)::value, NTC = t1 - t0;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            fresh();
            f4 acc[2][NTC];
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                const f4 bc = wload4(wrsrc(a.W->bch), chw * 4, (l * kD + 16 * (2 * p + c2)) * 4);
#pragma unroll
                for (int t = 0; t < NTC; ++t) acc[c2][t] = bc;
            }
            const wrsrc_t wr0 = wrsrc(a.W->wch_hi_img), wr1 = wrsrc(a.W->wch_lo_img), wr2 = wrsrc(a.W->wch_lo2_img);
            const int wsb = (((l * kWaves + w) * 2 + p) * 16) * 2 * 1024;
            typedef const __attribute__((address_space(3))) bf8* ldsp8;
            typedef const __attribute__((address_space(3))) __bf16* ldspb;
            ldspb pb[NTC];                            // lane (token, g) reads k = 32q + 8g .. +7 of its (clamped) row, per part
#pragma unroll
            for (int t = 0; t < NTC; ++t) pb[t] = (ldspb)(reinterpret_cast<const __bf16*>(U) + (rowc_of(t0 + t) - 16 * t0) * kUStride + 8 * g);
            bf8 An[3][2];
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                An[0][c2] = wload8h(wr0, lane * 16, wsb + c2 * 1024);
                An[1][c2] = wload8h(wr1, lane * 16, wsb + c2 * 1024);
                An[2][c2] = wload8h(wr2, lane * 16, wsb + c2 * 1024);
            }
            if (!LS_ABLATED(a, 1))
#pragma unroll 1
            for (int q = 0; q < 16; ++q) {
                bf8 A[3][2];
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) A[s][c2] = An[s][c2];
                const int qn = LS_ABLATED(a, 8) ? 0 : (q + 1 < 16) ? q + 1 : 15;
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    An[0][c2] = wload8h(wr0, lane * 16, wsb + (qn * 2 + c2) * 1024);
                    An[1][c2] = wload8h(wr1, lane * 16, wsb + (qn * 2 + c2) * 1024);
                    An[2][c2] = wload8h(wr2, lane * 16, wsb + (qn * 2 + c2) * 1024);
                }
#pragma unroll
                for (int t = 0; t < NTC; ++t) {
                    bf8 B[3];
#pragma unroll
                    for (int s = 0; s < 3; ++s) B[s] = *(ldsp8)(pb[t] + s * kPlane + 32 * q);
#pragma unroll
                    for (int i = 0; i < kSplitTerms; ++i)
#pragma unroll
                        for (int c2 = 0; c2 < 2; ++c2)
                            acc[c2][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[kSplitA[i]][c2], B[kSplitB[i]], acc[c2][t], 0, 0, 0);
                }
            }
            fresh();
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                for (int t = 0; t < NTC; ++t)
                    if (valid_of(t0 + t)) X[2 * p + c2][t0 + t] = silu_acc4(acc[c2][t], X[2 * p + c2][t0 + t]);
        }
    };

    // The same channel mixing with the weight fragments in a register ring (kRing).  One call is ONE pass: channel half p of the tiles
    // [t0, t1) of the staged chunk.  D k blocks are in flight ahead of the block being multiplied; the ring has D + 1 slots, block q of
    // a pass always lies in slot q % (D + 1), and the k loop is unrolled by D + 1 so that every slot index is a constant and nothing is
    // copied.  Step q first refills the slot that block q - 1 has just left -- with block q + D of this pass, or, during the last D
    // steps and once more after the last one, with the block of the NEXT pass that belongs in that slot (DN = the next pass's depth,
    // 0 = there is none) -- and then issues the MFMAs of block q: the same six terms per (q, t) in the same order, q ascending, so every
    // accumulator adds the sequence it always did.  The next pass's first blocks and its bias (BCn) are therefore in flight across the
    // SiLU epilogue and, between the chunks, across the barriers and ln_store_split: they need no LDS and nothing they read changes.
    // (With 3 slots, 16 = 5 * 3 + 1: slot 0 is the last to come free, so the next pass's block 0 is fetched after its block 1.  Rotating
    // each pass's slot numbering so that they come in order measured the same -- profiles/r20_weight_ring.md -- and was not kept.)
    // The layer's first pass has no predecessor: ring_prime issues its bias and first blocks before LayerNorm 2's output is staged, so
    // they arrive under that store and its barrier; the layer's last pass fetches nothing beyond its own slice (DN = 0).
    // No read leaves the images: a pass addresses blocks 0 .. 15 of its own slice (l, w, p), l < layers, and blocks 0 .. DN - 1 of the
    // slice `nbase` the caller names, which is another pass of the SAME layer and wave; and the three planes are read through
    // descriptors bounded to the `layers` slices of the image, so that a wrong offset would read zeros -- and fail the bitwise tests --
    // instead of faulting.
    bf8 WR[kRingSlots][3][2];
    f4 BCn[2];
    struct RingPlanes { wrsrc_t r[3]; };
    auto ring_planes = [&]() {
        const int wbytes = a.layers * (kWaves * 2 * 16 * 2 * 1024);
        return RingPlanes{{uniform_rsrc(a.W->wch_hi_img, wbytes), uniform_rsrc(a.W->wch_lo_img, wbytes), uniform_rsrc(a.W->wch_lo2_img, wbytes)}};
    };
    auto ring_base = [&](int l, int p) { return (((l * kWaves + w) * 2 + p) * 16) * 2 * 1024; };      // bytes, the same in all three planes
    auto ring_bias = [&](int l, int p) { return (l * kD + 32 * p) * 4; };
    auto ring_fetch = [&](const RingPlanes& wr, int slot, int off) {
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int s = 0; s < 3; ++s) WR[slot][s][c2] = wload8h(wr.r[s], lane * 16, off + c2 * 1024);
        // the scheduler must not sink the refill towards its use D blocks later: in the two-tile chunk it gathered the loads of a
        // whole turn at the loop's end, and the loop's first block then waited for vmcnt(0)
        __builtin_amdgcn_sched_barrier(0);
    };
    auto ring_prime = [&](int l) {
        const RingPlanes wr = ring_planes();
        const wrsrc_t wrb = wrsrc(a.W->bch);
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2) BCn[c2] = wload4(wrb, chw * 4, ring_bias(l, 0) + 64 * c2);
#pragma unroll
        for (int i = 0; i < kRing0; ++i) ring_fetch(wr, i, ring_base(l, 0) + (LS_ABLATED(a, 8) ? 0 : i * 2 * 1024));
    };
    // kEpiBeside: a block is NTC steps, one per token tile, each fenced with sched_barrier(0) so that the order below is the order
    // issued; all fragments of a block are read at its head, as in `block`.  In k block 15 the epilogue of tile t - 1, whose accumulators
    // are final since its own step, is spread over the MFMAs of tile t: 12 packed-f32 VALU and 16 transcendentals (weight 5/3 each), as
    // one VALU and one or two transcendentals behind every MFMA, which holds vector issue for 8 of its 16 cycles.  Only the pass's last
    // tile has no MFMAs behind it in its pass: its epilogue follows at once, so no accumulator lives beyond its pass, let alone across a
    // barrier.
    auto chmix_ring_pass = [&](int l, auto pc, auto t0c, auto t1c, auto dc, auto dnc, int nbase, int nbias) {
        constexpr int p = decltype(pc)::value, t0 = decltype(t0c)::value, t1 = decltype(t1c)::value, NTC = t1 - t0;
        constexpr int D = decltype(dc)::value, DN = decltype(dnc)::value, NS = D + 1;
        constexpr int QM = ((16 - D) / NS) * NS;       // blocks [0, QM): the rolled loop, whole turns of the ring, every refill from this pass
        static_assert(NS <= kRingSlots && DN <= kRingSlots, "ring slots");
        static_assert(QM > 0, "the rolled loop runs");
        fresh();
        if constexpr (kPrioFlip) {
            if (w >= 4) {                              // a scalar branch: s_setprio ignores EXEC
                __builtin_amdgcn_s_setprio(p == 0 ? 1 : 0);
            }
        }
        const RingPlanes wr = ring_planes();
        const wrsrc_t wrb = wrsrc(a.W->bch);
        const int wsb = ring_base(l, p);
        const int qb = LS_ABLATED(a, 8) ? 0 : 2 * 1024;                 // bytes from one k block to the next (ablation 8: every load is block 0)
        const int nsb = LS_ABLATED(a, 8) ? wsb : nbase;
        auto fetch = [&](int slot, int off) { ring_fetch(wr, slot, off); };
        f4 acc[2][NTC];
#pragma unroll
        for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
            for (int t = 0; t < NTC; ++t) acc[c2][t] = BCn[c2];
        typedef const __attribute__((address_space(3))) bf8* ldsp8;
        typedef const __attribute__((address_space(3))) __bf16* ldspb;
        ldspb pb[NTC];                            // lane (token, g) reads k = 32q + 8g .. +7 of its (clamped) row, per part
#pragma unroll
        for (int t = 0; t < NTC; ++t) pb[t] = (ldspb)(reinterpret_cast<const __bf16*>(U) + (rowc_of(t0 + t) - 16 * t0) * kUStride + 8 * g);
        auto block = [&](int q, int slot) {
            if (LS_ABLATED(a, 1)) return;
#pragma unroll
            for (int t = 0; t < NTC; ++t) {
                bf8 B[3];
#pragma unroll
                for (int s = 0; s < 3; ++s) B[s] = *(ldsp8)(pb[t] + s * kPlane + 32 * q);
#pragma unroll
                for (int i = 0; i < kSplitTerms; ++i)
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
                        acc[c2][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WR[slot][kSplitA[i]][c2], B[kSplitB[i]], acc[c2][t], 0, 0, 0);
            }
        };
        auto epi = [&](int t, const f4 (&av)[2]) {
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2)
                if (valid_of(t)) X[2 * p + c2][t] = silu_acc4(av[c2], X[2 * p + c2][t]);
            // sched_barrier holds the machine scheduler only: without a use here the arithmetic is sunk, before scheduling, to where X is
            // read next -- behind the barriers
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) asm volatile("" : "+v"(X[2 * p + c2][t]));
        };
        auto block_seq = [&](int q, int slot, bool last) {               // last: k block 15
            if (LS_ABLATED(a, 1)) return;
            bf8 B[NTC][3];
#pragma unroll
            for (int t = 0; t < NTC; ++t)
#pragma unroll
                for (int s = 0; s < 3; ++s) B[t][s] = *(ldsp8)(pb[t] + s * kPlane + 32 * q);
#pragma unroll
            for (int t = 0; t < NTC; ++t) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < kSplitTerms; ++i)
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
                        acc[c2][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WR[slot][kSplitA[i]][c2], B[t][kSplitB[i]], acc[c2][t], 0, 0, 0);
                if (last && t > 0) {
                    const int tp = t > 0 ? t - 1 : 0;                    // t = 0 is dead here, but its unrolled copy still needs an index in range
                    const f4 av[2] = {acc[0][tp], acc[1][tp]};
                    epi(t0 + tp, av);
#pragma unroll
                    for (int i = 0; i < kSplitTerms; ++i) {
                        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);      // one MFMA,
                        __builtin_amdgcn_sched_group_barrier(0x2, 1, 0);      // one packed-f32 VALU,
                        __builtin_amdgcn_sched_group_barrier(0x400, 1, 0);    // one transcendental;
                        __builtin_amdgcn_sched_group_barrier(0x8, 1, 0);      // one MFMA,
                        __builtin_amdgcn_sched_group_barrier(0x2, 1, 0);      // one VALU,
                        __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);    // two transcendentals
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        auto run = [&](int q, int slot, bool last) {
            if constexpr (kEpiBeside) block_seq(q, slot, last);
            else block(q, slot);
        };
#pragma unroll 1
        for (int q0 = 0; q0 < QM; q0 += NS) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                fetch((j + D) % NS, wsb + (q0 + j + D) * qb);
                run(q0 + j, j, false);
            }
        }
        // the last blocks, unrolled: the refills run out of this pass and go on with the next one
        if constexpr (DN > 0) {
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) BCn[c2] = wload4(wrb, chw * 4, nbias + 64 * c2);
#pragma unroll
            for (int f = NS; f < DN; ++f) fetch(f, nsb + f * qb);          // a deeper next pass: the slots this pass does not use
        }
#pragma unroll
        for (int q = QM; q <= 16; ++q) {
            const int f = (q + D) % NS;                                      // the slot block q - 1 has left
            if (q + D < 16) fetch(f, wsb + (q + D) * qb);
            else if (f < DN) fetch(f, nsb + f * qb);
            if (q < 16) run(q, q % NS, q == 15);
        }
        if constexpr (kEpiBeside) {
            const f4 av[2] = {acc[0][NTC - 1], acc[1][NTC - 1]};             // tiles t0 .. t1 - 2 are done
            epi(t1 - 1, av);
        } else {
            fresh();
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                for (int t = 0; t < NTC; ++t)
                    if (valid_of(t0 + t)) X[2 * p + c2][t0 + t] = silu_acc4(acc[c2][t], X[2 * p + c2][t0 + t]);
        }
    };

    // ================= TransMLP: 8 x MLPblock (mlp_module.py:67-91) ================================
    for (int l = 0; l < a.layers; ++l) {
        fresh();
        if constexpr (TRAIN) {
            // every sample has its own diffusion timestep: the two halves of the workgroup add different embedding rows
#pragma unroll
            for (int t = 0; t < kNT; ++t) {
                const int sample = min(2 * b + (row_of(t) >= S ? 1 : 0), a.tr_B - 1);
                const float* te = a.temb + (size_t)sample * a.temb_stride + chw;
                if (valid_of(t))
#pragma unroll
                    for (int cb = 0; cb < kCB; ++cb) X[cb][t] += *reinterpret_cast<const f4*>(te + 16 * cb);
            }
        } else {   // x = x + emb  (emb re-added at the input of EVERY block, mlp_module.py:68-69, 88-89)
            const float* te = a.temb + (size_t)b * a.temb_stride + chw;
            f4 e[kCB];
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb) e[cb] = *reinterpret_cast<const f4*>(te + 16 * cb);
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb)
#pragma unroll
                for (int t = 0; t < kNT; ++t)
                    if (valid_of(t)) X[cb][t] += e[cb];
        }
        // ---- block1: LN -> token-mixing Conv1d(S,S,1) -> SiLU -> residual -------------------------
        f4 alv[kCB], bev[kCB];                      // LN1 affine: in flight during the statistics and their barrier
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            alv[cb] = wload4(wrsrc(a.W->ln1a), chw * 4, (l * kD + 16 * cb) * 4);
            bev[cb] = wload4(wrsrc(a.W->ln1b), chw * 4, (l * kD + 16 * cb) * 4);
        }
        ln_stats(TRAIN ? a.tr_s1 + (size_t)l * a.tr_B * S * 2 : nullptr);
        stamp(2 + 8 * l);
        fresh();
        ln_store(std::true_type{}, alv, bev, TRAIN ? a.tr_x1 + (size_t)l * a.tr_B * S * kD : nullptr);
        // no workgroup barrier here: token mixing contracts over ROWS, so wave w only reads back the 64 channel columns
        // it has just written itself (LDS operations of one wave execute in order); the LN statistics barrier above
        // already ordered these stores after every wave's reads of the previous operand.
        __builtin_amdgcn_wave_barrier();
        stamp(3 + 8 * l);
        fresh();
        // out[d][r] = sum_r' u[r'][d] * WW[r][r']  as D[channel][row]: A = u^T from LDS, B = the block-diagonal
        // token weights (same for every workgroup, L1/L2 resident).  Tile by tile so only 18 B + 16 acc
        // registers are live; the k range of a tile covers just the sequence(s) whose rows it holds.
        if constexpr (PREC == 1) {
            if (!LS_ABLATED(a, 2)) {
                const __bf16* Th = reinterpret_cast<const __bf16*>(U);
                const __bf16* Tl = Th + NG * kGrpStride;
                const int slot = ((s16 & 3) << 2) | (s16 >> 2);      // channel i = 4g'+j' of a block lives in slot 4j'+g'
                const wrsrc_t wrh = wrsrc(a.W->ww_hi_img), wrl = wrsrc(a.W->ww_lo_img);
                const int wsb = l * kNT * KS * 1024;
#pragma unroll
                for (int t = 0; t < kNT; ++t) {
                    const float bt = valid_of(t) ? g1(a.W->btok_rows)[l * 80 + row_of(t)] : 0.f;
                    f4 acc[kCB];
#pragma unroll
                    for (int cb = 0; cb < kCB; ++cb) acc[cb] = (f4){bt, bt, bt, bt};
#pragma unroll
                    for (int ks = 0; ks < KS; ++ks) {
                        if (tokmix_needed32(S, t, ks)) {
                            const bf8 Bh = wload8h(wrh, lane * 16, wsb + (t * KS + ks) * 1024), Bl = wload8h(wrl, lane * 16, wsb + (t * KS + ks) * 1024);
                            bf8 Ah[kCB], Al[kCB];
                            if constexpr (kTokTr) {
                                typedef short s4v __attribute__((ext_vector_type(4)));
                                typedef __attribute__((address_space(3))) s4v* lds4;
                                const __bf16* Ph = reinterpret_cast<const __bf16*>(U);
                                const __bf16* Pl = Ph + R * kUStride;
                                // rows past the last one are clamped: their weights are 0 and the clamped row is finite
                                const int r0 = min(32 * ks + 8 * g + (s16 >> 2), R - 1), r1 = min(32 * ks + 8 * g + 4 + (s16 >> 2), R - 1);
                                const int c0 = 64 * w + 4 * (s16 & 3);
#pragma unroll
                                for (int cb = 0; cb < kCB; ++cb) {
                                    const s4v h0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(Ph + r0 * kUStride + c0 + 16 * cb));
                                    const s4v h1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(Ph + r1 * kUStride + c0 + 16 * cb));
                                    const s4v l0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(Pl + r0 * kUStride + c0 + 16 * cb));
                                    const s4v l1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(Pl + r1 * kUStride + c0 + 16 * cb));
                                    typedef short s8v __attribute__((ext_vector_type(8)));
                                    Ah[cb] = __builtin_bit_cast(bf8, __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7));
                                    Al[cb] = __builtin_bit_cast(bf8, __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7));
                                    (void)sizeof(s8v);
                                }
                            } else {
                                const int grp = (4 * ks + 3 < NG || 4 * ks + g < NG) ? 4 * ks + g : NG - 1;   // clamp: weights are 0 there
                                const int ao = grp * kGrpStride + (64 * w + slot) * 8;
#pragma unroll
                                for (int cb = 0; cb < kCB; ++cb) {
                                    Ah[cb] = *reinterpret_cast<const bf8*>(Th + ao + 16 * cb * 8);
                                    Al[cb] = *reinterpret_cast<const bf8*>(Tl + ao + 16 * cb * 8);
                                }
                            }
#pragma unroll
                            for (int cb = 0; cb < kCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al[cb], Bh, acc[cb], 0, 0, 0);
#pragma unroll
                            for (int cb = 0; cb < kCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[cb], Bl, acc[cb], 0, 0, 0);
#pragma unroll
                            for (int cb = 0; cb < kCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[cb], Bh, acc[cb], 0, 0, 0);
                        }
                    }
                    if (valid_of(t)) {
#pragma unroll
                        for (int cb = 0; cb < kCB; ++cb)
                            X[cb][t] = silu_acc4(acc[cb], X[cb][t]);
                    }
                }
            }
        } else if (!LS_ABLATED(a, 2)) {
            const wrsrc_t wrs = wrsrc(a.W->ww_img);
            const int wsb = l * kNT * MK * 256;
            // source-row addresses off pinned LDS bases (see the channel-mixing loop): row 4 m + g = base[m >> 3] + (m & 7) * 4 rows,
            // 64 B per channel block in the offset field; the one clamped row group (4 m + g >= R) has its own base
            typedef const __attribute__((address_space(3))) float* ldsp;
            constexpr int MB = (MK + 7) / 8;
            ldsp upb[MB];
#pragma unroll
            for (int k = 0; k < MB; ++k) upb[k] = (ldsp)(U + 64 * w + s16 + (32 * k + g) * kUStride);
            ldsp uplast = (ldsp)(U + 64 * w + s16 + min(4 * (MK - 1) + g, R - 1) * kUStride);
#pragma unroll
            for (int k = 0; k < MB; ++k) asm volatile("" : "+v"(upb[k]));
            asm volatile("" : "+v"(uplast));
#pragma unroll
            for (int t = 0; t < kNT; ++t) {
                float Bt[MK];
#pragma unroll
                for (int m = 0; m < MK; ++m)
                    if (tokmix_needed(S, t, m)) Bt[m] = wload1(wrs, lane * 4, wsb + (t * MK + m) * 256);
                const float bt = valid_of(t) ? g1(a.W->btok_rows)[l * 80 + row_of(t)] : 0.f;    // Conv1d bias of this row
                f4 acc[kCB];
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb) acc[cb] = (f4){bt, bt, bt, bt};
#pragma unroll
                for (int m = 0; m < MK; ++m) {
                    if (tokmix_needed(S, t, m)) {
                        ldsp src = (4 * m + 3 < R) ? upb[m >> 3] + (4 * (m & 7)) * kUStride : uplast;
#pragma unroll
                        for (int cb = 0; cb < kCB; ++cb)
                            acc[cb] = MFMA(src[16 * cb], Bt[m], acc[cb]);
                    }
                }
                if (valid_of(t)) {
                    if constexpr (TRAIN) {                // pre-activation of the token-mixing conv, for SiLU'
                        const int gr = grow_of(t);
                        if (gr >= 0 && !LS_TRAIN_ABL) {
                            float* dst = a.tr_a1 + ((size_t)l * a.tr_B * S + gr) * kD + chw;
#pragma unroll
                            for (int cb = 0; cb < kCB; ++cb) LS_TRAIN_ST(reinterpret_cast<f4*>(dst + 16 * cb), acc[cb]);
                        }
                    }
#pragma unroll
                    for (int cb = 0; cb < kCB; ++cb)
                        X[cb][t] = silu_acc4(acc[cb], X[cb][t]);
                }
            }
        }
        stamp(4 + 8 * l);
        fresh();
        // ---- block2: LN -> channel-mixing Linear(512,512) -> SiLU -> residual ---------------------
        f4 alv2[kCB], bev2[kCB];
        if constexpr (TRAIN) {   // training keeps LN2's affine explicit (alpha2 / beta2 get their own gradients)
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb) {
                alv2[cb] = wload4(wrsrc(a.W->ln2a), chw * 4, (l * kD + 16 * cb) * 4);
                bev2[cb] = wload4(wrsrc(a.W->ln2b), chw * 4, (l * kD + 16 * cb) * 4);
            }
        }
        ln_stats(TRAIN ? a.tr_s2 + (size_t)l * a.tr_B * S * 2 : nullptr);
        stamp(5 + 8 * l);      // its two barriers also order every wave's token-mix reads before the stores below
        if constexpr (!kSplitShared) {
            ln_store(std::integral_constant<bool, TRAIN>{}, alv2, bev2, TRAIN ? a.tr_x2 + (size_t)l * a.tr_B * S * kD : nullptr);
            __syncthreads();
            stamp(6 + 8 * l);
        }
        if constexpr (kSplitShared) {
            // ---- split-fp32, operand split once: W'.u with both operands split exactly into three bf16 parts, a = a0 + a1 + a2
            // (round-to-nearest: |a1| <= 2^-8 |a|, |a2| <= 2^-16 |a|); every bf16 x bf16 product is exact in fp32.  The weight planes come
            // split from the host (wch_hi / wch_lo / wch_lo2); the operand's three planes are written by ln_store_split, 48 rows at a
            // time (all R rows would need 3 * R * 1040 B = 218 KB), so a layer is: chunk 0 staged | barrier | tiles 0-2 mixed and added
            // to X | barrier (every wave is done reading chunk 0) | chunk 1 staged from the still unnormalised X of tiles 3-4 | barrier
            // | tiles 3-4 mixed.  mean / rstd of all rows come from the one ln_stats above.  All 5 token tiles run on
            // v_mfma_f32_16x16x32_bf16 (pad rows read the clamped last row, their outputs are dropped), no ragged-row VALU path.
            // Non-finite operands: Inf - Inf residuals are NaN, so an Inf in u or W' gives NaN (the fp32 MFMA may give Inf).
            typedef std::integral_constant<int, 0> T0;
            typedef std::integral_constant<int, kChunkTiles> T1;
            typedef std::integral_constant<int, kNT> T2;
            if constexpr (kRing) ring_prime(l);
            ln_store_split(T0{}, T1{});
            __syncthreads();
            stamp(6 + 8 * l);
            if constexpr (kRing) {
                // the four passes of the layer as one weight stream: each names the slice that follows it
                typedef std::integral_constant<int, 0> P0;
                typedef std::integral_constant<int, 1> P1;
                typedef std::integral_constant<int, kRing0> D0;
                typedef std::integral_constant<int, kRing1> D1;
                typedef std::integral_constant<int, 0> DX;                   // the layer's last pass is followed by nothing: it does not advance
                chmix_ring_pass(l, P0{}, T0{}, T1{}, D0{}, D0{}, ring_base(l, 1), ring_bias(l, 1));
                chmix_ring_pass(l, P1{}, T0{}, T1{}, D0{}, D1{}, ring_base(l, 0), ring_bias(l, 0));
                stamp(7 + 8 * l);
                __syncthreads();
                ln_store_split(T1{}, T2{});
                __syncthreads();
                stamp(8 + 8 * l);
                chmix_ring_pass(l, P0{}, T1{}, T2{}, D1{}, D1{}, ring_base(l, 1), ring_bias(l, 1));
                chmix_ring_pass(l, P1{}, T1{}, T2{}, D1{}, DX{}, ring_base(l, 1), ring_bias(l, 1));
            } else {
                chmix_split_chunk(l, T0{}, T1{});
                stamp(7 + 8 * l);
                __syncthreads();
                ln_store_split(T1{}, T2{});
                __syncthreads();
                stamp(8 + 8 * l);
                chmix_split_chunk(l, T1{}, T2{});
            }
        } else if constexpr (PREC == 1) {
            // ---- bf16x3 split precision: W'.u ~= hi_w.hi_u + hi_w.lo_u + lo_w.hi_u on v_mfma_f32_16x16x32_bf16 (fp32
            // accumulate; bf16 x bf16 products are exact in fp32; the dropped lo.lo term and the split residuals are
            // O(2^-16) relative).  These MFMAs run on the bf16 matrix cores, which do NOT share lanes with the fp32
            // VALU work of the other phases, and all 5 token tiles are cheap enough to run padded.
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                fresh();
                f4 acc[2][kNT];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    const f4 bc = wload4(wrsrc(a.W->bch), chw * 4, (l * kD + 16 * (2 * p + c2)) * 4);
#pragma unroll
                    for (int t = 0; t < kNT; ++t) acc[c2][t] = bc;
                }
                const wrsrc_t wrh = wrsrc(a.W->wch_hi_img), wrl = wrsrc(a.W->wch_lo_img);
                const int wsb = (((l * kWaves + w) * 2 + p) * 16) * 2 * 1024;
                const __bf16* Uh = reinterpret_cast<const __bf16*>(U);
                const __bf16* Ul = Uh + R * kUStride;
                int rofs[kNT];
#pragma unroll
                for (int t = 0; t < kNT; ++t) rofs[t] = rowc_of(t) * kUStride + 8 * g;
                bf8 Ahn[2], Aln[2];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) { Ahn[c2] = wload8h(wrh, lane * 16, wsb + c2 * 1024); Aln[c2] = wload8h(wrl, lane * 16, wsb + c2 * 1024); }
                if (!LS_ABLATED(a, 1))
#pragma unroll 2
                for (int q = 0; q < 16; ++q) {
                    bf8 Ah[2], Al[2], Bh[kNT], Bl[kNT];
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) { Ah[c2] = Ahn[c2]; Al[c2] = Aln[c2]; }
                    const int qn = (q + 1 < 16) ? q + 1 : 15;
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) {
                        Ahn[c2] = wload8h(wrh, lane * 16, wsb + (qn * 2 + c2) * 1024);
                        Aln[c2] = wload8h(wrl, lane * 16, wsb + (qn * 2 + c2) * 1024);
                    }
#pragma unroll
                    for (int t = 0; t < kNT; ++t) {
                        Bh[t] = *reinterpret_cast<const bf8*>(Uh + rofs[t] + 32 * q);
                        Bl[t] = *reinterpret_cast<const bf8*>(Ul + rofs[t] + 32 * q);
                    }
                    // term-major order: 10 independent accumulators between two MFMAs on the same one
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                        for (int t = 0; t < kNT; ++t)
                            acc[c2][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Al[c2], Bh[t], acc[c2][t], 0, 0, 0);
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                        for (int t = 0; t < kNT; ++t)
                            acc[c2][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[c2], Bl[t], acc[c2][t], 0, 0, 0);
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                        for (int t = 0; t < kNT; ++t)
                            acc[c2][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ah[c2], Bh[t], acc[c2][t], 0, 0, 0);
                }
                fresh();
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                    for (int t = 0; t < kNT; ++t)
                        if (valid_of(t)) {
                            X[2 * p + c2][t] = silu_acc4(acc[c2][t], X[2 * p + c2][t]);
                        }
                if (p == 0) stamp(7 + 8 * l);
            }
        } else if constexpr (PREC == 2) {
            // ---- split-fp32, -DLS_SPLIT_SHARED=0 (the earlier form, built for A/B only): the same arithmetic as above, but the operand
            // stays fp32 in LDS, all R rows at once, and each B fragment is
            // split in registers after its ds_read (split3_bf16, 44 VALU per 8 values) -- by every wave, for both p: 16 times per
            // value.  The terms kept (kSplitA / kSplitB,
            // ls_step_common.h) are accumulated smallest first so hi.hi lands last.  All 5 token tiles run on v_mfma_f32_16x16x32_bf16 (pad rows read the clamped last row, their
            // outputs are dropped), no ragged-row VALU path: the bf16 MFMAs leave the fp32 lanes to the split.
            // Non-finite operands: Inf - Inf residuals are NaN, so an Inf in u or W' gives NaN (the fp32 MFMA may give Inf).
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                fresh();
                f4 acc[2][kNT];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    const f4 bc = wload4(wrsrc(a.W->bch), chw * 4, (l * kD + 16 * (2 * p + c2)) * 4);
#pragma unroll
                    for (int t = 0; t < kNT; ++t) acc[c2][t] = bc;
                }
                const wrsrc_t wr0 = wrsrc(a.W->wch_hi_img), wr1 = wrsrc(a.W->wch_lo_img), wr2 = wrsrc(a.W->wch_lo2_img);
                const int wsb = (((l * kWaves + w) * 2 + p) * 16) * 2 * 1024;
                typedef const __attribute__((address_space(3))) f4* ldsp4;
                ldsp4 ub[kNT];                            // lane (token, g) reads k = 32q + 8g .. +7 of its (clamped) row
#pragma unroll
                for (int t = 0; t < kNT; ++t) ub[t] = (ldsp4)(U + rowc_of(t) * kUStride + 8 * g);
                bf8 An[3][2];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) {
                    An[0][c2] = wload8h(wr0, lane * 16, wsb + c2 * 1024);
                    An[1][c2] = wload8h(wr1, lane * 16, wsb + c2 * 1024);
                    An[2][c2] = wload8h(wr2, lane * 16, wsb + c2 * 1024);
                }
                if (!LS_ABLATED(a, 1))
#pragma unroll 1
                for (int q = 0; q < 16; ++q) {
                    bf8 A[3][2];
#pragma unroll
                    for (int s = 0; s < 3; ++s)
#pragma unroll
                        for (int c2 = 0; c2 < 2; ++c2) A[s][c2] = An[s][c2];
                    const int qn = (q + 1 < 16) ? q + 1 : 15;
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) {
                        An[0][c2] = wload8h(wr0, lane * 16, wsb + (qn * 2 + c2) * 1024);
                        An[1][c2] = wload8h(wr1, lane * 16, wsb + (qn * 2 + c2) * 1024);
                        An[2][c2] = wload8h(wr2, lane * 16, wsb + (qn * 2 + c2) * 1024);
                    }
#pragma unroll
                    for (int t = 0; t < kNT; ++t) {
                        bf8 B[3];
                        split3_bf16(ub[t][8 * q], ub[t][8 * q + 1], B[0], B[1], B[2]);
#pragma unroll
                        for (int i = 0; i < kSplitTerms; ++i)
#pragma unroll
                            for (int c2 = 0; c2 < 2; ++c2)
                                acc[c2][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[kSplitA[i]][c2], B[kSplitB[i]], acc[c2][t], 0, 0, 0);
                    }
                }
                fresh();
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                    for (int t = 0; t < kNT; ++t)
                        if (valid_of(t)) X[2 * p + c2][t] = silu_acc4(acc[c2][t], X[2 * p + c2][t]);
                if (p == 0) stamp(7 + 8 * l);
            }
        } else {
        // Rows 64..R-1 (6 of the 16 rows of tile 4) would waste 62 % of a fifth MFMA tile = 20 % of all channel-mix
        // MFMAs.  They are computed instead on the VALU pipe, in the shadow of the MFMAs of tiles 0..3, from the
        // same A-operand registers: lane (n, g) accumulates W[n][k(g)] * U[row][k(g)] over its k subset, the four
        // lane groups are summed with two cross-lane adds, and a 6 KB per-wave LDS patch turns [channel-lane][row]
        // into the residual layout [row-lane][channel-reg].
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            fresh();
            f4 acc[2][kFullTiles];
            float racc[2][NRV];
            f4 racc4[2][NRG];
            f4 bcv[2];                                    // Linear bias (+ W.beta of LN2); kept for the ragged rows' epilogue
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                const f4 bc = wload4(wrsrc(a.W->bch), chw * 4, (l * kD + 16 * (2 * p + c2)) * 4);
                bcv[c2] = bc;
#pragma unroll
                for (int t = 0; t < kFullTiles; ++t) acc[c2][t] = bc;
#pragma unroll
                for (int r = 0; r < NRV; ++r) racc[c2][r] = 0.f;
#pragma unroll
                for (int r = 0; r < NRG; ++r) racc4[c2][r] = (f4){0.f, 0.f, 0.f, 0.f};
            }
            // W fragments through a buffer descriptor (ls_step_common.h: 3.7 instead of 16.8 matrix-pipe cycles per load; same-box A/B
            // of this loop alone, TED B = 512: 1.4364 -> 1.4182 ms per step)
            const wrsrc_t wrs = wrsrc(a.W->wch_img);
            const int wsb = (((l * kWaves + w) * 2 + p) * 32) * 2 * 1024;       // this wave's slice of the image, bytes (wave-uniform)
            // Operand addresses: three 32-bit LDS bases made opaque to the compiler, everything else in the 16-bit offset field of the
            // ds_read (tiles 0-1 off `ub0`, tiles 2-3 off `ub2` = + 32 rows, the ragged rows off `ur`; + 64 B per k block).  Left to
            // itself hipcc keeps ONE base and rebuilds every address beyond 64 KB with a v_add_u32 in front of its read -- 9 per k block,
            // 576 per layer and wave, 2.5 matrix-pipe cycles each.
            typedef const __attribute__((address_space(3))) float* ldsp;
            typedef const __attribute__((address_space(3))) f4* ldsp4;
            ldsp ub0 = (ldsp)(U + s16 * kUStride + 4 * g);                // tile t: + 16*t*kUStride
            ldsp ub2 = ub0 + 32 * kUStride;
            // VALU path: remainder row r at + r*kUStride (all lanes the same row); MFMA path: lane's row (lane&3) of group rg at + 4*rg*kUStride
            ldsp ur = (ldsp)(U + (16 * kFullTiles + (kRemMfma ? (lane & 3) : 0)) * kUStride + 4 * g);
            asm volatile("" : "+v"(ub0), "+v"(ub2), "+v"(ur));
            f4 An[2];
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) An[c2] = wload4(wrs, lane * 16, wsb + c2 * 1024);
            if (!LS_ABLATED(a, 1))
#pragma unroll 2
            for (int q = 0; q < 32; ++q) {
                f4 A[2], Bv[kFullTiles], Ur[kRemMfma ? NRG : NRV];
#pragma unroll
                for (int c2 = 0; c2 < 2; ++c2) A[c2] = An[c2];
                {
                    const int qn = (q + 1 < 32) ? q + 1 : 31;       // branch-free prefetch (last one re-reads q=31)
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) An[c2] = wload4(wrs, lane * 16, wsb + (qn * 2 + c2) * 1024);
                }
#pragma unroll
                for (int t = 0; t < kFullTiles; ++t)
                    Bv[t] = *(ldsp4)((t < 2 ? ub0 : ub2) + 16 * (t & 1) * kUStride + 16 * q);
#pragma unroll
                for (int r = 0; r < (kRemMfma ? NRG : NRV); ++r)
                    Ur[r] = *(ldsp4)(ur + (kRemMfma ? 4 : 1) * r * kUStride + 16 * q);
                // Per k: [8 MFMAs][2*NREM scalar FMAs], order pinned.  A/B-tested on MI355X (tools/ab_variants.py, ms/step
                // at B=512): this 1.513 | [32 MFMA][8*NREM FMA] 1.526 | compiler's own order 1.627 (it hoists the FMAs
                // next to their ds_reads and stalls) | fine 2:3 interleave 1.646 | 5th MFMA tile instead of FMAs 1.645.
                // fp32 MFMA and fp32 VALU share the SIMD's FMA lanes on gfx950 (removing the FMAs saves exactly their
                // issue time), so the gain is the padding saved (6 rows of work instead of 16), not overlap; v_pk_fma_f32,
                // v_mfma_f32_4x4x1_16b (16 cycles/issue: 1.518 with rows padded to 8)
                // and s_setprio alternation between the two waves of a SIMD were measured and do not help.
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2)
#pragma unroll
                        for (int t = 0; t < kFullTiles; ++t) acc[c2][t] = MFMA(A[c2][j], Bv[t][j], acc[c2][t]);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int c2 = 0; c2 < 2; ++c2) {
                        if constexpr (kRemMfma) {
                            // block (g, n>>2) = {4 channels} x {4 rows} over the lane's own k subset: the A operand is the
                            // same register the 16x16x4 MFMAs use
#pragma unroll
                            for (int r = 0; r < NRG; ++r)
                                racc4[c2][r] = __builtin_amdgcn_mfma_f32_4x4x1f32(A[c2][j], Ur[r][j], racc4[c2][r], 0, 0, 0);
                        } else {
#pragma unroll
                            for (int r = 0; r < NRV; ++r) racc[c2][r] = fmaf(A[c2][j], Ur[r][j], racc[c2][r]);
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            fresh();
            // remainder rows: sum the 4 k-subsets, then [channel-lane][row] -> [row-lane][channel-reg] through LDS
            float* rem = REM + w * (2 * NREM * 16);
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                if constexpr (kRemMfma) {
#pragma unroll
                    for (int r = 0; r < NRG; ++r) {
                        f4 v = racc4[c2][r];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            v[i] = xor32_sum(xor16_sum(v[i]));
                        }
                        // lane (block = lane>>2, row = lane&3) holds channels 4*(s16>>2)..+3 of row 4r + (lane&3)
                        if (g == 0) *reinterpret_cast<f4*>(&rem[(c2 * NREM + 4 * r + (lane & 3)) * 16 + 4 * (s16 >> 2)]) = v;
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < NRV; ++r) {
                        float v = racc[c2][r];
                        v = xor32_sum(xor16_sum(v));
                        if (g == 0) rem[(c2 * NREM + r) * 16 + s16] = v;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int c2 = 0; c2 < 2; ++c2) {
                const int cb = 2 * p + c2;
                const f4 bc = bcv[c2];
#pragma unroll
                for (int t = 0; t < kFullTiles; ++t) {
                    if constexpr (TRAIN) {                // pre-activation of the channel-mixing linear
                        const int gr = grow_of(t);
                        if (gr >= 0 && !LS_TRAIN_ABL) LS_TRAIN_ST(reinterpret_cast<f4*>(a.tr_a2 + ((size_t)l * a.tr_B * S + gr) * kD + chw + 16 * cb), acc[c2][t]);
                    }
                    X[cb][t] = silu_acc4(acc[c2][t], X[cb][t]);
                }
                if (s16 < NREM) {
                    const f4 rv = *reinterpret_cast<const f4*>(&rem[(c2 * NREM + s16) * 16 + 4 * g]);
                    if constexpr (TRAIN) {
                        const int gr = grow_of(kFullTiles);
                        if (gr >= 0 && !LS_TRAIN_ABL) LS_TRAIN_ST(reinterpret_cast<f4*>(a.tr_a2 + ((size_t)l * a.tr_B * S + gr) * kD + chw + 16 * cb), rv + bc);
                    }
                    X[cb][kFullTiles] = silu_acc4(rv + bc, X[cb][kFullTiles]);
                }
            }
            __builtin_amdgcn_wave_barrier();
            if (p == 0) stamp(7 + 8 * l);
        }
        }
        stamp(9 + 8 * l);
        dump_trace(l + 1);
    }

    if constexpr (TRAIN) {         // poseFinal, the losses and everything else downstream are batch-level kernels
        store_rows(a.tr_xout, 0);
        return;
    }
    // ================= OutputProcess.poseFinal (RAG.py:205-211) ====================================
    stamp(2 + 8 * a.layers);
    fresh();
    __syncthreads();                       // every wave is done reading the last LN2 operand: U is free
    constexpr bool kOutFromRegs = (NOB <= 2);
    constexpr int OROWS = kOutFromRegs ? kWaves * R : R;      // rows of the OUT / partial buffer overlaid on U
    static_assert(OROWS * OSTR <= R * kUStride, "OUT overlay must fit the operand buffer");
    float* OUT = U;
    if constexpr (kOutFromRegs) {
        // Narrow output (TED, 27 features): every wave contracts over ITS OWN 64 channels straight from the residual
        // registers (the residual layout is a valid MFMA B operand; the weight image carries the matching k
        // permutation), writes a [R][32] partial, and the 8 partials are summed in the epilogue below.  No x -> LDS
        // round trip, no latency-bound k loop on two waves.
        f4 acc[NOB][kNT];
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
            for (int t = 0; t < kNT; ++t) acc[ob][t] = (f4){0.f, 0.f, 0.f, 0.f};
        const wrsrc_t wrs = wrsrc(a.W->wout_reg_img);
        const int wsb = w * NOB * kCB * 1024;
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
            for (int cb = 0; cb < kCB; ++cb) {
                const f4 A = wload4(wrs, lane * 16, wsb + (ob * kCB + cb) * 1024);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int t = 0; t < kNT; ++t) acc[ob][t] = MFMA(A[j], X[cb][t][j], acc[ob][t]);
            }
        stamp(3 + 8 * a.layers);
#pragma unroll
        for (int ob = 0; ob < NOB; ++ob)
#pragma unroll
            for (int t = 0; t < kNT; ++t)
                if (valid_of(t))
                    *reinterpret_cast<f4*>(&OUT[(w * R + row_of(t)) * OSTR + 16 * ob + 4 * g]) = acc[ob][t];
    } else {
#pragma unroll
        for (int t = 0; t < kNT; ++t)
            if (valid_of(t))
#pragma unroll
                for (int cb = 0; cb < kCB; ++cb)
                    *reinterpret_cast<f4*>(&U[row_of(t) * kUStride + chw + 16 * cb]) = X[cb][t];
        __syncthreads();
        f4 res[MAXU];
#pragma unroll
        for (int i = 0; i < MAXU; ++i) {
            const int u = w + kWaves * i;      // wave-uniform
            res[i] = (f4){0.f, 0.f, 0.f, 0.f};
            if (u < NU) {
                const int ob = u / kNT, t = u - ob * kNT;
                const int rc = (16 * t + s16 < R) ? 16 * t + s16 : R - 1;
                const wrsrc_t wrs = wrsrc(a.W->wout_img);
                const int wsb = ob * 32 * 1024;
                const float* up = &U[rc * kUStride + 4 * g];
                f4 a0 = (f4){0.f, 0.f, 0.f, 0.f}, a1 = a0;
                // eight weight fragments in flight ahead of their use (one load per 4 MFMAs: with four in flight, as `unroll 4` left
                // it, the L2 round trip was exposed -- in-kernel stamps: 154 k cycles for 98 k of MFMA issue at BEAT's 90 units)
                constexpr int QB = 8;
                f4 An[QB];
#pragma unroll
                for (int k = 0; k < QB; ++k) An[k] = wload4(wrs, lane * 16, wsb + k * 1024);
#pragma unroll 1
                for (int q0 = 0; q0 < 32; q0 += QB) {
                    f4 A[QB];
#pragma unroll
                    for (int k = 0; k < QB; ++k) A[k] = An[k];
                    const int qn = q0 + QB < 32 ? q0 + QB : q0;
#pragma unroll
                    for (int k = 0; k < QB; ++k) An[k] = wload4(wrs, lane * 16, wsb + (qn + k) * 1024);
#pragma unroll
                    for (int k = 0; k < QB; ++k) {
                        const f4 Bv = *reinterpret_cast<const f4*>(up + 16 * (q0 + k));
                        a0 = MFMA(A[k][0], Bv[0], a0);
                        a1 = MFMA(A[k][1], Bv[1], a1);
                        a0 = MFMA(A[k][2], Bv[2], a0);
                        a1 = MFMA(A[k][3], Bv[3], a1);
                    }
                }
                res[i] = a0 + a1;
            }
        }
        stamp(3 + 8 * a.layers);
        fresh();
        __syncthreads();                       // operand buffer is free: overlay OUT[row][c]
#pragma unroll
        for (int i = 0; i < MAXU; ++i) {
            const int u = w + kWaves * i;
            if (u < NU) {
                const int ob = u / kNT, t = u - ob * kNT;
                const int r = 16 * t + s16;
                if (r < R) *reinterpret_cast<f4*>(&OUT[r * OSTR + 16 * ob + 4 * g]) = res[i];
            }
        }
    }
    __syncthreads();
    auto out_at = [&](int r, int c) {
        if constexpr (kOutFromRegs) {
            float v = 0.f;
#pragma unroll
            for (int ww = 0; ww < kWaves; ++ww) v += OUT[(ww * R + r) * OSTR + c];
            return v;
        } else {
            return OUT[r * OSTR + c];
        }
    };

    // ====== CFG lerp (cfg_sampler.py:31) + posterior / DDIM update (gaussian_diffusion.py:260-282,
    //        507-558, 745-798), written back in the internal [B][T][JF] layout ======================
    {
        const float sc = (!PAIR && a.scale) ? a.scale[b] : 1.0f;
        const unsigned long long goff = a.call ? a.call->sample_offset : 0ull;
        for (int idx0 = tid; idx0 < (PAIR ? 2 : 1) * kT * JF; idx0 += 512) {
            const int sq = (PAIR && idx0 >= kT * JF) ? 1 : 0;
            const int idx = idx0 - sq * kT * JF;
            const int smp = PAIR ? 2 * b + sq : b;
            if (PAIR && smp >= a.batch) break;
            const size_t base = (size_t)smp * kT * JF;
            const unsigned long long gidx = goff + (unsigned long long)smp;
            const int f = idx / JF, c = idx - f * JF;
            const float bo = g1(a.W->bout)[c];
            float x0;
            if constexpr (PAIR) {
                x0 = out_at(sq * S + NPRE + f, c) + bo;           // scale == 1: the CFG combination is the cond output
            } else {
                const float oc = out_at(NPRE + f, c) + bo;
                const float ou = out_at(S + NPRE + f, c) + bo;
                if (a.fwd_c) a.fwd_c[base + idx] = oc;
                if (a.fwd_u) a.fwd_u[base + idx] = ou;
                x0 = ou + sc * (oc - ou);
            }
            if (a.clip_denoised) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
            if (a.x0_out) a.x0_out[base + idx] = x0;
            if (a.sampler != kNone) {
                const float xt = a.x_in[base + idx];
                float nz = 0.f;
                if (a.t_nonzero) {
                    if (a.noise) {
                        const size_t bn = a.const_noise ? 0 : (size_t)smp;
                        nz = a.noise[(bn * JF + c) * kT + f];
                    } else {
                        nz = philox_normal(a.call, gidx, a.step_id, 3u, (unsigned)(c * kT + f));
                    }
                }
                float xn;
                if (a.sampler == kDDPM) {
                    xn = a.c0 * x0 + a.c1 * xt;
                    if (a.t_nonzero) xn += a.c2 * nz;
                } else {
                    const float eps = (a.c0 * xt - x0) / a.c1;
                    xn = x0 * a.c2 + a.c3 * eps;
                    if (a.t_nonzero) xn += a.c4 * nz;
                }
                a.x_out[base + idx] = xn;
            }
        }
    }
    stamp(4 + 8 * a.layers);
}

}  // namespace ls
