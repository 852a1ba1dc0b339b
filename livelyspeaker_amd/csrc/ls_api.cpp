// Host side of the C-ABI declared in include/ls_hip.h: the handle's life cycle, the commit that uploads the weight images, the schedule,
// once-per-call preparation and the small utility exports.  The images themselves (MFMA operand order) are built on the host by
// ls_weights.cpp; the step plan and its launchers are in ls_plan.cpp, the diffusion loop and the single-step entries in ls_sample.cpp,
// the long-form entries (chained windows) in ls_chain_api.cpp; ls_handle.h holds what they share.  No torch types here; livelyspeaker_amd/_lib.py binds these symbols with ctypes.
#include "ls_handle.h"
#include "ls_weights.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace ls;

namespace {

// ls_commit_weights: resolve every key (a faulty one returns before anything is uploaded), build the host images the model needs
// (ls_weights.cpp), upload them, fill DevWeights, wait once.  A 34-frame model carries both forms: the fused kernels (one workgroup per
// sample) and the batch-level kernels small batches run on.  (Kernel comments that name build_fused_images or build_shared_weights mean
// fused_images and the once-per-call group below; each layout is stated once, in ls_weights.cpp.)
int build_images(ls_handle* h) {
    const WeightDims d{h->cfg.layers, h->S, h->R, h->JF, h->KIN, h->KPP, h->JFP, h->MK, h->KXQ, h->NOB, h->cfg.n_speakers, h->cfg.n_emotions,
                       h->fused, !h->fused && mix_supports(h->S)};
    Weights w;
    std::string msg;
    if (const int rc = resolve_weights(h->w, d, w, msg)) return fail(h, rc, "%s", msg.c_str());

    // one upload: a handle buffer and the host bytes that go into it (every source lives until the closing wait)
    struct Up { DevBuf* buf; const void* src; size_t bytes; };
    std::vector<Up> ups;
    auto up = [&](DevBuf& b, const auto& v) { ups.push_back({&b, v.data(), v.size() * sizeof(v[0])}); };
    auto raw = [&](DevBuf& b, const float* p, size_t n) { ups.push_back({&b, p, n * sizeof(float)}); };
    const LongImages lg = long_images(w, d);
    const Ln2Fold f = fold_ln2(w, d);
    up(h->lw_wt, lg.lw_wt); up(h->lw_bt, lg.lw_bt); up(h->lw_wc, lg.lw_wc); up(h->lw_bc, lg.lw_bc); up(h->lw_winx, lg.lw_winx); up(h->lw_wout, lg.lw_wout);
    up(h->ln1a, lg.ln1a); up(h->ln1b, lg.ln1b); up(h->ln2a, lg.ln2a); up(h->ln2b, lg.ln2b);
    Img wtp;
    if (d.S <= 160) {       // the fused token-mixing kernel's operand, its token axis padded to 48 (three tiles: the reference's 35 / 36 tokens)
                            // or to 160, and LayerNorm 2 folded around the channel-mixing product (ls_long.hip)
        h->tokpad = d.S <= 48 ? 48 : 160;
        wtp = lw_wtp(w, d, h->tokpad);
        up(h->lw_wtp, wtp); up(h->lw_wcf, f.w); up(h->lw_bcf, f.b); up(h->lw_wsum, f.wsum);
    } else {
        h->lw_wtp.release();
    }
    const MixerImages mx = d.mixer ? mixer_images(w, f, d) : MixerImages{};
    if (d.mixer) { up(h->mx_wtok, mx.mx_wtok); up(h->mx_wch, mx.mx_wch); }
    h->mx_npt = d.mixer && (d.JF + 15) / 16 <= 20 ? (d.JF + 15) / 16 : 0;     // poseFinal runs inside the mixer, or stays a GEMM (0)
    const Img wpose = mx_wpose(w, d, h->mx_npt);
    if (h->mx_npt > 0) up(h->mx_wpose, wpose);
    const FusedImages fu = d.fused ? fused_images(w, f, d) : FusedImages{};
    if (d.fused) {
        up(h->wch_hi_img, fu.wch_hi_img); up(h->wch_lo_img, fu.wch_lo_img); up(h->wch_lo2_img, fu.wch_lo2_img); up(h->ww_hi_img, fu.ww_hi_img);
        up(h->ww_lo_img, fu.ww_lo_img); up(h->wtok1_hi_img, fu.wtok1_hi_img); up(h->wtok1_lo_img, fu.wtok1_lo_img);
        up(h->wch_img, fu.wch_img); up(h->bch, f.b); up(h->wtail, fu.wtail); up(h->ww_img, fu.ww_img); up(h->wtok1_img, fu.wtok1_img);
        up(h->btok_rows, fu.btok_rows); up(h->winx_img, fu.winx_img); up(h->wout_img, fu.wout_img); up(h->wout_reg_img, fu.wout_reg_img); up(h->bout, fu.bout);
    } else {
        raw(h->bout, w.b_out, d.JF);
    }
    // once-per-call stage (audio encoder, static input projection, speaker style, timestep embedder): the same for both paths
    const CallImages ca = call_images(w, d);
    const size_t D = kD;
    raw(h->win_bias, w.b_in, D); up(h->win_pre, ca.win_pre); up(h->win_aud, ca.win_aud);
    for (int i = 0; i < 4; ++i) {
        raw(h->conv_w[i], w.conv_w[i], (size_t)kConvCout[i] * kConvCin[i] * 15); raw(h->conv_b[i], w.conv_b[i], kConvCout[i]);
        if (i > 0) up(h->conv_img[i], ca.conv_img[i]);
    }
    raw(h->spk_emb, w.spk_emb, (size_t)d.n_speakers * 256); up(h->ml_w, ca.ml_w); up(h->ml_b, ca.ml_b);
    raw(h->te_w0, w.te_w0, D * D); raw(h->te_b0, w.te_b0, D); raw(h->te_w2, w.te_w2, D * D); raw(h->te_b2, w.te_b2, D);
    if (d.n_emotions > 0) raw(h->emo_emb, w.emo_emb, (size_t)d.n_emotions * D);
    const Img pe = pe_table(kPeRows, kD);      // PositionalEncoding buffer (mlp_module.py:104-116), fp32 like the torch buffer
    up(h->pe, pe);

    int rc = LS_OK;
    for (const Up& u : ups)
        if ((rc = ingest(h, *u.buf, u.src, u.bytes, 0)) != LS_OK) break;
    if (rc == LS_OK && d.fused) {
        DevWeights dw{};
        auto u16 = [](const DevBuf& b) { return static_cast<const unsigned short*>(b.p); };
        dw.wch_img = h->wch_img.f(); dw.bch = h->bch.f(); dw.wsum = h->lw_wsum.f();
        dw.wch_hi_img = u16(h->wch_hi_img); dw.wch_lo_img = u16(h->wch_lo_img); dw.wch_lo2_img = u16(h->wch_lo2_img);
        dw.ww_hi_img = u16(h->ww_hi_img); dw.ww_lo_img = u16(h->ww_lo_img); dw.wtok1_hi_img = u16(h->wtok1_hi_img); dw.wtok1_lo_img = u16(h->wtok1_lo_img);
        dw.ln1a = h->ln1a.f(); dw.ln1b = h->ln1b.f(); dw.ln2a = h->ln2a.f(); dw.ln2b = h->ln2b.f();
        dw.ww_img = h->ww_img.f(); dw.wtok1_img = h->wtok1_img.f(); dw.btok_rows = h->btok_rows.f(); dw.wtail = h->wtail.f();
        dw.winx_img = h->winx_img.f(); dw.wout_img = h->wout_img.f(); dw.wout_reg_img = h->wout_reg_img.f(); dw.bout = h->bout.f();
        rc = ingest(h, h->devw, &dw, sizeof dw, 0);
    }
    const hipError_t e = hipStreamSynchronize(h->stream);      // the copies read host memory that dies with this call: wait on every exit
    if (rc != LS_OK) return rc;
    HIPCHK(h, e);
    return LS_OK;
}

}  // namespace

// temb[i] = time_embed(pe[timestep_map[i]])  (TimestepEmbedder, mlp_module.py:123-136), one row per schedule index
int ls::build_temb_rows(ls_handle* h, const long long* idx_dev, int n, DevBuf& tmp, DevBuf& out) {
    HIPCHK(h, tmp.ensure((size_t)2 * n * kD * sizeof(float)));
    HIPCHK(h, out.ensure((size_t)n * kD * sizeof(float)));
    float* rows = tmp.f();
    float* hid = tmp.f() + (size_t)n * kD;
    HIPCHK(h, launch_gather_rows(h->pe.f(), reinterpret_cast<const int64_t*>(idx_dev), rows, n, kD, kPeRows, h->stream));
    HIPCHK(h, launch_gemm_nt(rows, kD, h->te_w0.f(), kD, h->te_b0.f(), nullptr, 0, hid, kD, n, kD, kD, 1, h->stream));
    HIPCHK(h, launch_gemm_nt(hid, kD, h->te_w2.f(), kD, h->te_b2.f(), nullptr, 0, out.f(), kD, n, kD, kD, 0, h->stream));
    return LS_OK;
}

int ls::ensure_temb_table(ls_handle* h) {
    if (h->temb_valid) return LS_OK;
    int rc = upload(h, h->tmap_dev, h->tmap.data(), h->tmap.size() * sizeof(long long));
    if (rc != LS_OK) return rc;
    rc = build_temb_rows(h, static_cast<const long long*>(h->tmap_dev.p), h->n_steps, h->temb_tmp, h->temb);
    if (rc != LS_OK) return rc;
    h->temb_valid = true;
    return LS_OK;
}

// prepare_ms of an ls_prepare_async whose work has finished (called behind every stream synchronisation; `block`: wait for it)
void ls::resolve_prepare_timing(ls_handle* h, bool block) {
    if (!h->prepare_pending) return;
    if (block ? hipEventSynchronize(h->ev[5]) != hipSuccess : hipEventQuery(h->ev[5]) != hipSuccess) return;
    if (hipEventElapsedTime(&h->timing.prepare_ms, h->ev[4], h->ev[5]) == hipSuccess) h->prepare_pending = false;
}

// guidance scale 1 for the whole batch (what the reference's callers run: test_RAG_ted.py:183): out_u + 1 * (out_c - out_u) is out_c,
// so the sampling loop may skip the uncond pass (ls_sample_args.two_pass_always keeps both).  `scale`: the caller's [B] (host unless od)
int ls::prepare_scale(ls_handle* h, const float* scale, int B, int od, int* leading_ones) {
    hipStream_t st = h->stream;
    std::vector<float> sc((size_t)B);
    if (od) {           // read back the ingested copy on the handle's own stream: ordered behind the caller's stream (ls_stream_order)
        HIPCHK(h, hipMemcpyAsync(sc.data(), h->scale.p, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
    } else {
        memcpy(sc.data(), scale, (size_t)B * sizeof(float));
    }
    h->all_scale_one = true;
    for (float v : sc) if (v != 1.0f) { h->all_scale_one = false; break; }
    if (leading_ones) { int n = 0; while (n < B && sc[(size_t)n] == 1.0f) ++n; *leading_ones = n; }
    return LS_OK;
}

// WavEncoder (audio_enc.py:6-25) over B clips [B][audio_len] at `in`: conv -> [IN + LReLU fused into the next conv's staging] x3 -> conv;
// the audio features are left in c4 [B][256][T]
int ls::run_wav_encoder(ls_handle* h, const float* in, int B) {
    hipStream_t st = h->stream;
    const int* Lc = h->convL;
    DevBuf* outs[4] = {&h->c1, &h->c2, &h->c3, &h->c4};
    DevBuf* stats[3] = {&h->st1, &h->st2, &h->st3};
    const float* in_stats = nullptr;
    // every conv kernel also produces the InstanceNorm statistics of its own output (partials -> k_stats_merge), so the
    // activations are written once and read once
    {
        size_t need = 0;
        for (int i = 0; i < 3; ++i) {
            const size_t n = (size_t)B * kConvCout[i] * ((Lc[i + 1] + 63) / 64) * 4 * 3;
            if (n > need) need = n;
        }
        HIPCHK(h, h->spart.ensure(need * sizeof(float)));
    }
    for (int i = 0; i < 4; ++i) {
        HIPCHK(h, outs[i]->ensure((size_t)B * kConvCout[i] * Lc[i + 1] * sizeof(float)));
        float* ostats = nullptr;
        if (i < 3) {
            HIPCHK(h, stats[i]->ensure((size_t)B * kConvCout[i] * 2 * sizeof(float)));
            ostats = stats[i]->f();
        }
        if (i == 0)     // Cin = 1: a 15-tap FIR per channel, bound by the output write
            HIPCHK(h, launch_conv1_fwd(in, h->conv_w[0].f(), h->conv_b[0].f(), outs[0]->f(), ostats, h->spart.f(), B, Lc[0], Lc[1], kConvPad[0], st));
        else
            HIPCHK(h, launch_conv1d_mfma(in, in_stats, h->conv_img[i].f(), h->conv_b[i].f(), outs[i]->f(), ostats, h->spart.f(), B, kConvCin[i],
                                         kConvCout[i], Lc[i], Lc[i + 1], st));
        in_stats = ostats;
        in = outs[i]->f();
    }
    return LS_OK;
}

// speaker style (RAG.py:116-119): z = Embedding[vid]; mu, logvar = Linear(z); std = exp(0.5*logvar)
int ls::prepare_style(ls_handle* h, int B) {
    hipStream_t st = h->stream;
    HIPCHK(h, h->z.ensure((size_t)B * 256 * sizeof(float)));
    HIPCHK(h, h->z_mu.ensure((size_t)B * kD * sizeof(float)));
    HIPCHK(h, h->z_logvar.ensure((size_t)B * kD * sizeof(float)));
    HIPCHK(h, h->z_std.ensure((size_t)B * kD * sizeof(float)));
    HIPCHK(h, launch_gather_rows(h->spk_emb.f(), static_cast<const int64_t*>(h->vid.p), h->z.f(), B, 256, h->cfg.n_speakers, st));
    HIPCHK(h, h->z_ml.ensure((size_t)B * 2 * kD * sizeof(float)));
    HIPCHK(h, launch_gemm_nt(h->z.f(), 256, h->ml_w.f(), 256, h->ml_b.f(), nullptr, 0, h->z_ml.f(), 2 * kD, B, 2 * kD, 256, 0, st));
    HIPCHK(h, launch_split_style(h->z_ml.f(), h->z_mu.f(), h->z_logvar.f(), h->z_std.f(), B, st));
    return LS_OK;
}

// the step plan of a batch of B clips and the workspaces of its kernel families (every one held by address in a captured loop)
int ls::prepare_plan(ls_handle* h, int B) {
    { const int keepB = h->B; h->B = B; decide_path(h); h->B = keepB; }
    return plan_workspaces(h);
}

int ls::plan_workspaces(ls_handle* h) {
    hipStream_t st = h->stream;
    int rc;
    if (seg_n(h, 2) > 0) {      // exchange workspaces of the sample-split kernel: one launch's worth of (sample, pass) groups
        const int nco = seg_n(h, 2);
        int gcap = h->coop_groups_max;                  // the most groups any slicing keeps resident (LS_COOP_GROUPS caps all of them in -DLS_DEBUG builds)
        if (gcap == coop_cap(h->n_cu, 1))
            for (int ncb = 2; ncb <= 4; ncb *= 2) if (coop_cap(h->n_cu, ncb) > gcap) gcap = coop_cap(h->n_cu, ncb);
        const int groups = 2 * nco < gcap ? 2 * nco : gcap;
        bool fresh = false;
        if ((rc = ensure_pinned(h, h->co_x, (size_t)groups * 36 * kD * sizeof(float), &fresh)) != LS_OK) return rc;
        if (fresh) HIPCHK(h, hipMemsetAsync(h->co_x.p, 0, h->co_x.bytes, st));     // rows a 35-row pass never writes are pulled into LDS (never read)
        if ((rc = ensure_pinned(h, h->co_part, (size_t)groups * 8 * 36 * (size_t)h->NOB * 16 * sizeof(float))) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->co_gran, (size_t)groups * 2 * 36 * 8 * 2 * sizeof(unsigned long long))) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->co_flag, (size_t)groups * 16 * sizeof(unsigned long long))) != LS_OK) return rc;
        h->coop_groups = groups;
    }
    if (seg_n(h, 3) > 0) {      // CFG hand-off of the one-pass-per-workgroup kernel: each pass's output, one ticket word per sample
        const int npa = seg_n(h, 3);
        if ((rc = ensure_pinned(h, h->pa_out, (size_t)npa * 2 * h->T * h->JF * sizeof(float))) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->pa_cnt, (size_t)npa * sizeof(unsigned))) != LS_OK) return rc;
        HIPCHK(h, hipMemsetAsync(h->pa_cnt.p, 0, h->pa_cnt.bytes, st));
        h->pass_n = npa;
    }
    if (seg_n(h, 1) > 0) {      // workspaces of the batch-level path: token sequences of both passes (two buffers), row partials, poseFinal output
        const size_t nlo = seg_n(h, 1);
        const size_t rows = ((size_t)2 * nlo * h->S + 127) / 128 * 128;      // whole 128-row GEMM tiles (the fused channel-mixing product runs over the pad rows too)
        const size_t mpad = ((size_t)nlo * h->T + 127) / 128 * 128;           // x_t projection on whole 128-row tiles (k_long_padx)
        bool fresh1 = false, fresh2 = false;
        if ((rc = ensure_pinned(h, h->lx_proj, mpad * kD * sizeof(float))) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->lx_xpad, mpad * h->JFP * sizeof(float))) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->lx_X, rows * kD * sizeof(float), &fresh1)) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->lx_U, rows * kD * sizeof(float), &fresh2)) != LS_OK) return rc;
        if (fresh1 || fresh2) {                                               // fresh memory: the pad rows must hold finite values (their products are computed and discarded)
            HIPCHK(h, hipMemsetAsync(h->lx_X.p, 0, h->lx_X.bytes, st)); HIPCHK(h, hipMemsetAsync(h->lx_U.p, 0, h->lx_U.bytes, st));
        }
        if ((rc = ensure_pinned(h, h->lx_OUT, rows * (size_t)((h->JF + 127) / 128 * 128) * sizeof(float))) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->lx_part1, rows * 16 * sizeof(float), &fresh1)) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->lx_part2, rows * 16 * sizeof(float), &fresh2)) != LS_OK) return rc;
        if (fresh1 || fresh2) {
            HIPCHK(h, hipMemsetAsync(h->lx_part1.p, 0, h->lx_part1.bytes, st)); HIPCHK(h, hipMemsetAsync(h->lx_part2.p, 0, h->lx_part2.bytes, st));
        }
        // the one-launch mixer (a model whose token count it supports, unless ls_set_path(2) asked for the batch-level kernels): as many
        // (sample, pass) groups per launch as fit the chip with four workgroups each, a multiple of eight (the grid is dealt in sets of eight groups)
        const int was_cap = h->mix_cap;
        h->mix_cap = 0;
        // Measured on MI355X (profiles/r06_mixer_150_frames.md): a mixer launch costs ~0.50 ms however few of its 64 groups are used, the
        // batch-level kernels 0.25 ms + ~13-17 us per clip: `auto` (mode 0) takes the mixer when every launch is at least 7/8 full and the batch
        // is at most three launches (28-32, 60-64, 92-96 clips under CFG); ls_set_path(3) forces it, (2) forces the batch-level kernels.
        bool want_mix = !h->fused && h->mx_wch.p && h->path_mode != 2 && 2 * h->cfg.layers + 2 <= (int)kCoopEpochStride;
        if (want_mix && h->path_mode == 0) {
            const int full = h->n_cu / kMixSlices / 8 * 8, groups = (int)(2 * nlo), last = groups % full;
            want_mix = full >= 8 && groups <= 3 * full && groups >= full * 7 / 8 && (last == 0 || last >= full * 7 / 8);
        }
        if (want_mix) {
            int cap = h->n_cu / kMixSlices / 8 * 8;
            const int need = (int)((2 * nlo + 7) / 8 * 8);
            if (cap > need) cap = need;
            if (cap >= 8) {
                if ((rc = ensure_pinned(h, h->mx_xg, (size_t)cap * 32 * kMixRows * 16 * sizeof(float), &fresh1)) != LS_OK) return rc;
                if ((rc = ensure_pinned(h, h->mx_gran, (size_t)cap * (2 * kMixRows + 1) * kMixSlices * 2 * sizeof(unsigned long long))) != LS_OK) return rc;
                if (fresh1) HIPCHK(h, hipMemsetAsync(h->mx_xg.p, 0, h->mx_xg.bytes, st));       // rows a pass never writes are pulled into LDS (finite, never used)
                // partial poseFinal products of the whole batch: [2 B][4 slices][S][16 npt]
                if (h->mx_npt > 0 && (rc = ensure_pinned(h, h->mx_pout, (size_t)2 * nlo * kMixSlices * h->S * 16 * h->mx_npt * sizeof(float))) != LS_OK) return rc;
                h->mix_cap = cap;
            }
        }
        if (was_cap != h->mix_cap) free_graph(h);
    }
    return LS_OK;
}

extern "C" {

int ls_abi_version(void) { return LS_ABI_VERSION; }

const char* ls_last_error(const ls_handle* h) { return last_error(h); }

int ls_create(const ls_config* cfg, ls_handle** out) {
    if (!cfg || !out) return fail<ls_handle>(nullptr, LS_EINVAL, "ls_create: null argument");
    *out = nullptr;
    if (cfg->latent_dim != kD) return fail<ls_handle>(nullptr, LS_EUNSUPPORTED, "latent_dim must be %d", kD);
    if (cfg->nframes < cfg->n_pre_seq || cfg->nframes < 1 || cfg->nframes > 4096) return fail<ls_handle>(nullptr, LS_EINVAL, "nframes out of range");
    const int JF = cfg->njoints * cfg->nfeats;
    Variant var;
    if (JF == 27 && cfg->n_prefix_tokens == 1) var = kTED;
    else if (JF == 282 && cfg->n_prefix_tokens == 2) var = kBEAT;
    else return fail<ls_handle>(nullptr, LS_EUNSUPPORTED, "unsupported shape: J*F=%d with %d prefix tokens (built: 27/1 TED, 282/2 BEAT)",
                     JF, cfg->n_prefix_tokens);
    if (cfg->layers < 1 || cfg->layers > 64) return fail<ls_handle>(nullptr, LS_EINVAL, "layers out of range");
    if (cfg->n_prefix_tokens == 2 && cfg->n_emotions <= 0) return fail<ls_handle>(nullptr, LS_EINVAL, "BEAT variant needs n_emotions > 0");
    int L = cfg->audio_len;
    int convL[5];
    convL[0] = L;
    for (int i = 0; i < 4; ++i) {
        L = (L + 2 * kConvPad[i] - 15) / kConvStride[i] + 1;
        convL[i + 1] = L;
    }
    if (L != cfg->nframes) return fail<ls_handle>(nullptr, LS_EINVAL, "audio_len %d yields %d audio frames, need %d", cfg->audio_len, L, cfg->nframes);
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail<ls_handle>(nullptr, LS_EHIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));
    ls_handle* h = new ls_handle();
    h->cfg = *cfg;
    {   // chip geometry: the step-time models were measured on 256 CUs; rounds, residency and the throughput-bound terms follow the device
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, cfg->device);
        if (e != hipSuccess) return abandon(h, ls_destroy, fail<ls_handle>(nullptr, LS_EHIP, "hipGetDeviceProperties(%d): %s", cfg->device, hipGetErrorString(e)));
        h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        h->max_thr_cu = prop.maxThreadsPerMultiProcessor;
        h->coop_groups_max = 2 * h->n_cu / 8 < kCoopMaxGroups ? 2 * h->n_cu / 8 : kCoopMaxGroups;       // every slice of a launch must be resident: they wait for each other
        h->timing.n_cus = h->n_cu;
    }
#ifdef LS_DEBUG
    if (const char* ab = getenv("LS_ABLATE")) h->ablate = atoi(ab);
    if (const char* pr = getenv("LS_PROF")) { h->prof_on = true; h->prof_wg = atoi(pr); }
    if (const char* xm = getenv("LS_COOP_XMAP")) h->coop_xmap = atoi(xm);
    if (const char* mp = getenv("LS_MIX_POSE")) h->mix_pose = atoi(mp) != 0;
    if (const char* gm = getenv("LS_COOP_GROUPS")) h->coop_groups_max = atoi(gm);
    if (const char* nc = getenv("LS_COOP_NCB")) h->coop_ncb = atoi(nc) == 2 ? 2 : atoi(nc) == 4 ? 4 : atoi(nc) == 1 ? 1 : 0;
    if (const char* pw = getenv("LS_PASS_WAVES")) h->pass_waves_env = atoi(pw) == 8 ? 8 : atoi(pw) == 4 ? 4 : 0;
#endif
    h->var = var; h->JF = JF; h->T = cfg->nframes;
    h->fused = cfg->nframes == kT;          // the reference's 34 frames: fused step kernel; otherwise the long-sequence path
    h->S = h->T + cfg->n_prefix_tokens; h->R = 2 * h->S; h->MK = (h->R + 3) / 4;
    h->NOB = (JF + 15) / 16; h->KXQ = (JF + 15) / 16; h->JFP = (JF + 31) / 32 * 32;
    h->KIN = 2 * JF + 1 + kAudioFeat; h->KPP = (JF + 1 + 31) / 32 * 32;
    memcpy(h->convL, convL, sizeof convL);
    for (hipStream_t* ps : {&h->stream, &h->copy_stream}) {
        e = hipStreamCreateWithFlags(ps, hipStreamNonBlocking);
        if (e != hipSuccess) return abandon(h, ls_destroy, fail<ls_handle>(nullptr, LS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    }
    std::vector<hipEvent_t*> evs = {&h->ev_cs[0], &h->ev_cd[0], &h->ev_seg[0], &h->ev_cs[1], &h->ev_cd[1], &h->ev_seg[1]};
    for (auto& ev : h->ev) evs.push_back(&ev);
    for (hipEvent_t* pe : evs) {
        e = hipEventCreate(pe);
        if (e != hipSuccess) return abandon(h, ls_destroy, fail<ls_handle>(nullptr, LS_EHIP, "hipEventCreate: %s", hipGetErrorString(e)));
    }
    e = init_step_kernels();
    if (e != hipSuccess) return abandon(h, ls_destroy, fail<ls_handle>(nullptr, LS_EHIP, "hipFuncSetAttribute(step kernel LDS): %s", hipGetErrorString(e)));
    if (!h->fused && mix_supports(cfg->nframes + cfg->n_prefix_tokens)) {
        e = init_mix_kernels();
        if (e == hipSuccess) e = h->co_err.ensure(sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(h->co_err.p, 0, sizeof(unsigned), h->stream);
        if (e != hipSuccess) return abandon(h, ls_destroy, fail<ls_handle>(nullptr, LS_EHIP, "long-sequence mixer kernel setup: %s", hipGetErrorString(e)));
    }
    if (h->fused) {         // sample-split kernel: LDS opt-in and one launch's worth of exchange workspaces (independent of the batch)
        e = init_coop_kernels();
        if (e == hipSuccess) e = init_pass_kernels();
        if (e == hipSuccess) e = h->co_err.ensure(sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(h->co_err.p, 0, sizeof(unsigned), h->stream);
        if (e != hipSuccess) return abandon(h, ls_destroy, fail<ls_handle>(nullptr, LS_EHIP, "sample-split kernel setup: %s", hipGetErrorString(e)));
    }
#ifdef LS_DEBUG
    if (h->prof_on) {
        std::vector<unsigned long long> z((size_t)kWaves * kProfPoints, 0ull);
        if (upload(h, h->prof, z.data(), z.size() * sizeof(unsigned long long)) != LS_OK) { create_error<ls_handle>() = h->err; return abandon(h, ls_destroy, LS_EHIP); }
        std::vector<unsigned long long> zw(4096, 0ull);      // [1024][2] stamps | [2048] hardware ids (k_pass)
        if (upload(h, h->wgt, zw.data(), zw.size() * sizeof(unsigned long long)) != LS_OK) { create_error<ls_handle>() = h->err; return abandon(h, ls_destroy, LS_EHIP); }
    }
#endif
    CallParams cp{0, 0, 0, 0};
    if (upload(h, h->callp, &cp, sizeof cp) != LS_OK) { create_error<ls_handle>() = h->err; return abandon(h, ls_destroy, LS_EHIP); }
    *out = h;
    return LS_OK;
}

void ls_destroy(ls_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_graph(h);
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < 2; ++i)
        for (hipEvent_t ev : {h->ev_cs[i], h->ev_cd[i], h->ev_seg[i]}) if (ev) (void)hipEventDestroy(ev);
    if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;              // every DevBuf frees its memory
}

int ls_set_weight(ls_handle* h, const char* key, const float* data, size_t n) {
    if (!h || !key || (!data && n)) return fail(h, LS_EINVAL, "ls_set_weight: null argument");
    const std::string k(key);
    if (k.size() >= 3 && k.compare(k.size() - 3, 3, ".pe") == 0) return LS_OK;   // buffers, recomputed (mlp_module.py:104-116)
    h->w[k].assign(data, data + n);
    h->committed = false;
    return LS_OK;
}

int ls_commit_weights(ls_handle* h) {
    if (!h) return LS_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc = build_images(h);
    if (rc != LS_OK) return rc;
    h->committed = true;
    h->weights_version++;
    h->temb_valid = false;
    h->prepared = false;
    end_stream(h);
    free_graph(h);
    return LS_OK;
}

int ls_set_schedule(ls_handle* h, const ls_schedule* s) {
    if (!h || !s) return fail(h, LS_EINVAL, "ls_set_schedule: null argument");
    if (s->n_steps < 1) return fail(h, LS_EINVAL, "n_steps must be >= 1");
    const double* tabs[] = {s->sqrt_alphas_cumprod, s->sqrt_one_minus_alphas_cumprod, s->posterior_mean_coef1,
                            s->posterior_mean_coef2, s->posterior_log_variance_clipped, s->alphas_cumprod,
                            s->alphas_cumprod_prev, s->sqrt_recip_alphas_cumprod, s->sqrt_recipm1_alphas_cumprod};
    for (const double* t : tabs) if (!t) return fail(h, LS_EINVAL, "ls_set_schedule: null table");
    if (!s->timestep_map) return fail(h, LS_EINVAL, "ls_set_schedule: null timestep_map");
    const int n = s->n_steps;
    for (int i = 0; i < n; ++i)
        if (s->timestep_map[i] < 0 || s->timestep_map[i] >= kPeRows)
            return fail(h, LS_EINVAL, "timestep_map[%d]=%lld outside [0,%d)", i, (long long)s->timestep_map[i], kPeRows);
    h->n_steps = n;
    h->tmap.assign(s->timestep_map, s->timestep_map + n);
    std::vector<double>* dst[] = {&h->t_sac, &h->t_s1mac, &h->t_c1, &h->t_c2, &h->t_plv, &h->t_ac, &h->t_acp, &h->t_srac, &h->t_srm1ac};
    for (int k = 0; k < 9; ++k) dst[k]->assign(tabs[k], tabs[k] + n);
    h->have_sched = true;
    h->sched_version++;
    h->temb_valid = false;
    free_graph(h);
    return LS_OK;
}

static int prepare_impl(ls_handle* h, const ls_cond* c, bool wait) {
    if (!h || !c) return fail(h, LS_EINVAL, "ls_prepare: null argument");
    if (!h->committed) return fail(h, LS_ESTATE, "ls_prepare before ls_commit_weights");
    if (c->batch < 1) return fail(h, LS_EINVAL, "batch must be >= 1");
    if (!c->audio_input || !c->origin_x || !c->vid_indices || !c->scale) return fail(h, LS_EINVAL, "ls_prepare: null conditioning pointer");
    if (h->cfg.n_prefix_tokens == 2 && !c->emo) return fail(h, LS_EINVAL, "BEAT variant needs emo ids");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = c->batch, JF = h->JF, AL = h->cfg.audio_len;
    const int od = c->on_device;
    hipStream_t st = h->stream;
    int rc;
    HIPCHK(h, hipEventRecord(h->ev[4], st));
    // a device-resident waveform is read in place by conv1, its only consumer (74 MB at B = 512: the copy was 28 us of the stage):
    // ls_prepare synchronises before it returns, and ls_prepare_async's contract keeps device inputs valid until the next synchronising call
    if (!od && (rc = ingest(h, h->audio, c->audio_input, (size_t)B * AL * sizeof(float), od)) != LS_OK) return rc;
    if ((rc = ingest(h, h->origin_x, c->origin_x, (size_t)B * JF * h->T * sizeof(float), od)) != LS_OK) return rc;
    if ((rc = ingest(h, h->vid, c->vid_indices, (size_t)B * sizeof(int64_t), od)) != LS_OK) return rc;
    if ((rc = ingest(h, h->scale, c->scale, (size_t)B * sizeof(float), od)) != LS_OK) return rc;
    if (c->emo && (rc = ingest(h, h->emo, c->emo, (size_t)B * h->T * sizeof(int64_t), od)) != LS_OK) return rc;
    if (!wait && !od) {     // ls_prepare_async with HOST inputs: the caller may free / rewrite them as soon as we return
        HIPCHK(h, hipEventRecord(h->ev[6], st));
        HIPCHK(h, hipEventSynchronize(h->ev[6]));
    }
    h->seg_next = -1;       // a new conditioning ends any segmented loop in progress
    end_chain(h);           // ... and replaces a long-form call's, and a running stream's
    if ((rc = prepare_scale(h, c->scale, B, od)) != LS_OK) return rc;
    if ((rc = run_wav_encoder(h, od ? static_cast<const float*>(c->audio_input) : h->audio.f(), B)) != LS_OK) return rc;
    // ---- static part of input_mapping (RAG.py:110-114): columns JF.. of W_in act on [prefix poses | bit | audio]
    const int KPP = h->KPP;
    HIPCHK(h, h->feat_c.ensure((size_t)B * h->T * kAudioFeat * sizeof(float)));       // audio features [B*T][256]
    HIPCHK(h, h->feat_u.ensure((size_t)B * h->T * KPP * sizeof(float)));              // [prefix poses | bit | pad]
    HIPCHK(h, h->static_c.ensure((size_t)B * h->T * kD * sizeof(float)));
    HIPCHK(h, h->static_u.ensure((size_t)B * h->T * kD * sizeof(float)));
    HIPCHK(h, launch_build_feats(h->origin_x.f(), h->c4.f(), h->feat_u.f(), h->feat_c.f(), B, JF, KPP, h->cfg.n_pre_seq, st, h->T));
    // static_u = [prefix poses | bit] . Wpre^T + b;  static_c = static_u + audio . Waud^T  (K = KPP + 256 instead of 2 x that)
    HIPCHK(h, launch_gemm_nt(h->feat_u.f(), KPP, h->win_pre.f(), KPP, h->win_bias.f(), nullptr, 0, h->static_u.f(), kD, B * h->T, kD, KPP, 0, st));
    HIPCHK(h, launch_gemm_nt(h->feat_c.f(), kAudioFeat, h->win_aud.f(), kAudioFeat, nullptr, h->static_u.f(), kD, h->static_c.f(), kD, B * h->T, kD, kAudioFeat, 0, st));
    if ((rc = prepare_style(h, B)) != LS_OK) return rc;
    if (h->cfg.n_prefix_tokens == 2) {   // scripts_beat/model/RAG.py:125
        HIPCHK(h, h->emo_tok.ensure((size_t)B * kD * sizeof(float)));
        HIPCHK(h, launch_gather_rows(h->emo_emb.f(), static_cast<const int64_t*>(h->emo.p), h->emo_tok.f(), B, kD, h->cfg.n_emotions, st, h->T));   // y['emo'][:, 0]
    }
    if ((rc = prepare_plan(h, B)) != LS_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[5], st));
    if (wait) {
        HIPCHK(h, hipStreamSynchronize(st));
        HIPCHK(h, hipEventElapsedTime(&h->timing.prepare_ms, h->ev[4], h->ev[5]));
        h->prepare_pending = false;
    } else {
        h->timing.prepare_ms = -1.0f;          // until the work is known to be done (next synchronising call / ls_get_timing)
        h->prepare_pending = true;
    }
    if (h->B != B) { free_graph(h); h->rk_n = 0; }      // row keys (ls_set_row_keys) hold for one batch size
    h->B = B;
    h->prepared = true;
    return LS_OK;
}

int ls_prepare(ls_handle* h, const ls_cond* c) { return prepare_impl(h, c, true); }
// The same work enqueued on the handle's stream without waiting for it: everything that follows on this handle (ls_sample, ls_forward,
// ls_step) is stream-ordered behind it, so a caller can overlap the once-per-call stage with work on ANOTHER stream -- LivelySpeaker's
// SAG decode, which needs none of it (scripts/test_LivelySpeaker_ted.py:88-113 runs the two back to back).  Device-resident inputs
// must stay valid until the next call on this handle that synchronises; host inputs are staged as in ls_prepare.
int ls_prepare_async(ls_handle* h, const ls_cond* c) { return prepare_impl(h, c, false); }

int ls_stream_order(int device, void* first, void* then) {
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return LS_EHIP;
    hipError_t e = hipEventRecord(ev, static_cast<hipStream_t>(first));
    if (e == hipSuccess) e = hipStreamWaitEvent(static_cast<hipStream_t>(then), ev, 0);
    (void)hipEventDestroy(ev);          // released by the runtime once the recorded work has completed
    return e == hipSuccess ? LS_OK : LS_EHIP;
}

void* ls_stream(const ls_handle* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

int ls_philox_x_init(ls_handle* h, int batch, uint64_t seed, uint64_t sample_offset, int on_device, float* out) {
    if (!h || !out || batch < 1) return fail(h, LS_EINVAL, "ls_philox_x_init: bad argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t nx = (size_t)batch * h->JF * h->T * sizeof(float);
    HIPCHK(h, h->xtmp.ensure(nx));
    HIPCHK(h, h->xio.ensure(nx));
    h->call_host = CallParams{seed, sample_offset, h->tag_base, 0u};
    HIPCHK(h, hipMemcpyAsync(h->callp.p, &h->call_host, sizeof(CallParams), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_randn_fill(h->xtmp.f(), batch, h->JF, static_cast<const CallParams*>(h->callp.p), 0u, h->stream, h->T));
    int rc = egress_internal(h, h->xtmp.f(), out, batch, on_device);
    if (rc != LS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LS_OK;
}

uint64_t ls_torch_randn_advance(int64_t n, int32_t n_cu, int32_t max_threads_per_cu) {
    return torch_randn_advance(n, n_cu, max_threads_per_cu, nullptr);
}

int ls_torch_randn(ls_handle* h, uint64_t seed, uint64_t offset, int64_t n, float* out_device, int no_sync) {
    if (!h || !out_device || n < 1 || n >= (1ll << 31)) return fail(h, LS_EINVAL, "ls_torch_randn: bad argument");
    if (offset & 3) return fail(h, LS_EINVAL, "ls_torch_randn: the generator offset %llu is not a multiple of 4", (unsigned long long)offset);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->call_host = CallParams{seed, offset, h->tag_base, 0u};
    HIPCHK(h, hipMemcpyAsync(h->callp.p, &h->call_host, sizeof(CallParams), hipMemcpyHostToDevice, h->stream));
    TorchDrawArgs a{};
    a.call = static_cast<const CallParams*>(h->callp.p);
    a.nsteps = 1; a.ndraw = 1; a.last_step = -1; a.B = 1; a.JF = 1; a.T = 1;
    a.d[0] = torch_draw(out_device, 0, n, h->n_cu, h->max_thr_cu, 0, 0);
    HIPCHK(h, launch_torch_draws(a, h->stream));
    if (!no_sync) HIPCHK(h, hipStreamSynchronize(h->stream));
    return LS_OK;
}

int ls_set_torch_ring_bytes(ls_handle* h, uint64_t bytes) {
    if (!h || bytes < 1) return fail(h, LS_EINVAL, "ls_set_torch_ring_bytes: bad argument");
    h->trng_ring_bytes = (size_t)bytes;
    return LS_OK;
}

long long ls_read(ls_handle* h, const char* name, float* host_out, size_t capacity) {
    if (!h || !name || !host_out) return fail(h, LS_EINVAL, "ls_read: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const std::string n(name);
    const float* src = nullptr;
    size_t cnt = 0;
    const size_t B = (size_t)h->B;
#ifdef LS_DEBUG
    if (n == "prof" || n == "wgt" || n == "wgt_hw") {      // 64-bit stamps as pairs of 32-bit words; wgt_hw (k_pass): HW_ID | XCC_ID << 32 of every workgroup's wave 0
        if (!h->prof_on) return fail(h, LS_ESTATE, "LS_PROF not set");
        cnt = n == "prof" ? (size_t)kWaves * kProfPoints * 2 : 2048 * 2;
        if (cnt > capacity) return fail(h, LS_EINVAL, "capacity");
        const void* from = n == "prof" ? h->prof.p : static_cast<unsigned long long*>(h->wgt.p) + (n == "wgt_hw" ? 2048 : 0);
        HIPCHK(h, hipMemcpy(host_out, from, cnt * sizeof(float), hipMemcpyDeviceToHost));
        return (long long)cnt;
    }
#endif
    if (n == "temb") {
        if (!h->have_sched || !h->committed) return fail(h, LS_ESTATE, "temb needs weights and schedule");
        int rc = ensure_temb_table(h);
        if (rc != LS_OK) return rc;
        src = h->temb.f(); cnt = (size_t)h->n_steps * kD;
    } else {
        if (!h->prepared) return fail(h, LS_ESTATE, "ls_read('%s') before ls_prepare", name);
        if (n == "audio_feat") {
            HIPCHK(h, h->audio_feat.ensure(B * h->T * kAudioFeat * sizeof(float)));
            HIPCHK(h, launch_transpose_feat(h->c4.f(), h->audio_feat.f(), (int)B, h->stream, h->T));
            src = h->audio_feat.f(); cnt = B * h->T * kAudioFeat;
        } else if (n == "static_c") { src = h->static_c.f(); cnt = B * h->T * kD; }
        else if (n == "static_u") { src = h->static_u.f(); cnt = B * h->T * kD; }
        else if (n == "z_mu") { src = h->z_mu.f(); cnt = B * kD; }
        else if (n == "z_logvar") { src = h->z_logvar.f(); cnt = B * kD; }
        else if (n == "z_std") { src = h->z_std.f(); cnt = B * kD; }
        else if (n == "pass_tickets" && h->pa_cnt.p) { src = h->pa_cnt.f(); cnt = (size_t)h->pass_n; }      // raw words (diagnostics)
        else return fail(h, LS_EINVAL, "ls_read: unknown buffer '%s'", name);
    }
    if (cnt > capacity) return fail(h, LS_EINVAL, "ls_read('%s'): need %zu floats, capacity %zu", name, cnt, capacity);
    HIPCHK(h, hipMemcpyAsync(host_out, src, cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return (long long)cnt;
}

int ls_shard_range(int64_t total, int32_t world, int32_t rank, int64_t* first, int64_t* count) {
    if (total < 0 || world < 1 || rank < 0 || rank >= world || !first || !count) return LS_EINVAL;
    const int64_t base = total / world, extra = total % world;
    *count = base + (rank < extra ? 1 : 0);
    *first = (int64_t)rank * base + (rank < extra ? rank : extra);
    return LS_OK;
}

int ls_get_timing(const ls_handle* h, ls_timing* out) {
    if (!h || !out) return LS_EINVAL;
    resolve_prepare_timing(const_cast<ls_handle*>(h), false);      // an ls_prepare_async that has finished by now
    *out = h->timing;
    return LS_OK;
}

int ls_synchronize(ls_handle* h) {
    if (!h) return LS_EINVAL;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    resolve_prepare_timing(h, true);
    return LS_OK;
}

}  // extern "C"
