// Host side of ls_chain.hip: the chained-window engine behind the long-form entries of include/ls_hip.h.  A chain is a sequence of
// 34-frame windows of the prepared batch, each one ls_prepare's two static projections plus ls_sample's loop on device-resident inputs
// (run_window_loop, ls_sample.cpp), handed the last poses of the window before it.  There is one once-per-call stage (check_cond ->
// start_prepare -> ingest_cond -> size_batch_buffers -> finish_prepare) and one window runner (chain_args -> chain_begin -> run_window
// per window -> chain_finish); the entries hold what differs: where a window's audio features come from (all windows encoded ahead,
// packed for clips of different lengths, or one round at a time from the rings of a streaming session's active slots) and what stands
// around a window (k_chain_window ahead of it, k_edit_gather / k_edit_scatter -- with k_edit_start behind the decoder of a scripted
// edit; the compact edit runs them on a row table, one row per clip the window touches, behind k_cond_gather -- or k_pool_gather /
// k_pool_scatter).  There is one
// streaming session (session_open -> session_push -> session_push_run): a pool of slots that join and leave, and a stream, which is
// the pool whose slots were all joined at the open and are fed, given and closed alike.  The host-only plans are ls_chain_plan.cpp.
#include "ls_handle.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <vector>

using namespace ls;

namespace {

// ---- the once-per-call stage ----------------------------------------------------------------------------------------------------
// the refusals every conditioning shares; n_windows: null for a streaming session, which has none
int check_cond(ls_handle* h, const char* entry, int batch, const int32_t* n_windows, bool audio_ok, bool pointers_ok, bool emo_ok) {
    if (!h->committed) return fail(h, LS_ESTATE, "%s before ls_commit_weights", entry);
    if (!h->fused) return fail(h, LS_EUNSUPPORTED, "long-form synthesis chains the reference's %d-frame windows", kT);
    if (batch < 1 || (n_windows && *n_windows < 1)) return fail(h, LS_EINVAL, n_windows ? "batch and n_windows must be >= 1" : "batch must be >= 1");
    if (!audio_ok) return fail(h, LS_EINVAL, "%s: bad audio_samples / encoder_chunk", entry);
    if (!pointers_ok) return fail(h, LS_EINVAL, "%s: null conditioning pointer", entry);
    if (!emo_ok) return fail(h, LS_EINVAL, "BEAT variant needs emo ids");
    if (h->cfg.n_pre_seq < 1) return fail(h, LS_EINVAL, "long-form synthesis needs n_pre_seq >= 1 (the hand-off poses)");
    return LS_OK;
}

// the handle's prepared conditioning is replaced from here on; the stage's clock starts
int start_prepare(ls_handle* h) {
    h->prepared = h->lg_prepared = h->lg_ragged = h->lg_compact = false;
    h->seg_next = -1;
    HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
    return LS_OK;
}

// seed poses, speaker ids, guidance scales and (emo: [n_emo] ids, nullable) the emotion ids; leading_ones as in prepare_scale
int ingest_cond(ls_handle* h, int B, int od, const float* seed_poses, const int64_t* vid, const float* scale, const int64_t* emo, size_t n_emo,
                int* leading_ones = nullptr) {
    int rc;
    if ((rc = ingest(h, h->lg_seed, seed_poses, (size_t)B * h->JF * h->cfg.n_pre_seq * sizeof(float), od)) != LS_OK) return rc;
    if ((rc = ingest(h, h->vid, vid, (size_t)B * sizeof(int64_t), od)) != LS_OK) return rc;
    if ((rc = ingest(h, h->scale, scale, (size_t)B * sizeof(float), od)) != LS_OK) return rc;
    if (emo && (rc = ingest(h, h->lg_emo_ids, emo, n_emo * sizeof(int64_t), od)) != LS_OK) return rc;
    return prepare_scale(h, scale, B, od, leading_ones);
}

// The per-batch buffers of a window at batch B, in two steps with the encoder between them (ls_long_prepare's order of enqueues).
// origin_x: frames n_pre.. are zero (RAG.py:110); it is also k_build_feats' (unused) pose source, hence ahead of the encoder
int zero_origin_x(ls_handle* h, int B) {
    HIPCHK(h, h->origin_x.ensure((size_t)B * h->JF * h->T * sizeof(float)));
    HIPCHK(h, hipMemsetAsync(h->origin_x.p, 0, (size_t)B * h->JF * h->T * sizeof(float), h->stream));
    return LS_OK;
}
// feat_u: every row zero, k_chain_window writes the prefix rows per window
int size_batch_buffers(ls_handle* h, int B) {
    const int T = h->T;
    hipStream_t st = h->stream;
    HIPCHK(h, h->feat_u.ensure((size_t)B * T * h->KPP * sizeof(float)));
    HIPCHK(h, hipMemsetAsync(h->feat_u.p, 0, (size_t)B * T * h->KPP * sizeof(float), st));
    HIPCHK(h, h->static_c.ensure((size_t)B * T * kD * sizeof(float)));
    HIPCHK(h, h->static_u.ensure((size_t)B * T * kD * sizeof(float)));
    if (h->cfg.n_prefix_tokens == 2) HIPCHK(h, h->emo_tok.ensure((size_t)B * kD * sizeof(float)));
    return LS_OK;
}

// the stage's wait and prepare_ms
int finish_clock(ls_handle* h) {
    HIPCHK(h, hipEventRecord(h->ev[5], h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&h->timing.prepare_ms, h->ev[4], h->ev[5]));
    h->prepare_pending = false;
    return LS_OK;
}
// ... and the prepared batch of ls_long_prepare*.  Every buffer a captured loop reads moves only when the batch changes (as in
// ls_prepare): the graphs are dropped then and kept otherwise -- their keys hold the batch and the plan, so the next call finds them
int finish_prepare(ls_handle* h, int B) {
    const int rc = finish_clock(h);
    if (rc != LS_OK) return rc;
    if (h->B != B) free_graph(h);
    h->B = B;
    return LS_OK;
}

// ---- the window runner ----------------------------------------------------------------------------------------------------------
// One call of the engine.  wa is the ls_sample call every window makes: the eight sampler fields of the entry's arguments, device
// inputs, and per window its tapes.
struct ChainCall {
    ls_sample_args wa{};
    uint64_t seed = 0, sample_offset = 0;
    bool tape = false;
    int n_exec = 0;
    ls_sag* sag = nullptr;          // LivelySpeaker chain: every window starts from the decoder's output (chain_begin)
    void* sag_st = nullptr;
    float* sag_out = nullptr;       // where the decoder writes [B][JF][T]: the init plane itself, or a scripted edit's plane of its own
    int windows = 0, replays = 0;   // windows run; those served by a graph replay
    bool pair0 = false;             // the first window ran the single-pass form
    bool coop_used = false;         // some window ran the sample-split kernel (a ragged call's plan changes per window)
};

// One window: what changes from one to the next
struct Window {
    long long w = 0;                    // index in the chain: PHILOX draws at sample_offset + b + (w << 48)
    int Bw = 0;                         // clips that run it: slots [0, Bw) of every per-clip buffer
    const float* featc = nullptr;       // its audio features [Bw][T][256]
    const float* emo_tok = nullptr;     // BEAT: its emotion tokens [Bw][512]; null: the ones in emo_tok (a session's round: k_pool_gather wrote them)
    const float* text = nullptr;        // SAG: its text features [Bw][512]
    const float *x_init = nullptr, *eps_tape = nullptr, *noise_tape = nullptr, *inpaint_noise = nullptr;      // TAPE: its draws
    bool host_tapes = false;            // ... in host memory: uploaded here, one window at a time (a session's round: the staging does not grow with the call)
    bool host_inz = false;              // inpaint_noise is in host memory (a session's pinned call: ls_long_pool_pin_tape), uploaded likewise
    bool resident_inpaint = false;      // a timeline edit: the inpainting planes are on the device (k_edit_gather)
    const EditArgs* edit_start = nullptr;       // a scripted edit: behind the decode, k_edit_start puts cc.sag_out under the editable elements of the init plane
    CachePolicy policy = kReplace;
    bool first = false;                 // the first window of the call
    bool keyed = false;                 // a keyed pool's round: PHILOX rows draw at row_gidx (written ahead of the window), w is not used
};

// The call prologue, first half -- nothing here touches the device: the refusals every entry shares, and wa.  runs: the call runs at
// least one window (a push of a session may run none, and then needs neither tapes nor counters)
template <class Args>
int chain_args(ls_handle* h, const char* entry, const Args* a, bool runs, ChainCall& cc) {
    if (a->sampler != LS_SAMPLER_DDPM && a->sampler != LS_SAMPLER_DDIM) return fail(h, LS_EUNSUPPORTED, "%s: DDPM and DDIM loops only", entry);
    if (a->noise_mode != LS_NOISE_TAPE && a->noise_mode != LS_NOISE_PHILOX) return fail(h, LS_EUNSUPPORTED, "%s: TAPE and PHILOX noise only", entry);
    ls_sample_args& wa = cc.wa;
    wa.sampler = a->sampler; wa.noise_mode = a->noise_mode; wa.skip_timesteps = a->skip_timesteps; wa.on_device = 1;
    wa.use_graph = a->use_graph; wa.clip_denoised = a->clip_denoised; wa.two_pass_always = a->two_pass_always; wa.eta = a->eta;
    const int rc = check_sampler_args(h, &wa);
    if (rc != LS_OK) return rc;
    cc.seed = a->seed; cc.sample_offset = a->sample_offset;
    cc.tape = a->noise_mode == LS_NOISE_TAPE;
    cc.n_exec = h->n_steps - a->skip_timesteps;
    if (!runs) return LS_OK;
    if (cc.tape && (!a->x_init || !a->eps_tape || !a->noise_tape)) return fail(h, LS_EINVAL, "TAPE mode needs x_init, eps_tape and noise_tape");
    if (!cc.tape && (a->sample_offset >> 48 || (a->sample_offset + (unsigned long long)h->B) >> 48)) return fail(h, LS_EINVAL, "PHILOX: sample_offset + batch must stay below 2^48 (the window index sits above)");
    return LS_OK;
}

// ... second half, on the device: the timestep embeddings, and with a SAG decoder its output plane and its all-ones mask
int chain_begin(ls_handle* h, ChainCall& cc, ls_sag* sag) {
    int rc;
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    h->seg_next = -1;
    if (!sag) return LS_OK;
    cc.sag = sag; cc.sag_st = ls_sag_stream(sag);
    HIPCHK(h, h->lg_init.ensure((size_t)h->B * h->JF * h->T * sizeof(float))); HIPCHK(h, h->lg_mask.ensure((size_t)h->B * h->T));
    HIPCHK(h, hipMemsetAsync(h->lg_mask.p, 1, (size_t)h->B * h->T, h->stream));
    cc.wa.init_image = cc.sag_out = h->lg_init.f();
    return LS_OK;
}

// The window body.  feat_u / origin_x hold the window's prefix poses (whoever ran the window before it wrote them).  The loop's launches
// read the handle's buffers only (static_c / static_u, the tape buffers, xa / xb, callp), none of which moves between windows, so the
// graph captured for the first window (or by an earlier call with the same key) is replayed for every later one.  The result is
// x_plane(h, cc.n_exec).
int run_window(ls_handle* h, ChainCall& cc, const Window& win) {
    const int Bw = win.Bw, T = h->T, dev = h->cfg.device;
    hipStream_t st = h->stream;
    ls_sample_args& wa = cc.wa;
    int rc;
    if (win.first) cc.pair0 = single_pass(h, wa.two_pass_always);
    cc.coop_used = cc.coop_used || seg_n(h, 2) > 0;
    // the static projections with ls_prepare's arithmetic and shapes: static_u = feat_u . Wpre^T + b; static_c = static_u + feat_c . Waud^T
    HIPCHK(h, launch_gemm_nt(h->feat_u.f(), h->KPP, h->win_pre.f(), h->KPP, h->win_bias.f(), nullptr, 0, h->static_u.f(), kD, Bw * T, kD, h->KPP, 0, st));
    HIPCHK(h, launch_gemm_nt(win.featc, kAudioFeat, h->win_aud.f(), kAudioFeat, nullptr, h->static_u.f(), kD, h->static_c.f(), kD, Bw * T, kD, kAudioFeat, 0, st));
    if (win.emo_tok)
        HIPCHK(h, hipMemcpyAsync(h->emo_tok.p, win.emo_tok, (size_t)Bw * kD * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (cc.sag) {       // the decoder runs on its own handle's stream, ordered behind the hand-off and ahead of the loop by events
        if (ls_stream_order(dev, st, cc.sag_st) != LS_OK) return fail(h, LS_EHIP, "ls_stream_order failed");
        if (ls_sag_decode_async(cc.sag, Bw, h->origin_x.f(), win.text, static_cast<const unsigned char*>(h->lg_mask.p), cc.sag_out) != LS_OK)
            return fail(h, LS_EHIP, "SAG decode of window %lld: %s", win.w, ls_sag_last_error(cc.sag));
        if (ls_stream_order(dev, cc.sag_st, st) != LS_OK) return fail(h, LS_EHIP, "ls_stream_order failed");
        if (win.edit_start) HIPCHK(h, launch_edit_start(*win.edit_start, cc.sag_out, Bw, st));
    }
    if (cc.tape) {
        wa.x_init = win.x_init; wa.eps_tape = win.eps_tape; wa.noise_tape = win.noise_tape; wa.inpaint_noise = win.inpaint_noise;
        if (win.host_tapes) {
            const size_t per_x = (size_t)Bw * h->JF * T, per_e = (size_t)cc.n_exec * 2 * Bw * kD, per_n = (size_t)cc.n_exec * per_x;
            if ((rc = ingest(h, h->lg_x, win.x_init, per_x * sizeof(float), 0)) != LS_OK || (rc = ingest(h, h->lg_eps, win.eps_tape, per_e * sizeof(float), 0)) != LS_OK ||
                (rc = ingest(h, h->lg_nz, win.noise_tape, per_n * sizeof(float), 0)) != LS_OK) return rc;
            wa.x_init = h->lg_x.f(); wa.eps_tape = h->lg_eps.f(); wa.noise_tape = h->lg_nz.f();
        }
        if (win.inpaint_noise && win.host_inz) {
            if ((rc = ingest(h, h->lg_inz, win.inpaint_noise, (size_t)cc.n_exec * Bw * h->JF * T * sizeof(float), 0)) != LS_OK) return rc;
            wa.inpaint_noise = h->lg_inz.f();
        }
    }
    // The loop's advance_tags uploads call_host (24 bytes of pageable memory) as every ls_sample does: the runtime takes such a source into
    // its staging memory before hipMemcpyAsync returns, which is what makes rewriting it for the next window safe.  It is the one host ->
    // device copy per window; whether the runtime waits inside it is the runtime's business (not measured).
    h->call_host = CallParams{cc.seed, win.keyed ? 0ull : cc.sample_offset + ((unsigned long long)win.w << 48), h->tag_base, 0u};
    int replayed = 0;
    if ((rc = run_window_loop(h, &wa, win.resident_inpaint, win.first, win.policy, &replayed, win.keyed)) != LS_OK) return rc;
    cc.replays += replayed;
    ++cc.windows;
    return LS_OK;
}

// The call epilogue: the outputs of a host caller back (a null dst: none), the one wait of the call, and its ls_timing.  coop_check is
// forced by coop_used because a ragged call's plan at this point is not the plan its windows ran under; where the plan never changed
// the two agree.
struct Egress { void* dst; const void* src; size_t bytes; };
int chain_finish(ls_handle* h, const ChainCall& cc, std::initializer_list<Egress> outs) {
    hipStream_t st = h->stream;
    int rc;
    HIPCHK(h, hipEventRecord(h->ev[2], st));
    for (const Egress& o : outs)
        if (o.dst && (rc = egress(h, o.dst, o.src, o.bytes, 0)) != LS_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[3], st));
    HIPCHK(h, hipStreamSynchronize(st));
    if ((rc = coop_check(h, cc.coop_used)) != LS_OK) return rc;
    report_path(h, cc.pair0);
    HIPCHK(h, hipEventElapsedTime(&h->timing.loop_ms, h->ev[1], h->ev[2]));
    HIPCHK(h, hipEventElapsedTime(&h->timing.total_ms, h->ev[6], h->ev[3]));       // ev[6]: the first window's start (ev[0] is re-recorded by every window)
    h->timing.n_step_launches = cc.windows * cc.n_exec;
    h->timing.single_pass = cc.pair0 ? 1 : 0;
    h->timing.graph_replayed = cc.replays;       // windows served by a replay: all but the first after a capture, all on a warm handle
    h->timing.tape_upload_ms = 0.f;
    h->timing.n_segments = cc.windows;
    return LS_OK;
}

// ---- the element mask of a timeline edit ----------------------------------------------------------------------------------------
// The pair flags [W][B] of an element mask [B][JF][T_total] (ls_long_edit_mask and its kin), from which every mask plan is made.  A
// host mask is reduced by the host loop (edit_mask_flags).  A device mask stays where it is: k_edit_mask_pairs reduces it on the
// handle's stream and W * B bytes come back -- the one host wait a device mask adds to a call.  frames [B] (HOST, nullable): a ragged
// batch.  LS_EINVAL: a set byte at or beyond its clip's frames[b].
int mask_pair_flags(ls_handle* h, const char* entry, const unsigned char* mask, int on_device, int B, int W, const int32_t* frames,
                    std::vector<unsigned char>& flags) {
    const int JF = h->JF, T = h->T, npre = h->cfg.n_pre_seq;
    if (!on_device) {
        if (edit_mask_flags(B, W, T, npre, JF, mask, frames, flags) != LS_OK)
            return fail(h, LS_EINVAL, "%s: the element mask has a set byte at or beyond its clip's own frames[b]", entry);
        return LS_OK;
    }
    if (W > 65535) return fail(h, LS_EINVAL, "%s: a device mask of %d windows (at most 65535)", entry, W);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc;
    if (frames && (rc = upload(h, h->lg_edit_frames, frames, (size_t)B * sizeof(int32_t))) != LS_OK) return rc;
    HIPCHK(h, h->lg_edit_flags.ensure((size_t)W * B));
    HIPCHK(h, launch_edit_mask_pairs(mask, frames ? static_cast<const int*>(h->lg_edit_frames.p) : nullptr, static_cast<unsigned char*>(h->lg_edit_flags.p),
                                     B, W, JF, T, npre, h->stream));
    flags.assign((size_t)W * B, 0);
    HIPCHK(h, hipMemcpyAsync(flags.data(), h->lg_edit_flags.p, flags.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (unsigned char f : flags)
        if (f > 1) return fail(h, LS_EINVAL, "%s: the element mask has a set byte at or beyond its clip's own frames[b]", entry);
    return LS_OK;
}

// ---- streaming sessions ---------------------------------------------------------------------------------------------------------
// A session pool, and a stream: the pool whose slots were all joined at the open and are fed and closed together (pl_lockstep).
int session_is_open(ls_handle* h, const char* entry, bool stream) {
    const char* what = stream ? "stream" : "pool";
    if (h->pl_state == ls_handle::kStreamNone) return fail(h, LS_ESTATE, "%s before ls_long_%s_open", entry, what);
    if ((h->pl_lockstep != ls_handle::kPool) == stream) {       // otherwise: a session of the other kind has replaced it
        if (h->pl_lockstep == ls_handle::kLockstepClosed) return fail(h, LS_ESTATE, "%s: the stream is closed", entry);
        if (h->pl_state == ls_handle::kStreamOpen) return LS_OK;
        if (h->pl_state == ls_handle::kStreamFailed) return fail(h, LS_ESTATE, "%s: an earlier push of this %s failed; open a new one", entry, what);
    }
    return fail(h, LS_ESTATE, "%s: the %s was ended by a call that replaced the handle's prepared conditioning (ls_prepare, ls_long_prepare, "
                              "ls_commit_weights, ls_long_stream_open or ls_long_pool_open); open a new one", entry, what);
}

// what a session holds on the device, as allocated: rings, hand-off stores, held conditioning, round table, gathered windows, features
int64_t session_bytes(const ls_handle* h) {
    const size_t pins = h->pl_pin_P ? h->pl_pin_val.bytes + h->pl_pin_bit.bytes : 0;      // the pin store, where the session has one
    return (int64_t)(h->pl_ring.bytes + h->pl_hand.bytes + h->pl_vid.bytes + h->pl_emo_id.bytes + h->pl_scale.bytes + h->pl_emotok.bytes +
                     h->pl_text.bytes + h->pl_ctext.bytes + h->pl_table.bytes + h->lg_clips.bytes + h->lg_featc.bytes + pins);
}

// the held conditioning of the n slots from s on, from the caller (host or device) into the per-slot stores
int pool_hold(ls_handle* h, void* dst, const void* src, size_t bytes, int od) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return LS_OK;
}
int pool_hold_emo(ls_handle* h, int s, int n, const int64_t* ids, int od) {
    int64_t* at = static_cast<int64_t*>(h->pl_emo_id.p) + s;
    const int rc = pool_hold(h, at, ids, (size_t)n * sizeof(int64_t), od);
    if (rc != LS_OK) return rc;
    HIPCHK(h, launch_gather_rows(h->emo_emb.f(), at, h->pl_emotok.f() + (size_t)s * kD, n, kD, h->cfg.n_emotions, h->stream));
    for (int i = s; i < s + n; ++i) h->pl_have_emo[(size_t)i] = 1;
    return LS_OK;
}
int pool_hold_text(ls_handle* h, int s, int n, const float* rows, int od) {
    for (int i = s; i < s + n; ++i) h->pl_have_text[(size_t)i] = 1;
    return pool_hold(h, h->pl_text.f() + (size_t)s * kD, rows, (size_t)n * kD * sizeof(float), od);
}

// The buffers a captured loop holds by address among those a session's open sizes (the workspaces of the step plans and whatever a
// push sizes go through ensure_pinned).  THE GRAPH RULE of a session's open: the cached graphs are dropped exactly when one of these
// moved -- a graph's key holds the batch and the plan, its nodes hold these addresses, so a stream opened where nothing moved (again
// at the same batch, or at a smaller one) replays the loop the last one captured from its first window on.  A pool's open drops them
// whatever moved, for a reason of its own (session_open).
std::vector<const void*> loop_held(const ls_handle* h) {
    return {h->static_c.p, h->static_u.p, h->emo_tok.p, h->z_mu.p, h->z_std.p, h->scale.p, h->xa.p, h->xb.p, h->xtmp.p, h->xio.p,
            h->lg_init.p, h->eps_tape.p, h->noise_tape.p};
}

// Opening a session of S slots.  Every buffer a round touches is sized for S rows here -- the per-slot stores, the compact batch
// buffers, the WavEncoder's activations (one run on silence), the style buffers (one run on speaker 0), the loop's planes and tape
// buffers, the SAG plane and mask, and the workspaces of the step plans -- so that a push allocates only what depends on its own
// arguments (a host caller's tape staging and output; the tape buffers again when the schedule grew after the open), ahead of its
// first launch, with nothing in flight.  c: a stream (ls_long_stream_cond) -- its B clips join the B slots here, in batched copies, and
// only batch B is planned, under the form its own scales choose; null: a pool -- the slots are free, and every batch 1..S is planned
// under both forms of a step.
int session_open(ls_handle* h, int S, const ls_long_stream_cond* c) {
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int JF = h->JF, T = h->T, AL = h->cfg.audio_len, KPP = h->KPP, npre = h->cfg.n_pre_seq;
    const int R = (AL + LS_LONG_AUDIO_STRIDE + 3) / 4 * 4;       // a window and the stride to the next; whole float4 groups per slot
    const size_t nxS = (size_t)S * JF * T * sizeof(float), rowS = (size_t)S * kD * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    end_stream(h);
    h->pl_state = ls_handle::kStreamNone;       // a session that was open has ended; this one opens when everything below has succeeded
    if ((rc = start_prepare(h)) != LS_OK) return rc;
    const std::vector<const void*> was = loop_held(h);
    HIPCHK(h, h->pl_ring.ensure((size_t)S * R * sizeof(float)));
    HIPCHK(h, h->pl_hand.ensure((size_t)S * JF * npre * sizeof(float)));
    HIPCHK(h, h->pl_vid.ensure((size_t)S * sizeof(int64_t))); HIPCHK(h, h->pl_emo_id.ensure((size_t)S * sizeof(int64_t)));
    HIPCHK(h, h->pl_scale.ensure((size_t)S * sizeof(float)));
    HIPCHK(h, h->pl_emotok.ensure(rowS)); HIPCHK(h, h->pl_text.ensure(rowS)); HIPCHK(h, h->pl_ctext.ensure(rowS));
    HIPCHK(h, h->pl_table.ensure((size_t)S * kPoolRow * sizeof(int)));
    HIPCHK(h, h->lg_clips.ensure((size_t)S * AL * sizeof(float)));
    HIPCHK(h, h->lg_featc.ensure((size_t)S * T * kAudioFeat * sizeof(float)));
    HIPCHK(h, h->lg_featp.ensure((size_t)S * T * KPP * sizeof(float)));
    HIPCHK(h, h->vid.ensure((size_t)S * sizeof(int64_t))); HIPCHK(h, h->scale.ensure((size_t)S * sizeof(float)));
    HIPCHK(h, h->xa.ensure(nxS)); HIPCHK(h, h->xb.ensure(nxS)); HIPCHK(h, h->xtmp.ensure(nxS)); HIPCHK(h, h->xio.ensure(nxS));
    HIPCHK(h, h->lg_init.ensure(nxS)); HIPCHK(h, h->lg_mask.ensure((size_t)S * T));
    if (h->have_sched) {        // the tape buffers for the longest loop of the schedule (a push checks them again: the schedule may be set later)
        HIPCHK(h, h->eps_tape.ensure((size_t)h->n_steps * 2 * S * kD * sizeof(float))); HIPCHK(h, h->noise_tape.ensure(h->n_steps * nxS));
    }
    for (DevBuf* d : {&h->pl_vid, &h->pl_emo_id, &h->pl_scale, &h->pl_hand, &h->pl_emotok, &h->pl_text, &h->lg_clips, &h->vid, &h->scale})
        HIPCHK(h, hipMemsetAsync(d->p, 0, d->bytes, st));
    if ((rc = zero_origin_x(h, S)) != LS_OK || (rc = size_batch_buffers(h, S)) != LS_OK) return rc;
    if ((rc = run_wav_encoder(h, h->lg_clips.f(), S)) != LS_OK) return rc;
    if ((rc = prepare_style(h, S)) != LS_OK) return rc;
    std::vector<float> sc((size_t)S, 0.f);
    if (c) {            // the join of every slot: seed poses [B][JF][n_pre] are the hand-off store's layout
        const int od = c->on_device;
        if ((rc = pool_hold(h, h->pl_hand.p, c->seed_poses, (size_t)S * JF * npre * sizeof(float), od)) != LS_OK) return rc;
        if ((rc = pool_hold(h, h->pl_vid.p, c->vid_indices, (size_t)S * sizeof(int64_t), od)) != LS_OK) return rc;
        if ((rc = pool_hold(h, h->pl_scale.p, c->scale, (size_t)S * sizeof(float), od)) != LS_OK) return rc;
        if (od) HIPCHK(h, hipMemcpyAsync(sc.data(), h->pl_scale.p, (size_t)S * sizeof(float), hipMemcpyDeviceToHost, st));      // the one read-back, as in prepare_scale
        else memcpy(sc.data(), c->scale, (size_t)S * sizeof(float));
        HIPCHK(h, hipStreamSynchronize(st));          // the scales are read below; the caller's arrays are its own again
        h->all_scale_one = true;
        for (float v : sc) h->all_scale_one = h->all_scale_one && v == 1.0f;
        set_plan(h, S);
        if ((rc = plan_workspaces(h)) != LS_OK) return rc;
    } else {
        for (int pair = 0; pair < 2; ++pair)
            for (int b = 1; b <= S; ++b) {      // smallest first: the handle is left planned for S slots
                h->all_scale_one = pair != 0;
                set_plan(h, b);
                if ((rc = plan_workspaces(h)) != LS_OK) return rc;
            }
    }
    if ((rc = finish_clock(h)) != LS_OK) return rc;
    // the graph rule (loop_held).  A pool's rounds keep one loop per batch and form and never evict (kKeep), so a pool starts with the
    // whole cache to itself: its first round at a batch captures (tests/test_gpu_long_pool.py counts on it)
    if (!c || loop_held(h) != was) free_graph(h);
    h->B = S;
    h->pl_S = S; h->pl_R = R; h->pl_rounds = 0;
    h->pl_samples.assign((size_t)S, 0); h->pl_windows.assign((size_t)S, 0); h->pl_frames.assign((size_t)S, 0);
    h->pl_scale_host = sc;
    h->pl_open.assign((size_t)S, c ? 1 : 0); h->pl_have_emo.assign((size_t)S, 0); h->pl_have_text.assign((size_t)S, 0);
    h->pl_styled.clear();
    h->pl_keyed = false; h->pl_joins = 0; h->pl_key.assign((size_t)S, 0);
    h->pl_pin_H = h->pl_pin_P = 0; h->pl_pin_frames.clear(); h->pl_pin_tape = nullptr; h->pl_pin_tape_floats = 0;
    h->pl_lockstep = c ? ls_handle::kLockstep : ls_handle::kPool;
    h->pl_state = ls_handle::kStreamOpen;
    return LS_OK;
}

// The sampling calls of a push (ls_long_pool_pin_plan): the slots of call 0, then of call 1, ... in rows; per call its rows, whether
// it is a pinned (inpainting) call, and the round of ls_long_pool_plan it belongs to.  Without a pending pin the calls are the rounds.
struct PoolCalls { std::vector<int32_t> rows, counts, pinned, round; };

// the pending pinned frames of slot s that window w owns leave the host mirror: k_pool_pin_gather has cleared their bytes
void pins_consumed(ls_handle* h, int s, long long w) {
    const long long S = h->T - h->cfg.n_pre_seq, lo = w ? w * S + h->cfg.n_pre_seq : 0, hi = w * S + h->T;
    std::vector<long long>& v = h->pl_pin_frames[(size_t)s];
    v.erase(std::remove_if(v.begin(), v.end(), [&](long long n) { return n >= lo && n < hi; }), v.end());
}
PinArgs pin_args(const ls_handle* h) {
    PinArgs p{};
    p.val = h->pl_pin_val.f(); p.bit = static_cast<unsigned char*>(h->pl_pin_bit.p);
    p.S = h->pl_S; p.P = h->pl_pin_P; p.JF = h->JF; p.T = h->T;
    return p;
}
// every pin of slot s goes: the bytes of its whole ring, and the mirror
int pins_drop(ls_handle* h, int s) {
    if (!h->pl_pin_P || h->pl_pin_frames[(size_t)s].empty()) return LS_OK;
    PinArgs p = pin_args(h);
    p.slot = s; p.K = p.P;
    HIPCHK(h, launch_pool_pin_clear(p, h->stream));
    h->pl_pin_frames[(size_t)s].clear();
    return LS_OK;
}

// Everything of a push behind its argument checks.  win[s]: the windows slot s runs (ls_long_pool_plan), pc: the plan's calls, round
// after round (a round is one call, or with pinned poses two: its unpinned rows, then its pinned ones).  Ahead of every round each
// slot takes as much of its chunk as its ring has room for -- a slot's next window
// always fits behind the samples its earlier windows made dead -- so the rounds are the plan's whatever the chunk sizes.  Per call:
// k_pool_gather (a pinned call: and k_pool_pin_gather) -> WavEncoder -> k_build_feats at batch A, the per-batch stages at A, the
// window body, k_pool_scatter.  Nothing is allocated from the first launch on.
int session_push_run(ls_handle* h, const char* entry, const ls_long_pool_push_args* a, ChainCall& cc, const std::vector<int32_t>& win,
                     const PoolCalls& pc, int n_rounds, const std::vector<uint64_t>& row_keys) {
    const int S = h->pl_S, JF = h->JF, T = h->T, npre = h->cfg.n_pre_seq, AL = h->cfg.audio_len, R = h->pl_R, od = a->on_device, cap = a->capacity;
    const bool beat = h->cfg.n_prefix_tokens == 2, lockstep = h->pl_lockstep != ls_handle::kPool;
    const int n_calls = (int)pc.counts.size();
    const bool noised = !beat;          // the TED tree re-noises the kept motion of a pinned window, the BEAT tree does not
    bool any_pinned = false;
    for (int32_t p : pc.pinned) any_pinned = any_pinned || p != 0;
    const hipMemcpyKind kind = od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t st = h->stream;
    int rc;
    auto closing = [&](int s) { return a->closing && a->closing[s] && h->pl_open[(size_t)s]; };
    // the held conditioning: what this call passes holds for every window started from here on; consecutive slots given alike go in one copy
    for (int s = 0, n; s < S && a->given; s += n) {
        const int g = a->given[s];
        for (n = 1; s + n < S && a->given[s + n] == g;) ++n;
        if ((g & 1) && (rc = pool_hold_emo(h, s, n, a->emo + s, od)) != LS_OK) return rc;
        if ((g & 2) && (rc = pool_hold_text(h, s, n, a->text_features + (size_t)s * kD, od)) != LS_OK) return rc;
    }
    const size_t out_bytes = (size_t)S * JF * cap * sizeof(float), nxS = (size_t)S * JF * T * sizeof(float);
    float* out = a->frames;
    if (n_rounds > 0) {         // what the rounds need beyond the open's buffers, sized for S slots while nothing is in flight
        if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
        h->seg_next = -1;
        if (cc.tape) {
            if ((rc = ensure_pinned(h, h->eps_tape, (size_t)cc.n_exec * 2 * S * kD * sizeof(float))) != LS_OK || (rc = ensure_pinned(h, h->noise_tape, cc.n_exec * nxS)) != LS_OK) return rc;
            if (!od) { HIPCHK(h, h->lg_x.ensure(nxS)); HIPCHK(h, h->lg_eps.ensure((size_t)cc.n_exec * 2 * S * kD * sizeof(float))); HIPCHK(h, h->lg_nz.ensure(cc.n_exec * nxS)); }
            if (any_pinned && noised) {     // the re-noise tape of a pinned call
                if ((rc = ensure_pinned(h, h->inp_tape, cc.n_exec * nxS)) != LS_OK) return rc;
                if (!h->pl_pin_tape_od) HIPCHK(h, h->lg_inz.ensure(cc.n_exec * nxS));
            }
        }
        if (!row_keys.empty() && (rc = size_key_ring(h, S, cc.n_exec)) != LS_OK) return rc;       // grows only when the schedule or the ring's budget did since the pool was keyed
        if (!row_keys.empty() && h->pl_pin_P && noised && (rc = size_key_ring(h, S, cc.n_exec, true)) != LS_OK) return rc;     // ... the re-noise tape beside them, likewise
        if (h->pl_pin_P && ((rc = ensure_pinned(h, h->inp_maskf, nxS)) != LS_OK || (rc = ensure_pinned(h, h->inp_motion, nxS)) != LS_OK ||
                            (rc = ensure_pinned(h, h->fwd_cfg, nxS)) != LS_OK)) return rc;       // in place since ls_long_pool_pins
        if (a->sag) {
            cc.sag = a->sag; cc.sag_st = ls_sag_stream(a->sag);
            HIPCHK(h, hipMemsetAsync(h->lg_mask.p, 1, (size_t)S * T, st));
            cc.wa.init_image = cc.sag_out = h->lg_init.f();
        }
        if (!od) { HIPCHK(h, h->lg_timeline.ensure(out_bytes)); out = h->lg_timeline.f(); }
        HIPCHK(h, hipMemsetAsync(out, 0, out_bytes, st));      // a slot's row is zero behind its own frames
    }
    std::vector<long long> fed((size_t)S, 0);
    std::vector<int> pos((size_t)S), take((size_t)S), copies;
    auto feed = [&]() -> int {          // feed_copies: one strided copy per run of slots fed alike (a stream: one run)
        for (int s = 0; s < S; ++s) {
            const long long left = a->lengths[s] - fed[(size_t)s], room = R - (h->pl_samples[(size_t)s] - (long long)LS_LONG_AUDIO_STRIDE * h->pl_windows[(size_t)s]);
            take[(size_t)s] = (int)(left < room ? left : room);
            pos[(size_t)s] = (int)(h->pl_samples[(size_t)s] % R);
        }
        feed_copies(S, R, pos.data(), fed.data(), take.data(), copies);
        for (size_t i = 0; i < copies.size(); i += 5) {
            const int s = copies[i], n = copies[i + 1];
            const float* src = a->audio + (size_t)s * (size_t)a->n_max + (size_t)fed[(size_t)s] + (size_t)copies[i + 3];
            HIPCHK(h, hipMemcpy2DAsync(h->pl_ring.f() + (size_t)s * R + copies[i + 2], (size_t)R * sizeof(float), src, (size_t)a->n_max * sizeof(float),
                                       (size_t)copies[i + 4] * sizeof(float), (size_t)n, kind, st));
        }
        for (int s = 0; s < S; ++s)
            if (take[(size_t)s] > 0) { fed[(size_t)s] += take[(size_t)s]; h->pl_samples[(size_t)s] += take[(size_t)s]; }
        return LS_OK;
    };
    PoolArgs pa{};
    pa.table = static_cast<const int*>(h->pl_table.p);
    pa.ring = h->pl_ring.f(); pa.clips = h->lg_clips.f(); pa.hand = h->pl_hand.f(); pa.feat_u = h->feat_u.f(); pa.origin_x = h->origin_x.f();
    pa.vid_s = static_cast<const int64_t*>(h->pl_vid.p); pa.scale_s = h->pl_scale.f(); pa.vid = static_cast<int64_t*>(h->vid.p); pa.scale = h->scale.f();
    if (beat) { pa.emo_tok_s = h->pl_emotok.f(); pa.emo_tok = h->emo_tok.f(); }
    if (a->sag) { pa.text_s = h->pl_text.f(); pa.text = h->pl_ctext.f(); }
    pa.frames = out;
    pa.S = S; pa.AL = AL; pa.R = R; pa.JF = JF; pa.T = T; pa.KPP = h->KPP; pa.n_pre = npre; pa.T_total = cap;
    std::vector<int> t_off((size_t)S, 0), table((size_t)S * kPoolRow, 0);
    PinArgs pin = pin_args(h);
    pin.table = pa.table; pin.motion = h->inp_motion.f(); pin.maskf = h->inp_maskf.f();
    const size_t per_n = (size_t)cc.n_exec * JF * T;        // floats of one row's noise tape
    size_t at = 0, at_inz = 0;  // position in pc.rows = rows of the calls run so far (the packed tapes); likewise among the pinned calls' rows (the re-noise tape)
    int fed_round = -1;
    for (int q = 0; q < n_calls; ++q) {
        const int A = pc.counts[(size_t)q];
        const bool pinned = pc.pinned[(size_t)q] != 0;
        if (pc.round[(size_t)q] != fed_round) {         // once per round, ahead of its first call
            if ((rc = feed()) != LS_OK) return rc;
            fed_round = pc.round[(size_t)q];
        }
        const int32_t* slots = pc.rows.data() + at;
        bool ones = true;
        for (int i = 0; i < A; ++i) {
            const int s = slots[i];
            const long long w = h->pl_windows[(size_t)s], lo = w * LS_LONG_AUDIO_STRIDE, have = h->pl_samples[(size_t)s] - lo;
            const int valid = (int)(have < AL ? (have < 0 ? 0 : have) : AL), f0 = w == 0 ? 0 : npre;
            if (valid < AL && !(closing(s) && fed[(size_t)s] == a->lengths[s])) return fail(h, LS_ESTATE, "%s: window %lld of slot %d is not complete", entry, w, s);
            if (t_off[(size_t)s] + T - f0 > cap) return fail(h, LS_ESTATE, "%s: slot %d runs more frames than the call was planned for", entry, s);
            int* row = &table[(size_t)i * kPoolRow];
            row[0] = s; row[1] = (int)(lo % R); row[2] = valid; row[3] = f0; row[4] = t_off[(size_t)s];
            row[5] = pinned ? (int)(w * (T - npre) % h->pl_pin_P) : 0;         // a pinned call: where the window's frame 0 sits in the slot's pin ring
            ones = ones && h->pl_scale_host[(size_t)s] == 1.0f;
        }
        // the round's table: one upload of pageable memory, taken into the runtime's staging memory before the call returns (as call_host is)
        HIPCHK(h, hipMemcpyAsync(h->pl_table.p, table.data(), (size_t)A * kPoolRow * sizeof(int), hipMemcpyHostToDevice, st));
        // a keyed pool: the round's rows of the key table, likewise; the captured loop of batch A reads them from row_gidx
        if (!row_keys.empty()) HIPCHK(h, hipMemcpyAsync(h->row_gidx.p, row_keys.data() + at, (size_t)A * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        HIPCHK(h, launch_pool_gather(pa, A, st));
        if (pinned) HIPCHK(h, launch_pool_pin_gather(pin, A, st));      // the inpainting planes of rows [0, A); the bytes it reads set are cleared
        if ((rc = run_wav_encoder(h, h->lg_clips.f(), A)) != LS_OK) return rc;
        HIPCHK(h, launch_build_feats(h->origin_x.f(), h->c4.f(), h->lg_featp.f(), h->lg_featc.f(), A, JF, h->KPP, 0, st, T));
        // from here on the handle is prepared for a batch of A: its scales decide the single-pass form, its size the step plan
        h->B = A;
        h->all_scale_one = ones;
        set_plan(h, A);
        if ((rc = plan_workspaces(h)) != LS_OK) return rc;
        // The speaker style of rows [0, A) is a function of the round's slots and their speaker ids.  Only prepare_style writes the style
        // buffers (z, z_ml, z_mu, z_logvar, z_std: the step kernels read them), and every caller of it but this one and session_open
        // ends the session first (ls_prepare*, ls_long_prepare); a join that changes a slot's speaker empties pl_styled.  So the style
        // of the same slots as last time is in place, and a stream styles once.
        if (h->pl_styled.size() != (size_t)A || !std::equal(slots, slots + A, h->pl_styled.begin())) {
            h->pl_styled.clear();
            if ((rc = prepare_style(h, A)) != LS_OK) return rc;
            h->pl_styled.assign(slots, slots + A);
        }
        Window wn;
        wn.w = h->pl_rounds; wn.Bw = A; wn.featc = h->lg_featc.f(); wn.text = a->sag ? h->pl_ctext.f() : nullptr; wn.first = q == 0;
        wn.resident_inpaint = pinned;       // the reference's inpainting branch on the planes k_pool_pin_gather filled; its own captured loop
        cc.wa.inpaint_noised = pinned && noised ? 1 : 0;
        // a pool: a batch size met once is met again, and kKeep never destroys a graph under the replays in flight.  A stream without
        // pins has one batch and one key per call: a key that is not cached replaces what is.  A stream WITH pins has two loops at its
        // batch, the plain one and the inpainting one, and one push may run both with no host wait between them: it keeps both, like a
        // pool (ls_long_pool_pins emptied the cache, so both fit)
        wn.policy = lockstep && !h->pl_pin_P ? kReplace : kKeep;
        wn.keyed = !row_keys.empty();
        if (cc.tape) {
            wn.x_init = a->x_init + at * JF * T; wn.eps_tape = a->eps_tape + at * cc.n_exec * 2 * kD; wn.noise_tape = a->noise_tape + at * cc.n_exec * JF * T;
            wn.host_tapes = !od;
            if (pinned && noised) { wn.inpaint_noise = h->pl_pin_tape + at_inz * per_n; wn.host_inz = !h->pl_pin_tape_od; }
        }
        if ((rc = run_window(h, cc, wn)) != LS_OK) return rc;
        pa.prev = x_plane(h, cc.n_exec);
        HIPCHK(h, launch_pool_scatter(pa, A, st));
        for (int i = 0; i < A; ++i) {
            if (pinned) pins_consumed(h, slots[i], h->pl_windows[(size_t)slots[i]]);
            t_off[(size_t)slots[i]] += T - table[(size_t)i * kPoolRow + 3];
            ++h->pl_windows[(size_t)slots[i]];
        }
        ++h->pl_rounds;         // sampling calls since the open: the PHILOX window index of the next one
        at += (size_t)A;
        if (pinned) at_inz += (size_t)A;
    }
    if ((rc = feed()) != LS_OK) return rc;
    bool any = false;
    for (int s = 0; s < S; ++s) {
        if (fed[(size_t)s] != a->lengths[s]) return fail(h, LS_ESTATE, "%s: no room in the ring of slot %d and no window to run", entry, s);
        any = any || fed[(size_t)s] > 0;
        h->pl_frames[(size_t)s] += t_off[(size_t)s];
        if (a->n_frames) a->n_frames[s] = t_off[(size_t)s];
        if (closing(s)) {
            if ((rc = pins_drop(h, s)) != LS_OK) return rc;        // the pins the clip never reached
            h->pl_open[(size_t)s] = 0;
        }
    }
    if (a->n_rounds) *a->n_rounds = n_rounds;
    if (n_rounds == 0) {        // no sampling work: a host chunk is the caller's again once its copies are done, a device chunk is read in stream order
        if ((!od && any) || a->given) { HIPCHK(h, hipEventRecord(h->ev[6], st)); HIPCHK(h, hipEventSynchronize(h->ev[6])); }
        return LS_OK;
    }
    return chain_finish(h, cc, {{od ? nullptr : a->frames, out, out_bytes}});
}

// The re-noise tape ls_long_pool_pin_tape handed over is the next push's alone: however that push ends -- refused by its entry, refused
// here, or run -- the handle forgets the caller's pointer
struct ForgetTape {
    ls_handle* h;
    ~ForgetTape() { h->pl_pin_tape = nullptr; h->pl_pin_tape_floats = 0; }
};

// A push of a session behind its entry's own refusals: the plan, the refusals the plan decides, the sampler arguments, the rounds.
// Nothing ahead of session_push_run touches the device.
int session_push(ls_handle* h, const char* entry, const ls_long_pool_push_args* a) {
    const int S = h->pl_S;
    const ForgetTape forget_tape{h};
    if (!a->lengths || a->n_max < 0 || (a->n_max > 0 && !a->audio)) return fail(h, LS_EINVAL, "%s: lengths, and audio with n_max > 0", entry);
    if (a->capacity < 0 || (a->capacity > 0 && !a->frames)) return fail(h, LS_EINVAL, "%s: capacity without frames", entry);
    if (a->emo && h->cfg.n_prefix_tokens != 2) return fail(h, LS_EINVAL, "%s: emo is a BEAT conditioning", entry);
    if (a->text_features && !a->sag) return fail(h, LS_EINVAL, "%s: text_features without sag", entry);
    std::vector<int32_t> closing((size_t)S, 0), open((size_t)S, 0), win((size_t)S, 0), frames((size_t)S, 0);
    for (int s = 0; s < S; ++s) {
        if (a->lengths[s] < 0 || a->lengths[s] > a->n_max) return fail(h, LS_EINVAL, "%s: lengths[%d] = %lld outside [0, %lld]", entry, s, (long long)a->lengths[s], (long long)a->n_max);
        open[(size_t)s] = h->pl_open[(size_t)s];
        closing[(size_t)s] = a->closing && a->closing[s];
        if (a->given && ((a->given[s] & ~3) || ((a->given[s] & 1) && !a->emo) || ((a->given[s] & 2) && !a->text_features) || (a->given[s] && !open[(size_t)s])))
            return fail(h, LS_EINVAL, "%s: given[%d] = %d names conditioning that was not passed, or a slot that is not open", entry, s, a->given[s]);
    }
    int32_t n_rounds = 0, n_entries = 0;
    const std::vector<int64_t> before(h->pl_samples.begin(), h->pl_samples.end()), ran(h->pl_windows.begin(), h->pl_windows.end());
    if (ls_long_pool_plan(S, h->cfg.audio_len, before.data(), ran.data(), a->lengths, closing.data(), open.data(), win.data(), frames.data(), nullptr, 0, &n_rounds, &n_entries) != LS_OK)
        return fail(h, LS_EINVAL, "%s: samples for a slot that is not open, or closing a slot that was fed no sample", entry);
    std::vector<int32_t> rounds((size_t)n_entries);
    if (ls_long_pool_plan(S, h->cfg.audio_len, before.data(), ran.data(), a->lengths, closing.data(), open.data(), win.data(), nullptr, rounds.data(), n_entries, &n_rounds, &n_entries) != LS_OK)
        return fail(h, LS_EINVAL, "%s: ls_long_pool_plan failed", entry);
    for (int s = 0; s < S; ++s) {
        if (frames[(size_t)s] > a->capacity) return fail(h, LS_EINVAL, "%s: slot %d runs %d windows = %d frames, capacity is %d", entry, s, win[(size_t)s], frames[(size_t)s], a->capacity);
        if (win[(size_t)s] > 0 && ran[(size_t)s] == 0) {        // the slot's first window: what it needs must be held by now
            const int g = a->given ? a->given[s] : 0;
            if (h->cfg.n_prefix_tokens == 2 && !h->pl_have_emo[(size_t)s] && !(g & 1)) return fail(h, LS_EINVAL, "%s: the BEAT variant's first window needs emo ids (slot %d)", entry, s);
            if (a->sag && !h->pl_have_text[(size_t)s] && !(g & 2)) return fail(h, LS_EINVAL, "%s: sag needs text_features for the first window (slot %d)", entry, s);
        }
    }
    // the sampling calls: the rounds, each split where pending pins say so (ls_long_pool_pin_plan; without pins: the rounds themselves)
    PoolCalls pc;
    int32_t n_calls = 0;
    long long pinned_rows = 0;
    {
        std::vector<int32_t> first;
        std::vector<int64_t> pend;
        if (h->pl_pin_P) {
            first.assign((size_t)S + 1, 0);
            for (int s = 0; s < S; ++s) {
                pend.insert(pend.end(), h->pl_pin_frames[(size_t)s].begin(), h->pl_pin_frames[(size_t)s].end());
                first[(size_t)s + 1] = (int32_t)pend.size();
            }
        }
        const int32_t* pf = h->pl_pin_P ? first.data() : nullptr;
        const int64_t* pn = pend.empty() ? nullptr : pend.data();
        int32_t n_rows = 0;
        if (ls_long_pool_pin_plan(S, h->T, h->cfg.n_pre_seq, ran.data(), win.data(), pf, pn, nullptr, 0, nullptr, nullptr, nullptr, 0, &n_calls, &n_rows) != LS_OK || n_rows != n_entries)
            return fail(h, LS_EINVAL, "%s: ls_long_pool_pin_plan failed", entry);
        pc.rows.resize((size_t)n_entries); pc.counts.resize((size_t)n_calls); pc.pinned.resize((size_t)n_calls); pc.round.resize((size_t)n_calls);
        if (n_calls > 0 && ls_long_pool_pin_plan(S, h->T, h->cfg.n_pre_seq, ran.data(), win.data(), pf, pn, pc.rows.data(), n_entries, pc.counts.data(), pc.pinned.data(),
                                                 pc.round.data(), n_calls, &n_calls, &n_rows) != LS_OK)
            return fail(h, LS_EINVAL, "%s: ls_long_pool_pin_plan failed", entry);
        for (int q = 0; q < n_calls; ++q) pinned_rows += pc.pinned[(size_t)q] ? pc.counts[(size_t)q] : 0;
    }
    if (pinned_rows > 0 && a->sag) return fail(h, LS_EUNSUPPORTED, "%s: a pinned window with sag is not built (it would start from edit_start(motion, mask, sag_out))", entry);
    ChainCall cc;
    int rc;
    if ((rc = chain_args(h, entry, a, n_rounds > 0, cc)) != LS_OK) return rc;
    if (pinned_rows > 0 && cc.tape && h->cfg.n_prefix_tokens != 2) {       // TED re-noises the kept motion: the pinned calls' third tape
        const long long need = pinned_rows * cc.n_exec * h->JF * h->T;
        if (!h->pl_pin_tape || h->pl_pin_tape_floats != need)
            return fail(h, LS_EINVAL, "%s: TAPE mode with pinned windows needs the re-noise tape of its %lld pinned rows (%lld floats, ls_long_pool_pin_tape), got %lld",
                        entry, pinned_rows, need, h->pl_pin_tape ? h->pl_pin_tape_floats : 0ll);
    }
    std::vector<uint64_t> row_keys;         // a keyed pool under PHILOX: one gidx per row of every call (ls_long_pool_keys); empty otherwise
    if (n_rounds > 0 && !cc.tape && h->pl_keyed) {
        std::vector<uint64_t> round_keys((size_t)n_entries);
        int32_t n_keys = 0;
        const int krc = ls_long_pool_keys(S, h->pl_key.data(), ran.data(), win.data(), round_keys.data(), n_entries, &n_keys);
        if (krc == LS_ESTATE) return fail(h, LS_ESTATE, "%s: a clip of a keyed pool runs at most 2^16 windows; let it leave and join again under another key", entry);
        if (krc != LS_OK || n_keys != n_entries) return fail(h, LS_EINVAL, "%s: ls_long_pool_keys failed", entry);
        // the table is in round order; a round's calls hold the same rows, the unpinned ones first: each row keeps its slot's key
        std::vector<uint64_t> of_slot((size_t)n_rounds * S, 0);
        for (size_t i = 0, r = 0; r < (size_t)n_rounds; ++r)
            for (int s = 0; s < S; ++s)
                if (win[(size_t)s] > (int)r) of_slot[r * S + (size_t)s] = round_keys[i++];
        row_keys.resize((size_t)n_entries);
        for (size_t q = 0, i = 0; q < (size_t)n_calls; ++q)
            for (int k = 0; k < pc.counts[q]; ++k, ++i) row_keys[i] = of_slot[(size_t)pc.round[q] * S + pc.rows[i]];
    } else if (n_rounds > 0 && !cc.tape) {
        if ((a->sample_offset + (unsigned long long)S) >> 48) return fail(h, LS_EINVAL, "PHILOX: sample_offset + capacity must stay below 2^48 (the round index sits above)");
        if (h->pl_rounds + n_calls > (1 << 16)) return fail(h, LS_ESTATE, "%s: PHILOX keys a round by its index since open, which stays below 2^16; open a new session", entry);
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    rc = session_push_run(h, entry, a, cc, win, pc, n_rounds, row_keys);
    if (rc != LS_OK) {      // rings and hand-off stores may be half written: the session is over, the handle is not
        h->pl_state = ls_handle::kStreamFailed;
        (void)hipStreamSynchronize(h->stream);
    }
    return rc;
}

}  // namespace

extern "C" {

// Once-per-call stage of a long-form call (ls_long_cond in ls_hip.h).  The WavEncoder has no term that couples clips (InstanceNorm is per
// clip and channel), so the W * B clip-windows go through it in chunks of any size and leave the features ls_prepare would compute for
// each window at batch B; k_build_feats turns a chunk's conv4 block into its rows of the feature store (its feat_p half goes to a scratch:
// the prefix rows are k_chain_window's).  Everything else is ls_prepare's own stage at batch B.
int ls_long_prepare(ls_handle* h, const ls_long_cond* c) {
    if (!h || !c) return fail(h, LS_EINVAL, "ls_long_prepare: null argument");
    int rc;
    if ((rc = check_cond(h, "ls_long_prepare", c->batch, &c->n_windows, c->audio_samples >= 1 && c->encoder_chunk >= 0,
                         c->audio && c->seed_poses && c->vid_indices && c->scale, h->cfg.n_prefix_tokens != 2 || c->emo)) != LS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = c->batch, W = c->n_windows, JF = h->JF, T = h->T, AL = h->cfg.audio_len, KPP = h->KPP, od = c->on_device;
    const size_t L = (size_t)AL + (size_t)(W - 1) * LS_LONG_AUDIO_STRIDE, Lin = (size_t)c->audio_samples < L ? (size_t)c->audio_samples : L;
    const int chunk = c->encoder_chunk > 0 ? c->encoder_chunk : 256;
    const hipMemcpyKind kind = od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    hipStream_t st = h->stream;
    end_stream(h);
    if ((rc = start_prepare(h)) != LS_OK) return rc;
    HIPCHK(h, h->lg_audio.ensure((size_t)B * L * sizeof(float)));
    if (Lin < L) HIPCHK(h, hipMemsetAsync(h->lg_audio.p, 0, (size_t)B * L * sizeof(float), st));
    HIPCHK(h, hipMemcpy2DAsync(h->lg_audio.p, L * sizeof(float), c->audio, (size_t)c->audio_samples * sizeof(float), Lin * sizeof(float), B, kind, st));
    if ((rc = ingest_cond(h, B, od, c->seed_poses, c->vid_indices, c->scale, c->emo, (size_t)W * B)) != LS_OK) return rc;
    if (!od) HIPCHK(h, hipStreamSynchronize(st));       // host inputs are the caller's again
    // ---- WavEncoder over the clip-windows cw = w * B + b, `chunk` at a time
    const int ncw = W * B, nmax = chunk < ncw ? chunk : ncw;
    HIPCHK(h, h->lg_clips.ensure((size_t)nmax * AL * sizeof(float)));
    HIPCHK(h, h->lg_featc.ensure((size_t)ncw * T * kAudioFeat * sizeof(float)));
    HIPCHK(h, h->lg_featp.ensure((size_t)nmax * T * KPP * sizeof(float)));
    if ((rc = zero_origin_x(h, B)) != LS_OK) return rc;
    for (int cw0 = 0; cw0 < ncw; cw0 += chunk) {
        const int n = ncw - cw0 < chunk ? ncw - cw0 : chunk;
        for (int cw = cw0; cw < cw0 + n;) {             // one strided copy per run of clips of the same window
            const int w = cw / B, b = cw - w * B, run = (B - b) < (cw0 + n - cw) ? (B - b) : (cw0 + n - cw);
            HIPCHK(h, hipMemcpy2DAsync(h->lg_clips.f() + (size_t)(cw - cw0) * AL, (size_t)AL * sizeof(float),
                                       h->lg_audio.f() + (size_t)b * L + (size_t)w * LS_LONG_AUDIO_STRIDE, L * sizeof(float), (size_t)AL * sizeof(float), run,
                                       hipMemcpyDeviceToDevice, st));
            cw += run;
        }
        if ((rc = run_wav_encoder(h, h->lg_clips.f(), n)) != LS_OK) return rc;
        HIPCHK(h, launch_build_feats(h->origin_x.f(), h->c4.f(), h->lg_featp.f(), h->lg_featc.f() + (size_t)cw0 * T * kAudioFeat, n, JF, KPP, 0, st, T));
    }
    // ---- per-batch stages, once: the buffers, style, emotion tokens, plan
    if ((rc = size_batch_buffers(h, B)) != LS_OK) return rc;
    if ((rc = prepare_style(h, B)) != LS_OK) return rc;
    if (h->cfg.n_prefix_tokens == 2) {
        HIPCHK(h, h->lg_emotok.ensure((size_t)W * B * kD * sizeof(float)));
        HIPCHK(h, launch_gather_rows(h->emo_emb.f(), static_cast<const int64_t*>(h->lg_emo_ids.p), h->lg_emotok.f(), W * B, kD, h->cfg.n_emotions, st));
    }
    if ((rc = prepare_plan(h, B)) != LS_OK) return rc;
    if ((rc = finish_prepare(h, B)) != LS_OK) return rc;
    h->lg_W = W; h->lg_L = L;
    h->lg_prepared = true;      // `prepared` stays false: the static projections exist per window, inside ls_long_sample only
    return LS_OK;
}

// ls_long_prepare for clips of different lengths (ls_hip.h): the encoder sees only the clip-windows that exist, gathered from the
// caller's waveform by k_long_gather_clips and stored packed, window-major in slot order; every window batch is planned and every
// workspace a captured loop holds by address is sized for all of them here, so that nothing moves once ls_long_sample has begun.
// The speaker style is ls_long_sample's (per window batch).
int ls_long_prepare_ragged(ls_handle* h, const ls_long_cond* c, const int64_t* audio_lengths) {
    if (!h || !c || !audio_lengths) return fail(h, LS_EINVAL, "ls_long_prepare_ragged: null argument");
    int rc;
    if ((rc = check_cond(h, "ls_long_prepare_ragged", c->batch, &c->n_windows, c->audio_samples >= 1 && c->encoder_chunk >= 0,
                         c->audio && c->seed_poses && c->vid_indices && c->scale, h->cfg.n_prefix_tokens != 2 || c->emo)) != LS_OK) return rc;
    if (c->audio_samples > 0x7fffffffLL) return fail(h, LS_EINVAL, "ls_long_prepare_ragged: audio_samples beyond 2^31 - 1");
    const int B = c->batch, W = c->n_windows, JF = h->JF, T = h->T, AL = h->cfg.audio_len, KPP = h->KPP, od = c->on_device;
    for (int b = 0; b < B; ++b)
        if (audio_lengths[b] < 1 || audio_lengths[b] > c->audio_samples)
            return fail(h, LS_EINVAL, "audio_lengths[%d] = %lld outside [1, %lld]", b, (long long)audio_lengths[b], (long long)c->audio_samples);
    std::vector<int> row, wins, bw;
    long_plan_drop(B, AL, audio_lengths, row, wins, bw);
    if ((int)bw.size() != W) return fail(h, LS_EINVAL, "n_windows is %d, the longest clip needs %d", W, (int)bw.size());
    std::vector<int> off((size_t)W + 1, 0);
    for (int w = 0; w < W; ++w) off[(size_t)w + 1] = off[(size_t)w] + bw[(size_t)w];
    const int total = off[(size_t)W];
    std::vector<int> table((size_t)total * 2), lens((size_t)B);
    for (int w = 0, p = 0; w < W; ++w)
        for (int s = 0; s < bw[(size_t)w]; ++s, ++p) { table[(size_t)2 * p] = row[(size_t)s]; table[(size_t)2 * p + 1] = w; }
    for (int b = 0; b < B; ++b) lens[(size_t)b] = (int)audio_lengths[b];          // <= audio_samples, checked; the kernel compares in 64 bits
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int chunk = c->encoder_chunk > 0 ? c->encoder_chunk : 256;
    if (chunk > 32768) chunk = 32768;                   // one grid row per clip-window of a chunk
    hipStream_t st = h->stream;
    end_stream(h);
    if ((rc = start_prepare(h)) != LS_OK) return rc;
    // a device-resident waveform is read in place (the call waits before it returns); a host one is uploaded as it is, unpadded
    const float* audio = c->audio;
    if (!od) {
        if ((rc = ingest(h, h->lg_audio, c->audio, (size_t)B * (size_t)c->audio_samples * sizeof(float), 0)) != LS_OK) return rc;
        audio = h->lg_audio.f();
    }
    if ((rc = ingest_cond(h, B, od, c->seed_poses, c->vid_indices, c->scale, c->emo, (size_t)W * B, &h->lg_scale_ones)) != LS_OK) return rc;
    if ((rc = ingest(h, h->lg_row, row.data(), (size_t)B * sizeof(int), 0)) != LS_OK) return rc;
    if ((rc = ingest(h, h->lg_lens, lens.data(), (size_t)B * sizeof(int), 0)) != LS_OK) return rc;
    if ((rc = upload(h, h->lg_table, table.data(), table.size() * sizeof(int))) != LS_OK) return rc;      // waits: host inputs and these temporaries are free again
    // ---- WavEncoder over the packed clip-windows p = lg_off[w] + slot, `chunk` at a time
    const int nmax = chunk < total ? chunk : total;
    HIPCHK(h, h->lg_clips.ensure((size_t)nmax * AL * sizeof(float)));
    HIPCHK(h, h->lg_featc.ensure((size_t)total * T * kAudioFeat * sizeof(float)));
    HIPCHK(h, h->lg_featp.ensure((size_t)nmax * T * KPP * sizeof(float)));
    if ((rc = zero_origin_x(h, B)) != LS_OK) return rc;
    for (int p0 = 0; p0 < total; p0 += chunk) {
        const int n = total - p0 < chunk ? total - p0 : chunk;
        HIPCHK(h, launch_long_gather_clips(audio, static_cast<const int*>(h->lg_table.p) + (size_t)2 * p0, static_cast<const int*>(h->lg_lens.p), h->lg_clips.f(), n, AL,
                                           (long long)c->audio_samples, LS_LONG_AUDIO_STRIDE, st));
        if ((rc = run_wav_encoder(h, h->lg_clips.f(), n)) != LS_OK) return rc;
        HIPCHK(h, launch_build_feats(h->origin_x.f(), h->c4.f(), h->lg_featp.f(), h->lg_featc.f() + (size_t)p0 * T * kAudioFeat, n, JF, KPP, 0, st, T));
    }
    if ((rc = size_batch_buffers(h, B)) != LS_OK) return rc;        // at the whole batch: window 0's
    if (h->cfg.n_prefix_tokens == 2) {                  // the emotion tokens of every window's active clips
        HIPCHK(h, h->lg_emotok.ensure((size_t)W * B * kD * sizeof(float)));
        for (int w = 0; w < W; ++w)                     // ids of (window, slot) pairs that do not run are never read
            HIPCHK(h, launch_gather_rows(h->emo_emb.f(), static_cast<const int64_t*>(h->lg_emo_ids.p) + (size_t)w * B, h->lg_emotok.f() + (size_t)w * B * kD,
                                         bw[(size_t)w], kD, h->cfg.n_emotions, st));
    }
    // ---- the plan and the workspaces of every window batch, smallest first: the handle is left planned for the whole batch
    for (int w = W - 1; w >= 0; --w) {
        if (w + 1 < W && bw[(size_t)w] == bw[(size_t)w + 1]) continue;
        h->all_scale_one = h->lg_scale_ones >= bw[(size_t)w];
        set_plan(h, bw[(size_t)w]);
        if ((rc = plan_workspaces(h)) != LS_OK) return rc;
    }
    if ((rc = finish_prepare(h, B)) != LS_OK) return rc;
    h->lg_W = W; h->lg_L = (size_t)c->audio_samples;
    h->lg_bw = bw; h->lg_off = off;
    h->lg_prepared = h->lg_ragged = true;
    return LS_OK;
}

// Long-form synthesis (ls_long_sample_args in ls_hip.h): per window the hand-off kernel, then the window body; one wait at the end.
//
// After ls_long_prepare_ragged window w runs the lg_bw[w] clips that still have audio: slots [0, lg_bw[w]) of every per-clip buffer
// (the clips are held longest-first), the packed stores at lg_off[w].  Each window is then, decision for decision, a call at batch
// lg_bw[w]: its scales decide the single-pass form, its batch the step plan (set_plan), the plan the workspaces' accounting
// (plan_workspaces; ls_long_prepare_ragged sized them for every window, so nothing a captured loop holds moves here), and the speaker
// style runs at that batch.  A window batch that serves two or more windows is captured once and replayed; one that serves a single
// window runs as stream launches unless an earlier call left its graph behind.
int ls_long_sample(ls_handle* h, const ls_long_sample_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_long_sample: null argument");
    if (!h->lg_prepared) return fail(h, LS_ESTATE, "ls_long_sample before ls_long_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_long_sample before ls_set_schedule");
    if (!a->timeline) return fail(h, LS_EINVAL, "ls_long_sample: null timeline");
    if (a->sag && !a->text_features) return fail(h, LS_EINVAL, "ls_long_sample: sag without text_features");
    const bool rg = h->lg_ragged, beat = h->cfg.n_prefix_tokens == 2;
    const int B = h->B, W = h->lg_W, JF = h->JF, T = h->T, npre = h->cfg.n_pre_seq, od = a->on_device;
    const int Tt = T + (W - 1) * (T - npre);
    if (rg && ((int)h->lg_bw.size() != W || (int)h->lg_off.size() != W + 1 || h->lg_bw[0] != B)) return fail(h, LS_ESTATE, "ls_long_sample: the ragged plan does not match the prepared batch");
    auto batch_of = [&](int w) { return rg ? h->lg_bw[(size_t)w] : B; };                      // clips that run window w
    auto first_of = [&](int w) { return (size_t)(rg ? h->lg_off[(size_t)w] : w * B); };       // clip-windows ahead of window w in the packed stores
    ChainCall cc;
    int rc;
    if ((rc = chain_args(h, "ls_long_sample", a, true, cc)) != LS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = chain_begin(h, cc, a->sag)) != LS_OK) return rc;
    hipStream_t st = h->stream;
    const int n_exec = cc.n_exec;
    const size_t per_x = (size_t)JF * T, per_e = (size_t)n_exec * 2 * kD, per_n = (size_t)n_exec * per_x;     // floats per clip-window: x_T, eps tape, noise tape
    const size_t nelem = (size_t)B * per_x, nx = nelem * sizeof(float), total = first_of(W);
    // host tapes / text features: one upload per call; device ones are read in place
    const float *xs = a->x_init, *es = a->eps_tape, *ns = a->noise_tape, *tx = a->text_features;
    if (cc.tape && !od) {
        if ((rc = ingest(h, h->lg_x, xs, total * per_x * sizeof(float), 0)) != LS_OK || (rc = ingest(h, h->lg_eps, es, total * per_e * sizeof(float), 0)) != LS_OK ||
            (rc = ingest(h, h->lg_nz, ns, total * per_n * sizeof(float), 0)) != LS_OK) return rc;
        xs = h->lg_x.f(); es = h->lg_eps.f(); ns = h->lg_nz.f();
    }
    if (a->sag && !od) { if ((rc = ingest(h, h->lg_text, tx, (size_t)W * B * kD * sizeof(float), 0)) != LS_OK) return rc; tx = h->lg_text.f(); }
    float* tl = a->timeline;
    float* wd = a->windows;
    if (!od) {
        HIPCHK(h, h->lg_timeline.ensure((size_t)B * JF * Tt * sizeof(float)));
        if (wd) HIPCHK(h, h->lg_windows.ensure(W * nx));
        tl = h->lg_timeline.f();
        if (wd) wd = h->lg_windows.f();
    }
    if (rg) {
        // what a clip does not reach stays zero: its timeline beyond its own frames, its raw windows from its window count on
        HIPCHK(h, hipMemsetAsync(tl, 0, (size_t)B * JF * Tt * sizeof(float), st));
        if (wd) HIPCHK(h, hipMemsetAsync(wd, 0, W * nx, st));
        // Room in the graph cache for the batches this call captures (at most the cache's bound; the rest run as stream launches), made
        // now: nothing of this call is in flight yet.  The same window batches as the last ragged call: its graphs are this call's.
        if (h->graphs_for != h->lg_bw) {
            int repeated = 0;
            for (int w = 1; w < W; ++w) if (h->lg_bw[(size_t)w] == h->lg_bw[(size_t)w - 1] && (w < 2 || h->lg_bw[(size_t)w - 1] != h->lg_bw[(size_t)w - 2])) ++repeated;
            if (repeated > ls_handle::kGraphCacheMax) repeated = ls_handle::kGraphCacheMax;
            if ((int)h->graphs.size() + repeated > ls_handle::kGraphCacheMax) free_graph(h);
            h->graphs_for = h->lg_bw;
        }
    }
    ChainArgs ca{};
    ca.seed = h->lg_seed.f(); ca.timeline = tl;
    ca.JF = JF; ca.T = T; ca.KPP = h->KPP; ca.n_pre = npre; ca.T_total = Tt;
    ca.row = rg ? static_cast<const int*>(h->lg_row.p) : nullptr;
    int styled = 0;
    for (int w = 0; w <= W; ++w) {
        const int Bw = w < W ? batch_of(w) : 0, Bprev = w ? batch_of(w - 1) : 0;
        // hand-off: window w - 1 leaves through the timeline, window w's prefix poses enter feat_u / origin_x
        ca.prev = w ? x_plane(h, n_exec) : nullptr;
        ca.feat_u = w < W ? h->feat_u.f() : nullptr; ca.origin_x = h->origin_x.f();
        ca.f0 = w == 1 ? 0 : npre; ca.t_off = w <= 1 ? 0 : T + (w - 2) * (T - npre);
        ca.window = (w && wd) ? wd + (size_t)(w - 1) * nelem : nullptr;
        ca.n_next = Bw;
        HIPCHK(h, launch_chain_window(ca, w ? Bprev : Bw, st));
        if (w == W) break;
        Window win;
        win.w = w; win.Bw = Bw; win.first = w == 0;
        if (rg) {           // from here on the handle is prepared for a batch of Bw
            h->B = Bw;
            h->all_scale_one = h->lg_scale_ones >= Bw;
            set_plan(h, Bw);
            if ((rc = plan_workspaces(h)) != LS_OK) return rc;
            if (styled != Bw && (rc = prepare_style(h, Bw)) != LS_OK) return rc;
            styled = Bw;
            int serves = 0;
            for (int v = 0; v < W; ++v) serves += h->lg_bw[(size_t)v] == Bw;
            win.policy = serves >= 2 ? kKeep : kReplayOnly;
        }
        win.featc = h->lg_featc.f() + first_of(w) * T * kAudioFeat;
        if (beat) win.emo_tok = h->lg_emotok.f() + (size_t)w * B * kD;
        if (a->sag) win.text = tx + (size_t)w * B * kD;
        if (cc.tape) { win.x_init = xs + first_of(w) * per_x; win.eps_tape = es + first_of(w) * per_e; win.noise_tape = ns + first_of(w) * per_n; }
        if ((rc = run_window(h, cc, win)) != LS_OK) return rc;
    }
    if (rg) {               // leave the handle as ls_long_prepare_ragged left it: prepared for the whole batch
        h->B = B;
        h->all_scale_one = h->lg_scale_ones >= B;
        set_plan(h, B);
        if ((rc = plan_workspaces(h)) != LS_OK) return rc;
    }
    return chain_finish(h, cc, {{od ? nullptr : a->timeline, tl, (size_t)B * JF * Tt * sizeof(float)}, {od || !wd ? nullptr : a->windows, wd, W * nx}});
}

// Timeline edit (ls_long_edit_args in ls_hip.h): the window body over the windows of ls_long_edit_plan, with k_edit_gather ahead of a
// window and k_edit_scatter behind it in place of the hand-off kernel, and the loop run with the inpainting branch on the planes the
// gather left on the device.  The loop's key holds the inpainting form.  One wait at the end.
//
// With a SAG decoder (a scripted edit) the gather always leaves the slice in the init plane, the window body decodes (x = the
// window's origin_x, z = its text features, mask = ones) into a plane of its own, lg_sag, and k_edit_start stores that plane's
// editable elements over the init plane behind the decode: the loop starts from q_sample(where(keep, slice, decoder output)) at
// every skip_timesteps >= 0.  The start's q_sample is enqueued ahead of the captured loop (begin_loop), so the loop's key is the
// unscripted edit's.  ls_long_edit is this entry with no decoder.
//
// With an ELEMENT MASK (ls_long_edit_mask) the same code runs: the windows come from the mask's pair flags in place of the ranges,
// and the three edit kernels read the mask (EditArgs::emask) in place of the rectangle.  Nothing else differs; the range entries
// are the mask-less case.
static int long_edit_run(ls_handle* h, const ls_long_edit_args* a, ls_sag* sag, const float* text_features, const unsigned char* emask, bool mask_form) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_long_edit: null argument");
    if (sag && !text_features) return fail(h, LS_EINVAL, "ls_long_edit_sag: sag without text_features");
    if (text_features && !sag) return fail(h, LS_EINVAL, "ls_long_edit_sag: text_features without sag");
    if (!h->lg_prepared) return fail(h, LS_ESTATE, "ls_long_edit before ls_long_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_long_edit before ls_set_schedule");
    if (h->lg_ragged) return fail(h, LS_EUNSUPPORTED, "ls_long_edit: a handle prepared by ls_long_prepare_ragged is not edited (ragged batches are not built)");
    if (!a->timeline) return fail(h, LS_EINVAL, "ls_long_edit: null timeline");
    if (mask_form && !emask) return fail(h, LS_EINVAL, "ls_long_edit_mask: null element_mask");
    if (mask_form && (a->frame_lo || a->frame_hi || a->channels))
        return fail(h, LS_EINVAL, "ls_long_edit_mask: the element mask and frame_lo / frame_hi / channels exclude each other");
    if (!mask_form && (!a->frame_lo || !a->frame_hi)) return fail(h, LS_EINVAL, "ls_long_edit: null frame_lo / frame_hi");
    if (a->windows_capacity < 0 || (a->windows_capacity > 0 && !a->windows_run)) return fail(h, LS_EINVAL, "ls_long_edit: windows_capacity without windows_run");
    const int B = h->B, W = h->lg_W, JF = h->JF, T = h->T, npre = h->cfg.n_pre_seq, od = a->on_device;
    const int Tt = T + (W - 1) * (T - npre);
    // per clip [lo, hi) and the channel bytes; a clip with no channel selected is not edited
    std::vector<int32_t> lo((size_t)B), hi((size_t)B), range((size_t)2 * B), flags((size_t)W);
    std::vector<unsigned char> chan((size_t)B * JF, 1);
    int rc;
    int32_t We = 0;
    if (mask_form) {        // window w runs iff some clip has an editable element in it
        std::vector<unsigned char> pairs;
        if ((rc = mask_pair_flags(h, "ls_long_edit_mask", emask, od, B, W, nullptr, pairs)) != LS_OK) return rc;
        for (int w = 0; w < W; ++w) {
            for (int b = 0; b < B; ++b) flags[(size_t)w] |= pairs[(size_t)w * B + b] ? 1 : 0;
            We += flags[(size_t)w];
        }
        if (We < 1) return fail(h, LS_EINVAL, "ls_long_edit_mask: no window holds an editable element (the mask is empty)");
    }
    for (int b = 0; b < B && !mask_form; ++b) {
        lo[(size_t)b] = a->frame_lo[b]; hi[(size_t)b] = a->frame_hi[b];
        if (lo[(size_t)b] < 0 || lo[(size_t)b] > hi[(size_t)b] || hi[(size_t)b] > Tt)
            return fail(h, LS_EINVAL, "ls_long_edit: clip %d: frames [%d, %d) are no range inside [0, %d]", b, lo[(size_t)b], hi[(size_t)b], Tt);
        if (a->channels) {
            bool any = false;
            for (int c = 0; c < JF; ++c) any |= (chan[(size_t)b * JF + c] = a->channels[(size_t)b * JF + c] ? 1 : 0) != 0;
            if (!any) hi[(size_t)b] = lo[(size_t)b];
        }
        range[(size_t)2 * b] = lo[(size_t)b]; range[(size_t)2 * b + 1] = hi[(size_t)b];
    }
    if (!mask_form) {
        if (ls_long_edit_plan(B, W, T, npre, lo.data(), hi.data(), flags.data(), &We) != LS_OK) return fail(h, LS_EINVAL, "ls_long_edit: bad frame ranges");
        if (We < 1) return fail(h, LS_EINVAL, "ls_long_edit: no window holds an editable element (every range is empty)");
    }
    ChainCall cc;
    if ((rc = chain_args(h, "ls_long_edit", a, true, cc)) != LS_OK) return rc;
    const bool noised = a->inpaint_noised != 0, beat = h->cfg.n_prefix_tokens == 2;
    if (cc.tape && noised && !a->inpaint_noise) return fail(h, LS_EINVAL, "TAPE mode with inpaint_noised needs inpaint_noise");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = chain_begin(h, cc, sag)) != LS_OK) return rc;
    hipStream_t st = h->stream;
    const size_t nelem = (size_t)B * JF * T, nx = nelem * sizeof(float);
    const size_t per_e = (size_t)cc.n_exec * 2 * B * kD, per_n = (size_t)cc.n_exec * nelem;      // floats per window: eps tape, noise tape
    // the ranges and channel bytes, or a host caller's mask: one upload per call (a device mask is read where it is)
    if (!mask_form) {
        if ((rc = upload(h, h->lg_edit_range, range.data(), range.size() * sizeof(int32_t))) != LS_OK) return rc;
        if ((rc = upload(h, h->lg_edit_chan, chan.data(), chan.size())) != LS_OK) return rc;
    } else if (!od) {
        if ((rc = ingest(h, h->lg_edit_mask, emask, (size_t)B * JF * Tt, 0)) != LS_OK) return rc;
        emask = static_cast<const unsigned char*>(h->lg_edit_mask.p);
    }
    const float *xs = a->x_init, *es = a->eps_tape, *ns = a->noise_tape, *iz = noised ? a->inpaint_noise : nullptr;
    if (cc.tape && !od) {
        if ((rc = ingest(h, h->lg_x, xs, We * nx, 0)) != LS_OK || (rc = ingest(h, h->lg_eps, es, We * per_e * sizeof(float), 0)) != LS_OK ||
            (rc = ingest(h, h->lg_nz, ns, We * per_n * sizeof(float), 0)) != LS_OK) return rc;
        xs = h->lg_x.f(); es = h->lg_eps.f(); ns = h->lg_nz.f();
        if (iz) { if ((rc = ingest(h, h->lg_inz, iz, We * per_n * sizeof(float), 0)) != LS_OK) return rc; iz = h->lg_inz.f(); }
    }
    const float* tx = text_features;        // host text features: one upload per call, as in ls_long_sample
    if (sag && !od) { if ((rc = ingest(h, h->lg_text, tx, (size_t)W * B * kD * sizeof(float), 0)) != LS_OK) return rc; tx = h->lg_text.f(); }
    float* tl = a->timeline;
    float* wd = a->windows;
    if (!od) {
        if ((rc = ingest(h, h->lg_timeline, a->timeline, (size_t)B * JF * Tt * sizeof(float), 0)) != LS_OK) return rc;
        tl = h->lg_timeline.f();
        if (wd) { HIPCHK(h, h->lg_windows.ensure(We * nx)); wd = h->lg_windows.f(); }
    }
    const bool from_image = a->skip_timesteps > 0 || sag;
    if (from_image) HIPCHK(h, h->lg_init.ensure(nx));
    if (sag) { HIPCHK(h, h->lg_sag.ensure(nx)); cc.sag_out = h->lg_sag.f(); }      // the decoder's own plane, sized before the first window
    // the planes k_edit_gather fills are held by address in the captured loop: sized before the first window
    if ((rc = ensure_pinned(h, h->inp_maskf, nx)) != LS_OK || (rc = ensure_pinned(h, h->inp_motion, nx)) != LS_OK) return rc;
    EditArgs ea{};
    ea.timeline = tl; ea.seed = h->lg_seed.f();
    if (mask_form) ea.emask = emask;
    else { ea.range = static_cast<const int*>(h->lg_edit_range.p); ea.chan = static_cast<const unsigned char*>(h->lg_edit_chan.p); }
    ea.feat_u = h->feat_u.f(); ea.origin_x = h->origin_x.f(); ea.init = from_image ? h->lg_init.f() : nullptr;
    ea.JF = JF; ea.T = T; ea.KPP = h->KPP; ea.n_pre = npre; ea.T_total = Tt;
    cc.wa.init_image = ea.init;
    cc.wa.inpaint_noised = noised ? 1 : 0;
    for (int w = 0, e = 0; w < W; ++w) {
        if (!flags[(size_t)w]) continue;
        ea.w = w; ea.motion = h->inp_motion.f(); ea.maskf = h->inp_maskf.f();
        HIPCHK(h, launch_edit_gather(ea, B, st));
        Window win;
        win.w = w; win.Bw = B; win.first = e == 0; win.resident_inpaint = true;
        win.featc = h->lg_featc.f() + (size_t)w * B * T * kAudioFeat;
        if (beat) win.emo_tok = h->lg_emotok.f() + (size_t)w * B * kD;
        if (sag) { win.text = tx + (size_t)w * B * kD; win.edit_start = &ea; }
        if (cc.tape) {
            win.x_init = xs + (size_t)e * nelem; win.eps_tape = es + (size_t)e * per_e; win.noise_tape = ns + (size_t)e * per_n;
            win.inpaint_noise = iz ? iz + (size_t)e * per_n : nullptr;
        }
        if ((rc = run_window(h, cc, win)) != LS_OK) return rc;
        ea.sample = x_plane(h, cc.n_exec); ea.window = wd ? wd + (size_t)e * nelem : nullptr;
        HIPCHK(h, launch_edit_scatter(ea, B, st));
        ++e;
    }
    if ((rc = chain_finish(h, cc, {{od ? nullptr : a->timeline, tl, (size_t)B * JF * Tt * sizeof(float)}, {od || !wd ? nullptr : a->windows, wd, We * nx}})) != LS_OK) return rc;
    for (int w = 0, k = 0; w < W && a->windows_run; ++w)
        if (flags[(size_t)w] && k < a->windows_capacity) a->windows_run[k++] = w;
    if (a->n_windows_run) *a->n_windows_run = We;
    return LS_OK;
}

int ls_long_edit_sag(ls_handle* h, const ls_long_edit_args* a, ls_sag* sag, const float* text_features) {
    return long_edit_run(h, a, sag, text_features, nullptr, false);
}
int ls_long_edit(ls_handle* h, const ls_long_edit_args* a) { return long_edit_run(h, a, nullptr, nullptr, nullptr, false); }
int ls_long_edit_mask(ls_handle* h, const ls_long_edit_args* a, ls_sag* sag, const float* text_features, const unsigned char* element_mask) {
    return long_edit_run(h, a, sag, text_features, element_mask, true);
}

// The pair flags of an element mask as k_edit_mask_pairs computes them (ls_hip.h): a host mask is uploaded first, so the kernel runs
// either way.  flags: HOST [n_windows][batch].
int ls_long_edit_mask_pairs(ls_handle* h, const unsigned char* element_mask, int32_t on_device, int32_t batch, int32_t n_windows, const int32_t* frames,
                            unsigned char* flags) {
    if (!h || !element_mask || !flags) return fail(h, LS_EINVAL, "ls_long_edit_mask_pairs: null argument");
    if (!h->committed) return fail(h, LS_ESTATE, "ls_long_edit_mask_pairs before ls_commit_weights");
    const int T = h->T, npre = h->cfg.n_pre_seq;
    if (batch < 1 || n_windows < 1 || npre < 1 || T <= npre) return fail(h, LS_EINVAL, "ls_long_edit_mask_pairs: batch and n_windows must be >= 1");
    const long long S = T - npre, Tt = T + (long long)(n_windows - 1) * S;
    for (int b = 0; b < batch && frames; ++b)
        if (frames[b] < T || frames[b] > Tt || (frames[b] - T) % S) return fail(h, LS_EINVAL, "ls_long_edit_mask_pairs: frames[%d] = %d is no stitched length", b, frames[b]);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc;
    if (!on_device) {
        if ((rc = ingest(h, h->lg_edit_mask, element_mask, (size_t)batch * h->JF * (size_t)Tt, 0)) != LS_OK) return rc;
        element_mask = static_cast<const unsigned char*>(h->lg_edit_mask.p);
    }
    std::vector<unsigned char> got;
    rc = mask_pair_flags(h, "ls_long_edit_mask_pairs", element_mask, 1, batch, n_windows, frames, got);
    if (got.size() == (size_t)n_windows * batch) memcpy(flags, got.data(), got.size());
    return rc;
}

// Once-per-call stage of a COMPACT timeline edit (ls_hip.h): the plan of ls_long_edit_plan_compact from the ranges, the channels and
// (audio_lengths) the clips' own window counts; the per-clip conditioning held at batch B in the caller's order; the WavEncoder over
// the plan's clip-windows alone, gathered by k_long_gather_clips from a (clip, window) table and stored packed in plan order; every
// window batch planned under the single-pass decision of its own rows and its workspaces sized, so that nothing a captured loop holds
// by address moves once ls_long_edit_compact has begun.  The speaker style is ls_long_edit_compact's (per window batch).
// With an ELEMENT MASK (ls_long_prepare_edit_mask; host or device as c->on_device says) the plan comes from the mask's pair flags
// through the same edit_plan_of_flags; the flags are kept, and the run's mask must give them again.
static int long_prepare_edit_run(ls_handle* h, const ls_long_cond* c, const int64_t* audio_lengths, const int32_t* frame_lo, const int32_t* frame_hi,
                                 const unsigned char* channels, const unsigned char* emask, bool mask_form) {
    if (!h || !c || (mask_form ? !emask : (!frame_lo || !frame_hi))) return fail(h, LS_EINVAL, "ls_long_prepare_edit: null argument");
    int rc;
    if ((rc = check_cond(h, "ls_long_prepare_edit", c->batch, &c->n_windows, c->audio_samples >= 1 && c->encoder_chunk >= 0,
                         c->audio && c->seed_poses && c->vid_indices && c->scale, h->cfg.n_prefix_tokens != 2 || c->emo)) != LS_OK) return rc;
    if (c->audio_samples > 0x7fffffffLL) return fail(h, LS_EINVAL, "ls_long_prepare_edit: audio_samples beyond 2^31 - 1");
    const int B = c->batch, W = c->n_windows, JF = h->JF, T = h->T, AL = h->cfg.audio_len, KPP = h->KPP, npre = h->cfg.n_pre_seq, od = c->on_device;
    std::vector<int> lens((size_t)B, (int)c->audio_samples);
    std::vector<int32_t> frames;
    if (audio_lengths) {
        for (int b = 0; b < B; ++b)
            if (audio_lengths[b] < 1 || audio_lengths[b] > c->audio_samples)
                return fail(h, LS_EINVAL, "audio_lengths[%d] = %lld outside [1, %lld]", b, (long long)audio_lengths[b], (long long)c->audio_samples);
        std::vector<int> row, wins, bw;
        long_plan_drop(B, AL, audio_lengths, row, wins, bw);
        if ((int)bw.size() != W) return fail(h, LS_EINVAL, "n_windows is %d, the longest clip needs %d", W, (int)bw.size());
        frames.resize((size_t)B);
        for (int s = 0; s < B; ++s) frames[(size_t)row[(size_t)s]] = T + (wins[(size_t)s] - 1) * (T - npre);
        for (int b = 0; b < B; ++b) lens[(size_t)b] = (int)audio_lengths[b];
    }
    std::vector<unsigned char> chan;
    if (channels) { chan.resize((size_t)B * JF); for (size_t i = 0; i < chan.size(); ++i) chan[i] = channels[i] ? 1 : 0; }
    const int32_t* fr = audio_lengths ? frames.data() : nullptr;
    const unsigned char* ch = channels ? chan.data() : nullptr;
    int32_t We = 0, np = 0;
    std::vector<unsigned char> pairs;       // the mask form: its pair flags [W][B]
    if (mask_form) {
        if ((rc = mask_pair_flags(h, "ls_long_prepare_edit_mask", emask, od, B, W, fr, pairs)) != LS_OK) return rc;
        if (edit_plan_of_flags(B, W, pairs.data(), nullptr, nullptr, 0, nullptr, 0, &We, &np) != LS_OK) return fail(h, LS_EINVAL, "ls_long_prepare_edit_mask: the plan does not fit");
        if (np < 1) return fail(h, LS_EINVAL, "ls_long_prepare_edit_mask: no window holds an editable element (the mask is empty)");
    } else {
        if (ls_long_edit_plan_compact(B, W, T, npre, frame_lo, frame_hi, ch, JF, fr, nullptr, nullptr, 0, nullptr, 0, &We, &np) != LS_OK)
            return fail(h, LS_EINVAL, "ls_long_prepare_edit: a frame range is no range inside its clip's timeline (0 <= lo <= hi <= %s)", audio_lengths ? "frames[b]" : "T_total");
        if (np < 1) return fail(h, LS_EINVAL, "ls_long_prepare_edit: no window holds an editable element (every range is empty)");
    }
    std::vector<int32_t> cw((size_t)We), cn((size_t)We), crows((size_t)np), coff((size_t)We + 1, 0);
    if ((mask_form ? edit_plan_of_flags(B, W, pairs.data(), cw.data(), cn.data(), We, crows.data(), np, &We, &np)
                   : ls_long_edit_plan_compact(B, W, T, npre, frame_lo, frame_hi, ch, JF, fr, cw.data(), cn.data(), We, crows.data(), np, &We, &np)) != LS_OK)
        return fail(h, LS_EINVAL, "ls_long_prepare_edit: ls_long_edit_plan_compact failed");
    for (int e = 0; e < We; ++e) coff[(size_t)e + 1] = coff[(size_t)e] + cn[(size_t)e];
    std::vector<int> table((size_t)np * 2);
    for (int e = 0, p = 0; e < We; ++e)
        for (int r = 0; r < cn[(size_t)e]; ++r, ++p) { table[(size_t)2 * p] = crows[(size_t)p]; table[(size_t)2 * p + 1] = cw[(size_t)e]; }
    // the editable test of the kernels: a clip without a selected channel is not edited
    std::vector<int32_t> range((size_t)2 * B);
    std::vector<unsigned char> chan_dev((size_t)B * JF, 1);
    for (int b = 0; b < B && !mask_form; ++b) {
        range[(size_t)2 * b] = frame_lo[b]; range[(size_t)2 * b + 1] = frame_hi[b];
        if (channels) memcpy(&chan_dev[(size_t)b * JF], &chan[(size_t)b * JF], (size_t)JF);
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int chunk = c->encoder_chunk > 0 ? c->encoder_chunk : 256;
    if (chunk > 32768) chunk = 32768;                   // one grid row per clip-window of a chunk
    hipStream_t st = h->stream;
    end_stream(h);
    if ((rc = start_prepare(h)) != LS_OK) return rc;
    // a device-resident waveform is read in place (the call waits before it returns); a host one is uploaded as it is, unpadded
    const float* audio = c->audio;
    if (!od) {
        if ((rc = ingest(h, h->lg_audio, c->audio, (size_t)B * (size_t)c->audio_samples * sizeof(float), 0)) != LS_OK) return rc;
        audio = h->lg_audio.f();
    }
    if ((rc = ingest_cond(h, B, od, c->seed_poses, c->vid_indices, c->scale, c->emo, (size_t)W * B)) != LS_OK) return rc;
    // the per-clip stores: h->vid / h->scale are the rows of the window in flight from here on (k_cond_gather)
    if ((rc = ingest(h, h->lg_cvid, h->vid.p, (size_t)B * sizeof(int64_t), 1)) != LS_OK) return rc;
    if ((rc = ingest(h, h->lg_cscale_dev, h->scale.p, (size_t)B * sizeof(float), 1)) != LS_OK) return rc;
    std::vector<float> sc((size_t)B);
    if (od) HIPCHK(h, hipMemcpyAsync(sc.data(), h->lg_cscale_dev.p, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, st));
    else memcpy(sc.data(), c->scale, (size_t)B * sizeof(float));
    if ((rc = ingest(h, h->lg_lens, lens.data(), (size_t)B * sizeof(int), 0)) != LS_OK) return rc;
    if ((rc = ingest(h, h->lg_crows_dev, crows.data(), (size_t)np * sizeof(int32_t), 0)) != LS_OK) return rc;
    if ((rc = ingest(h, h->lg_edit_range, range.data(), range.size() * sizeof(int32_t), 0)) != LS_OK) return rc;
    if ((rc = ingest(h, h->lg_edit_chan, chan_dev.data(), chan_dev.size(), 0)) != LS_OK) return rc;
    if ((rc = upload(h, h->lg_table, table.data(), table.size() * sizeof(int))) != LS_OK) return rc;      // waits: host inputs and these temporaries are free again
    // ---- WavEncoder over the plan's clip-windows, `chunk` at a time
    const int nmax = chunk < np ? chunk : np;
    HIPCHK(h, h->lg_clips.ensure((size_t)nmax * AL * sizeof(float)));
    HIPCHK(h, h->lg_featc.ensure((size_t)np * T * kAudioFeat * sizeof(float)));
    HIPCHK(h, h->lg_featp.ensure((size_t)nmax * T * KPP * sizeof(float)));
    if ((rc = zero_origin_x(h, B)) != LS_OK) return rc;
    for (int p0 = 0; p0 < np; p0 += chunk) {
        const int n = np - p0 < chunk ? np - p0 : chunk;
        HIPCHK(h, launch_long_gather_clips(audio, static_cast<const int*>(h->lg_table.p) + (size_t)2 * p0, static_cast<const int*>(h->lg_lens.p), h->lg_clips.f(), n, AL,
                                           (long long)c->audio_samples, LS_LONG_AUDIO_STRIDE, st));
        if ((rc = run_wav_encoder(h, h->lg_clips.f(), n)) != LS_OK) return rc;
        HIPCHK(h, launch_build_feats(h->origin_x.f(), h->c4.f(), h->lg_featp.f(), h->lg_featc.f() + (size_t)p0 * T * kAudioFeat, n, JF, KPP, 0, st, T));
    }
    // ---- per-batch stages at batch B: the buffers, the style buffers' room, the emotion tokens of every (window, clip)
    if ((rc = size_batch_buffers(h, B)) != LS_OK) return rc;
    if ((rc = prepare_style(h, B)) != LS_OK) return rc;          // sizes z .. z_std for B rows (a window's own style overwrites its rows)
    if (h->cfg.n_prefix_tokens == 2) {
        HIPCHK(h, h->lg_emotok.ensure((size_t)W * B * kD * sizeof(float)));
        HIPCHK(h, launch_gather_rows(h->emo_emb.f(), static_cast<const int64_t*>(h->lg_emo_ids.p), h->lg_emotok.f(), W * B, kD, h->cfg.n_emotions, st));
    }
    // ---- the plan and the workspaces of every window batch under its own rows' scales; the handle is left planned for the whole batch
    bool all_ones = true;
    for (float v : sc) all_ones = all_ones && v == 1.0f;
    for (int e = 0; e < We; ++e) {
        bool ones = true;
        for (int r = 0; r < cn[(size_t)e]; ++r) ones = ones && sc[(size_t)crows[(size_t)coff[(size_t)e] + r]] == 1.0f;
        h->all_scale_one = ones;
        set_plan(h, cn[(size_t)e]);
        if ((rc = plan_workspaces(h)) != LS_OK) return rc;
    }
    h->all_scale_one = all_ones;
    set_plan(h, B);
    if ((rc = plan_workspaces(h)) != LS_OK) return rc;
    if ((rc = finish_prepare(h, B)) != LS_OK) return rc;
    h->lg_W = W; h->lg_L = (size_t)c->audio_samples;
    h->lg_cw = cw; h->lg_cn = cn; h->lg_coff = coff; h->lg_crows = crows; h->lg_cscale = sc;
    if (mask_form) { h->lg_clo.clear(); h->lg_chi.clear(); h->lg_cchan.clear(); }
    else { h->lg_clo.assign(frame_lo, frame_lo + B); h->lg_chi.assign(frame_hi, frame_hi + B); h->lg_cchan = chan; }
    h->lg_cflags = pairs; h->lg_cframes = frames;
    h->lg_compact = true;       // lg_prepared stays false: ls_long_sample and ls_long_edit need the features of all W * B clip-windows
    return LS_OK;
}

int ls_long_prepare_edit(ls_handle* h, const ls_long_cond* c, const int64_t* audio_lengths, const int32_t* frame_lo, const int32_t* frame_hi,
                         const unsigned char* channels) {
    return long_prepare_edit_run(h, c, audio_lengths, frame_lo, frame_hi, channels, nullptr, false);
}
int ls_long_prepare_edit_mask(ls_handle* h, const ls_long_cond* c, const int64_t* audio_lengths, const unsigned char* element_mask) {
    return long_prepare_edit_run(h, c, audio_lengths, nullptr, nullptr, nullptr, element_mask, true);
}

// The compact timeline edit (ls_long_edit_compact_args in ls_hip.h): per planned window k_cond_gather, the style at the window's
// batch, k_edit_gather on the window's row table, the window body (keyed PHILOX rows: the clip's index, not the row's), k_edit_scatter.
// One wait at the end.  With an ELEMENT MASK (ls_long_edit_compact_mask) the kernels read the mask in place of the rectangle; the
// mask's pair flags are made again (host loop, or k_edit_mask_pairs and W * B bytes back) and must be the prepared ones.
static int long_edit_compact_run(ls_handle* h, const ls_long_edit_compact_args* a, ls_sag* sag, const float* text_features, const unsigned char* emask,
                                 bool mask_form) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_long_edit_compact: null argument");
    if (sag && !text_features) return fail(h, LS_EINVAL, "ls_long_edit_compact: sag without text_features");
    if (text_features && !sag) return fail(h, LS_EINVAL, "ls_long_edit_compact: text_features without sag");
    if (!h->lg_compact) return fail(h, LS_ESTATE, "ls_long_edit_compact before ls_long_prepare_edit");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_long_edit_compact before ls_set_schedule");
    if (!a->timeline) return fail(h, LS_EINVAL, "ls_long_edit_compact: null timeline");
    if (mask_form && !emask) return fail(h, LS_EINVAL, "ls_long_edit_compact_mask: null element_mask");
    if (mask_form && (a->frame_lo || a->frame_hi || a->channels))
        return fail(h, LS_EINVAL, "ls_long_edit_compact_mask: the element mask and frame_lo / frame_hi / channels exclude each other");
    if (!mask_form && (!a->frame_lo || !a->frame_hi)) return fail(h, LS_EINVAL, "ls_long_edit_compact: null frame_lo / frame_hi");
    if (a->windows_capacity < 0 || (a->windows_capacity > 0 && !a->windows_run)) return fail(h, LS_EINVAL, "ls_long_edit_compact: windows_capacity without windows_run");
    const int B = h->B, W = h->lg_W, JF = h->JF, T = h->T, npre = h->cfg.n_pre_seq, od = a->on_device;
    const int Tt = T + (W - 1) * (T - npre), We = (int)h->lg_cw.size(), np = h->lg_coff[(size_t)We];
    int rc;
    if (mask_form) {
        if (h->lg_cflags.size() != (size_t)W * B) return fail(h, LS_EINVAL, "ls_long_edit_compact_mask: the handle was prepared by ls_long_prepare_edit (ranges), not by ls_long_prepare_edit_mask");
        std::vector<unsigned char> pairs;
        if ((rc = mask_pair_flags(h, "ls_long_edit_compact_mask", emask, od, B, W, h->lg_cframes.empty() ? nullptr : h->lg_cframes.data(), pairs)) != LS_OK) return rc;
        if (pairs != h->lg_cflags) return fail(h, LS_EINVAL, "ls_long_edit_compact_mask: the element mask differs from the one ls_long_prepare_edit_mask planned (other clip-windows hold its editable elements)");
    } else if ((int)h->lg_clo.size() != B || !std::equal(h->lg_clo.begin(), h->lg_clo.end(), a->frame_lo) || !std::equal(h->lg_chi.begin(), h->lg_chi.end(), a->frame_hi))
        return fail(h, LS_EINVAL, "ls_long_edit_compact: the frame ranges differ from the ones ls_long_prepare_edit planned");
    if (!mask_form && (a->channels != nullptr) != !h->lg_cchan.empty())
        return fail(h, LS_EINVAL, "ls_long_edit_compact: the channels differ from the ones ls_long_prepare_edit planned");
    for (size_t i = 0; i < h->lg_cchan.size() && !mask_form; ++i)
        if ((a->channels[i] != 0) != (h->lg_cchan[i] != 0)) return fail(h, LS_EINVAL, "ls_long_edit_compact: the channels differ from the ones ls_long_prepare_edit planned");
    ChainCall cc;
    if ((rc = chain_args(h, "ls_long_edit_compact", a, true, cc)) != LS_OK) return rc;
    const bool noised = a->inpaint_noised != 0, beat = h->cfg.n_prefix_tokens == 2;
    if (cc.tape && noised && !a->inpaint_noise) return fail(h, LS_EINVAL, "TAPE mode with inpaint_noised needs inpaint_noise");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = chain_begin(h, cc, sag)) != LS_OK) return rc;
    hipStream_t st = h->stream;
    const int n_exec = cc.n_exec;
    int Amax = 0;
    for (int n : h->lg_cn) Amax = n > Amax ? n : Amax;
    const size_t per_x = (size_t)JF * T, per_e = (size_t)n_exec * 2 * kD, per_n = (size_t)n_exec * per_x;     // floats per clip-window: x_T, eps tape, noise tape
    const size_t nxA = (size_t)Amax * per_x * sizeof(float);
    const float *xs = a->x_init, *es = a->eps_tape, *ns = a->noise_tape, *iz = noised ? a->inpaint_noise : nullptr;
    if (cc.tape && !od) {
        if ((rc = ingest(h, h->lg_x, xs, np * per_x * sizeof(float), 0)) != LS_OK || (rc = ingest(h, h->lg_eps, es, np * per_e * sizeof(float), 0)) != LS_OK ||
            (rc = ingest(h, h->lg_nz, ns, np * per_n * sizeof(float), 0)) != LS_OK) return rc;
        xs = h->lg_x.f(); es = h->lg_eps.f(); ns = h->lg_nz.f();
        if (iz) { if ((rc = ingest(h, h->lg_inz, iz, np * per_n * sizeof(float), 0)) != LS_OK) return rc; iz = h->lg_inz.f(); }
    }
    const float* tx = text_features;        // host text features: one upload per call, as in ls_long_edit_sag
    if (sag && !od) { if ((rc = ingest(h, h->lg_text, tx, (size_t)W * B * kD * sizeof(float), 0)) != LS_OK) return rc; tx = h->lg_text.f(); }
    float* tl = a->timeline;
    float* wd = a->windows;
    if (!od) {
        if ((rc = ingest(h, h->lg_timeline, a->timeline, (size_t)B * JF * Tt * sizeof(float), 0)) != LS_OK) return rc;
        tl = h->lg_timeline.f();
        if (wd) { HIPCHK(h, h->lg_windows.ensure(np * per_x * sizeof(float))); wd = h->lg_windows.f(); }
        if (mask_form) {        // a host caller's mask: one upload per call
            if ((rc = ingest(h, h->lg_edit_mask, emask, (size_t)B * JF * Tt, 0)) != LS_OK) return rc;
            emask = static_cast<const unsigned char*>(h->lg_edit_mask.p);
        }
    }
    const bool from_image = a->skip_timesteps > 0 || sag;
    if (from_image) HIPCHK(h, h->lg_init.ensure(nxA));
    if (sag) { HIPCHK(h, h->lg_sag.ensure(nxA)); HIPCHK(h, h->lg_ctext.ensure((size_t)B * kD * sizeof(float))); cc.sag_out = h->lg_sag.f(); }
    // Everything a captured loop holds by address, for the largest window batch, before the first window: the x planes, the inpainting
    // planes, the denoiser's output, the tape buffers or the keyed ring.  Nothing is in flight yet, so a buffer that moves may drop
    // the cached graphs here; none moves from the first window on, and none at all in an identical second call.
    HIPCHK(h, h->xtmp.ensure(nxA)); HIPCHK(h, h->xio.ensure(nxA));      // begin_loop's staging planes: grown now, not under a window in flight
    if ((rc = ensure_pinned(h, h->xa, nxA)) != LS_OK || (rc = ensure_pinned(h, h->xb, nxA)) != LS_OK || (rc = ensure_pinned(h, h->fwd_cfg, nxA)) != LS_OK ||
        (rc = ensure_pinned(h, h->inp_maskf, nxA)) != LS_OK || (rc = ensure_pinned(h, h->inp_motion, nxA)) != LS_OK) return rc;
    if (cc.tape) {
        if ((rc = ensure_pinned(h, h->eps_tape, (size_t)Amax * per_e * sizeof(float))) != LS_OK || (rc = ensure_pinned(h, h->noise_tape, (size_t)Amax * per_n * sizeof(float))) != LS_OK) return rc;
        if (iz && (rc = ensure_pinned(h, h->inp_tape, (size_t)Amax * per_n * sizeof(float))) != LS_OK) return rc;
    } else if ((rc = size_key_ring(h, Amax, n_exec, noised)) != LS_OK) return rc;
    // room in the graph cache for this plan's window batches (one loop per batch size and form), made now; the same batches as the
    // last compact call: its graphs are this call's
    {
        std::vector<int> sizes(h->lg_cn.begin(), h->lg_cn.end());
        std::sort(sizes.begin(), sizes.end());
        sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
        sizes.push_back(-1);                            // never a ragged ls_long_sample's batches
        if (h->graphs_for != sizes) {
            const int want = (int)sizes.size() - 1 < ls_handle::kGraphCacheMax ? (int)sizes.size() - 1 : ls_handle::kGraphCacheMax;
            if ((int)h->graphs.size() + want > ls_handle::kGraphCacheMax) free_graph(h);
            h->graphs_for = sizes;
        }
    }
    // PHILOX: the key of every row of every window, in plan order; a window's rows go to row_gidx ahead of its loop (pageable memory,
    // taken into the runtime's staging memory before the copy call returns, as call_host is)
    std::vector<uint64_t> keys;
    if (!cc.tape) {
        keys.resize((size_t)np);
        for (int e = 0; e < We; ++e)
            for (int r = h->lg_coff[(size_t)e]; r < h->lg_coff[(size_t)e + 1]; ++r)
                keys[(size_t)r] = a->sample_offset + (uint64_t)h->lg_crows[(size_t)r] + ((uint64_t)h->lg_cw[(size_t)e] << 48);
    }
    EditArgs ea{};
    ea.timeline = tl; ea.seed = h->lg_seed.f();
    if (mask_form) ea.emask = emask;
    else { ea.range = static_cast<const int*>(h->lg_edit_range.p); ea.chan = static_cast<const unsigned char*>(h->lg_edit_chan.p); }
    ea.feat_u = h->feat_u.f(); ea.origin_x = h->origin_x.f(); ea.init = from_image ? h->lg_init.f() : nullptr;
    ea.motion = h->inp_motion.f(); ea.maskf = h->inp_maskf.f();
    ea.JF = JF; ea.T = T; ea.KPP = h->KPP; ea.n_pre = npre; ea.T_total = Tt;
    cc.wa.init_image = ea.init;
    cc.wa.inpaint_noised = noised ? 1 : 0;
    CondGatherArgs ga{};
    ga.vid_c = static_cast<const int64_t*>(h->lg_cvid.p); ga.scale_c = h->lg_cscale_dev.f();
    ga.vid = static_cast<int64_t*>(h->vid.p); ga.scale = h->scale.f();
    const int32_t* styled = nullptr;        // the rows the style buffers hold: a window with the rows of the one before it keeps them
    int styled_n = 0;
    // however the windows end, the handle is left as ls_long_prepare_edit left it: planned for the whole batch (its workspaces exist)
    struct WholeBatch {
        ls_handle* h; int B;
        void restore() const {
            h->B = B;
            h->all_scale_one = true;
            for (float v : h->lg_cscale) h->all_scale_one = h->all_scale_one && v == 1.0f;
            set_plan(h, B);
        }
        ~WholeBatch() { restore(); }
    } whole{h, B};
    for (int e = 0; e < We; ++e) {
        const int w = h->lg_cw[(size_t)e], A = h->lg_cn[(size_t)e];
        const size_t off = (size_t)h->lg_coff[(size_t)e];
        const int32_t* rows = h->lg_crows.data() + off;
        const int* rows_dev = static_cast<const int*>(h->lg_crows_dev.p) + off;
        // from here on the handle is prepared for a batch of A: its rows' scales decide the single-pass form, its size the step plan
        bool ones = true;
        for (int r = 0; r < A; ++r) ones = ones && h->lg_cscale[(size_t)rows[r]] == 1.0f;
        h->B = A;
        h->all_scale_one = ones;
        set_plan(h, A);
        if ((rc = plan_workspaces(h)) != LS_OK) return rc;
        ga.rows = rows_dev;
        if (beat) { ga.emo_tok_c = h->lg_emotok.f() + (size_t)w * B * kD; ga.emo_tok = h->emo_tok.f(); }
        if (sag) { ga.text_c = tx + (size_t)w * B * kD; ga.text = h->lg_ctext.f(); }
        HIPCHK(h, launch_cond_gather(ga, A, st));
        if (styled_n != A || !std::equal(rows, rows + A, styled)) {
            if ((rc = prepare_style(h, A)) != LS_OK) return rc;
            styled = rows; styled_n = A;
        }
        ea.w = w; ea.rows = rows_dev;
        HIPCHK(h, launch_edit_gather(ea, A, st));
        if (!cc.tape) HIPCHK(h, hipMemcpyAsync(h->row_gidx.p, keys.data() + off, (size_t)A * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        Window win;
        win.w = w; win.Bw = A; win.first = e == 0; win.resident_inpaint = true; win.policy = kKeep; win.keyed = !cc.tape;
        win.featc = h->lg_featc.f() + off * T * kAudioFeat;
        if (sag) { win.text = h->lg_ctext.f(); win.edit_start = &ea; }
        if (cc.tape) {
            win.x_init = xs + off * per_x; win.eps_tape = es + off * per_e; win.noise_tape = ns + off * per_n;
            win.inpaint_noise = iz ? iz + off * per_n : nullptr;
        }
        if ((rc = run_window(h, cc, win)) != LS_OK) return rc;
        ea.sample = x_plane(h, n_exec); ea.window = wd ? wd + off * per_x : nullptr;
        HIPCHK(h, launch_edit_scatter(ea, A, st));
    }
    whole.restore();
    if ((rc = chain_finish(h, cc, {{od ? nullptr : a->timeline, tl, (size_t)B * JF * Tt * sizeof(float)}, {od || !wd ? nullptr : a->windows, wd, np * per_x * sizeof(float)}})) != LS_OK) return rc;
    for (int k = 0; k < We && a->windows_run && k < a->windows_capacity; ++k) a->windows_run[k] = h->lg_cw[(size_t)k];
    if (a->n_windows_run) *a->n_windows_run = We;
    if (a->rows_run) *a->rows_run = np;
    return LS_OK;
}

int ls_long_edit_compact(ls_handle* h, const ls_long_edit_compact_args* a, ls_sag* sag, const float* text_features) {
    return long_edit_compact_run(h, a, sag, text_features, nullptr, false);
}
int ls_long_edit_compact_mask(ls_handle* h, const ls_long_edit_compact_args* a, ls_sag* sag, const float* text_features, const unsigned char* element_mask) {
    return long_edit_compact_run(h, a, sag, text_features, element_mask, true);
}

// Opening a stream (ls_long_stream_cond in ls_hip.h): a session of `batch` slots, every slot joined from the caller's arrays
int ls_long_stream_open(ls_handle* h, const ls_long_stream_cond* c) {
    if (!h || !c) return fail(h, LS_EINVAL, "ls_long_stream_open: null argument");
    const int rc = check_cond(h, "ls_long_stream_open", c->batch, nullptr, true, c->seed_poses && c->vid_indices && c->scale, true);
    return rc != LS_OK ? rc : session_open(h, c->batch, c);
}

// Opening a session pool (ls_hip.h): a session of `capacity` free slots
int ls_long_pool_open(ls_handle* h, int32_t capacity) {
    if (!h) return fail(h, LS_EINVAL, "ls_long_pool_open: null argument");
    const int rc = check_cond(h, "ls_long_pool_open", capacity, nullptr, true, true, true);
    if (rc != LS_OK) return rc;
    if (capacity > 1024) return fail(h, LS_EINVAL, "ls_long_pool_open: capacity %d beyond 1024 slots", capacity);
    return session_open(h, capacity, nullptr);
}

int ls_long_pool_join(ls_handle* h, const ls_long_pool_join_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_long_pool_join: null argument");
    int rc;
    if ((rc = session_is_open(h, "ls_long_pool_join", false)) != LS_OK) return rc;
    if (a->slot < 0 || a->slot >= h->pl_S) return fail(h, LS_EINVAL, "ls_long_pool_join: slot %d outside [0, %d)", a->slot, h->pl_S);
    if (h->pl_open[(size_t)a->slot]) return fail(h, LS_ESTATE, "ls_long_pool_join: slot %d is occupied", a->slot);
    if (!a->seed_poses || !a->vid_index || !a->scale) return fail(h, LS_EINVAL, "ls_long_pool_join: null conditioning pointer");
    if (h->cfg.n_prefix_tokens == 2 ? !a->emo : a->emo != nullptr) return fail(h, LS_EINVAL, h->cfg.n_prefix_tokens == 2 ? "BEAT variant needs emo ids" : "ls_long_pool_join: emo is a BEAT conditioning");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int s = a->slot, od = a->on_device;
    const size_t hand = (size_t)h->JF * h->cfg.n_pre_seq;
    if (std::find(h->pl_styled.begin(), h->pl_styled.end(), s) != h->pl_styled.end()) h->pl_styled.clear();       // the slot's speaker changes
    if ((rc = pins_drop(h, s)) != LS_OK) return rc;         // a new clip starts with no pin
    if ((rc = pool_hold(h, h->pl_hand.f() + (size_t)s * hand, a->seed_poses, hand * sizeof(float), od)) != LS_OK) return rc;
    if ((rc = pool_hold(h, static_cast<int64_t*>(h->pl_vid.p) + s, a->vid_index, sizeof(int64_t), od)) != LS_OK) return rc;
    if ((rc = pool_hold(h, h->pl_scale.f() + s, a->scale, sizeof(float), od)) != LS_OK) return rc;
    h->pl_have_emo[(size_t)s] = h->pl_have_text[(size_t)s] = 0;
    if (a->emo && (rc = pool_hold_emo(h, s, 1, a->emo, od)) != LS_OK) return rc;
    if (a->text_features && (rc = pool_hold_text(h, s, 1, a->text_features, od)) != LS_OK) return rc;
    float sc = 0.f;
    if (od) HIPCHK(h, hipMemcpyAsync(&sc, h->pl_scale.f() + s, sizeof(float), hipMemcpyDeviceToHost, h->stream));      // the one read-back, as in prepare_scale
    else sc = *a->scale;
    HIPCHK(h, hipStreamSynchronize(h->stream));          // the caller's arrays are its own again
    h->pl_scale_host[(size_t)s] = sc;
    h->pl_samples[(size_t)s] = h->pl_windows[(size_t)s] = h->pl_frames[(size_t)s] = 0;     // the ring position with them: sample n sits at n % R
    h->pl_open[(size_t)s] = 1;
    h->pl_key[(size_t)s] = (uint64_t)h->pl_joins++ & ((1ull << 48) - 1);       // a keyed pool's default: joins since open
    return LS_OK;
}

// A pool whose PHILOX draws follow the clip (ls_hip.h): on a pool nobody has joined yet.  The draws' ring and the key table are sized
// here for every batch up to the pool's capacity, like everything else a pool's captured loops hold.
int ls_long_pool_keyed(ls_handle* h, int32_t on) {
    if (!h) return fail(h, LS_EINVAL, "ls_long_pool_keyed: null argument");
    int rc;
    if ((rc = session_is_open(h, "ls_long_pool_keyed", false)) != LS_OK) return rc;
    if (h->pl_joins != 0) return fail(h, LS_ESTATE, "ls_long_pool_keyed: after the pool's first join");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (on && (rc = size_key_ring(h, h->pl_S, h->have_sched ? h->n_steps : 1)) != LS_OK) return rc;
    h->pl_keyed = on != 0;
    return LS_OK;
}

int ls_long_pool_set_key(ls_handle* h, int32_t slot, uint64_t key) {
    if (!h) return fail(h, LS_EINVAL, "ls_long_pool_set_key: null argument");
    const int rc = session_is_open(h, "ls_long_pool_set_key", false);
    if (rc != LS_OK) return rc;
    if (slot < 0 || slot >= h->pl_S) return fail(h, LS_EINVAL, "ls_long_pool_set_key: slot %d outside [0, %d)", slot, h->pl_S);
    if (key >> 48) return fail(h, LS_EINVAL, "ls_long_pool_set_key: key %llu is not below 2^48 (the window index sits above)", (unsigned long long)key);
    if (!h->pl_keyed) return fail(h, LS_ESTATE, "ls_long_pool_set_key: the pool is not keyed (ls_long_pool_keyed)");
    if (!h->pl_open[(size_t)slot] || h->pl_windows[(size_t)slot] != 0) return fail(h, LS_ESTATE, "ls_long_pool_set_key: slot %d is not open, or has run a window", slot);
    h->pl_key[(size_t)slot] = key;
    return LS_OK;
}

// Pinned poses (ls_hip.h): the entries serve a pool and a stream alike -- a stream is the pool whose slots move together
static int pins_session(ls_handle* h, const char* entry, bool enabled) {
    const int rc = session_is_open(h, entry, h->pl_lockstep != ls_handle::kPool);
    if (rc != LS_OK) return rc;
    if (enabled && !h->pl_pin_P) return fail(h, LS_ESTATE, "%s: the session has no pins (ls_long_pool_pins)", entry);
    return LS_OK;
}

// Enabling pins: where ls_long_pool_keyed acts -- an open pool nobody has joined, a stream nothing has been pushed to.  The store,
// the staging of a pin call, the inpainting planes and the denoiser's output plane are sized here for the session's S slots: no
// buffer a captured loop holds by address moves later, and a session without pins allocates none of them.
int ls_long_pool_pins(ls_handle* h, int32_t horizon) {
    if (!h) return fail(h, LS_EINVAL, "ls_long_pool_pins: null argument");
    int rc;
    if ((rc = pins_session(h, "ls_long_pool_pins", false)) != LS_OK) return rc;
    const bool stream = h->pl_lockstep != ls_handle::kPool;
    if (stream ? (h->pl_rounds != 0 || h->pl_samples[0] != 0) : h->pl_joins != 0)
        return fail(h, LS_ESTATE, "ls_long_pool_pins: after the %s", stream ? "stream's first push" : "pool's first join");
    if (h->pl_pin_P) return fail(h, LS_ESTATE, "ls_long_pool_pins: the session has pins already (horizon %d)", h->pl_pin_H);
    if (horizon < h->T || horizon > (1 << 20)) return fail(h, LS_EINVAL, "ls_long_pool_pins: horizon %d outside [%d, 2^20]", horizon, h->T);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int S = h->pl_S, P = (horizon + 3) / 4 * 4;
    const size_t elems = (size_t)S * P * h->JF, nxS = (size_t)S * h->JF * h->T * sizeof(float);
    HIPCHK(h, h->pl_pin_val.ensure(elems * sizeof(float))); HIPCHK(h, h->pl_pin_bit.ensure(elems));
    HIPCHK(h, hipMemsetAsync(h->pl_pin_val.p, 0, h->pl_pin_val.bytes, h->stream)); HIPCHK(h, hipMemsetAsync(h->pl_pin_bit.p, 0, h->pl_pin_bit.bytes, h->stream));
    HIPCHK(h, h->pl_pin_poses.ensure((size_t)P * h->JF * sizeof(float))); HIPCHK(h, h->pl_pin_mask.ensure((size_t)P * h->JF));
    HIPCHK(h, h->pl_pin_pos.ensure((size_t)P * sizeof(int)));
    if ((rc = ensure_pinned(h, h->inp_maskf, nxS)) != LS_OK || (rc = ensure_pinned(h, h->inp_motion, nxS)) != LS_OK || (rc = ensure_pinned(h, h->fwd_cfg, nxS)) != LS_OK) return rc;
    if (h->pl_keyed && h->cfg.n_prefix_tokens != 2 && (rc = size_key_ring(h, S, h->have_sched ? h->n_steps : 1, true)) != LS_OK) return rc;
    // the TED tree's re-noise tape of a pinned TAPE call and its host staging, for the longest loop of the schedule -- as session_open
    // sizes the other tape buffers; a push checks them again, ahead of its first launch, because the schedule may be set (or grow) later
    if (h->cfg.n_prefix_tokens != 2 && h->have_sched) {
        if ((rc = ensure_pinned(h, h->inp_tape, h->n_steps * nxS)) != LS_OK) return rc;
        HIPCHK(h, h->lg_inz.ensure(h->n_steps * nxS));
    }
    // a stream keeps its plain and its inpainting loop side by side from here on (kKeep in session_push_run): both fit in an empty cache
    if (stream) free_graph(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->pl_pin_H = horizon; h->pl_pin_P = P;
    h->pl_pin_frames.assign((size_t)S, {});
    h->pl_pin_tape = nullptr; h->pl_pin_tape_floats = 0;
    return LS_OK;
}

// the refusals of a frame list, none of which touches the device: n frames, distinct, each in [frames_out, frames_out + horizon)
static int pin_frames_ok(ls_handle* h, const char* entry, int slot, int n, const int64_t* frames, std::vector<int>& pos) {
    if (slot < 0 || slot >= h->pl_S) return fail(h, LS_EINVAL, "%s: slot %d outside [0, %d)", entry, slot, h->pl_S);
    if (!h->pl_open[(size_t)slot]) return fail(h, LS_ESTATE, "%s: slot %d is not open", entry, slot);
    if (n < 1 || n > h->pl_pin_H || !frames) return fail(h, LS_EINVAL, "%s: %d frames (1 .. the horizon %d), or a null list", entry, n, h->pl_pin_H);
    const long long lo = h->pl_frames[(size_t)slot], hi = lo + h->pl_pin_H;
    std::vector<int64_t> sorted(frames, frames + n);
    std::sort(sorted.begin(), sorted.end());
    for (int k = 0; k < n; ++k) {
        if (sorted[(size_t)k] < lo || sorted[(size_t)k] >= hi)
            return fail(h, LS_EINVAL, "%s: frame %lld of slot %d outside [%lld, %lld): frames_out .. frames_out + horizon", entry, (long long)sorted[(size_t)k], slot, lo, hi);
        if (k && sorted[(size_t)k] == sorted[(size_t)k - 1]) return fail(h, LS_EINVAL, "%s: frame %lld is named twice", entry, (long long)sorted[(size_t)k]);
    }
    pos.resize((size_t)n);
    for (int k = 0; k < n; ++k) pos[(size_t)k] = (int)(frames[k] % h->pl_pin_P);
    return LS_OK;
}

int ls_long_pool_pin(ls_handle* h, int32_t slot, int32_t n, const int64_t* frames, const float* poses, const unsigned char* mask, int32_t on_device) {
    if (!h) return fail(h, LS_EINVAL, "ls_long_pool_pin: null argument");
    int rc;
    std::vector<int> pos;
    if ((rc = pins_session(h, "ls_long_pool_pin", true)) != LS_OK || (rc = pin_frames_ok(h, "ls_long_pool_pin", slot, n, frames, pos)) != LS_OK) return rc;
    if (!poses) return fail(h, LS_EINVAL, "ls_long_pool_pin: null poses");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t elems = (size_t)h->JF * n;
    PinArgs p = pin_args(h);
    p.slot = slot; p.K = n; p.poses = poses; p.mask = mask; p.pos = static_cast<const int*>(h->pl_pin_pos.p);
    if (!on_device) {
        HIPCHK(h, hipMemcpyAsync(h->pl_pin_poses.p, poses, elems * sizeof(float), hipMemcpyHostToDevice, st));
        p.poses = h->pl_pin_poses.f();
        if (mask) {
            HIPCHK(h, hipMemcpyAsync(h->pl_pin_mask.p, mask, elems, hipMemcpyHostToDevice, st));
            p.mask = static_cast<const unsigned char*>(h->pl_pin_mask.p);
        }
    }
    HIPCHK(h, hipMemcpyAsync(h->pl_pin_pos.p, pos.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(h, launch_pool_pin_store(p, st));
    HIPCHK(h, hipStreamSynchronize(st));            // the caller's arrays are its own again
    std::vector<long long>& v = h->pl_pin_frames[(size_t)slot];
    v.insert(v.end(), frames, frames + n);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return LS_OK;
}

int ls_long_pool_unpin(ls_handle* h, int32_t slot, int32_t n, const int64_t* frames) {
    if (!h) return fail(h, LS_EINVAL, "ls_long_pool_unpin: null argument");
    int rc;
    if ((rc = pins_session(h, "ls_long_pool_unpin", true)) != LS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (!frames && n == 0) {                        // the whole slot, open or not
        if (slot < 0 || slot >= h->pl_S) return fail(h, LS_EINVAL, "ls_long_pool_unpin: slot %d outside [0, %d)", slot, h->pl_S);
        if ((rc = pins_drop(h, slot)) != LS_OK) return rc;
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return LS_OK;
    }
    std::vector<int> pos;
    if ((rc = pin_frames_ok(h, "ls_long_pool_unpin", slot, n, frames, pos)) != LS_OK) return rc;
    PinArgs p = pin_args(h);
    p.slot = slot; p.K = n; p.pos = static_cast<const int*>(h->pl_pin_pos.p);
    HIPCHK(h, hipMemcpyAsync(h->pl_pin_pos.p, pos.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, launch_pool_pin_clear(p, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<long long>& v = h->pl_pin_frames[(size_t)slot];
    v.erase(std::remove_if(v.begin(), v.end(), [&](long long f) { return std::find(frames, frames + n, (int64_t)f) != frames + n; }), v.end());
    return LS_OK;
}

// the re-noise tape of the NEXT push's pinned calls (TAPE mode, the TED tree): packed call after call, [n_exec, A, J, F, T] each; the
// push checks its size against its plan and forgets it.  A null tape takes one back.
int ls_long_pool_pin_tape(ls_handle* h, const float* inpaint_noise, int64_t n_floats, int32_t on_device) {
    if (!h) return fail(h, LS_EINVAL, "ls_long_pool_pin_tape: null argument");
    const int rc = pins_session(h, "ls_long_pool_pin_tape", true);
    if (rc != LS_OK) return rc;
    if (n_floats < 0 || (n_floats > 0) != (inpaint_noise != nullptr)) return fail(h, LS_EINVAL, "ls_long_pool_pin_tape: %lld floats with%s a tape", (long long)n_floats, inpaint_noise ? "" : "out");
    h->pl_pin_tape = inpaint_noise; h->pl_pin_tape_floats = n_floats; h->pl_pin_tape_od = on_device ? 1 : 0;
    return LS_OK;
}

int ls_long_pool_pin_info(const ls_handle* h, int32_t capacity, int32_t* pending, int64_t misc[2]) {
    if (!h || capacity < 0) return LS_EINVAL;
    const bool in = h->pl_state != ls_handle::kStreamNone && h->pl_pin_P > 0;
    for (int s = 0; s < capacity && pending; ++s) pending[s] = in && s < h->pl_S ? (int32_t)h->pl_pin_frames[(size_t)s].size() : 0;
    if (misc) { misc[0] = in ? h->pl_pin_H : 0; misc[1] = in ? h->pl_pin_P : 0; }
    return LS_OK;
}

int ls_long_pool_push(ls_handle* h, const ls_long_pool_push_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_long_pool_push: null argument");
    const ForgetTape forget_tape{h};
    const int rc = session_is_open(h, "ls_long_pool_push", false);
    if (rc != LS_OK) return rc;
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_long_pool_push before ls_set_schedule");
    return session_push(h, "ls_long_pool_push", a);
}

// A push of a stream: its own refusals, then the session's push with every slot fed, given and closed alike.  The packed tapes of
// rounds at batch B are the stream's [k, B, ...] tapes, the round index is the window index.
int ls_long_stream_push(ls_handle* h, const ls_long_stream_push_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_long_stream_push: null argument");
    const ForgetTape forget_tape{h};
    int rc;
    if ((rc = session_is_open(h, "ls_long_stream_push", true)) != LS_OK) return rc;
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_long_stream_push before ls_set_schedule");
    if (a->n_samples < 0 || (a->n_samples > 0 && !a->audio)) return fail(h, LS_EINVAL, "ls_long_stream_push: n_samples %lld with%s audio", (long long)a->n_samples, a->audio ? "" : "out");
    int64_t first = 0, k = 0;
    if (ls_long_stream_plan(h->pl_samples[0], a->n_samples, h->cfg.audio_len, a->closing, &first, &k) != LS_OK)
        return fail(h, LS_EINVAL, "ls_long_stream_push: closing a stream that was fed no sample");
    if (first != h->pl_windows[0]) return fail(h, LS_ESTATE, "ls_long_stream_push: %lld windows have run, %lld were complete", h->pl_windows[0], (long long)first);
    const int64_t need = k == 0 ? 0 : k * (h->T - h->cfg.n_pre_seq) + (first == 0 ? h->cfg.n_pre_seq : 0);
    if (need > a->capacity) return fail(h, LS_EINVAL, "ls_long_stream_push: this call runs %lld windows = %lld frames, capacity is %d", (long long)k, (long long)need, a->capacity);
    const size_t B = (size_t)h->pl_S;
    const std::vector<int64_t> lengths(B, a->n_samples);
    const std::vector<int32_t> closing(B, a->closing ? 1 : 0), given(B, (a->emo ? 1 : 0) | (a->text_features ? 2 : 0));
    std::vector<int32_t> n_frames(B, 0);
    int32_t n_rounds = 0;
    ls_long_pool_push_args pa{};
    pa.sampler = a->sampler; pa.noise_mode = a->noise_mode; pa.skip_timesteps = a->skip_timesteps; pa.on_device = a->on_device;
    pa.use_graph = a->use_graph; pa.clip_denoised = a->clip_denoised; pa.two_pass_always = a->two_pass_always; pa.eta = a->eta;
    pa.capacity = a->capacity; pa.n_max = a->n_samples; pa.audio = a->audio;
    pa.lengths = lengths.data(); pa.closing = closing.data(); pa.given = given[0] ? given.data() : nullptr;
    pa.emo = a->emo; pa.sag = a->sag; pa.text_features = a->text_features;
    pa.x_init = a->x_init; pa.eps_tape = a->eps_tape; pa.noise_tape = a->noise_tape; pa.seed = a->seed; pa.sample_offset = a->sample_offset;
    pa.frames = a->frames; pa.n_frames = n_frames.data(); pa.n_rounds = &n_rounds;
    if ((rc = session_push(h, "ls_long_stream_push", &pa)) != LS_OK) return rc;
    if (a->n_frames) *a->n_frames = n_frames[0];
    if (a->n_windows) *a->n_windows = n_rounds;
    if (a->closing) h->pl_lockstep = ls_handle::kLockstepClosed;
    return LS_OK;
}

int ls_long_stream_info(const ls_handle* h, int64_t out[4]) {
    if (!h || !out) return LS_EINVAL;
    const bool stream = h->pl_state != ls_handle::kStreamNone && h->pl_lockstep != ls_handle::kPool;       // slot 0 speaks for all
    out[0] = stream ? h->pl_samples[0] : 0; out[1] = stream ? h->pl_windows[0] : 0; out[2] = stream ? h->pl_frames[0] : 0;
    out[3] = stream ? session_bytes(h) : 0;
    return LS_OK;
}

int ls_long_pool_info(const ls_handle* h, int32_t capacity, int64_t* samples_in, int64_t* windows_run, int64_t* frames_out, int32_t* open, int64_t misc[4]) {
    if (!h || capacity < 0) return LS_EINVAL;
    const int S = h->pl_state == ls_handle::kStreamNone || h->pl_lockstep != ls_handle::kPool ? 0 : h->pl_S;
    for (int s = 0; s < capacity; ++s) {
        const bool in = s < S;
        if (samples_in) samples_in[s] = in ? h->pl_samples[(size_t)s] : 0;
        if (windows_run) windows_run[s] = in ? h->pl_windows[(size_t)s] : 0;
        if (frames_out) frames_out[s] = in ? h->pl_frames[(size_t)s] : 0;
        if (open) open[s] = in ? h->pl_open[(size_t)s] : 0;        // of a pool that has ended: as it stood then (misc[3] tells)
    }
    if (misc) {
        misc[0] = S;
        misc[1] = S == 0 ? 0 : session_bytes(h);
        misc[2] = S == 0 ? 0 : h->pl_rounds;
        misc[3] = S != 0 && h->pl_state == ls_handle::kStreamOpen;
    }
    return LS_OK;
}

}  // extern "C"
