// Host side of the C-ABI declared in include/ls_hip.h: everything that runs diffusion steps.  The sampling loop exists once (begin_loop ->
// enqueue_loop | enqueue_plms -> finish_loop; stream launches or a captured hipGraph; draws from whole-call tapes, segmented tapes, Philox (in the step kernels, or keyed per row through the ring: ls_philox_rows.hip) or
// torch's GPU stream; run_window_loop is the same loop without its wait, for the chained windows of ls_chain_api.cpp), next to the single-step entries that enqueue the same launches on caller-held tensors (ls_forward, ls_step, ls_plms_step),
// and the likelihood loop (ls_bpd: per schedule index q_sample, the denoiser alone and k_vb_terms, through the same capture-or-enqueue) with ls_vb_terms.
#include "ls_handle.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

using namespace ls;

namespace {

void fill_common(ls_handle* h, StepArgs& a) {
    memset(&a, 0, sizeof a);
    a.static_c = h->static_c.f(); a.static_u = h->static_u.f();
    a.z_mu = h->z_mu.f(); a.z_std = h->z_std.f();
    a.emo_tok = h->cfg.n_prefix_tokens == 2 ? h->emo_tok.f() : nullptr;
    a.scale = h->scale.f();
    a.call = static_cast<const CallParams*>(h->callp.p);
    a.W = static_cast<const DevWeights*>(h->devw.p);
    a.layers = h->cfg.layers;
    a.sampler = kNone;
#ifdef LS_DEBUG
    a.ablate = h->ablate;
    a.prof = h->prof_on ? static_cast<unsigned long long*>(h->prof.p) : nullptr;
    a.prof_wg = h->prof_wg;
    a.wgt = h->prof_on ? static_cast<unsigned long long*>(h->wgt.p) : nullptr;
#endif
}

// per-step scalars, cast fp64 -> fp32 exactly like _extract_into_tensor (gaussian_diffusion.py:1651-1664)
void fill_sampler(ls_handle* h, StepArgs& a, int sampler, int i, float eta) {
    a.t_nonzero = i != 0;
    if (sampler == LS_SAMPLER_DDPM) {
        a.sampler = kDDPM;
        a.c0 = (float)h->t_c1[i];                                  // posterior_mean_coef1 (:268-271)
        a.c1 = (float)h->t_c2[i];
        a.c2 = expf(0.5f * (float)h->t_plv[i]);                    // exp(0.5*log_variance) (:556)
    } else if (sampler == LS_SAMPLER_DDIM_REVERSE) {
        // ddim_reverse_sample (:857-893): the DDIM epilogue's form with alphas_cumprod_next = append(alphas_cumprod[1:], 0.0) (:178) in
        // place of alphas_cumprod_prev, no noise term at any t
        a.sampler = kDDIM;
        a.t_nonzero = 0;
        const float abn = i + 1 < h->n_steps ? (float)h->t_ac[i + 1] : 0.0f;
        a.c0 = (float)h->t_srac[i];
        a.c1 = (float)h->t_srm1ac[i];
        a.c2 = sqrtf(abn);                                         // (:888-891), fp32 on the cast value
        a.c3 = sqrtf(1.0f - abn);
        a.c4 = 0.0f;
    } else {
        a.sampler = kDDIM;
        const float ab = (float)h->t_ac[i], abp = (float)h->t_acp[i];
        a.c0 = (float)h->t_srac[i];                                // _predict_eps_from_xstart (:418-422)
        a.c1 = (float)h->t_srm1ac[i];
        const float sigma = eta * sqrtf((1.0f - abp) / (1.0f - ab)) * sqrtf(1.0f - ab / abp);   // (:781-785), fp32
        a.c2 = sqrtf(abp);                                         // (:790-793)
        a.c3 = sqrtf(1.0f - abp - sigma * sigma);
        a.c4 = sigma;
    }
}

// p_mean_variance's inpainting inputs (gaussian_diffusion.py:314-320) -> device, mask and motion in the internal [B][T][JF] layout
// The first half: the two planes the update kernel reads, and the re-noise tape.  It is all of the staging when the planes are filled on
// the device (a timeline edit, ls_chain_api.cpp: k_edit_gather wrote them ahead of the loop).
int stage_inpaint_planes(ls_handle* h, const float* noise, size_t noise_elems, int on_device) {
    const size_t nx = (size_t)h->B * h->JF * h->T * sizeof(float);
    int rc;
    if ((rc = ensure_pinned(h, h->inp_maskf, nx)) != LS_OK || (rc = ensure_pinned(h, h->inp_motion, nx)) != LS_OK) return rc;
    if (noise && (rc = ingest_pinned(h, h->inp_tape, noise, noise_elems * sizeof(float), on_device)) != LS_OK) return rc;
    return LS_OK;
}
int stage_inpainting(ls_handle* h, const unsigned char* mask, const float* motion, const float* noise, size_t noise_elems, int on_device) {
    const int B = h->B, JF = h->JF;
    const size_t nelem = (size_t)B * JF * h->T, nx = nelem * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ingest_pinned(h, h->inp_m8, mask, nelem, on_device)) != LS_OK) return rc;
    HIPCHK(h, h->xtmp.ensure(nx)); HIPCHK(h, h->xio.ensure(nx));
    if ((rc = stage_inpaint_planes(h, noise, noise_elems, on_device)) != LS_OK) return rc;
    HIPCHK(h, launch_bytes_to_float(static_cast<const unsigned char*>(h->inp_m8.p), h->xio.f(), nelem, st));
    HIPCHK(h, launch_to_internal(h->xio.f(), h->inp_maskf.f(), B, JF, st, h->T));
    return ingest_internal(h, motion, h->inp_motion.f(), B, on_device);
}

// LS_SAMPLER_PLMS: the planes of plms_buf (stride in floats through *stride); a captured loop holds their addresses
int plms_planes(ls_handle* h, size_t nelem, size_t* stride) {
    *stride = (nelem + 3) & ~(size_t)3;
    return ensure_pinned(h, h->plms_buf, 5 * *stride * sizeof(float));
}

// the launch behind a denoiser launch with sampler = kNone that left the model output in fwd_cfg: plms_sample's update at schedule index i
// (:1059-1096).  Tables cast fp64 -> fp32 per step like _extract_into_tensor, the two square roots in fp32 on the cast value.
hipError_t run_plms_update(ls_handle* h, int mode, int i, int nh, const float* x_t, const float* x_mid, const float* const* hist, float* out,
                           float* eps_out, float* pred_out, int clip, size_t nelem, hipStream_t st) {
    PlmsArgs p{};
    p.x_t = x_t; p.x0 = h->fwd_cfg.f(); p.x_mid = x_mid;
    for (int j = 0; j < 3; ++j) p.hist[j] = (hist && j < (mode == kPlmsEulerB ? 1 : nh)) ? hist[j] : nullptr;
    p.out = out; p.eps_out = eps_out; p.pred_out = pred_out;
    p.n = nelem; p.mode = mode; p.nh = nh; p.clip = clip; p.t_nonzero = i != 0;
    const float abp = (float)h->t_acp[i];
    p.c0 = (float)h->t_srac[i]; p.c1 = (float)h->t_srm1ac[i];
    p.c2 = sqrtf(abp); p.c3 = sqrtf(1.0f - abp);
    if (mode == kPlmsEulerB) {
        if (i < 1) return hipErrorInvalidValue;
        p.d0 = (float)h->t_srac[i - 1]; p.d1 = (float)h->t_srm1ac[i - 1];
    }
    return launch_plms_update(p, st);
}

// One step of the inpainting branch, two launches: the denoiser alone (CFG-combined model output -> fwd_cfg), then mix + clamp +
// update with the coefficients fill_sampler left in `s`.  inoise: the re-noise draw of q_sample (noised), dump: nullable pred_xstart copy
int enqueue_inpaint_step(ls_handle* h, const StepArgs& s, int i, bool noised, const float* inoise, float* dump, int B, bool pair) {
    StepArgs m = s;
    m.sampler = kNone; m.clip_denoised = 0; m.x0_out = h->fwd_cfg.f(); m.x_out = nullptr; m.noise = nullptr;
    HIPCHK(h, run_step(h, m, B, pair, h->stream));
    InpaintArgs ia{};
    ia.x_t = s.x_in; ia.x0 = h->fwd_cfg.f(); ia.maskf = h->inp_maskf.f(); ia.motion = h->inp_motion.f();
    ia.renoise = noised && i > 0;                                      // `if t[0] > 0` (:318)
    ia.inoise = ia.renoise ? inoise : nullptr;
    ia.noise = s.noise; ia.const_noise = s.const_noise; ia.out = s.x_out; ia.dump = dump;
    ia.call = s.call; ia.step_id = s.step_id;
    ia.JF = h->JF; ia.T = h->T; ia.sampler = s.sampler; ia.t_nonzero = s.t_nonzero; ia.clip = s.clip_denoised;
    if (i > 0) { ia.qa = (float)h->t_sac[i - 1]; ia.qb = (float)h->t_s1mac[i - 1]; }       // q_sample(., t - 1), cast like _extract_into_tensor
    ia.c0 = s.c0; ia.c1 = s.c1; ia.c2 = s.c2; ia.c3 = s.c3; ia.c4 = s.c4;
    HIPCHK(h, launch_inpaint_update(ia, B, h->stream));
    return LS_OK;
}

// upload timing of a slot whose copy has been enqueued: wait for it (long done in steady state) and add it to the loop's total
int close_upload(ls_handle* h, int slot) {
    if (!h->upload_open[slot]) return LS_OK;
    HIPCHK(h, hipEventSynchronize(h->ev_cd[slot]));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev_cs[slot], h->ev_cd[slot]));
    h->seg_upload_ms += ms;
    h->upload_open[slot] = false;
    return LS_OK;
}

// Per-call constants of a loop: what ls_sample (and every piece of a segmented loop) derives from its arguments once.
struct LoopCall {
    const ls_sample_args* a;
    int B, n_exec;                  // n_exec executed steps: ordinal k = 0 .. n_exec - 1 runs schedule index n_exec - 1 - k
    size_t nelem;                   // elements of one x plane
    bool pair, tape, tdev, plms, inpaint, inp_noised;
    bool keyed;                     // PHILOX with per-row keys: the draws come from row_gidx through the ring (ls_philox_rows.hip)
    bool inp_resident;              // the inpainting planes were filled on the device ahead of the loop (run_window_loop): no mask / motion to ingest
    int ring_k;                     // TORCH_DEVICE / keyed: steps per ring refill
    size_t plms_stride;             // PLMS: floats between the planes of plms_buf
    TorchDrawArgs tda;              // TORCH_DEVICE: the per-step draws (stage_loop_inputs), and what x_T's draw shares with them
    unsigned long long x_adv;       // TORCH_DEVICE: generator offset x_T's draw consumed ahead of the steps'
};
LoopCall loop_call(const ls_handle* h, const ls_sample_args* a) {
    LoopCall c{};
    c.a = a; c.B = h->B; c.n_exec = h->n_steps - a->skip_timesteps; c.nelem = (size_t)h->B * h->JF * h->T;
    c.pair = single_pass(h, a->two_pass_always);
    c.tape = a->noise_mode == LS_NOISE_TAPE; c.tdev = a->noise_mode == LS_NOISE_TORCH_DEVICE; c.plms = a->sampler == LS_SAMPLER_PLMS;
    c.inpaint = a->inpaint_mask != nullptr; c.inp_noised = c.inpaint && a->inpaint_noised;
    c.tda.call = static_cast<const CallParams*>(h->callp.p);
    c.tda.B = h->B; c.tda.JF = h->JF; c.tda.T = h->T; c.tda.last_step = c.n_exec - 1;
    c.x_adv = (c.tdev && !a->x_init) ? torch_randn_advance((long long)c.nelem, h->n_cu, h->max_thr_cu, nullptr) : 0ull;
    return c;
}

int check_dump_args(ls_handle* h, const ls_sample_args* a) {
    if (a->n_dump > 0 && (a->sampler != LS_SAMPLER_DDPM || !a->dump_steps || !a->dump_out))
        return fail(h, LS_EINVAL, "dump_steps: DDPM only (ddim_sample_loop raises NotImplementedError, gaussian_diffusion.py:919-920)");
    return LS_OK;
}

// Where the random inputs of one model evaluation / one step are: device pointers, or null = drawn inside the kernel (Philox, keyed by
// step_id).  Each source of a loop answers "where are the draws of evaluation e / executed step k": whole-call tapes, a segment's
// device slot (r: the step's index inside the piece), slot k % K of the TORCH_DEVICE ring, or nothing (Philox).
struct Draws { const float* eps_c; const float* eps_u; const float* noise; const float* inz; unsigned step_id; };
const float* at(const float* p, size_t off) { return p ? p + off : p; }
Draws draws_at(const LoopCall& c, const DevBuf& eps, const DevBuf& noise, const float* inz, size_t e, size_t k, unsigned id) {
    const size_t ne = (size_t)c.B * kD;
    return {eps.f() + 2 * e * ne, eps.f() + (2 * e + 1) * ne, at(noise.f(), k * c.nelem), at(inz, k * c.nelem), id};
}
Draws slot_draws(const ls_handle* h, const LoopCall& c, int slot, int r, int k) { return draws_at(c, h->eps_slot[slot], h->noise_slot[slot], nullptr, r, r, (unsigned)k); }
Draws loop_draws(const ls_handle* h, const LoopCall& c, unsigned e, int k) {
    if (c.tape) return draws_at(c, h->eps_tape, h->noise_tape, h->inp_tape.f(), e, k, e);
    if (c.tdev || c.keyed) return draws_at(c, h->trng_eps, h->trng_noise, c.inp_noised ? h->trng_inz.f() : nullptr, k % c.ring_k, k % c.ring_k, (unsigned)k);
    return {nullptr, nullptr, nullptr, nullptr, e};
}
// what a keyed loop's two draw launches share (ls_philox_rows.hip): the key table, the ring, the shapes
RowDrawArgs row_draw_args(const ls_handle* h, const LoopCall& c) {
    RowDrawArgs r{};
    r.call = static_cast<const CallParams*>(h->callp.p); r.gidx = static_cast<const unsigned long long*>(h->row_gidx.p);
    r.eps = h->trng_eps.f(); r.noise = h->trng_noise.f(); r.inz = c.inp_noised ? h->trng_inz.f() : nullptr;
    r.B = c.B; r.JF = h->JF; r.T = h->T; r.last_step = c.n_exec - 1;
    return r;
}
// refill the ring with steps k .. k + K - 1 (stream order: the steps that read it before are done)
int refill_ring(ls_handle* h, const LoopCall& c, int k) {
    const int nsteps = c.n_exec - k < c.ring_k ? c.n_exec - k : c.ring_k;
    if (c.keyed) {
        RowDrawArgs r = row_draw_args(h, c);
        r.k0 = k; r.nsteps = nsteps;
        HIPCHK(h, launch_row_draws(r, h->stream));
        return LS_OK;
    }
    TorchDrawArgs g = c.tda;
    g.k0 = k; g.nsteps = nsteps;
    g.rel0 = c.x_adv + (unsigned long long)k * c.tda.step_adv;
    HIPCHK(h, launch_torch_draws(g, h->stream));
    return LS_OK;
}

// The one builder of a loop's StepArgs.  eval_args: the denoiser alone at index i (a PLMS evaluation); step_args: step k of a DDPM / DDIM loop.
StepArgs eval_args(ls_handle* h, int i, const float* x_in, const Draws& d) {
    StepArgs s;
    fill_common(h, s);
    s.x_in = x_in;
    s.temb = h->temb.f() + (size_t)i * kD; s.temb_stride = 0;      // model timestep timestep_map[i] (_WrappedModel)
    s.step_id = d.step_id;
    s.eps_c = d.eps_c; s.eps_u = d.eps_u;
    return s;
}
StepArgs step_args(ls_handle* h, const LoopCall& c, int k, const Draws& d) {
    const ls_sample_args* a = c.a;
    const int i = c.n_exec - 1 - k;
    StepArgs s = eval_args(h, i, x_plane(h, k), d);
    fill_sampler(h, s, a->sampler, i, a->eta);
    s.clip_denoised = a->clip_denoised;
    s.x_out = x_plane(h, k + 1);
    s.noise = d.noise; s.const_noise = a->const_noise;
    for (int j = 0; j < a->n_dump; ++j)
        if (a->dump_steps[j] == k) s.x0_out = h->dump.f() + (size_t)j * c.nelem;
    return s;
}

// The loop's start: x_T in the internal layout (gaussian_diffusion.py:700-707 / :972-977), init_image -> q_sample at the first
// executed index (:709-716 / :979-986), the dump planes, and this call's hand-off tags.  tags_first: ls_sample moves the tags (and
// with them uploads call_host, which x_T's own draw reads) ahead of x_T; a segmented loop, whose x_T is always the caller's, behind it.
int begin_loop(ls_handle* h, const LoopCall& c, bool tags_first) {
    const ls_sample_args* a = c.a;
    const int B = c.B, JF = h->JF, od = a->on_device;
    const size_t nx = c.nelem * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    if ((rc = ensure_pinned(h, h->xa, nx)) != LS_OK || (rc = ensure_pinned(h, h->xb, nx)) != LS_OK) return rc;
    HIPCHK(h, h->xtmp.ensure(nx)); HIPCHK(h, h->xio.ensure(nx));
    if (tags_first && (rc = advance_tags(h, st)) != LS_OK) return rc;
    if (a->x_init) {
        if ((rc = ingest_internal(h, a->x_init, h->xa.f(), B, od)) != LS_OK) return rc;
    } else if (c.tdev) {
        TorchDrawArgs xa = c.tda;     // randn(*shape) at the generator's offset, then (const_noise) [[0]].repeat(B, 1, 1, 1)
        xa.k0 = 0; xa.nsteps = 1; xa.ndraw = 1; xa.last_step = -1;
        xa.d[0] = torch_draw(h->xio.f(), 0, (long long)c.nelem, h->n_cu, h->max_thr_cu, 0, 0);
        HIPCHK(h, launch_torch_draws(xa, st));
        if (a->const_noise) HIPCHK(h, launch_bcast_first(h->xio.f(), B, JF * h->T, st));
        HIPCHK(h, launch_to_internal(h->xio.f(), h->xa.f(), B, JF, st, h->T));
    } else if (c.keyed) {
        RowDrawArgs r = row_draw_args(h, c);
        r.x = h->xa.f();
        HIPCHK(h, launch_row_xt(r, st));
    } else {
        HIPCHK(h, launch_randn_fill(h->xa.f(), B, JF, static_cast<const CallParams*>(h->callp.p), 0u, st, h->T));
    }
    const int first_index = c.n_exec - 1;
    if (a->init_image || a->skip_timesteps > 0) {
        if (a->init_image) {
            if ((rc = ingest_internal(h, a->init_image, h->xtmp.f(), B, od)) != LS_OK) return rc;
        } else {
            HIPCHK(h, hipMemsetAsync(h->xtmp.p, 0, nx, st));
        }
        HIPCHK(h, launch_q_sample(h->xtmp.f(), h->xa.f(), h->xa.f(), c.nelem, (float)h->t_sac[first_index], (float)h->t_s1mac[first_index], st));
    }
    if (a->n_dump > 0 && (rc = ensure_pinned(h, h->dump, (size_t)a->n_dump * nx)) != LS_OK) return rc;
    if (!tags_first && (rc = advance_tags(h, st)) != LS_OK) return rc;
    return LS_OK;
}

// The loop's end: x_0 and the dump planes back in the caller's layout, wait, check, and the call's ls_timing.  segmented: the last
// piece of a segmented loop (no graph; its tape uploads are closed and reported).
int finish_loop(ls_handle* h, const LoopCall& c, int n_step_launches, int graph_replayed, bool segmented) {
    const ls_sample_args* a = c.a;
    hipStream_t st = h->stream;
    int rc;
    HIPCHK(h, hipEventRecord(h->ev[2], st));
    if ((rc = egress_internal(h, x_plane(h, c.n_exec), a->out, c.B, a->on_device)) != LS_OK) return rc;
    for (int d = 0; d < a->n_dump; ++d)
        if ((rc = egress_internal(h, h->dump.f() + (size_t)d * c.nelem, a->dump_out + (size_t)d * c.nelem, c.B, a->on_device)) != LS_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[3], st));
    HIPCHK(h, hipStreamSynchronize(st));
    resolve_prepare_timing(h, true);
    if (segmented && ((rc = close_upload(h, 0)) != LS_OK || (rc = close_upload(h, 1)) != LS_OK)) return rc;
    if ((rc = coop_check(h)) != LS_OK) return rc;
    report_path(h, c.pair);
    HIPCHK(h, hipEventElapsedTime(&h->timing.loop_ms, h->ev[1], h->ev[2]));
    HIPCHK(h, hipEventElapsedTime(&h->timing.total_ms, h->ev[0], h->ev[3]));
    h->timing.n_step_launches = n_step_launches;
    h->timing.single_pass = c.pair ? 1 : 0;
    h->timing.graph_replayed = graph_replayed;
    h->timing.tape_upload_ms = segmented ? h->seg_upload_ms : 0.f;
    h->timing.n_segments = segmented ? h->seg_index : 1;
    return LS_OK;
}

// for i = T-1-skip ... 0 (gaussian_diffusion.py:724-743 / :994-1014): one linear chain on the handle's stream
int enqueue_loop(ls_handle* h, const LoopCall& c) {
    hipStream_t st = h->stream;
    int rc;
    HIPCHK(h, coop_reset(h, st));              // a memset node at the head of the captured loop: replays start from zeroed granules
    for (int k = 0; k < c.n_exec; ++k) {
        if ((c.tdev || c.keyed) && k % c.ring_k == 0 && (rc = refill_ring(h, c, k)) != LS_OK) return rc;
        const Draws d = loop_draws(h, c, (unsigned)k, k);
        StepArgs s = step_args(h, c, k, d);
        if (c.inpaint) {
            if ((rc = enqueue_inpaint_step(h, s, c.n_exec - 1 - k, c.inp_noised, d.inz, s.x0_out, c.B, c.pair)) != LS_OK) return rc;
            continue;
        }
        s.xpad_ready = k > 0;                      // long-sequence path: the previous step's update kernel wrote this step's padded x_t
        HIPCHK(h, run_step(h, s, c.B, c.pair, st));
    }
    return LS_OK;
}

// One plms_sample step at schedule index i (gaussian_diffusion.py:1016-1098): the denoiser alone (model output -> fwd_cfg) and
// k_plms_update.  first (no history): Euler A to x_mid, the model again at i - 1 on x_mid, Euler B; otherwise the multistep update
// over the nh newest planes of hist.  This step's eps goes to eps_out, the first evaluation's clamped pred_xstart to pred_out (nullable).
struct PlmsPlanes { const float* x_in; float* x_out; float* mid; float* eps_out; float* pred_out; const float* hist[3]; };
int enqueue_plms_step(ls_handle* h, int i, bool first, int nh, const PlmsPlanes& p, const Draws ev[2], int clip, bool pair, size_t nelem) {
    hipStream_t st = h->stream;
    StepArgs m = eval_args(h, i, p.x_in, ev[0]);
    m.x0_out = h->fwd_cfg.f();
    HIPCHK(h, run_step(h, m, h->B, pair, st));
    if (!first) {
        HIPCHK(h, run_plms_update(h, kPlmsMulti, i, nh, p.x_in, nullptr, p.hist, p.x_out, p.eps_out, p.pred_out, clip, nelem, st));
        return LS_OK;
    }
    HIPCHK(h, run_plms_update(h, kPlmsEulerA, i, 0, p.x_in, nullptr, nullptr, p.mid, p.eps_out, p.pred_out, clip, nelem, st));
    m = eval_args(h, i - 1, p.mid, ev[1]);
    m.x0_out = h->fwd_cfg.f();
    HIPCHK(h, run_step(h, m, h->B, pair, st));
    const float* h1[3] = {p.eps_out, nullptr, nullptr};
    HIPCHK(h, run_plms_update(h, kPlmsEulerB, i, 1, p.x_in, p.mid, h1, p.x_out, nullptr, nullptr, clip, nelem, st));
    return LS_OK;
}

// LS_SAMPLER_PLMS (:1016-1211): n_exec steps over plms_buf -- a ring of four eps planes (step k writes plane k & 3 and reads the up
// to three before it) and x_mid.  One linear chain on the handle's stream, like enqueue_loop.
int enqueue_plms(ls_handle* h, const LoopCall& c) {
    HIPCHK(h, coop_reset(h, h->stream));
    float* const ring = h->plms_buf.f();
    unsigned e = 0;                                 // evaluation counter: index into eps_tape / Philox step_id
    for (int k = 0; k < c.n_exec; ++k) {
        const bool first = k == 0;
        const int nh = first ? 0 : (c.a->plms_order < k + 1 ? c.a->plms_order : k + 1) - 1;
        PlmsPlanes p{x_plane(h, k), x_plane(h, k + 1), ring + 4 * c.plms_stride, ring + (size_t)(k & 3) * c.plms_stride, nullptr, {nullptr, nullptr, nullptr}};
        for (int j = 0; j < nh; ++j) p.hist[j] = ring + (size_t)((k - 1 - j) & 3) * c.plms_stride;
        const Draws ev[2] = {loop_draws(h, c, e, k), first ? loop_draws(h, c, e + 1, k) : Draws{}};
        e += first ? 2 : 1;
        const int rc = enqueue_plms_step(h, c.n_exec - 1 - k, first, nh, p, ev, c.a->clip_denoised, c.pair, c.nelem);
        if (rc != LS_OK) return rc;
    }
    return LS_OK;
}

// steps of a batch of B that fit in the ring's budget (ls_set_torch_ring_bytes): at least one, at most the loop
int ring_steps(const ls_handle* h, int B, bool inp_noised, int n_exec) {
    const size_t per_step = ((size_t)2 * B * kD + (size_t)B * h->JF * h->T * (inp_noised ? 2 : 1)) * sizeof(float);
    const size_t fit = h->trng_ring_bytes / per_step;
    return fit < 1 ? 1 : fit > (size_t)n_exec ? n_exec : (int)fit;
}

// What the loop reads besides x: whole-call tapes, the PLMS planes, the inpainting inputs, the TORCH_DEVICE rings and their draws.
// Every buffer here is held by address in a captured loop, hence ensure_pinned / ingest_pinned throughout.
int stage_loop_inputs(ls_handle* h, LoopCall& c) {
    const ls_sample_args* a = c.a;
    const int B = c.B, od = a->on_device;
    const size_t nelem = c.nelem, nx = nelem * sizeof(float);
    int rc;
    if (c.tape) {
        const int n_eval = c.n_exec + (c.plms ? 1 : 0);
        if ((rc = ingest_pinned(h, h->eps_tape, a->eps_tape, (size_t)n_eval * 2 * B * kD * sizeof(float), od)) != LS_OK) return rc;
        if (!c.plms && (rc = ingest_pinned(h, h->noise_tape, a->noise_tape, (size_t)c.n_exec * nx, od)) != LS_OK) return rc;
    }
    if (c.plms && (rc = plms_planes(h, nelem, &c.plms_stride)) != LS_OK) return rc;
    if (c.inpaint) {
        if (!c.inp_resident && !a->inpainted_motion) return fail(h, LS_EINVAL, "inpaint_mask without inpainted_motion");
        if (c.tape && c.inp_noised && !a->inpaint_noise) return fail(h, LS_EINVAL, "TAPE mode with inpaint_noised needs inpaint_noise");
        const float* inz = (c.tape && c.inp_noised) ? a->inpaint_noise : nullptr;
        rc = c.inp_resident ? stage_inpaint_planes(h, inz, (size_t)c.n_exec * nelem, od)
                            : stage_inpainting(h, a->inpaint_mask, a->inpainted_motion, inz, (size_t)c.n_exec * nelem, od);
        if (rc != LS_OK) return rc;
    }
    if ((c.plms || c.inpaint) && (rc = ensure_pinned(h, h->fwd_cfg, nx)) != LS_OK) return rc;      // the denoiser alone leaves the model output here
    if (c.tdev || c.keyed) {
        const size_t eps_step = (size_t)2 * B * kD;
        c.ring_k = ring_steps(h, B, c.inp_noised, c.n_exec);
        if ((rc = ensure_pinned(h, h->trng_eps, eps_step * c.ring_k * sizeof(float))) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->trng_noise, nx * c.ring_k)) != LS_OK) return rc;
        if (c.inp_noised && (rc = ensure_pinned(h, h->trng_inz, nx * c.ring_k)) != LS_OK) return rc;
    }
    if (c.tdev) {
        const size_t eps_step = (size_t)2 * B * kD;
        // per step, in the reference's order: the style eps of the cond and the uncond pass (RAG.py:10-13, 120: randn_like of a
        // [B, 1, 512] std), the inpainting branch's q_sample re-noise while t > 0 (gaussian_diffusion.py:318), the step noise randn_like(x)
        // in x's memory order (:543 / :787; [T][B][J][F] from the second step on, _ref_strides in gaussian_diffusion.py)
        TorchDrawArgs& tda = c.tda;
        int nd = 0;
        tda.d[nd++] = torch_draw(h->trng_eps.f(), eps_step, (long long)B * kD, h->n_cu, h->max_thr_cu, 0, 0);
        tda.d[nd++] = torch_draw(h->trng_eps.f() + (size_t)B * kD, eps_step, (long long)B * kD, h->n_cu, h->max_thr_cu, 0, 0);
        if (c.inp_noised) tda.d[nd++] = torch_draw(h->trng_inz.f(), nelem, (long long)nelem, h->n_cu, h->max_thr_cu, 0, 1);
        tda.d[nd++] = torch_draw(h->trng_noise.f(), nelem, (long long)nelem, h->n_cu, h->max_thr_cu, 1, 0);
        tda.ndraw = nd;
        tda.step_adv = 0;
        for (int d = 0; d < nd; ++d) tda.step_adv += tda.d[d].adv;
    }
    return LS_OK;
}

// everything a captured loop bakes in besides device addresses (those: ensure_pinned).  Whether the call has an init_image is NOT
// among it, at skip_timesteps == 0 or otherwise: x_T and the init image's q_sample are begin_loop's, enqueued ahead of the capture
// on every path, and the captured chain starts from whatever they left in xa.  A scripted timeline edit (ls_long_edit_sag) at
// skip_timesteps == 0 counts on this: it replays the loop an unscripted edit with the same arguments captured, and the reverse.
std::string loop_key(const ls_handle* h, const LoopCall& c) {
    const ls_sample_args* a = c.a;
    char keybuf[256];
    snprintf(keybuf, sizeof keybuf, "P%d B%d s%d e%a k%d n%d c%d cl%d w%u v%u p%d d%d L%lld", h->precision, c.B, a->sampler, (double)a->eta,
             a->skip_timesteps, a->noise_mode, a->const_noise, a->clip_denoised, h->weights_version, h->sched_version, (int)c.pair, a->n_dump, plan_code(h));
    std::string key = keybuf;
    if (c.inpaint) key += c.inp_noised ? " I2" : " I1";
    if (c.plms) key += " O" + std::to_string(a->plms_order);
    if (c.tdev) key += " R" + std::to_string(c.ring_k) + (a->x_init ? "x" : "X");
    if (c.keyed) key += " K" + std::to_string(c.ring_k);        // the draws come from row_gidx: never the loop an unkeyed call captured
    for (int d = 0; d < a->n_dump; ++d) key += "," + std::to_string(a->dump_steps[d]);      // the whole list, however long
    return key;
}

// a chain of launches as stream launches, or as a captured graph (captured when the key is not cached, replayed otherwise).  What a
// missing key does to the cache: CachePolicy in ls_handle.h.
template <class Enqueue>
int run_captured(ls_handle* h, bool use_graph, const std::string& key, Enqueue enqueue, int* graph_replayed, CachePolicy policy = kReplace) {
    hipStream_t st = h->stream;
    *graph_replayed = 0;
    if (!use_graph) return enqueue();
    size_t at = 0;
    while (at < h->graphs.size() && h->graphs[at].key != key) ++at;
    if (at == h->graphs.size()) {
        if (policy == kReplayOnly || (policy == kKeep && (int)h->graphs.size() >= ls_handle::kGraphCacheMax)) return enqueue();
        if (policy == kReplace) free_graph(h);
        HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int rc = enqueue();
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamEndCapture(st, &g);
        if (rc != LS_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess) return fail(h, LS_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        hipGraphExec_t x = nullptr;
        e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
        if (e != hipSuccess) { (void)hipGraphDestroy(g); return fail(h, LS_EHIP, "hipGraphInstantiate: %s", hipGetErrorString(e)); }
        at = h->graphs.size();
        h->graphs.push_back({key, g, x, h->coop_launches});
        if (policy == kReplace) HIPCHK(h, hipEventRecord(h->ev[1], st));    // exclude capture/instantiate from loop_ms
    } else {
        *graph_replayed = 1;
        h->coop_launches = h->graphs[at].coop_launches;     // what enqueue() would have counted: advance_tags sizes the next call's tag range by it
    }
    HIPCHK(h, hipGraphLaunch(h->graphs[at].exec, st));
    return LS_OK;
}

// the sampling loop through run_captured
int run_loop(ls_handle* h, const LoopCall& c, int* graph_replayed, CachePolicy policy = kReplace) {
    return run_captured(h, c.a->use_graph != 0, c.a->use_graph ? loop_key(h, c) : std::string(),
                        [&]() { return c.plms ? enqueue_plms(h, c) : enqueue_loop(h, c); }, graph_replayed, policy);
}

// ---- the variational bound (ls_bpd / ls_vb_terms) ----------------------------------------------------------------------------
// k_vb_terms' coefficient rows, cast fp64 -> fp32 like _extract_into_tensor; held by address in a captured column loop
int ensure_bpd_coef(ls_handle* h) {
    if (h->bpd_coef_valid && h->bpd_coef_version == h->sched_version) return LS_OK;
    std::vector<float> coef((size_t)h->n_steps * 8, 0.f);
    for (int i = 0; i < h->n_steps; ++i) {
        float* c = &coef[(size_t)i * 8];
        c[0] = (float)h->t_c1[i]; c[1] = (float)h->t_c2[i]; c[2] = (float)h->t_plv[i]; c[3] = (float)h->t_srac[i]; c[4] = (float)h->t_srm1ac[i];
    }
    int rc;
    if ((rc = ensure_pinned(h, h->bpd_coef, coef.size() * sizeof(float))) != LS_OK) return rc;
    if ((rc = upload(h, h->bpd_coef, coef.data(), coef.size() * sizeof(float))) != LS_OK) return rc;
    h->bpd_coef_version = h->sched_version;
    h->bpd_coef_valid = true;
    return LS_OK;
}

// columns [k0, k0 + n) of calc_bpd_loop (:1615-1632): per column q_sample (PHILOX: with the draw of its noise), the denoiser alone, k_vb_terms.  One linear chain.
int enqueue_bpd(ls_handle* h, const ls_bpd_args* a, bool pair, size_t nelem) {
    hipStream_t st = h->stream;
    const int B = h->B, T = h->n_steps;
    const bool tape = a->noise_mode == LS_NOISE_TAPE;
    const size_t ne = (size_t)B * kD;
    float* const out = h->bpd_out.f();
    HIPCHK(h, coop_reset(h, st));
    for (int r = 0; r < a->col_count; ++r) {
        const int k = a->col_begin + r, i = T - 1 - k;
        const float* nz = tape ? h->bpd_tape.f() + (size_t)r * nelem : h->bpd_nz.f();
        if (tape)
            HIPCHK(h, launch_q_sample(h->bpd_x0.f(), nz, h->bpd_xt.f(), nelem, (float)h->t_sac[i], (float)h->t_s1mac[i], st));
        else        // the draw and q_sample in one launch
            HIPCHK(h, launch_q_sample_philox(h->bpd_x0.f(), h->bpd_nz.f(), h->bpd_xt.f(), B, h->JF, h->T, static_cast<const CallParams*>(h->callp.p),
                                             (unsigned)k, (float)h->t_sac[i], (float)h->t_s1mac[i], st));
        const Draws d = tape ? Draws{h->eps_tape.f() + 2 * r * ne, h->eps_tape.f() + (2 * r + 1) * ne, nullptr, nullptr, (unsigned)k}
                             : Draws{nullptr, nullptr, nullptr, nullptr, (unsigned)k};
        StepArgs m = eval_args(h, i, h->bpd_xt.f(), d);
        m.x0_out = h->fwd_cfg.f();
        HIPCHK(h, run_step(h, m, B, pair, st));
        VbArgs v{};
        v.x_start = h->bpd_x0.f(); v.x_t = h->bpd_xt.f(); v.noise = nz; v.pred = h->fwd_cfg.f();
        v.table = h->bpd_coef.f(); v.index = i; v.n_steps = T; v.n = (int)(nelem / B); v.clip = a->clip_denoised;
        v.vb = out; v.xstart_mse = out + (size_t)B * T; v.mse = out + (size_t)2 * B * T;
        v.out_stride = T; v.out_col = k;
        HIPCHK(h, launch_vb_terms(v, B, st));
    }
    return LS_OK;
}

// ls_sample with seg_count > 0: one piece of a TAPE-mode loop (see ls_sample_args in ls_hip.h)
int sample_segment(ls_handle* h, const ls_sample_args* a) {
    if (a->noise_mode != LS_NOISE_TAPE) return fail(h, LS_EINVAL, "segmented sampling is for TAPE mode (PHILOX needs no tapes)");
    if (a->inpaint_mask) return fail(h, LS_EUNSUPPORTED, "the inpainting branch is not combined with segmented tapes");
    if (!a->eps_tape || !a->noise_tape) return fail(h, LS_EINVAL, "segment needs eps_tape and noise_tape");
    int rc;
    if ((rc = check_dump_args(h, a)) != LS_OK) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const LoopCall c = loop_call(h, a);
    const int B = c.B, od = a->on_device, n_exec = c.n_exec;
    if (a->seg_begin < 0 || a->seg_begin + a->seg_count > n_exec) return fail(h, LS_EINVAL, "segment [%d, %d) outside the loop's %d steps", a->seg_begin, a->seg_begin + a->seg_count, n_exec);
    const bool last = a->seg_begin + a->seg_count == n_exec;
    if (last && !a->out) return fail(h, LS_EINVAL, "ls_sample: null out");
    const size_t nx = c.nelem * sizeof(float);
    hipStream_t st = h->stream;
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    if (a->seg_begin == 0) {
        if (!a->x_init) return fail(h, LS_EINVAL, "TAPE mode needs x_init");
        if ((rc = begin_loop(h, c, false)) != LS_OK) return rc;
        HIPCHK(h, coop_reset(h, st));
        h->seg_next = 0; h->seg_index = 0; h->seg_skip = a->skip_timesteps; h->seg_sampler = a->sampler; h->seg_upload_ms = 0.f;
        h->slot_used[0] = h->slot_used[1] = false;
        HIPCHK(h, hipEventRecord(h->ev[1], st));
    } else if (a->seg_begin != h->seg_next || a->skip_timesteps != h->seg_skip || a->sampler != h->seg_sampler) {
        return fail(h, LS_ESTATE, "segment starts at step %d but the loop in progress expects %d (segments run in order, same sampler / skip)",
                    a->seg_begin, h->seg_next);
    }
    const int slot = h->seg_index & 1;
    const size_t eps_step = (size_t)2 * B * kD, eps_bytes = eps_step * a->seg_count * sizeof(float), nz_bytes = nx * a->seg_count;
    if (h->slot_used[slot]) {
        HIPCHK(h, hipStreamWaitEvent(h->copy_stream, h->ev_seg[slot], 0));     // the steps that read this slot two segments ago
        if ((rc = close_upload(h, slot)) != LS_OK) return rc;
    }
    if (h->eps_slot[slot].bytes < eps_bytes || h->noise_slot[slot].bytes < nz_bytes) {
        HIPCHK(h, hipStreamSynchronize(st));                                   // growing a slot frees memory the queued steps may read
        HIPCHK(h, h->eps_slot[slot].ensure(eps_bytes)); HIPCHK(h, h->noise_slot[slot].ensure(nz_bytes));
    }
    hipStream_t cs = od ? st : h->copy_stream;     // device tapes: in stream order; host tapes: uploaded beside the previous piece's steps
    if (!od) HIPCHK(h, hipEventRecord(h->ev_cs[slot], cs));
    HIPCHK(h, hipMemcpyAsync(h->eps_slot[slot].p, a->eps_tape, eps_bytes, od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, cs));
    HIPCHK(h, hipMemcpyAsync(h->noise_slot[slot].p, a->noise_tape, nz_bytes, od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, cs));
    if (!od) {
        HIPCHK(h, hipEventRecord(h->ev_cd[slot], cs));
        h->upload_open[slot] = true;
        HIPCHK(h, hipStreamWaitEvent(st, h->ev_cd[slot], 0));
        if ((rc = close_upload(h, slot ^ 1)) != LS_OK) return rc;              // the PREVIOUS segment's host buffers are free from here on
    }
    for (int k = a->seg_begin; k < a->seg_begin + a->seg_count; ++k) {
        StepArgs s = step_args(h, c, k, slot_draws(h, c, slot, k - a->seg_begin, k));
        HIPCHK(h, run_step(h, s, B, c.pair, st));
    }
    HIPCHK(h, hipEventRecord(h->ev_seg[slot], st));
    h->slot_used[slot] = true;
    h->seg_next = a->seg_begin + a->seg_count;
    h->seg_index++;
    if (!last) return LS_OK;
    if ((rc = finish_loop(h, c, n_exec, 0, true)) != LS_OK) return rc;
    h->seg_next = -1;
    return LS_OK;
}

}  // namespace

// the checks of ls_sample that hold for whole-call and segmented loops alike, and for every window of a chain
int ls::check_sampler_args(ls_handle* h, const ls_sample_args* a) {
    const bool plms = a->sampler == LS_SAMPLER_PLMS;
    if (a->sampler != LS_SAMPLER_DDPM && a->sampler != LS_SAMPLER_DDIM && !plms)
        return fail(h, LS_EINVAL, a->sampler == LS_SAMPLER_DDIM_REVERSE ? "ls_sample: DDIM_REVERSE is a single step (ls_step); the reference has no reverse loop" : "bad sampler");
    if (a->noise_mode != LS_NOISE_TAPE && a->noise_mode != LS_NOISE_PHILOX && a->noise_mode != LS_NOISE_TORCH_DEVICE)
        return fail(h, LS_EINVAL, "bad noise_mode");
    if (a->skip_timesteps < 0 || a->skip_timesteps >= h->n_steps) return fail(h, LS_EINVAL, "skip_timesteps out of range");
    if (!plms && a->plms_order != 0) return fail(h, LS_EINVAL, "plms_order is for LS_SAMPLER_PLMS only");
    if (plms) {
        if (a->plms_order == 1) return fail(h, LS_EINVAL, "PLMS: a loop of order 1 fails in the reference at its first step (no history); order 1 is DDIM with eta = 0");
        if (a->plms_order < 2 || a->plms_order > 4) return fail(h, LS_EINVAL, "PLMS: order %d outside 1..4", a->plms_order);
        if (h->n_steps - a->skip_timesteps < 2) return fail(h, LS_EINVAL, "PLMS needs at least two executed steps (the first one evaluates the model at t - 1)");
        if (a->n_dump > 0 || a->dump_steps || a->const_noise || a->eta != 0.0f) return fail(h, LS_EINVAL, "PLMS takes no dump_steps, const_noise or eta");
        if (a->seg_count > 0 || a->seg_begin != 0) return fail(h, LS_EUNSUPPORTED, "PLMS: segmented tapes are not built");
        if (a->inpaint_mask || a->inpainted_motion || a->inpaint_noise) return fail(h, LS_EUNSUPPORTED, "PLMS is not combined with the inpainting branch");
        if (a->noise_mode == LS_NOISE_TORCH_DEVICE) return fail(h, LS_EUNSUPPORTED, "PLMS: TORCH_DEVICE draws are not generated in the loop; hand them in as device tapes (TAPE mode)");
        if (a->noise_mode == LS_NOISE_TAPE && a->noise_tape) return fail(h, LS_EINVAL, "PLMS draws no step noise: noise_tape must be NULL");
    }
    return LS_OK;
}

// The loop of one window of a chain (ls_chain_api.cpp): ls_sample's begin -> stage -> capture-or-enqueue on a filled ls_sample_args,
// without its wait; the caller has set call_host, and the result is x_plane(h, n_exec).  resident_inpaint: the inpainting branch on
// planes the caller filled on the device (a->inpaint_noised says whether they are re-noised).  first: the call's first window, whose
// start (ev[6]; ev[0] is re-recorded by every window's begin_loop) and loop start (ev[1]) time the call.
int ls::run_window_loop(ls_handle* h, const ls_sample_args* a, bool resident_inpaint, bool first, CachePolicy policy, int* graph_replayed, bool keyed) {
    LoopCall c = loop_call(h, a);
    c.keyed = keyed && a->noise_mode == LS_NOISE_PHILOX;
    if (resident_inpaint) { c.inpaint = true; c.inp_noised = a->inpaint_noised != 0; c.inp_resident = true; }
    int rc;
    if ((rc = begin_loop(h, c, true)) != LS_OK) return rc;
    if (first) HIPCHK(h, hipEventRecord(h->ev[6], h->stream));
    if ((rc = stage_loop_inputs(h, c)) != LS_OK) return rc;
    if (first) HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    return run_loop(h, c, graph_replayed, policy);
}

int ls::size_key_ring(ls_handle* h, int B, int n_exec, bool inp_noised) {
    size_t eps = 0, nz = 0;
    for (int b = 1; b <= B; ++b) {
        const size_t k = (size_t)ring_steps(h, b, inp_noised, n_exec);
        eps = std::max(eps, k * 2 * b * kD * sizeof(float)); nz = std::max(nz, k * b * h->JF * h->T * sizeof(float));
    }
    int rc;
    if ((rc = ensure_pinned(h, h->trng_eps, eps)) != LS_OK || (rc = ensure_pinned(h, h->trng_noise, nz)) != LS_OK) return rc;
    if (inp_noised && (rc = ensure_pinned(h, h->trng_inz, nz)) != LS_OK) return rc;
    return ensure_pinned(h, h->row_gidx, (size_t)B * sizeof(unsigned long long));
}

namespace {

// ls_step with one schedule index per sample: the denoiser with one timestep-embedding row per sample (what ls_forward does),
// pred_xstart -> fwd_cfg; then the posterior / DDIM update with per-sample coefficients as its own elementwise kernel, both driven by
// the index vector on the device
int enqueue_per_sample_step(ls_handle* h, const ls_step_args* a, StepArgs& s, bool pair) {
    const int B = h->B;
    hipStream_t st = h->stream;
    int rc;
    char ck[64];
    snprintf(ck, sizeof ck, "s%d e%a v%u", a->sampler, (double)a->eta, h->sched_version);
    if (h->coef_key != ck) {
        std::vector<float> coef((size_t)h->n_steps * 8, 0.f);
        for (int i = 0; i < h->n_steps; ++i) {
            StepArgs t;
            fill_sampler(h, t, a->sampler, i, a->eta);
            float* c = &coef[(size_t)i * 8];
            c[0] = t.t_nonzero ? 1.f : 0.f; c[1] = t.c0; c[2] = t.c1; c[3] = t.c2; c[4] = t.c3; c[5] = t.c4;
        }
        if ((rc = upload(h, h->coef, coef.data(), coef.size() * sizeof(float))) != LS_OK) return rc;
        h->coef_key = ck;
    }
    if ((rc = ingest(h, h->tidx, a->indices, (size_t)B * sizeof(int64_t), a->indices_on_device)) != LS_OK) return rc;
    if (!a->indices_on_device) HIPCHK(h, hipStreamSynchronize(st));        // a host index vector may be a temporary of the caller
    HIPCHK(h, h->tfwd.ensure((size_t)B * kD * sizeof(float)));
    HIPCHK(h, launch_gather_rows(h->temb.f(), static_cast<const int64_t*>(h->tidx.p), h->tfwd.f(), B, kD, h->n_steps, st));
    s.temb = h->tfwd.f(); s.temb_stride = kD;
    HIPCHK(h, run_step(h, s, B, pair, st));
    HIPCHK(h, launch_sampler_update(s.x_in, h->fwd_cfg.f(), h->noise.f(), h->coef.f(), static_cast<const int64_t*>(h->tidx.p), h->n_steps,
                                    s.x_out, B, h->JF, h->T, a->sampler == LS_SAMPLER_DDPM ? kDDPM : kDDIM, st));
    return LS_OK;
}

}  // namespace

extern "C" {

int ls_forward(ls_handle* h, const ls_forward_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_forward: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_forward before ls_prepare");
    if (!a->x || !a->timesteps || !a->eps_cond || !a->eps_uncond) return fail(h, LS_EINVAL, "ls_forward: null input");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, od = a->on_device;
    const size_t nx = (size_t)B * h->JF * h->T * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    HIPCHK(h, h->xa.ensure(nx));
    if ((rc = ingest_internal(h, a->x, h->xa.f(), B, od)) != LS_OK) return rc;
    HIPCHK(h, h->eps.ensure((size_t)2 * B * kD * sizeof(float)));
    if ((rc = ingest_eps_pair(h, h->eps.f(), a->eps_cond, a->eps_uncond, od)) != LS_OK) return rc;
    if ((rc = ingest(h, h->tidx, a->timesteps, (size_t)B * sizeof(int64_t), od)) != LS_OK) return rc;
    if ((rc = build_temb_rows(h, static_cast<const long long*>(h->tidx.p), B, h->tfwd_tmp, h->tfwd)) != LS_OK) return rc;
    HIPCHK(h, h->fwd_c.ensure(nx)); HIPCHK(h, h->fwd_u.ensure(nx)); HIPCHK(h, h->fwd_cfg.ensure(nx));
    StepArgs s;
    fill_common(h, s);
    s.x_in = h->xa.f();
    s.fwd_c = h->fwd_c.f(); s.fwd_u = h->fwd_u.f(); s.x0_out = h->fwd_cfg.f();
    s.eps_c = h->eps.f(); s.eps_u = h->eps.f() + (size_t)B * kD;
    s.temb = h->tfwd.f(); s.temb_stride = kD;
    if (a->trace && !h->fused) return fail(h, LS_EUNSUPPORTED, "the residual-stream trace is an output of the fused step kernel only");
    if (a->trace) {
        HIPCHK(h, h->trace.ensure((size_t)B * (h->cfg.layers + 1) * h->R * kD * sizeof(float)));
        s.trace = h->trace.f();
    }
    if ((rc = advance_tags(h, st)) != LS_OK) return rc;
    HIPCHK(h, coop_reset(h, st));
    HIPCHK(h, run_step(h, s, B, false, st));      // model(x, t, y) parity entry: both passes always
    float* outs[3] = {a->out_cond, a->out_uncond, a->out_cfg};
    const float* srcs[3] = {h->fwd_c.f(), h->fwd_u.f(), h->fwd_cfg.f()};
    for (int i = 0; i < 3; ++i)
        if (outs[i] && (rc = egress_internal(h, srcs[i], outs[i], B, od)) != LS_OK) return rc;
    if (a->trace && (rc = egress(h, a->trace, h->trace.f(), (size_t)B * (h->cfg.layers + 1) * h->R * kD * sizeof(float), od)) != LS_OK) return rc;
    return sync_and_check(h, a->no_sync, od);
}

int ls_step(ls_handle* h, const ls_step_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_step: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_step before ls_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_step before ls_set_schedule");
    if (!a->indices && (a->index < 0 || a->index >= h->n_steps)) return fail(h, LS_EINVAL, "step index %d outside [0,%d)", a->index, h->n_steps);
    const bool reverse = a->sampler == LS_SAMPLER_DDIM_REVERSE;
    if (a->sampler != LS_SAMPLER_DDPM && a->sampler != LS_SAMPLER_DDIM && !reverse)
        return fail(h, LS_EINVAL, a->sampler == LS_SAMPLER_PLMS ? "ls_step: PLMS steps go through ls_plms_step" : "bad sampler");
    if (!a->x || !a->eps_cond || !a->eps_uncond || (!a->noise && !reverse) || !a->sample) return fail(h, LS_EINVAL, "ls_step: null pointer");
    if (reverse && a->eta != 0.0f) return fail(h, LS_EINVAL, "DDIM_REVERSE: the reverse ODE is the deterministic path only (eta == 0)");
    if (reverse && a->inpaint_mask) return fail(h, LS_EUNSUPPORTED, "DDIM_REVERSE is not combined with the inpainting branch");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, JF = h->JF, od = a->on_device;
    const size_t nx = (size_t)B * JF * h->T * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    // one schedule index per sample (the reference's `t` is a [B] tensor, gaussian_diffusion.py:507-558 / :745-798).  HOST indices
    // are validated and a constant vector takes the fused uniform path; DEVICE indices are never read by the host (no round trip
    // in a step-by-step caller): they always take the per-sample path and are clamped into the table on the device.
    bool per_sample = false;
    int index = a->index;
    if (a->indices && a->indices_on_device) {
        per_sample = true;
    } else if (a->indices) {
        for (int b = 0; b < B; ++b) {
            if (a->indices[b] < 0 || a->indices[b] >= h->n_steps)
                return fail(h, LS_EINVAL, "indices[%d] = %lld outside [0,%d)", b, (long long)a->indices[b], h->n_steps);
            if (a->indices[b] != a->indices[0]) per_sample = true;
        }
        index = (int)a->indices[0];
    }
    if (per_sample && !h->fused) return fail(h, LS_EUNSUPPORTED, "per-sample timesteps: fused (34-frame) path only");
    const bool inpaint = a->inpaint_mask != nullptr;
    if (inpaint && per_sample) return fail(h, LS_EUNSUPPORTED, "the inpainting branch takes a uniform step index (the reference tests t[0])");
    if (inpaint && !a->inpainted_motion) return fail(h, LS_EINVAL, "inpaint_mask without inpainted_motion");
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    HIPCHK(h, h->xa.ensure(nx)); HIPCHK(h, h->xb.ensure(nx)); HIPCHK(h, h->fwd_cfg.ensure(nx));
    if ((rc = ingest_internal(h, a->x, h->xa.f(), B, od)) != LS_OK) return rc;
    HIPCHK(h, h->eps.ensure((size_t)2 * B * kD * sizeof(float)));
    if ((rc = ingest_eps_pair(h, h->eps.f(), a->eps_cond, a->eps_uncond, od)) != LS_OK) return rc;
    if (a->noise) {
        if ((rc = ingest(h, h->noise, a->noise, nx, od)) != LS_OK) return rc;
    } else {                    // DDIM_REVERSE: no noise term (t_nonzero = 0); the kernels still get a valid plane
        HIPCHK(h, h->noise.ensure(nx));
        HIPCHK(h, hipMemsetAsync(h->noise.p, 0, nx, st));
    }
    if ((rc = advance_tags(h, st)) != LS_OK) return rc;
    HIPCHK(h, coop_reset(h, st));
    StepArgs s;
    fill_common(h, s);
    s.clip_denoised = a->clip_denoised;
    s.x_in = h->xa.f(); s.x_out = h->xb.f(); s.x0_out = h->fwd_cfg.f();
    s.eps_c = h->eps.f(); s.eps_u = h->eps.f() + (size_t)B * kD;
    const bool pair = single_pass(h, a->two_pass_always);
    if (!per_sample) {          // one schedule index: the sampler's arithmetic rides in the step kernel (inpainting: in its update kernel)
        fill_sampler(h, s, a->sampler, index, a->eta);
        s.noise = h->noise.f();
        s.temb = h->temb.f() + (size_t)index * kD; s.temb_stride = 0;
    }
    if (inpaint) {
        if ((rc = stage_inpainting(h, a->inpaint_mask, a->inpainted_motion, a->inpaint_noise, (size_t)B * JF * h->T, od)) != LS_OK) return rc;
        if ((rc = enqueue_inpaint_step(h, s, index, a->inpaint_noise != nullptr, h->inp_tape.f(), nullptr, B, pair)) != LS_OK) return rc;
    } else if (!per_sample) {
        HIPCHK(h, run_step(h, s, B, pair, st));
    } else {
        if ((rc = enqueue_per_sample_step(h, a, s, pair)) != LS_OK) return rc;
    }
    if ((rc = egress_internal(h, h->xb.f(), a->sample, B, od)) != LS_OK) return rc;
    if (a->pred_xstart) {
        HIPCHK(h, h->xtmp.ensure(nx));
        if ((rc = egress_internal(h, h->fwd_cfg.f(), a->pred_xstart, B, od, h->xtmp.f())) != LS_OK) return rc;
    }
    return sync_and_check(h, a->no_sync, od);
}

int ls_q_sample(ls_handle* h, int index, int on_device, size_t n, const float* x_start, const float* noise, float* out) {
    if (!h || !x_start || !noise || !out) return fail(h, LS_EINVAL, "ls_q_sample: null argument");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_q_sample before ls_set_schedule");
    if (index < 0 || index >= h->n_steps) return fail(h, LS_EINVAL, "index out of range");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const float a = (float)h->t_sac[index], b = (float)h->t_s1mac[index];
    hipStream_t st = h->stream;
    if (on_device) {
        HIPCHK(h, launch_q_sample(x_start, noise, out, n, a, b, st));
    } else {
        int rc;
        if ((rc = ingest(h, h->xio, x_start, n * sizeof(float), 0)) != LS_OK) return rc;
        if ((rc = ingest(h, h->xtmp, noise, n * sizeof(float), 0)) != LS_OK) return rc;
        HIPCHK(h, launch_q_sample(h->xio.f(), h->xtmp.f(), h->xio.f(), n, a, b, st));
        if ((rc = egress(h, out, h->xio.f(), n * sizeof(float), 0)) != LS_OK) return rc;
    }
    HIPCHK(h, hipStreamSynchronize(st));
    return LS_OK;
}

// Per-row Philox keys of ls_sample (ls_hip.h): the table a keyed loop reads, uploaded here; rk_n says for how many rows it holds
int ls_set_row_keys(ls_handle* h, const uint64_t* keys, int32_t n) {
    if (!h || n < 0 || (n > 0 && !keys)) return fail(h, LS_EINVAL, "ls_set_row_keys: null argument or negative count");
    h->rk_n = 0;
    if (n == 0) return LS_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    int rc;
    if ((rc = ensure_pinned(h, h->row_gidx, (size_t)n * sizeof(uint64_t))) != LS_OK) return rc;
    if ((rc = upload(h, h->row_gidx, keys, (size_t)n * sizeof(uint64_t))) != LS_OK) return rc;      // waits: the keys are the caller's again
    h->rk_n = n;
    return LS_OK;
}

// validate -> begin -> stage tapes / rings -> capture-or-enqueue -> finish
int ls_sample(ls_handle* h, const ls_sample_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_sample: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_sample before ls_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_sample before ls_set_schedule");
    int rc;
    if ((rc = check_sampler_args(h, a)) != LS_OK) return rc;
    if (h->rk_n > 0 && a->noise_mode != LS_NOISE_PHILOX) return fail(h, LS_EINVAL, "ls_sample: row keys are set (ls_set_row_keys) and the noise mode is not PHILOX");
    if (a->seg_count > 0) return sample_segment(h, a);
    h->seg_next = -1;
    if (!a->out) return fail(h, LS_EINVAL, "ls_sample: null out");
    LoopCall c = loop_call(h, a);
    if (c.tape && (!a->x_init || !a->eps_tape || (!a->noise_tape && !c.plms))) return fail(h, LS_EINVAL, "TAPE mode needs x_init, eps_tape and noise_tape");
    if (!c.tape && !c.tdev && a->const_noise) return fail(h, LS_EUNSUPPORTED, "const_noise is supported in TAPE and TORCH_DEVICE modes only");
    if (c.tdev && (a->sample_offset & 3)) return fail(h, LS_EINVAL, "TORCH_DEVICE: the generator offset %llu is not a multiple of 4", (unsigned long long)a->sample_offset);
    if ((rc = check_dump_args(h, a)) != LS_OK) return rc;
    if (h->rk_n > 0) {          // ls_set_row_keys
        if (h->rk_n != c.B) return fail(h, LS_EINVAL, "ls_sample: %d row keys are set, the prepared batch is %d", h->rk_n, c.B);
        if (a->sample_offset != 0) return fail(h, LS_EINVAL, "ls_sample: row keys replace sample_offset + b; sample_offset must be 0");
        if (c.plms || c.inpaint) return fail(h, LS_EUNSUPPORTED, "ls_sample: row keys are not combined with PLMS or the inpainting branch");
        c.keyed = true;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    h->call_host = CallParams{a->seed, a->sample_offset, h->tag_base, 0u};      // uploaded by begin_loop's advance_tags with this call's tag base
    if ((rc = begin_loop(h, c, true)) != LS_OK) return rc;
    if ((rc = stage_loop_inputs(h, c)) != LS_OK) return rc;
    int replayed = 0;
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    if ((rc = run_loop(h, c, &replayed)) != LS_OK) return rc;
    return finish_loop(h, c, c.n_exec + (c.plms ? 1 : 0), replayed, false);      // model evaluations: PLMS's first step makes two
}

// One plms_sample (gaussian_diffusion.py:1016-1098): the launches an LS_SAMPLER_PLMS loop makes for that step, on caller-held tensors.
int ls_plms_step(ls_handle* h, const ls_plms_step_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_plms_step: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_plms_step before ls_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_plms_step before ls_set_schedule");
    if (a->index < 0 || a->index >= h->n_steps) return fail(h, LS_EINVAL, "step index %d outside [0,%d)", a->index, h->n_steps);
    if (a->order < 1 || a->order > 4) return fail(h, LS_EINVAL, "PLMS: order %d outside 1..4", a->order);
    if (a->n_hist < 0 || a->n_hist > 3) return fail(h, LS_EINVAL, "PLMS: n_hist %d outside 0..3", a->n_hist);
    if (!a->x || !a->eps_cond || !a->eps_uncond || !a->sample) return fail(h, LS_EINVAL, "ls_plms_step: null pointer");
    const bool first = a->n_hist == 0;
    if (first && a->order == 1) return fail(h, LS_EINVAL, "PLMS: order 1 without a history fails in the reference (old_out is None)");
    if (first && a->index < 1) return fail(h, LS_EINVAL, "PLMS: the first step of a loop evaluates the model at index - 1; index must be >= 1");
    if (first && (!a->eps_cond2 || !a->eps_uncond2)) return fail(h, LS_EINVAL, "PLMS: the first step needs the style eps of its second evaluation");
    for (int j = 0; j < a->n_hist; ++j) if (!a->hist[j]) return fail(h, LS_EINVAL, "PLMS: hist[%d] is null", j);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, JF = h->JF, od = a->on_device;
    const size_t nelem = (size_t)B * JF * h->T, nx = nelem * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    size_t ps = 0;
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    if ((rc = plms_planes(h, nelem, &ps)) != LS_OK) return rc;
    HIPCHK(h, h->xa.ensure(nx)); HIPCHK(h, h->xb.ensure(nx)); HIPCHK(h, h->fwd_cfg.ensure(nx)); HIPCHK(h, h->xtmp.ensure(nx));
    float* const ring = h->plms_buf.f();
    if ((rc = ingest_internal(h, a->x, h->xa.f(), B, od)) != LS_OK) return rc;
    // old_eps, newest first, into planes 0 .. n_hist - 1; this step's eps goes to plane 3; pred_xstart of the FIRST evaluation (clamped) to xtmp
    const int nh = (a->order < a->n_hist + 1 ? a->order : a->n_hist + 1) - 1;
    PlmsPlanes p{h->xa.f(), h->xb.f(), ring + 4 * ps, ring + 3 * ps, h->xtmp.f(), {nullptr, nullptr, nullptr}};
    for (int j = 0; j < nh; ++j) {
        if ((rc = ingest_internal(h, a->hist[a->n_hist - 1 - j], ring + (size_t)j * ps, B, od)) != LS_OK) return rc;
        p.hist[j] = ring + (size_t)j * ps;
    }
    const size_t ne = (size_t)B * kD;
    HIPCHK(h, h->eps.ensure(4 * ne * sizeof(float)));
    if ((rc = ingest_eps_pair(h, h->eps.f(), a->eps_cond, a->eps_uncond, od)) != LS_OK) return rc;
    if (first && (rc = ingest_eps_pair(h, h->eps.f() + 2 * ne, a->eps_cond2, a->eps_uncond2, od)) != LS_OK) return rc;
    if ((rc = advance_tags(h, st)) != LS_OK) return rc;
    HIPCHK(h, coop_reset(h, st));
    const Draws ev[2] = {{h->eps.f(), h->eps.f() + ne, nullptr, nullptr, 0u}, {h->eps.f() + 2 * ne, h->eps.f() + 3 * ne, nullptr, nullptr, 0u}};
    if ((rc = enqueue_plms_step(h, a->index, first, nh, p, ev, a->clip_denoised, single_pass(h, a->two_pass_always), nelem)) != LS_OK) return rc;
    if ((rc = egress_internal(h, p.x_out, a->sample, B, od)) != LS_OK) return rc;
    if (a->pred_xstart && (rc = egress_internal(h, p.pred_out, a->pred_xstart, B, od)) != LS_OK) return rc;
    if (a->eps_out && (rc = egress_internal(h, p.eps_out, a->eps_out, B, od)) != LS_OK) return rc;
    return sync_and_check(h, a->no_sync, od);
}

// _vb_terms_bpd's arithmetic (gaussian_diffusion.py:1226-1246) and the two MSEs of calc_bpd_loop (:1630-1632) on caller-held planes
int ls_vb_terms(ls_handle* h, const ls_vb_terms_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_vb_terms: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_vb_terms before ls_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_vb_terms before ls_set_schedule");
    if (!a->x_start || !a->x_t || !a->pred_xstart || !a->vb_out || !a->xstart_mse_out || (a->noise && !a->mse_out))
        return fail(h, LS_EINVAL, "ls_vb_terms: null pointer");
    if (!a->indices && (a->index < 0 || a->index >= h->n_steps)) return fail(h, LS_EINVAL, "schedule index %d outside [0,%d)", a->index, h->n_steps);
    const int B = h->B, od = a->on_device;
    if (a->indices && !a->indices_on_device)
        for (int b = 0; b < B; ++b)
            if (a->indices[b] < 0 || a->indices[b] >= h->n_steps)
                return fail(h, LS_EINVAL, "indices[%d] = %lld outside [0,%d)", b, (long long)a->indices[b], h->n_steps);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const size_t nelem = (size_t)B * h->JF * h->T, nx = nelem * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ensure_bpd_coef(h)) != LS_OK) return rc;
    if ((rc = ensure_pinned(h, h->bpd_x0, nx)) != LS_OK || (rc = ensure_pinned(h, h->bpd_xt, nx)) != LS_OK ||
        (rc = ensure_pinned(h, h->bpd_nz, nx)) != LS_OK || (rc = ensure_pinned(h, h->fwd_cfg, nx)) != LS_OK) return rc;
    HIPCHK(h, h->xtmp.ensure((size_t)3 * B * sizeof(float)));
    if ((rc = ingest_internal(h, a->x_start, h->bpd_x0.f(), B, od)) != LS_OK) return rc;
    if ((rc = ingest_internal(h, a->x_t, h->bpd_xt.f(), B, od)) != LS_OK) return rc;
    if ((rc = ingest_internal(h, a->pred_xstart, h->fwd_cfg.f(), B, od)) != LS_OK) return rc;
    if (a->noise && (rc = ingest_internal(h, a->noise, h->bpd_nz.f(), B, od)) != LS_OK) return rc;
    if (a->indices) {
        if ((rc = ingest(h, h->tidx, a->indices, (size_t)B * sizeof(int64_t), a->indices_on_device)) != LS_OK) return rc;
        if (!a->indices_on_device) HIPCHK(h, hipStreamSynchronize(st));        // a host index vector may be a temporary of the caller
    }
    VbArgs v{};
    v.x_start = h->bpd_x0.f(); v.x_t = h->bpd_xt.f(); v.noise = a->noise ? h->bpd_nz.f() : nullptr; v.pred = h->fwd_cfg.f();
    v.table = h->bpd_coef.f(); v.indices = a->indices ? static_cast<const int64_t*>(h->tidx.p) : nullptr;
    v.index = a->indices ? 0 : a->index; v.n_steps = h->n_steps; v.n = h->JF * h->T; v.clip = a->clip_denoised;
    float* const out = h->xtmp.f();
    v.vb = out; v.xstart_mse = out + B; v.mse = out + 2 * B; v.out_stride = 1; v.out_col = 0;
    HIPCHK(h, launch_vb_terms(v, B, st));
    if ((rc = egress(h, a->vb_out, out, (size_t)B * sizeof(float), od)) != LS_OK) return rc;
    if ((rc = egress(h, a->xstart_mse_out, out + B, (size_t)B * sizeof(float), od)) != LS_OK) return rc;
    if (a->noise && (rc = egress(h, a->mse_out, out + 2 * B, (size_t)B * sizeof(float), od)) != LS_OK) return rc;
    if (a->pred_out && (rc = egress_internal(h, h->fwd_cfg.f(), a->pred_out, B, od)) != LS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(st));
    return LS_OK;
}

// validate -> stage x_start and the tapes -> capture-or-enqueue the column loop -> the call's columns back
int ls_bpd(ls_handle* h, const ls_bpd_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_bpd: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_bpd before ls_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_bpd before ls_set_schedule");
    if (a->noise_mode == LS_NOISE_TORCH_DEVICE) return fail(h, LS_EUNSUPPORTED, "ls_bpd: TORCH_DEVICE draws are not generated in the column loop");
    if (h->rk_n > 0 && a->noise_mode == LS_NOISE_PHILOX) return fail(h, LS_EUNSUPPORTED, "ls_bpd: row keys (ls_set_row_keys) are not built for the column loop");
    if (a->noise_mode != LS_NOISE_TAPE && a->noise_mode != LS_NOISE_PHILOX) return fail(h, LS_EINVAL, "bad noise_mode");
    if (a->col_begin < 0 || a->col_count < 1 || a->col_count > h->n_steps - a->col_begin)
        return fail(h, LS_EINVAL, "columns [%d, %d + %d) outside the schedule's %d", a->col_begin, a->col_begin, a->col_count, h->n_steps);
    if (!a->x_start || !a->vb || !a->xstart_mse || !a->mse) return fail(h, LS_EINVAL, "ls_bpd: null pointer");
    const bool tape = a->noise_mode == LS_NOISE_TAPE;
    if (tape && (!a->noise_tape || !a->eps_tape)) return fail(h, LS_EINVAL, "TAPE mode needs noise_tape and eps_tape");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    h->seg_next = -1;
    const int B = h->B, T = h->n_steps, od = a->on_device, n = a->col_count;
    const size_t nelem = (size_t)B * h->JF * h->T, nx = nelem * sizeof(float);
    const bool pair = single_pass(h, a->two_pass_always);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    if ((rc = ensure_bpd_coef(h)) != LS_OK) return rc;
    h->call_host = CallParams{a->seed, a->sample_offset, h->tag_base, 0u};
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    if ((rc = ensure_pinned(h, h->bpd_x0, nx)) != LS_OK || (rc = ensure_pinned(h, h->bpd_xt, nx)) != LS_OK ||
        (rc = ensure_pinned(h, h->fwd_cfg, nx)) != LS_OK || (rc = ensure_pinned(h, h->bpd_out, (size_t)3 * B * T * sizeof(float))) != LS_OK) return rc;
    HIPCHK(h, h->xio.ensure(nx));
    if ((rc = advance_tags(h, st)) != LS_OK) return rc;
    if ((rc = ingest_internal(h, a->x_start, h->bpd_x0.f(), B, od)) != LS_OK) return rc;
    if (tape) {
        if ((rc = ingest_pinned(h, h->eps_tape, a->eps_tape, (size_t)n * 2 * B * kD * sizeof(float), od)) != LS_OK) return rc;
        if ((rc = ingest_pinned(h, h->noise_tape, a->noise_tape, (size_t)n * nx, od)) != LS_OK) return rc;
        if ((rc = ensure_pinned(h, h->bpd_tape, (size_t)n * nx)) != LS_OK) return rc;
        HIPCHK(h, launch_to_internal(h->noise_tape.f(), h->bpd_tape.f(), n * B, h->JF, st, h->T));      // every column's plane at once
    } else if ((rc = ensure_pinned(h, h->bpd_nz, nx)) != LS_OK) {
        return rc;
    }
    char key[192];
    snprintf(key, sizeof key, "BPD P%d B%d n%d cl%d w%u v%u p%d L%lld b%d k%d", h->precision, B, a->noise_mode, a->clip_denoised,
             h->weights_version, h->sched_version, (int)pair, plan_code(h), a->col_begin, n);
    int replayed = 0;
    HIPCHK(h, hipEventRecord(h->ev[1], st));
    if ((rc = run_captured(h, a->use_graph != 0, key, [&]() { return enqueue_bpd(h, a, pair, nelem); }, &replayed)) != LS_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[2], st));
    float* const outs[3] = {a->vb, a->xstart_mse, a->mse};
    for (int j = 0; j < 3; ++j)
        HIPCHK(h, hipMemcpy2DAsync(outs[j] + a->col_begin, (size_t)T * sizeof(float), h->bpd_out.f() + (size_t)j * B * T + a->col_begin,
                                   (size_t)T * sizeof(float), (size_t)n * sizeof(float), (size_t)B, od ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipEventRecord(h->ev[3], st));
    HIPCHK(h, hipStreamSynchronize(st));
    resolve_prepare_timing(h, true);
    if ((rc = coop_check(h)) != LS_OK) return rc;
    report_path(h, pair);
    HIPCHK(h, hipEventElapsedTime(&h->timing.loop_ms, h->ev[1], h->ev[2]));
    HIPCHK(h, hipEventElapsedTime(&h->timing.total_ms, h->ev[0], h->ev[3]));
    h->timing.n_step_launches = n;
    h->timing.single_pass = pair ? 1 : 0;
    h->timing.graph_replayed = replayed;
    h->timing.tape_upload_ms = 0.f;
    h->timing.n_segments = 1;
    return LS_OK;
}

}  // extern "C"
