/*
 * ls_hip.h -- C-ABI of the MI355X-native RAG denoising / diffusion-sampling engine.
 *
 * The reference (zyhbili/LivelySpeaker) is pure Python/PyTorch: it has no FFI, plugin registry
 * or operator API for this path.  Its "operator interface" is the pair
 *     model(x, timesteps, y=dict)                      scripts/model/RAG.py:98-133
 *     diffusion.p_sample_loop / ddim_sample_loop(...)  scripts/diffusion/gaussian_diffusion.py:608-671, 895-943
 * The entry points below are what a ctypes binding on the reference side would call to replace
 * those two; each cites the reference code it stands in for.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * LS_E* code and never throws across the ABI; ls_last_error() gives the message.  One handle owns
 * one GPU (one HIP stream, its captured hipGraphs, all device buffers); a handle is not
 * thread-safe, distinct handles are independent.  Pointers in ls_cond / ls_sample_args /
 * ls_forward_args are host pointers unless the struct's on_device flag is set, in which case they
 * are device pointers on the handle's GPU.  The library never frees or retains caller memory.
 * All tensors are fp32, C-contiguous, in the reference's layouts ([B, njoints, nfeats, nframes]).
 */
#ifndef LS_HIP_H
#define LS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LS_ABI_VERSION 5

enum {
    LS_OK = 0,
    LS_EINVAL = -1,   /* bad argument / shape / unknown key            */
    LS_ESTATE = -2,   /* call order (weights / schedule / prepare missing) */
    LS_EHIP = -3,     /* a HIP runtime call failed                     */
    LS_ENOMEM = -4,
    LS_EUNSUPPORTED = -5
};

/* PLMS: plms_sample_loop (gaussian_diffusion.py:1016-1211), ls_sample only (single steps: ls_plms_step).
 * DDIM_REVERSE: ddim_reverse_sample (:857-893), ls_step only. */
enum { LS_SAMPLER_DDPM = 0, LS_SAMPLER_DDIM = 1, LS_SAMPLER_PLMS = 2, LS_SAMPLER_DDIM_REVERSE = 3 };
/* TORCH_DEVICE: the reference's draws as a GPU run of it makes them, from torch's device generator (Philox4x32-10 behind torch's
 * grid-stride launch geometry, ls_torch_randn), generated on the device inside the loop: bitwise torch.randn / randn_like on the
 * handle's GPU, in the reference's order, shapes and memory orders (as the TAPE tapes of the torch_cpu mode are drawn). */
enum { LS_NOISE_TAPE = 0, LS_NOISE_PHILOX = 1, LS_NOISE_TORCH_DEVICE = 2 };
/* Arithmetic of the channel-mixing GEMM (92 % of the FLOPs).
 * FP32 (default): in the fused step kernel, split-fp32: both fp32 operands split exactly into three bf16 parts
 *   (a = a0 + a1 + a2, round-to-nearest splits) and the partial products of v_mfma_f32_16x16x32_bf16 kept down to the
 *   terms of order 2^-16 (six of the nine), accumulated in fp32 smallest first; an fp32-class product error (bound: DESIGN.md section 2,
 *   measured accuracy: section 4).  The other
 *   step kernels (sample-split, one-pass-per-workgroup, batch-level) run it on v_mfma_f32_16x16x4_f32.  A non-finite operand
 *   makes the split residuals NaN, so an Inf input gives NaN where the fp32 MFMA may give Inf: non-finite either way.
 * FP32_MFMA: v_mfma_f32_16x16x4_f32 everywhere (exact fp32 products, the pre-split kernel; kept for A/B runs and audits).
 * BF16X3 (opt-in): each fp32 operand split into bf16 hi+lo, three v_mfma_f32_16x16x32_bf16 per product
 *   (hi.hi + hi.lo + lo.hi, fp32 accumulate): ~2^-16 relative product error, parity-gated at the 1e-3 contract. */
enum { LS_PRECISION_FP32 = 0, LS_PRECISION_BF16X3 = 1, LS_PRECISION_FP32_MFMA = 2 };

typedef struct ls_handle ls_handle;

/* Static shape of the denoiser: RAG.__init__ (scripts/model/RAG.py:17-77; BEAT variant
 * scripts_beat/model/RAG.py:56,72-74) + get_model_args (scripts/mdm_utils/model_util.py:20-37). */
typedef struct ls_config {
    int32_t njoints;          /* 9 (TED) | 47 (BEAT)                               */
    int32_t nfeats;           /* 3 | 6                                             */
    int32_t nframes;          /* 34 = the reference's (token-mixing conv fixes it): fused step kernel.  Any other
                                 value selects the synthetic long-sequence path (e.g. 150 frames, BASELINE configs[4]'s
                                 wording; the reference cannot run it -- perf-only, checked against this repo's oracle) */
    int32_t n_prefix_tokens;  /* 1 = [style] | 2 = [style, emotion]                */
    int32_t n_pre_seq;        /* 4 prefix poses (RAG.py:70)                        */
    int32_t latent_dim;       /* 512                                               */
    int32_t layers;           /* 8                                                 */
    int32_t audio_len;        /* 36267 | 36266 raw samples -> 34 audio frames (must yield nframes) */
    int32_t n_speakers;       /* 1400 (RAG.py:65)                                  */
    int32_t n_emotions;       /* 0 | 8                                             */
    int32_t device;           /* HIP device ordinal                                */
    int32_t reserved;
} ls_config;

/* GaussianDiffusion.__init__ tables after SpacedDiffusion (gaussian_diffusion.py:168-204,
 * respace.py:74-88), fp64 as the reference keeps them; cast to fp32 per step exactly like
 * _extract_into_tensor (gaussian_diffusion.py:1651-1664).  Each array has n_steps entries. */
typedef struct ls_schedule {
    int32_t n_steps;
    int32_t reserved;
    const int64_t* timestep_map;                 /* _WrappedModel, respace.py:125-130 */
    const double* sqrt_alphas_cumprod;           /* q_sample, :240-258               */
    const double* sqrt_one_minus_alphas_cumprod;
    const double* posterior_mean_coef1;          /* q_posterior_mean_variance :260-282 */
    const double* posterior_mean_coef2;
    const double* posterior_log_variance_clipped;/* p_sample :507-558 (FIXED_SMALL)  */
    const double* alphas_cumprod;                /* ddim_sample :745-798             */
    const double* alphas_cumprod_prev;
    const double* sqrt_recip_alphas_cumprod;     /* _predict_eps_from_xstart :418-422 */
    const double* sqrt_recipm1_alphas_cumprod;
} ls_schedule;

/* model_kwargs['y'] of the callers (scripts/test_RAG_ted.py:64-70): only the keys RAG.forward
 * reads.  origin_x is NOT mutated here (the Python shim reproduces RAG.py:110's in-place zeroing). */
typedef struct ls_cond {
    int32_t batch;
    int32_t on_device;
    const float* audio_input;   /* [B, audio_len]                                  */
    const float* origin_x;      /* [B, J, F, T]; frames >= n_pre_seq are ignored   */
    const int64_t* vid_indices; /* [B] < n_speakers                                */
    const int64_t* emo;         /* [B, T] emotion ids as the callers hold y['emo'] (frame 0 is read,
                                   scripts_beat/model/RAG.py:125), or NULL (TED); same shape as ls_train_batch.emo */
    const float* scale;         /* [B] guidance scale (cfg_sampler.py:31)          */
} ls_cond;

/* One call of p_sample_loop / ddim_sample_loop with ClassifierFreeSampleModel as the model. */
typedef struct ls_sample_args {
    int32_t sampler;            /* LS_SAMPLER_*                                     */
    int32_t noise_mode;         /* LS_NOISE_*                                       */
    int32_t skip_timesteps;     /* gaussian_diffusion.py:712 / :982                 */
    int32_t const_noise;        /* :545-546 / :706-707 (TAPE and TORCH_DEVICE modes) */
    int32_t on_device;
    int32_t use_graph;          /* 1: capture the step loop in a hipGraph and replay */
    int32_t clip_denoised;      /* clamp pred_xstart to [-1,1] (callers pass False)  */
    int32_t two_pass_always;    /* 0: when every scale == 1 the uncond pass is skipped (out_u + 1*(out_c - out_u) = out_c,
                                   cfg_sampler.py:31; the callers run guidance_param = 1); 1: always evaluate both passes.
                                   NOT bit-identical: in fp32 out_u + 1*(out_c - out_u) differs from out_c by up to one rounding
                                   of the larger term, so the two settings agree to ~1e-5 on samples (tests: <= 3e-4), not bitwise;
                                   with 0, ls_step / ls_forward-style raw outputs of the uncond pass are not produced. */
    float eta;                  /* DDIM eta (callers never pass it: 0)              */
    int32_t n_dump;             /* dump_steps (DDPM only, :660-671)                 */
    const int32_t* dump_steps;  /* executed-step counters (0 = first executed step), host memory */
    float* dump_out;            /* [n_dump, B, J, F, T] pred_xstart                 */
    const float* x_init;        /* [B,J,F,T] x_T = the loop's first randn; NULL only with PHILOX or TORCH_DEVICE (the loop draws x_T;
                                   given = the reference's `noise=`, no x_T draw) */
    const float* init_image;    /* [B,J,F,T] or NULL (zeros when skip_timesteps>0)  */
    const float* eps_tape;      /* TAPE: [n_exec, 2, B, latent_dim] style eps (cond, uncond) */
    const float* noise_tape;    /* TAPE: [n_exec, B, J, F, T] per-step randn_like(x) */
    uint64_t seed;              /* PHILOX key; TORCH_DEVICE: the torch device generator's seed (initial_seed())          */
    uint64_t sample_offset;     /* PHILOX: global index of sample 0 (shard-invariant streams); TORCH_DEVICE: the generator's
                                   Philox offset (get_offset(), a multiple of 4) before the loop's first draw.  The draws of
                                   the loop advance it by a total that depends on the shapes only (ls_torch_randn_advance per
                                   draw); the caller sets the generator there afterwards.  Both values are read from device
                                   memory by the captured loop: a replay takes new ones without a recapture. */
    float* out;                 /* [B, J, F, T]                                     */
    /* Segmented TAPE mode (seg_count > 0): this call runs the executed-step counters [seg_begin, seg_begin + seg_count) of the loop
     * and eps_tape / noise_tape hold THOSE steps only ([seg_count, 2, B, D] / [seg_count, B, J, F, T]) -- the reference's
     * "identical seeds" mode draws two style eps and one randn_like(x) per step from the host generator
     * (gaussian_diffusion.py:700-743, RAG.py:120), 4 GB for 512 clips x 1000 steps if drawn in one piece.  seg_begin == 0 starts the
     * loop (x_init / init_image are read then); x_t stays in the handle between segments; segments must follow each other in
     * order; `out` (and dump_out) are written by the segment that ends the loop, which is also the only one that waits for the GPU.
     * Host tapes (on_device == 0) are uploaded on the handle's COPY stream into a two-slot device buffer while the previous
     * segment's steps run; they should be page-locked, and a segment's host buffers may be reused as soon as the NEXT segment call
     * has returned.  Plain launches (use_graph is ignored).  seg_count == 0: the whole loop in one call (everything above). */
    int32_t seg_begin;
    int32_t seg_count;
    /* p_mean_variance's inpainting branch (gaussian_diffusion.py:314-320; BEAT tree scripts_beat/...:319), off while inpaint_mask is
     * NULL: every step's (CFG-combined) model output is replaced, where the mask is set, by the given motion -- re-noised with
     * q_sample(inpainted_motion, t - 1) while t > 0 when inpaint_noised (the TED tree: its randn_like is inpaint_noise[k] in TAPE mode,
     * the device stream 4 in PHILOX mode), as it is otherwise (the BEAT tree) -- before clip_denoised and the sampler update.  The loop
     * then runs the denoiser and the update as two launches per step.  Not combined with segments. */
    const unsigned char* inpaint_mask;   /* [B,J,F,T] bytes (non-zero = take the given motion), or NULL           */
    const float* inpainted_motion;       /* [B,J,F,T]                                                            */
    const float* inpaint_noise;          /* TAPE + inpaint_noised: [n_exec,B,J,F,T]; entries of steps with t == 0 unused */
    int32_t inpaint_noised;
    /* LS_SAMPLER_PLMS: the order of the multistep method, 2..4 (0 with every other sampler).  The loop makes n_exec + 1 model
     * evaluations: the first executed step evaluates at (x, i) and at (mean_pred, i - 1) (the pseudo improved Euler start, :1066-1073),
     * every later step once, with Adams-Bashforth over the last min(order, steps so far) eps (:1075-1090).  TAPE mode: eps_tape is
     * [n_exec + 1, 2, B, latent_dim] in evaluation order and noise_tape is NULL (PLMS draws no step noise); PHILOX mode: evaluation e
     * uses the style-eps streams of step_id = e.  At least two executed steps.  Not combined with TORCH_DEVICE, dump_steps,
     * const_noise, eta, segments or the inpainting arguments. */
    int32_t plms_order;
} ls_sample_args;

/* One RAG.forward pair (cond / uncond) and optionally the CFG combination, for model(x,t,y)
 * parity (RAG.py:98-133, cfg_sampler.py:24-31). Any of the three outputs may be NULL. */
typedef struct ls_forward_args {
    int32_t on_device;
    int32_t no_sync;            /* on_device only: return without waiting for the GPU (order consumers with ls_stream_order) */
    const float* x;             /* [B,J,F,T]                                        */
    const int64_t* timesteps;   /* [B] model-scale t in [0, 5000)                   */
    const float* eps_cond;      /* [B, latent_dim] randn_like of reparameterize (RAG.py:12) */
    const float* eps_uncond;    /* [B, latent_dim]                                  */
    float* out_cond;            /* [B,J,F,T]                                        */
    float* out_uncond;
    float* out_cfg;             /* out_u + scale*(out_c - out_u)                    */
    float* trace;               /* debug: [B, layers+1, 2*S, latent_dim] residual stream, or NULL */
} ls_forward_args;

/* One p_sample / ddim_sample step (gaussian_diffusion.py:507-558, 745-798) at schedule index i -- or, as the reference's
 * signature allows (`t` is a [B] tensor), at one schedule index PER SAMPLE (`indices`). */
typedef struct ls_step_args {
    int32_t sampler;            /* LS_SAMPLER_DDPM | DDIM | DDIM_REVERSE (x_{t+1} of the deterministic DDIM ODE: the DDIM arithmetic with
                                   alphas_cumprod_next = append(alphas_cumprod[1:], 0) in place of alphas_cumprod_prev, eta and noise unused) */
    int32_t index;              /* schedule index i (model sees timestep_map[i]); ignored when indices != NULL */
    int32_t on_device;
    float eta;
    int32_t clip_denoised;
    int32_t two_pass_always;    /* as in ls_sample_args                             */
    const float* x;             /* [B,J,F,T]                                        */
    const float* eps_cond;
    const float* eps_uncond;
    const float* noise;         /* [B,J,F,T]; may be NULL with DDIM_REVERSE         */
    float* sample;              /* [B,J,F,T]                                        */
    float* pred_xstart;         /* [B,J,F,T] or NULL                                */
    const int64_t* indices;     /* [B] schedule index per sample, or NULL (uniform `index`).  When the entries differ the denoiser runs
                                   with one timestep-embedding row per sample and the posterior / DDIM update is a separate
                                   elementwise kernel with per-sample coefficients (same arithmetic as the fused epilogue).  HOST
                                   indices are validated (a constant vector takes the fused path); DEVICE indices
                                   (indices_on_device) are never read by the host -- no round trip in a step-by-step caller --
                                   always take the per-sample path and are clamped into [0, n_steps). */
    int32_t no_sync;            /* on_device only: return without waiting for the GPU (order consumers with ls_stream_order) */
    int32_t indices_on_device;
    const unsigned char* inpaint_mask;   /* as in ls_sample_args; uniform `index` only                          */
    const float* inpainted_motion;
    const float* inpaint_noise;          /* [B,J,F,T] the randn_like of q_sample(inpainted_motion, t - 1), or NULL = un-noised */
} ls_step_args;

/* One plms_sample step (gaussian_diffusion.py:1016-1098) at the uniform schedule index `index`.  n_hist = entries of old_out["old_eps"]
 * handed in (0..3, oldest first; a longer list: its last three).  n_hist == 0 is the first call of a loop (order > 1, index >= 1): two
 * model evaluations, the second at (mean_pred, index - 1) with its own style eps (eps_cond2 / eps_uncond2).  Otherwise one evaluation
 * and Adams-Bashforth of order min(order, n_hist + 1).  Launches what an LS_SAMPLER_PLMS loop launches for that step. */
typedef struct ls_plms_step_args {
    int32_t index;
    int32_t order;              /* 1..4 (1 needs n_hist >= 1: the reference fails without a history)            */
    int32_t n_hist;
    int32_t on_device;
    int32_t clip_denoised;      /* clamps pred_xstart BEFORE eps is derived from it (p_mean_variance, :365-371) */
    int32_t two_pass_always;
    int32_t no_sync;            /* on_device only, as in ls_step_args                                           */
    int32_t reserved;
    const float* x;             /* [B,J,F,T]                                                                    */
    const float* eps_cond;      /* [B, latent_dim] style eps of the (first) evaluation                          */
    const float* eps_uncond;
    const float* eps_cond2;     /* second evaluation (n_hist == 0), else NULL                                   */
    const float* eps_uncond2;
    const float* hist[3];       /* [B,J,F,T] each, oldest first                                                 */
    float* sample;              /* [B,J,F,T]                                                                    */
    float* pred_xstart;         /* [B,J,F,T] of the first evaluation, or NULL                                   */
    float* eps_out;             /* [B,J,F,T] this step's eps (first evaluation), the entry appended to old_eps; or NULL */
} ls_plms_step_args;

typedef struct ls_timing {
    float prepare_ms;           /* last ls_prepare, GPU time (HIP events on the handle's stream); -1 while an ls_prepare_async is in flight */
    float loop_ms;              /* last ls_sample: first step launch .. last step done */
    float total_ms;             /* last ls_sample incl. layout conversion and copies */
    int32_t n_step_launches;    /* model evaluations of the last loop (PLMS: executed steps + 1) */
    int32_t graph_replayed;     /* 1 if the loop ran as a hipGraph replay           */
    int32_t single_pass;        /* 1 if the loop ran the single-pass (scale == 1) kernel */
    float tape_upload_ms;       /* segmented TAPE mode: summed GPU-side duration of the tape uploads of the last loop (copy stream) */
    int32_t n_segments;         /* segments the last loop ran in (1 = one call)     */
    int32_t step_path;          /* kernels the last loop's steps ran on: 0 one workgroup per sample (fused), 1 batch-level, 2 sample-split, 3 one workgroup per (sample, pass) */
    int32_t tail_samples;       /* a batch the plan splits (e.g. full fused rounds + a partial one): samples of the second piece, run on ... */
    int32_t tail_path;          /* ... 1 the batch-level, 2 the sample-split, 3 the one-pass-per-workgroup kernels (0: none) */
    int32_t tail2_samples;      /* third piece of the plan (e.g. 416 clips = 256 fused + 128 one-pass-per-workgroup + 32 sample-split) */
    int32_t tail2_path;
    int32_t n_cus;              /* compute units of the handle's device (hipDeviceProp.multiProcessorCount): what the plans and the
                                   sample-split kernel's residency are derived from */
    int32_t coop_slices;        /* slice workgroups per (sample, pass) the sample-split piece of the last loop ran with: 8 | 4 | 2 (0: the plan had no such piece);
                                   a long-sequence model (nframes != 34, step_path 1): 4 = its eight blocks ran in the one-launch mixer kernel, 0 = as batch-level launches */
} ls_timing;

int ls_abi_version(void);
int ls_create(const ls_config* cfg, ls_handle** out);
void ls_destroy(ls_handle* h);
const char* ls_last_error(const ls_handle* h);   /* h may be NULL: error of the last failed ls_create */

/* load_state_dict (scripts/mdm_utils/model_util.py:5-10): key = reference state-dict key, data =
 * fp32 host array of n elements.  '*.pe' buffers are accepted and ignored (recomputed).
 * ls_commit_weights builds the MFMA-ordered device images; it fails if a required key is missing. */
int ls_set_weight(ls_handle* h, const char* key, const float* data, size_t n);
int ls_commit_weights(ls_handle* h);

int ls_set_precision(ls_handle* h, int mode);             /* LS_PRECISION_*; default FP32 */
/* Which kernels a 34-frame model's steps run on.  0 (default): chosen per prepared batch -- the fused kernel gives every sample a
 * workgroup (= one CU: a step costs one CU's time for eight layers however small the batch); the sample-split kernel spreads a
 * sample over 16 workgroups (2 CFG passes x 8 channel slices) that exchange LayerNorm partials and rows through L2 inside ONE launch
 * per step, and takes the small batches; 1: always one workgroup per sample; 2: the batch-level kernels of the long-sequence path
 * (21 launches per step; exact fp32, both CFG passes always evaluated); 3: always the sample-split kernel (exact fp32); 4: always the
 * one-pass-per-workgroup kernel (a workgroup of 4 waves per (sample, CFG pass), two independent workgroups per CU, the passes combined by
 * the later of the two: half-CU granularity, exact fp32; grids of up to one workgroup per CU run as 8-wave workgroups, larger ones as
 * 4-wave workgroups, two per CU); 5: the same kernel with the 4-wave / two-per-CU form at EVERY grid size (what mode 4 and the plans of
 * a device with fewer CUs reach only beyond one workgroup per CU; this selector pins that form to the reference's fixtures); 6 / 7 / 8:
 * the sample-split kernel with its slicing forced to 4 / 2 / 8 channel slices per (sample, CFG pass) (mode 3 chooses per piece).  Same
 * arithmetic every way, different summation order: results agree to ~1e-5, not bitwise.  Takes effect at the next ls_prepare;
 * ls_timing.step_path reports what ran.
 * A long-sequence model (nframes != 34) always runs on the batch-level kernels, except that with 145..160 tokens the eight blocks and
 * poseFinal of a SAMPLING loop run in one launch of the sample-split mixer (ls_timing.coop_slices == 4; 3 launches per step instead of
 * 21) where every launch is at least 7/8 full: 28-32 / 60-64 / 92-96 clips on 256 compute units.  There mode 2 forces the batch-level
 * kernels and mode 3 the mixer at every batch size; the other modes return LS_EUNSUPPORTED.  Steps with per-sample timesteps (ls_step, ls_forward) keep
 * the batch-level kernels. */
int ls_set_path(ls_handle* h, int mode);
/* The plan mode 0 makes for `batch` clips on a device of `n_cus` compute units, without a handle or a GPU (what ls_prepare decides, exposed
 * for inspection and for the CPU test suite): out10 = {pieces, then (kernel family as in ls_timing.step_path, first clip, clips) for up to
 * three pieces}; *ms (nullable) = the step-time model's estimate.  beat: 0 TED / 1 BEAT cost table; single_pass: every guidance scale is 1. */
int ls_plan_query(int beat, int batch, int single_pass, int precision, int n_cus, int* out10, float* ms);
/* Slice workgroups per (sample, CFG pass) -- 8, 4 or 2 -- the sample-split kernel uses for a plan piece of `groups` (sample, pass) groups
 * (clips x 2 under CFG, clips x 1 in the single-pass form) on a device of `n_cus` compute units; negative error code otherwise. */
int ls_plan_coop_slices(int beat, int groups, int n_cus);
int ls_set_schedule(ls_handle* h, const ls_schedule* s);
int ls_prepare(ls_handle* h, const ls_cond* c);           /* once per sampling call */
/* The same, enqueued on the handle's stream WITHOUT waiting: later calls on this handle are ordered behind it, so the caller may
 * overlap it with work on another stream (LivelySpeaker: the SAG decode, scripts/test_LivelySpeaker_ted.py:88-113, needs none of it).
 * Device-resident inputs must stay valid until the next synchronising call on this handle; HOST inputs (on_device == 0) have been
 * copied out of the caller's buffers when the call returns (it waits for those copies, not for the kernels);
 * ls_timing.prepare_ms reads -1 until the work is known to be done. */
int ls_prepare_async(ls_handle* h, const ls_cond* c);
int ls_sample(ls_handle* h, const ls_sample_args* a);
int ls_forward(ls_handle* h, const ls_forward_args* a);

/* ---- Long-form synthesis: W windows of T = nframes frames chained on the device.  Window w reads the audio samples
 * [w * audio_stride, w * audio_stride + audio_len) of every clip (audio_stride = 32000: T - n_pre_seq = 30 frames at 15 fps of 16 kHz
 * audio) and is conditioned on the last n_pre_seq poses of window w - 1 (window 0: on seed_poses), the way origin_x[..., :n_pre_seq]
 * conditions one clip (RAG.py:110-112).  ls_long_prepare runs the WavEncoder over all W * B clip-windows once, in chunks, and the
 * per-batch stages of ls_prepare (speaker style, guidance scales, step plan, workspaces) once at batch B; it replaces the handle's
 * prepared conditioning.  ls_long_sample then runs, per window, with no copy from the device and no synchronisation in
 * between: the hand-off kernel (ls_chain.hip), the two static projections of ls_prepare, and the loop of ls_sample (its captured
 * graph is replayed per window).  Fused 34-frame models only. */
#define LS_LONG_AUDIO_STRIDE 32000
typedef struct ls_long_cond {
    int32_t batch;
    int32_t n_windows;          /* W >= 1                                                                             */
    int32_t on_device;
    int32_t encoder_chunk;      /* clip-windows per WavEncoder pass (bounds its workspaces: ~1.5 MB per clip); 0: 256 */
    int64_t audio_samples;      /* L: samples per clip in `audio`; shorter than audio_len + (W-1) * audio_stride = zero-padded at the
                                   end, longer = the rest is not read                                                 */
    const float* audio;         /* [B, L]                                                                             */
    const float* seed_poses;    /* [B, J, F, n_pre_seq]: origin_x[..., :n_pre_seq] of window 0                        */
    const int64_t* vid_indices; /* [B]                                                                                */
    const int64_t* emo;         /* [W, B] one emotion id per window and clip (y['emo'][:, 0] of that window), or NULL (TED) */
    const float* scale;         /* [B]                                                                                */
} ls_long_cond;
int ls_long_prepare(ls_handle* h, const ls_long_cond* c);

/* ---- Clips of different lengths in one long-form call: a clip's windows stop when its audio has ended.
 * Clip b of audio_lengths[b] samples runs W_b = max(1, ceil((audio_lengths[b] - audio_len) / audio_stride) + 1) windows.  The clips
 * are held in SLOTS, stably sorted by W_b, longest first (ties keep the caller's order), so the B_w clips with W_b > w that run window w
 * are slots [0, B_w) of every per-clip buffer, and window w is a sampling call at batch B_w: its own step plan, its own single-pass
 * decision (the scales of its clips), its own captured loop.  ls_long_plan_drop is that plan (no handle, no GPU): slot_row [batch] =
 * the caller's clip behind each slot, slot_windows [batch] = its W_b, active[w] = B_w for w < min(W_max, active_capacity) (B_0 = batch),
 * *n_windows = W_max.  slot_row, slot_windows and active may be NULL (active: with active_capacity 0).
 *
 * ls_long_prepare_ragged takes c->audio [B, L] (L = c->audio_samples), c->seed_poses and audio_lengths (host, [B], each in [1, L]) in
 * the CALLER's clip order -- it reads them through the slot table -- and c->vid_indices [B], c->scale [B] and c->emo [W_max, B] in
 * SLOT order (row s = clip slot_row[s]); c->n_windows must be W_max.  Samples at and beyond audio_lengths[b] are never read and count
 * as zero.  Only the sum of B_w clip-windows that exist go through the WavEncoder.  ls_long_sample then runs window w at batch B_w:
 *   - text_features [W_max, B, latent_dim] is in slot order too; entries of (w, slot) pairs that do not run are not read;
 *   - TAPE: the tapes are packed, window after window: x_init [sum B_w, J, F, T], then per window eps [n_exec, 2, B_w, latent_dim] and
 *     noise [n_exec, B_w, J, F, T], each concatenated over the windows -- the draws of one sampling call per window at batch B_w;
 *   - PHILOX: slot s of window w draws the streams of global sample index sample_offset + s + (w << 48): the streams follow the
 *     slot, so a batch that is already longest-first gets the draws of the equal-length call;
 *   - timeline and windows are in the caller's order and zeroed first: clip b's timeline is 0 from frame T + (W_b - 1)(T - n_pre_seq)
 *     on, its raw windows w >= W_b are 0;
 *   - ls_timing: n_segments = W_max, n_step_launches = W_max * n_exec, graph_replayed = the windows served by a replay.  A window batch
 *     that serves two or more windows is captured once (the handle caches a few graphs); one that serves a single window runs as
 *     stream launches, which give the same bits.
 * Device-resident length arrays are not built. */
int ls_long_plan_drop(int32_t batch, int32_t audio_len, const int64_t* audio_lengths, int32_t* slot_row, int32_t* slot_windows,
                      int32_t* active, int32_t active_capacity, int32_t* n_windows);
int ls_long_prepare_ragged(ls_handle* h, const ls_long_cond* c, const int64_t* audio_lengths);

struct ls_sag;
typedef struct ls_long_sample_args {
    int32_t sampler;            /* LS_SAMPLER_DDPM | LS_SAMPLER_DDIM                                                  */
    int32_t noise_mode;         /* LS_NOISE_TAPE | LS_NOISE_PHILOX                                                    */
    int32_t skip_timesteps;
    int32_t on_device;
    int32_t use_graph;
    int32_t clip_denoised;
    int32_t two_pass_always;
    float eta;
    const float* x_init;        /* TAPE: [W, B, J, F, T] x_T of every window; PHILOX: NULL                            */
    const float* eps_tape;      /* TAPE: [W, n_exec, 2, B, latent_dim]                                                */
    const float* noise_tape;    /* TAPE: [W, n_exec, B, J, F, T]                                                      */
    uint64_t seed;              /* PHILOX: one key per call                                                           */
    uint64_t sample_offset;     /* PHILOX: global index of clip 0; window w draws the streams of global sample index
                                   sample_offset + b + (w << 48) (ls_philox.h), so batch + sample_offset < 2^48       */
    struct ls_sag* sag;         /* LivelySpeaker chain: window w starts from q_sample(decoder(x = origin_x_w, z = text_features[w],
                                   mask = ones)) as ls_sample's init_image; NULL: from zeros when skip_timesteps > 0  */
    const float* text_features; /* with sag: [W, B, latent_dim]                                                       */
    float* timeline;            /* [B, J, F, T + (W - 1) * (T - n_pre_seq)]: window 0's frames, then frames n_pre_seq.. of each later one */
    float* windows;             /* [W, B, J, F, T] the raw windows, or NULL                                           */
} ls_long_sample_args;
int ls_long_sample(ls_handle* h, const ls_long_sample_args* a);

/* ---- Edit a stretch of a long-form timeline: masked re-synthesis of the windows it touches (ls_long_edit, after ls_long_prepare with
 * the conditioning of the call that made the timeline).  With S = T - n_pre_seq, window w covers the timeline frames [w S, w S + T) and
 * OWNS [0, T) for w = 0, [w S + n_pre_seq, w S + T) otherwise (the stitching of ls_long_sample).  Element (b, c, f) of window w is
 * EDITABLE iff channels[b][c] is set, frame_lo[b] <= w S + f < frame_hi[b], and frame w S + f is owned by w.  The windows with at least
 * one editable element of at least one clip run, in ascending order, all B clips each (ls_long_edit_plan is that set; no handle, no
 * GPU): the window's T frames are read from the timeline as it stands by then; they are ls_sample's inpainted_motion, with
 * inpaint_mask = not editable, its first n_pre_seq frames condition the window as origin_x (window 0: the prepared seed_poses), and with
 * skip_timesteps > 0 they are its init_image as well; the loop is ls_sample's (two launches per step, see inpaint_mask there); the
 * editable elements of its result are stored into the timeline and nothing else of the timeline is written.  A window behind the last
 * one that ran is not resampled even where its conditioning frames changed (widen the range to have it resampled), and a clip whose
 * range misses a running window runs in it with every element kept.
 * Not built: PLMS, const_noise, dump_steps; in this dense form also handles of ls_long_prepare_ragged and encoding only the edited
 * windows' audio -- both are ls_long_prepare_edit / ls_long_edit_compact's, further down.  Anything but one rectangle per clip --
 * several stretches, pinned keyframes, joints per stretch -- is ls_long_edit_mask's, further down still. */
typedef struct ls_long_edit_args {
    int32_t sampler;            /* LS_SAMPLER_DDPM | LS_SAMPLER_DDIM                                                  */
    int32_t noise_mode;         /* LS_NOISE_TAPE | LS_NOISE_PHILOX                                                    */
    int32_t skip_timesteps;
    int32_t on_device;          /* timeline, windows and the tapes are device pointers                                */
    int32_t use_graph;
    int32_t clip_denoised;
    int32_t two_pass_always;
    float eta;
    int32_t inpaint_noised;     /* the given motion is re-noised with q_sample(., t - 1) while t > 0 (the TED tree)   */
    int32_t windows_capacity;   /* entries of windows_run (0 with NULL)                                               */
    const int32_t* frame_lo;    /* HOST [B]: clip b is edited on the frames [frame_lo[b], frame_hi[b]), 0 <= lo <= hi <= T_total */
    const int32_t* frame_hi;    /* HOST [B]; lo == hi: the clip is not edited                                         */
    const unsigned char* channels; /* HOST bytes [B, J*F] (non-zero = the channel is edited), or NULL: every channel  */
    float* timeline;            /* [B, J, F, T + (W - 1) S], edited in place (a host one: uploaded, edited, downloaded) */
    float* windows;             /* [We, B, J, F, T] the raw samples of the We windows that ran, or NULL               */
    int32_t* windows_run;       /* HOST, nullable: the first min(We, windows_capacity) windows that ran, ascending    */
    int32_t* n_windows_run;     /* HOST, nullable: We                                                                  */
    /* TAPE: the draws of the We windows that ran, in ascending window order */
    const float* x_init;        /* [We, B, J, F, T]                                                                   */
    const float* eps_tape;      /* [We, n_exec, 2, B, latent_dim]                                                     */
    const float* noise_tape;    /* [We, n_exec, B, J, F, T]                                                           */
    const float* inpaint_noise; /* [We, n_exec, B, J, F, T] with inpaint_noised                                       */
    uint64_t seed;              /* PHILOX: one key per call                                                           */
    uint64_t sample_offset;     /* PHILOX: window w draws at sample_offset + b + (w << 48), as in ls_long_sample: a window's
                                   streams do not depend on which other windows run                                   */
} ls_long_edit_args;
/* window_flags [n_windows] (nullable): 1 where the window runs; *n_out: how many do.  LS_EINVAL on a range outside [0, T + (W - 1) S]
 * or with lo > hi. */
int ls_long_edit_plan(int32_t batch, int32_t n_windows, int32_t T, int32_t n_pre, const int32_t* lo, const int32_t* hi,
                      int32_t* window_flags, int32_t* n_out);
int ls_long_edit(ls_handle* h, const ls_long_edit_args* a);

/* ---- ls_long_edit with the LivelySpeaker start: a script-guided edit.  The windows, their order, inpaint_mask / inpainted_motion /
 * origin_x, the draws (the decoder draws nothing) and the scatter of the editable elements are ls_long_edit's.  What changes is the
 * image a window that runs starts from: with sag_out = decoder(x = origin_x_w, z = text_features[w], mask = ones) [B, J, F, T],
 *     init_w = editable ? sag_out : the window's slice of the timeline
 * is ls_sample's init_image at EVERY skip_timesteps >= 0 (at 0: q_sample(init_w, n_steps - 1, x_T), gaussian_diffusion.py:709-716, as
 * in ls_long_sample with sag).  origin_x_w holds the first n_pre_seq frames of the slice as the earlier windows of this call left the
 * timeline (window 0: the seed poses), so the decoder of window w + 1 sees what window w has just written.  A clip whose range misses
 * a running window starts from its slice there (its decoder output is unused), and with `channels` only the selected channels start
 * from the decoder.  text_features is [W, B, latent_dim], W the prepared windows; rows of windows that do not run are not read; a
 * host array (device iff a->on_device) is uploaded once per call.  Per window: k_edit_gather, the decoder on its own stream, ordered
 * by events, k_edit_start (ls_chain.hip), the loop, k_edit_scatter; one wait at the end; the captured loop is the one ls_long_edit
 * with the same arguments captures.  sag == NULL and text_features == NULL: ls_long_edit.  One without the other: LS_EINVAL, ahead of
 * any launch, as is everything ls_long_edit refuses.
 * Not built: what ls_long_edit does not build; the SAG encoder as the source of text_features. */
int ls_long_edit_sag(ls_handle* h, const ls_long_edit_args* a, struct ls_sag* sag, const float* text_features);

/* ---- The COMPACT timeline edit: only the clip-windows an edit touches run, and clips of different lengths are edited in one call.
 * ls_long_edit runs every clip in every window that runs and needs all W * B clip-windows of audio encoded; here the unit is the PAIR
 * (clip b, window w).  The pair is in the plan iff clip b has an editable element in window w by ls_long_edit's rule (frame_lo[b] <=
 * w S + f < frame_hi[b] on a frame that w OWNS, and at least one channel of the clip selected) and, with `frames`, w < W_b = (frames[b]
 * - T) / S + 1.  Window w runs iff some pair names it; its ROWS are the clips of its pairs in ascending clip order; the windows run
 * in ascending order.  ls_long_edit_plan_compact is that plan (no handle, no GPU): windows [n_run] and counts [n_run] (the windows
 * that run and their row counts |A_w|), rows [n_pairs] (the row tables, window after window), *n_windows_run, *n_pairs = sum |A_w|.
 * A call with windows == counts == NULL (window_capacity 0) and rows == NULL (row_capacity 0) returns the two counts alone.
 * channels: bytes [batch, n_channels], or NULL = every channel.  frames: [batch] or NULL (every clip has all n_windows windows).
 * LS_EINVAL: a range outside [0, T + (W - 1) S] -- outside [0, frames[b]] with frames --, lo > hi, a frames[b] that is not T + k S
 * with 0 <= k < n_windows, a capacity that does not hold the plan.  A plan without a pair is no error here (the entries below refuse
 * it).  Property: without frames the windows that run are ls_long_edit_plan's for the same ranges.
 *
 * ls_long_prepare_edit is the once-per-call stage, everything in the CALLER's clip order (no slots, no reordering).  c as for
 * ls_long_prepare (c->emo [W, B]); audio_lengths (HOST [B], each in [1, c->audio_samples]) or NULL = every clip holds c->audio_samples
 * samples.  With audio_lengths, c->n_windows must be the longest clip's window count and frames[b] = T + (W_b - 1) S follows from
 * audio_lengths[b] as in ls_long_prepare_ragged.  Seed poses, speaker ids, guidance scales and emotion tokens are held per clip at
 * batch B; the WavEncoder runs over the n_pairs clip-windows of the plan alone, gathered from the caller's waveform through a (clip,
 * window) table in chunks of c->encoder_chunk (nothing at or beyond a clip's length is read: it counts as zero), its features packed in
 * plan order.  Every window batch is planned and its workspaces sized here.  An empty plan: LS_EINVAL.
 *
 * ls_long_edit_compact runs the planned windows.  Window w is ONE sampling call at batch |A_w| on its rows, decision for decision:
 * its own step plan, its own single-pass decision (the scales of its rows), the speaker style computed at that batch from its rows'
 * speaker ids (three small launches; it is not gathered from a batch-B result, because the projection's kernel is chosen by shape
 * and the contract is the call at batch |A_w|, bit for bit), the inpainting planes cut from the timeline by the row-table forms of
 * k_edit_gather / k_edit_start / k_edit_scatter.  Arguments:
 *   - frame_lo / frame_hi / channels must repeat what ls_long_prepare_edit was given (LS_EINVAL otherwise);
 *   - TAPE: the tapes are packed window after window at batch |A_w| -- x_init [n_pairs, J, F, T], then per window eps [n_exec, 2,
 *     |A_w|, latent_dim], noise and (inpaint_noised) inpaint_noise [n_exec, |A_w|, J, F, T], each concatenated over the windows that
 *     run: the packing ls_long_prepare_ragged documents;
 *   - PHILOX: row r of window w draws EVERY stream at global index sample_offset + rows_w[r] + (w << 48) -- the clip's index, not the
 *     row's -- so a clip draws what ls_long_edit and ls_long_sample draw for it, whichever other clips run beside it.  The draws come
 *     from a key table through device tapes (ls_philox_rows.hip), the inpainting branch's re-noise stream included;
 *   - windows (nullable): [n_pairs, J, F, T] the raw samples, row after row in plan order;
 *   - windows_run / n_windows_run as in ls_long_edit; *rows_run = n_pairs;
 *   - sag with text_features [W, B, latent_dim] (clip order): the scripted edit of ls_long_edit_sag; rows of pairs outside the plan
 *     are not used.  One without the other: LS_EINVAL.
 *   - ls_timing: n_segments = We (windows that ran), n_step_launches = We * n_exec, graph_replayed = the windows served by a replay.
 * GRAPH CACHE: one captured loop per (batch size, single-pass form) is kept and replayed by every window and every later call with
 * that key (the cache holds a few; a key that does not fit runs as stream launches, which give the same bits).  Room is made before
 * the first window, while nothing is in flight, and no graph is destroyed under a replay.  Every buffer a captured loop holds by
 * address is sized for the largest window batch before the first capture, so an identical second call replays every window.
 * Refusals come ahead of any launch and leave the handle usable: a handle not prepared by ls_long_prepare_edit (LS_ESTATE; ls_long_edit
 * and ls_long_sample refuse such a handle in turn), other ranges or channels than the prepared ones (LS_EINVAL), samplers other than
 * DDPM / DDIM and noise other than TAPE / PHILOX (LS_EUNSUPPORTED).
 * Not built: PLMS, const_noise, dump_steps, device-resident lengths, resampling the windows behind the last edited one. */
typedef struct ls_long_edit_compact_args {
    int32_t sampler;            /* the fields of ls_long_edit_args, with the same meanings ...                        */
    int32_t noise_mode;
    int32_t skip_timesteps;
    int32_t on_device;
    int32_t use_graph;
    int32_t clip_denoised;
    int32_t two_pass_always;
    float eta;
    int32_t inpaint_noised;
    int32_t windows_capacity;
    const int32_t* frame_lo;    /* HOST [B]                                                                           */
    const int32_t* frame_hi;    /* HOST [B]                                                                           */
    const unsigned char* channels; /* HOST bytes [B, J*F] or NULL                                                     */
    float* timeline;            /* [B, J, F, T + (W - 1) S], edited in place                                          */
    float* windows;             /* [n_pairs, J, F, T] or NULL                                                         */
    int32_t* windows_run;       /* HOST, nullable                                                                     */
    int32_t* n_windows_run;     /* HOST, nullable: We                                                                 */
    const float* x_init;        /* TAPE, packed: [n_pairs, J, F, T]                                                   */
    const float* eps_tape;      /* per window [n_exec, 2, |A_w|, latent_dim], concatenated                            */
    const float* noise_tape;    /* per window [n_exec, |A_w|, J, F, T], concatenated                                  */
    const float* inpaint_noise; /* likewise, with inpaint_noised                                                      */
    uint64_t seed;
    uint64_t sample_offset;     /* PHILOX: clip b draws, in window w, at sample_offset + b + (w << 48)                */
    int32_t* rows_run;          /* ... and, HOST, nullable: n_pairs, the clip-windows that ran                        */
} ls_long_edit_compact_args;
int ls_long_edit_plan_compact(int32_t batch, int32_t n_windows, int32_t T, int32_t n_pre, const int32_t* lo, const int32_t* hi,
                              const unsigned char* channels, int32_t n_channels, const int32_t* frames, int32_t* windows,
                              int32_t* counts, int32_t window_capacity, int32_t* rows, int32_t row_capacity, int32_t* n_windows_run,
                              int32_t* n_pairs);
int ls_long_prepare_edit(ls_handle* h, const ls_long_cond* c, const int64_t* audio_lengths, const int32_t* frame_lo,
                         const int32_t* frame_hi, const unsigned char* channels);
int ls_long_edit_compact(ls_handle* h, const ls_long_edit_compact_args* a, struct ls_sag* sag, const float* text_features);

/* ---- Timeline edits by ELEMENT MASK: "editable" as data instead of as a rectangle.  element_mask is bytes [B, J*F, N] in the
 * timeline's own layout (N = T + (W - 1) S), NON-ZERO = EDITABLE (the opposite of ls_sample's inpaint_mask, which marks what is kept).
 * Element (b, c, f) of window w is editable iff element_mask[b, c, w S + f] != 0 and frame w S + f is OWNED by w ([0, T) for w = 0,
 * [w S + n_pre_seq, w S + T) otherwise: ls_long_edit's ownership, unchanged); with frames (a ragged batch) additionally w < W_b, and a
 * set byte at or beyond frames[b] is LS_EINVAL, not a silent no-op.  Several stretches per clip, pinned keyframes inside a stretch,
 * other joints in other stretches and single features are all masks.  The range form is the mask channels[b][c] && lo_b <= n < hi_b:
 * for such a mask every output of every entry below equals the range entry's bit for bit.
 *
 * The entries are the range entries' own code with the rule swapped: the same window body, the same three kernels (k_edit_gather /
 * k_edit_start / k_edit_scatter read the mask when EditArgs::emask is set), the same captured loop, graph cache, tapes, PHILOX keys,
 * outputs and refusals.  A kept element of the timeline is never written, nor is a kept element of a scripted edit's start plane.
 *   - ls_long_edit_plan_mask (no handle, no GPU): ls_long_edit_plan_compact for a HOST mask [batch, n_channels, N]; the pair (b, w) is
 *     in the plan iff the clip has a set byte on a frame w owns.  Every plan, range or mask, is made from such PAIR FLAGS [W][B] by one
 *     definition.  LS_EINVAL: a set byte at or beyond frames[b], a frames[b] that is no stitched length, a capacity that does not
 *     hold the plan.  An empty plan is no error here; the run entries refuse it.
 *   - ls_long_edit_mask: ls_long_edit / ls_long_edit_sag (sag and text_features both NULL or both set).  The dense form: window w runs
 *     iff SOME clip has an editable element in it.
 *   - ls_long_prepare_edit_mask / ls_long_edit_compact_mask: ls_long_prepare_edit / ls_long_edit_compact.  The run must be given the
 *     mask the prepare was given: its pair flags are made again and compared (LS_EINVAL where they differ -- the plan, which is all the
 *     prepare derived from the mask, would be another one).  A handle prepared by ls_long_prepare_edit is refused here and vice versa.
 *   - in all of them a->frame_lo, a->frame_hi and a->channels must be NULL (LS_EINVAL otherwise), and element_mask is a DEVICE
 *     pointer iff on_device (a->on_device; c->on_device for the prepare).  A host mask is reduced to flags by a host loop and uploaded
 *     once per call.  A device mask stays on the device: k_edit_mask_pairs (ls_chain.hip; one workgroup per clip-window) reduces it
 *     and only W * B flag bytes cross to the host -- the one host wait a device mask adds ahead of the call's own.
 *   - ls_long_edit_mask_pairs: those flags [n_windows, batch] to the HOST as the kernel computes them (a host mask is uploaded first),
 *     geometry from the handle (after ls_commit_weights).  A set byte beyond frames[b]: flag 2 and LS_EINVAL.
 * Not built: masks on a running stream or pool, bit-packed masks, soft (fractional) masks. */
int ls_long_edit_plan_mask(int32_t batch, int32_t n_windows, int32_t T, int32_t n_pre, const unsigned char* element_mask, int32_t n_channels,
                           const int32_t* frames, int32_t* windows, int32_t* counts, int32_t window_capacity, int32_t* rows,
                           int32_t row_capacity, int32_t* n_windows_run, int32_t* n_pairs);
int ls_long_edit_mask(ls_handle* h, const ls_long_edit_args* a, struct ls_sag* sag, const float* text_features, const unsigned char* element_mask);
int ls_long_prepare_edit_mask(ls_handle* h, const ls_long_cond* c, const int64_t* audio_lengths, const unsigned char* element_mask);
int ls_long_edit_compact_mask(ls_handle* h, const ls_long_edit_compact_args* a, struct ls_sag* sag, const float* text_features,
                              const unsigned char* element_mask);
int ls_long_edit_mask_pairs(ls_handle* h, const unsigned char* element_mask, int32_t on_device, int32_t batch, int32_t n_windows,
                            const int32_t* frames, unsigned char* flags);

/* ---- Streaming long-form synthesis: the chain of ls_long_sample, fed audio in chunks of any size.  Window w runs as soon as its last
 * sample has arrived (audio_stride * w + audio_len <= samples fed), conditioned on the last n_pre_seq poses of window w - 1 (window 0:
 * seed_poses), and leaves T frames (window 0) or T - n_pre_seq frames in the output of the push that ran it.  The frames of all pushes,
 * concatenated along the frame axis, are bit for bit the timeline ls_long_prepare + ls_long_sample give for the concatenated audio
 * (without n_windows: the windows that cover it), whatever the chunking.
 *
 * ls_long_stream_plan (no handle, no GPU) is the one definition of the windows a call runs: with samples_before samples fed so far and
 * samples_new more, windows [*first_window, *first_window + *n_windows) run; closing != 0 adds the windows that cover the total with
 * silence behind its last sample (W = max(1, ceil((total - audio_len) / audio_stride) + 1) in all; the total must be >= 1).
 *
 * ls_long_stream_open opens a session of B slots (the session pool further down, at capacity B) and joins every slot from the arrays of
 * ls_long_stream_cond; a stream is that pool with all slots fed, given and closed alike, planned for batch B alone under the form its
 * own guidance scales choose.  It REPLACES the handle's prepared conditioning, as ls_prepare does; in turn any call that replaces it
 * (ls_prepare*, ls_long_prepare*, ls_commit_weights, ls_long_pool_open, a second ls_long_stream_open) ends the stream: the next
 * ls_long_stream_push returns LS_ESTATE and the handle stays usable.  A stream opened again at a batch whose buffers are in place
 * replays the loop the last one captured from its first window on.
 *
 * Device memory does not grow with the stream: per clip a ring of audio_len + audio_stride samples, the hand-off poses and the held
 * conditioning; one gathered window [B, audio_len], one window's audio features [B, T, 256].
 * A chunk larger than the ring's free space is consumed in pieces with the completed windows run in between.  One host wait per call
 * that ran a window; a call that ran none waits only for the copy of a HOST chunk (or of emo / text_features) out of the caller's
 * buffer (a device chunk must stay valid until the handle's stream has read it: order its reuse with ls_stream_order).  A row of
 * `frames` is zero behind the frames the call wrote.
 * PHILOX keys window w at w << 48 and the key must not repeat: a push that would run window 2^16 returns LS_ESTATE (about 36 hours of
 * audio; open a new stream).
 * Clips that join and leave, each with its own lengths: the session pool further down (ls_long_pool_*).
 * Not built: edits of frames a running stream has already returned (frames still to come can be pinned: ls_long_pool_pins further
 * down serves a stream too), PLMS, const_noise, dump_steps, a non-blocking push. */
typedef struct ls_long_stream_cond {
    int32_t batch;
    int32_t on_device;
    const float* seed_poses;    /* [B, J, F, n_pre_seq]: origin_x[..., :n_pre_seq] of window 0                        */
    const int64_t* vid_indices; /* [B]                                                                                */
    const float* scale;         /* [B]                                                                                */
} ls_long_stream_cond;
typedef struct ls_long_stream_push_args {
    int32_t sampler;            /* LS_SAMPLER_DDPM | LS_SAMPLER_DDIM; these eight fields as in ls_long_sample_args    */
    int32_t noise_mode;         /* LS_NOISE_TAPE | LS_NOISE_PHILOX                                                    */
    int32_t skip_timesteps;
    int32_t on_device;          /* audio, emo, text_features, the tapes and frames are device pointers                */
    int32_t use_graph;
    int32_t clip_denoised;
    int32_t two_pass_always;
    float eta;
    int32_t closing;            /* the stream's last call: run the windows still owed, zero-padded; later pushes are refused */
    int32_t capacity;           /* frames per row of `frames`; at least what the windows of this call produce         */
    int64_t n_samples;          /* n >= 0: samples per clip in `audio`                                                */
    const float* audio;         /* [B, n] (NULL with n == 0)                                                          */
    const int64_t* emo;         /* [B] emotion ids held from this call on (BEAT), or NULL: the ids held so far        */
    struct ls_sag* sag;         /* LivelySpeaker chain, as in ls_long_sample_args; NULL: none                         */
    const float* text_features; /* with sag: [B, latent_dim] held from this call on, or NULL: the features held so far */
    const float* x_init;        /* TAPE: [k, B, J, F, T] x_T of the k windows this call runs (ls_long_stream_plan)    */
    const float* eps_tape;      /* TAPE: [k, n_exec, 2, B, latent_dim]                                                */
    const float* noise_tape;    /* TAPE: [k, n_exec, B, J, F, T]                                                      */
    uint64_t seed;              /* PHILOX: the same key in every call of a stream                                     */
    uint64_t sample_offset;     /* PHILOX: window w < 2^16 draws at sample_offset + b + (w << 48), as in ls_long_sample */
    float* frames;              /* [B, J, F, capacity]: the new frames of this call's windows, in order (NULL with capacity 0) */
    int32_t* n_frames;          /* HOST, nullable: frames written per row                                             */
    int32_t* n_windows;         /* HOST, nullable: windows run                                                        */
} ls_long_stream_push_args;
int ls_long_stream_plan(int64_t samples_before, int64_t samples_new, int32_t audio_len, int32_t closing, int64_t* first_window,
                        int64_t* n_windows);
int ls_long_stream_open(ls_handle* h, const ls_long_stream_cond* c);
int ls_long_stream_push(ls_handle* h, const ls_long_stream_push_args* a);
/* out = {samples fed, windows run, frames written, device bytes the stream holds} of the handle's current or last stream (zeros before
 * the first ls_long_stream_open, and once a pool has been opened since).  The bytes are the session's count, as ls_long_pool_info's
 * misc[1] at capacity B: rings, hand-off stores, held conditioning (speaker ids, scales, emotion ids and tokens, text features and
 * their compact rows), the round table, the gathered windows and one window's features, as allocated */
int ls_long_stream_info(const ls_handle* h, int64_t out[4]);

/* ---- Session pool: streaming long-form synthesis with clips that join and leave.  A pool holds `capacity` SLOTS; each open slot is
 * one stream of its own (its audio ring, its hand-off poses, its held conditioning, its sample and window counters), fed at its own
 * rate.  A push takes a ragged chunk -- lengths[s] samples for slot s -- and runs, ROUND after round, the windows that are complete:
 * round r holds, in ascending slot order, the slots that still have a complete, unrun window after r earlier rounds of this call, and
 * is ONE sampling call at batch A = its size on those slots (its own step plan, its own single-pass decision from the scales of those
 * slots, its own captured loop, kept in the graph cache by batch).  Per slot the windows, their audio, their hand-off and their
 * stitching are those of ls_long_stream_push on that slot alone.
 *
 * ls_long_pool_plan (no handle, no GPU) is the one definition of what a call runs.  Per slot it is ls_long_stream_plan(samples_in[s],
 * samples_new[s], audio_len, closing[s]); n_windows[s] is that call's count, frames[s] the frames slot s gets (34 for its window 0,
 * 30 for each later one), *n_rounds = max n_windows[s], and round_slots (nullable; round_capacity entries) takes the slots of round 0,
 * then of round 1, ...: *n_entries = sum of n_windows in all.  LS_EINVAL: a null array, a negative count, windows_run[s] that is not
 * the number of windows complete on samples_in[s], samples for a slot that is not open, a closing slot that was fed no sample at all,
 * round_slots too short.  The closing flag of a slot that is not open is ignored.
 *
 * ls_long_pool_open allocates everything for `capacity` slots -- rings, hand-off stores, held conditioning, one gathered window, one
 * window's features, the loop's buffers and the workspaces of the step plans of every batch 1..capacity -- so that no buffer a
 * captured loop holds by address moves before the pool ends.  It REPLACES the handle's prepared conditioning and ends a running
 * stream (the two are one kind of session, and a handle holds one); any call that replaces the conditioning ends the pool in turn (the next push or join returns LS_ESTATE, the handle stays
 * usable).  ls_long_pool_join fills a free slot (LS_ESTATE on an occupied one) and draws nothing; a slot whose closing flag is set
 * in a push is free again after the windows it was owed.  A failure inside a push marks the pool failed (LS_ESTATE from then on).
 *
 * Noise.  TAPE: the tapes are packed round after round, each round the draws of one sampling call at batch A (x_init [A, J, F, T],
 * eps_tape [n_exec, 2, A, latent_dim], noise_tape [n_exec, A, J, F, T]).  PHILOX: row r of the pool's q-th round since open draws at
 * sample_offset + r + (q << 48): the key of ls_long_stream_push whenever the pool is used like a stream (all slots joined in order and
 * fed alike), and otherwise NOT independent of the push schedule; a push that would take q to 2^16 returns LS_ESTATE.
 * PHILOX on a KEYED pool (ls_long_pool_keyed(h, 1) after the open, ahead of the first join): every slot holds a key in [0, 2^48) --
 * the number of joins since the open until ls_long_pool_set_key replaces it, after the slot's join and ahead of its first window
 * (LS_ESTATE later) -- and the clip in slot s draws in its OWN window w (windows_run[s], 0 again after a join) at key[s] + (w << 48)
 * under the pool's one seed; sample_offset is not read.  A clip's frames are then a function of the weights, the schedule, its own
 * audio and conditioning, the seed and its key: not of the other slots, the slot index, the chunking or the pool's age.  They are
 * what ls_long_sample gives for that audio at sample_offset = key -- bit for bit where both run the same kernel family at the same
 * batch, and otherwise as far apart as two kernel families are.  Two open slots may hold the same key (same audio and conditioning:
 * same frames); nothing polices it.  A clip runs at most 2^16 windows (LS_ESTATE beyond); the pool's round count is no limit.
 * ls_long_pool_keys (no handle, no GPU) is the one definition of a round's key table, in ls_long_pool_plan's row order: the row of
 * slot s in round r draws at keys[s] + ((windows_run[s] + r) << 48); LS_EINVAL for a key >= 2^48, LS_ESTATE for a window >= 2^16 (of
 * slots with n_windows[s] > 0; the others are not looked at), row_keys nullable (row_capacity entries), *n_entries = sum of n_windows.
 * The draws of a keyed round are written by ls_philox_rows.hip into the ring LS_NOISE_TORCH_DEVICE uses (ls_set_torch_ring_bytes),
 * sized at ls_long_pool_keyed for every batch up to the capacity, from a key table the captured loop reads at a fixed address.
 * One host wait per call that ran a round; a call that ran none waits only for the copy of a HOST chunk.
 * Not built: device-resident lengths, ls_long_edit on frames a pool has already returned (frames still to come can be pinned:
 * ls_long_pool_pins below), PLMS, const_noise, dump_steps, sharded
 * calls, a non-blocking push. */
typedef struct ls_long_pool_join_args {
    int32_t slot;
    int32_t on_device;          /* the five pointers are device pointers                                              */
    const float* seed_poses;    /* [J, F, n_pre_seq]: origin_x[..., :n_pre_seq] of the slot's window 0                */
    const int64_t* vid_index;   /* [1]                                                                                */
    const float* scale;         /* [1]; a device scale costs one read-back                                            */
    const int64_t* emo;         /* [1] emotion id held from the join on (BEAT: required), or NULL                     */
    const float* text_features; /* [latent_dim] held from the join on, or NULL                                        */
} ls_long_pool_join_args;
typedef struct ls_long_pool_push_args {
    int32_t sampler;            /* these eight fields as in ls_long_sample_args                                       */
    int32_t noise_mode;
    int32_t skip_timesteps;
    int32_t on_device;          /* audio, emo, text_features, the tapes and frames are device pointers                */
    int32_t use_graph;
    int32_t clip_denoised;
    int32_t two_pass_always;
    float eta;
    int32_t capacity;           /* frames per row of `frames`; at least the most any slot gets in this call           */
    int32_t reserved;
    int64_t n_max;              /* row stride of `audio` in samples, >= every lengths[s]                              */
    const float* audio;         /* [S, n_max] (NULL with n_max == 0); row s holds lengths[s] samples for slot s       */
    const int64_t* lengths;     /* HOST [S], each in [0, n_max]; 0 for a slot that is not open                        */
    const int32_t* closing;     /* HOST [S], nullable: slot s leaves after the windows it is still owed, zero-padded  */
    const int32_t* given;       /* HOST [S], nullable: bit 0: emo[s] replaces the held id, bit 1: text_features[s]    */
    const int64_t* emo;         /* [S] (read where given), nullable                                                   */
    struct ls_sag* sag;         /* LivelySpeaker chain, as in ls_long_sample_args; NULL: none                         */
    const float* text_features; /* with sag: [S, latent_dim] (read where given), nullable                             */
    const float* x_init;        /* TAPE: packed round after round, see above                                          */
    const float* eps_tape;
    const float* noise_tape;
    uint64_t seed;              /* PHILOX: the same key in every call of a pool                                       */
    uint64_t sample_offset;
    float* frames;              /* [S, J, F, capacity]: slot s's new frames from column 0 on, zero behind them (NULL with capacity 0) */
    int32_t* n_frames;          /* HOST [S], nullable: frames written per slot                                        */
    int32_t* n_rounds;          /* HOST, nullable: rounds run                                                         */
} ls_long_pool_push_args;
int ls_long_pool_plan(int32_t n_slots, int32_t audio_len, const int64_t* samples_in, const int64_t* windows_run, const int64_t* samples_new,
                      const int32_t* closing, const int32_t* open, int32_t* n_windows, int32_t* frames, int32_t* round_slots,
                      int32_t round_capacity, int32_t* n_rounds, int32_t* n_entries);
int ls_long_pool_open(ls_handle* h, int32_t capacity);
int ls_long_pool_join(ls_handle* h, const ls_long_pool_join_args* a);
int ls_long_pool_push(ls_handle* h, const ls_long_pool_push_args* a);
int ls_long_pool_keyed(ls_handle* h, int32_t on);
int ls_long_pool_set_key(ls_handle* h, int32_t slot, uint64_t key);
int ls_long_pool_keys(int32_t n_slots, const uint64_t* keys, const int64_t* windows_run, const int32_t* n_windows, uint64_t* row_keys,
                      int32_t row_capacity, int32_t* n_entries);
/* per slot (arrays of `capacity` entries, each nullable): samples fed, windows run, frames written, open; misc = {slots of the pool,
 * device bytes the pool holds (rings, hand-off stores, held conditioning, gathered window, one window's features), rounds run since
 * open, 1 while the pool is open} of the handle's current or last pool (a pool that has ended: as it stood then) -- zeros before the
 * first ls_long_pool_open */
int ls_long_pool_info(const ls_handle* h, int32_t capacity, int64_t* samples_in, int64_t* windows_run, int64_t* frames_out, int32_t* open,
                      int64_t misc[4]);
/* ---- Pinned poses for frames a session has yet to make: "be in this pose at frame 412".  Slot s has a series of frames n = 0, 1, ...
 * (the numbering of frames_out).  Window w covers series frames 30 w .. 30 w + 33 and OWNS all 34 of them for w = 0 and the frames
 * 30 w + 4 .. otherwise (the ownership of a timeline edit).  A PIN is a target value for one element (c, n) of a frame the slot has
 * not returned yet.  When the window that owns n runs, it runs through the inpainting branch of p_mean_variance
 * (gaussian_diffusion.py:314-320; the TED tree re-noises the kept motion, the BEAT tree does not: n_prefix_tokens decides, as in
 * edit_long) with inpainting_mask = true exactly on the pinned elements of the frames the window owns -- the prefix frames of a
 * window w > 0 are never kept, the window before owned them -- and inpainted_motion = the pinned values there, zero elsewhere.  A
 * window whose owned frames carry no pin runs exactly as without pins.
 *
 * A push still runs ls_long_pool_plan's rounds; each round is split into at most two sampling CALLS: first its unpinned rows, in
 * ascending slot order, as a plain call, then its pinned rows, in ascending slot order, as an inpainting call; an empty half is
 * skipped.  So a clip without a pin never enters the inpainting kernels because a neighbour has one, and a session with no pending
 * pin makes precisely the calls it makes without pins.  ls_long_pool_pin_plan (no handle, no GPU) is the one definition: from
 * windows_run [S], n_windows [S] (ls_long_pool_plan's) and the pending pinned frames of each slot (CSR: slot s holds pin_frames
 * [pin_first[s], pin_first[s + 1]), in any order; both null: no pins) it gives the calls in order -- call_counts / call_pinned /
 * call_rounds [call_capacity] (rows, 1 = inpainting call, the round it belongs to; each nullable) and the slots of call 0, then of
 * call 1, ... in call_rows [row_capacity] (nullable) -- *n_calls and *n_entries = sum of n_windows.  LS_EINVAL: a null count array,
 * a negative count or frame, a CSR that does not ascend from 0, an output array too short.
 * Every call is one public sampling call: the tapes of a TAPE push are packed CALL after call (each the draws of one sampling call
 * at its batch; the re-noise tape of the pinned calls, [n_exec, A, J, F, T] each, is handed over by ls_long_pool_pin_tape ahead of
 * the next push of the session -- the handle forgets the pointer when that push returns, run or refused -- and read by it alone), un-keyed PHILOX draws row r of the q-th call since the open at sample_offset + r + (q << 48)
 * with the re-noise on the inpainting stream (4), as ls_sample does, and a keyed pool keeps the clip's key and its own window, the
 * re-noise being the third tape of ls_philox_rows.hip.  misc[2] of ls_long_pool_info counts calls.
 *
 * ls_long_pool_pins(h, horizon) enables pins on an open pool ahead of its first join (on a stream: ahead of its first push) and is
 * where everything they need is allocated, for every batch 1..S, while nothing is in flight: the store -- per slot a ring of P =
 * horizon rounded up to a multiple of 4 frames, [S][P][J F] values and bytes, frame n at n % P -- the inpainting planes and the
 * denoiser's output plane -- and, where the schedule is set by then, the TED tree's re-noise tape buffer for its longest loop (the
 * number of executed steps is a push's argument: a push checks that buffer again ahead of its first launch, as it does for the
 * other tape buffers).  horizon >= nframes (LS_EINVAL otherwise).  A session that never calls it allocates nothing new.
 * ls_long_pool_pin(h, slot, n, frames, poses, mask, on_device): frames HOST [n], distinct, each in [frames_out[slot],
 * frames_out[slot] + horizon); poses [J, F, n]; mask [J, F, n] bytes, non-zero = pinned, NULL = the whole pose; on_device: poses
 * and mask are device pointers.  Elements the mask leaves out keep what an earlier call pinned.  LS_EINVAL / LS_ESTATE before
 * anything is uploaded: pins not enabled, a slot that is not open, n outside [1, horizon], a frame out of range or named twice.
 * ls_long_pool_unpin(h, slot, n, frames) drops the pins of those frames (same range; a frame that holds none is no error), frames
 * NULL with n == 0: of the whole slot.  ls_long_pool_join clears the slot's pins, and a slot that leaves drops the pins its clip
 * never reached.  ls_long_pool_pin_info: pending pinned frames per slot (nullable, `capacity` entries), misc = {horizon, P}; zeros
 * where the session has no pins.  With sag= a push that would run a pinned window returns LS_EUNSUPPORTED.
 * Not built: pins on frames already returned, pins with sag= (a pinned window would start from edit_start(motion, mask, sag_out)
 * at the pinned elements: a kernel form of its own), soft (fractional) pins, device-resident frame lists. */
int ls_long_pool_pin_plan(int32_t n_slots, int32_t T, int32_t n_pre, const int64_t* windows_run, const int32_t* n_windows,
                          const int32_t* pin_first, const int64_t* pin_frames, int32_t* call_rows, int32_t row_capacity,
                          int32_t* call_counts, int32_t* call_pinned, int32_t* call_rounds, int32_t call_capacity, int32_t* n_calls,
                          int32_t* n_entries);
int ls_long_pool_pins(ls_handle* h, int32_t horizon);
int ls_long_pool_pin(ls_handle* h, int32_t slot, int32_t n, const int64_t* frames, const float* poses, const unsigned char* mask,
                     int32_t on_device);
int ls_long_pool_unpin(ls_handle* h, int32_t slot, int32_t n, const int64_t* frames);
int ls_long_pool_pin_tape(ls_handle* h, const float* inpaint_noise, int64_t n_floats, int32_t on_device);
int ls_long_pool_pin_info(const ls_handle* h, int32_t capacity, int32_t* pending, int64_t misc[2]);
int ls_step(ls_handle* h, const ls_step_args* a);
int ls_plms_step(ls_handle* h, const ls_plms_step_args* a);
/* elementwise q_sample (gaussian_diffusion.py:240-258) at schedule index i; pointers per on_device */
int ls_q_sample(ls_handle* h, int index, int on_device, size_t n, const float* x_start,
                const float* noise, float* out);

/* ---- the variational bound in bits per dimension (calc_bpd_loop, gaussian_diffusion.py:1591-1646) -------------------------------
 * Under START_X + FIXED_SMALL the model's variance is the true posterior's, so a column of the bound needs x_0, x_t, the model's
 * pred_xstart and the q_sample noise only.  k_vb_terms (csrc/ls_bpd.hip) evaluates, per sample and in fp32 in the reference's
 * operation order (losses.py:33-39, :62-75),
 *   vb         = mean(normal_kl(q_posterior(x_0, x_t), p(x_t))) / ln 2 when t > 0, the discretized decoder NLL / ln 2 when t == 0
 *                (chosen per sample, as th.where(t == 0, ...) does, :1245),
 *   xstart_mse = mean((pred_xstart - x_0)^2)                                                                   (:1630),
 *   mse        = mean((_predict_eps_from_xstart(x_t, t, pred_xstart) - noise)^2)                               (:1631-1632),
 * with one deterministic fixed-tree reduction per sample (no atomics: a graph replay equals plain launches bit for bit).
 *
 * ls_vb_terms: that kernel alone on caller-given planes [B,J,F,T] (B = the prepared batch): the second half of _vb_terms_bpd.
 * Schedule index: `indices` [B] int64 (per sample; host values are validated, device values clamped into the table) or, when it is
 * NULL, the uniform `index`.  noise NULL: mse is not computed (mse_out is then ignored).  clip_denoised: pred_xstart is clamped to
 * [-1, 1] first (process_xstart); pred_out (nullable) receives the plane the terms were computed from.  Outputs [B]. */
typedef struct ls_vb_terms_args {
    int32_t index;
    int32_t on_device;
    int32_t indices_on_device;
    int32_t clip_denoised;
    const int64_t* indices;
    const float* x_start;
    const float* x_t;
    const float* pred_xstart;
    const float* noise;
    float* vb_out;
    float* xstart_mse_out;
    float* mse_out;
    float* pred_out;
} ls_vb_terms_args;
int ls_vb_terms(ls_handle* h, const ls_vb_terms_args* a);

/* ls_bpd: columns [col_begin, col_begin + col_count) of calc_bpd_loop on the schedule of ls_set_schedule; column k belongs to schedule
 * index n_steps - 1 - k.  Per column: q_sample(x_start, t, noise_k), one denoiser launch (sampler = none: whatever kernel family and
 * plan the prepared batch gets, as a PLMS evaluation) and k_vb_terms.  Columns do not depend on each other: a call over a sub-range
 * gives bitwise the columns of the whole call.
 * Noise: TAPE -- noise_tape [col_count,B,J,F,T] and eps_tape [col_count,2,B,latent_dim] hold THIS call's columns, in the reference's
 * draw order per column (randn_like(x_start), then the style eps of the cond and the uncond pass); PHILOX -- column k uses step_id = k
 * of the step-noise stream (3) and the style-eps streams (1, 2), keyed by sample_offset + b (shard-invariant); TORCH_DEVICE returns
 * LS_EUNSUPPORTED.  vb / xstart_mse / mse: [B, n_steps] row-major (host or device per on_device); only this call's columns are
 * written.  use_graph: the column loop is captured and replayed like ls_sample's.  ls_timing: n_step_launches = col_count. */
typedef struct ls_bpd_args {
    int32_t noise_mode;         /* LS_NOISE_TAPE | LS_NOISE_PHILOX                   */
    int32_t on_device;
    int32_t use_graph;
    int32_t clip_denoised;
    int32_t two_pass_always;    /* as in ls_sample_args                              */
    int32_t col_begin;
    int32_t col_count;
    int32_t reserved;
    const float* x_start;       /* [B,J,F,T]                                         */
    const float* noise_tape;
    const float* eps_tape;
    uint64_t seed;              /* PHILOX key                                        */
    uint64_t sample_offset;     /* PHILOX: global index of sample 0                  */
    float* vb;
    float* xstart_mse;
    float* mse;
} ls_bpd_args;
int ls_bpd(ls_handle* h, const ls_bpd_args* a);

/* The x_T draw of PHILOX mode on its own (what ls_sample uses when x_init == NULL): out [batch,J,F,T] ~ N(0,1),
 * stream keyed by (seed, sample_offset + b). Lets tests check the device RNG's moments and shard-invariance. */
int ls_philox_x_init(ls_handle* h, int batch, uint64_t seed, uint64_t sample_offset, int on_device, float* out);
/* Per-row Philox keys of ls_sample: row b of the next PHILOX calls at batch n draws every stream (x_T, the two style eps per step, the
 * step noise) at gidx = keys[b] -- the whole 64-bit value ls_philox.h puts into c[2], c[3] -- in place of sample_offset + b, so any
 * subset of a larger call's rows, in any order, can be drawn again.  keys: HOST [n], copied before the call returns.  They hold
 * until (NULL, 0) clears them or ls_prepare runs at another batch.  With keys set ls_sample returns LS_EINVAL for a batch other
 * than n, a noise mode other than PHILOX or a nonzero sample_offset, and LS_EUNSUPPORTED for PLMS and the inpainting branch (ls_bpd
 * under PHILOX: LS_EUNSUPPORTED); the long-form entries do not read them.  The draws are written by ls_philox_rows.hip into the
 * ring LS_NOISE_TORCH_DEVICE uses (ls_set_torch_ring_bytes) with ls_philox.h's own arithmetic: keys[b] = o + b gives the bits of
 * sample_offset = o. */
int ls_set_row_keys(ls_handle* h, const uint64_t* keys, int32_t n);

/* ---- torch's device normal stream (LS_NOISE_TORCH_DEVICE) -----------------------------------------------------------------
 * ls_torch_randn_advance: how far torch.randn(n) (float32) on a device of n_cu compute units and max_threads_per_cu threads per CU
 * (hipDeviceProp multiProcessorCount / maxThreadsPerMultiProcessor) moves the device generator's offset: 4 * ceil(n / (4 * 256 * G)),
 * G = min(ceil(n / 256), n_cu * (max_threads_per_cu / 256)); 0 for n <= 0 or a geometry torch cannot launch.  Host arithmetic only.
 * ls_torch_randn: fill DEVICE memory out_device[n] with what torch.randn(n) draws from a generator at (seed, offset) on the handle's
 * GPU (n < 2^31, offset a multiple of 4); the caller moves the generator on by ls_torch_randn_advance.  no_sync: do not wait for it.
 * ls_set_torch_ring_bytes: device memory a TORCH_DEVICE loop keeps its draws in (default 256 MB): the ring holds as many steps as fit
 * (at least one) and is refilled by one generator launch per that many steps. */
uint64_t ls_torch_randn_advance(int64_t n, int32_t n_cu, int32_t max_threads_per_cu);
int ls_torch_randn(ls_handle* h, uint64_t seed, uint64_t offset, int64_t n, float* out_device, int no_sync);
int ls_set_torch_ring_bytes(ls_handle* h, uint64_t bytes);

/* Read back a prepared intermediate into host memory (parity tests of the once-per-call stages):
 * "audio_feat" [B,T,256], "static_c"/"static_u" [B,T,D], "z_mu"/"z_logvar"/"z_std" [B,D],
 * "temb" [n_steps,D].  Returns the element count, or a negative error. */
long long ls_read(ls_handle* h, const char* name, float* host_out, size_t capacity);

/* Multi-GPU sharding of one batch (the reference's dist_util.py:18-41 is a stub): the path has no
 * per-step exchange, so a C-ABI integrator shards by (1) splitting the batch contiguously with ls_shard_range, (2) giving every
 * rank's handle the same weights (broadcast them with whatever communicator the host application has -- RCCL ncclBroadcast of
 * the arrays passed to ls_set_weight), (3) passing ls_sample_args.sample_offset = first so the PHILOX streams follow the global
 * sample index (results do not depend on the GPU count), (4) gathering the [count, J, F, T] outputs.  livelyspeaker_amd/shard.py
 * is that recipe over torch.distributed.  Rank r of `world` owns samples [first, first + count). */
int ls_shard_range(int64_t total, int32_t world, int32_t rank, int64_t* first, int64_t* count);
int ls_get_timing(const ls_handle* h, ls_timing* out);
int ls_synchronize(ls_handle* h);

/* Stream ordering instead of host synchronisation.  Every handle runs on its own non-blocking HIP stream, which nothing orders
 * against the caller's streams.  ls_stream_order(device, first, then): work enqueued on `then` AFTER this call waits for the work
 * enqueued on `first` BEFORE it (an event recorded on `first`, hipStreamWaitEvent on `then`); both are hipStream_t values
 * (NULL = the device's default stream).  A caller whose inputs were produced on its own stream orders (its stream, handle stream)
 * before an entry point instead of synchronising the host, and (handle stream, its stream) after a no_sync call before it
 * consumes device outputs.  The accessors return each handle's stream. */
int ls_stream_order(int device, void* first, void* then);
void* ls_stream(const ls_handle* h);

/* ---- torch's CPU normal stream, natively ("identical seeds" mode off the Python critical path) ----------------------------------
 * The reference draws every normal of a sampling loop from torch's global CPU generator (gaussian_diffusion.py:700-743; RAG.py:10-13,
 * 120), so torch.manual_seed(s) fixes the sample.  These two entry points make the same draws from the same state: `state` is the
 * 5056-byte blob of torch.get_rng_state() (mt19937 words + the cached Box-Muller sample), updated in place -- hand it back with
 * torch.set_rng_state().  Host memory only; no GPU involved.  n_threads workers share the transcendental part.
 * ls_trng_randn: torch.randn(n), float32 contiguous (n >= 16: the 16-block float Box-Muller; n < 16: the per-element double path).
 * ls_trng_fill_steps: the per-step draws of n_steps sampling steps in the reference's order -- randn(B,1,D) of the cond pass, of the
 * uncond pass, then randn_like(x) -- into eps [n_steps][2][B][D] and noise [n_steps][B][J][F][T]; x is the model-output-shaped view
 * (memory order [T][B][J][F], consumed in that order by torch's per-element path) except at the first step when first_contiguous.
 * variant: the float transform of the contiguous draws -- 0 = libm (torch's DEFAULT-capability kernel), 1..4 = the Cephes polynomials
 * of torch's AVX2 / AVX512 kernels under the four ways their multiply-adds can have been contracted to FMAs; livelyspeaker_amd finds
 * the variant that reproduces torch bit for bit once per process and keeps torch's generator if none does. */
int ls_trng_randn(uint8_t* state, size_t state_bytes, float* out, size_t n, int variant, int n_threads);
int ls_trng_fill_steps(uint8_t* state, size_t state_bytes, int B, int D, int J, int F, int T, int n_steps, int first_contiguous,
                       float* eps, float* noise, int variant, int n_threads);
/* The per-element double pairs whose samples are stored as floats are evaluated by a vectorised restatement and taken from it only when
 * every double within its error margin rounds to the same float; the others go through libm as in torch (ls_torch_rng.cpp).
 * ls_trng_stats: pairs evaluated / pairs sent back to libm so far in this process.  ls_trng_pairs_debug (tests): the vectorised
 * evaluation alone over np pairs (4 np words) next to libm's doubles; isa 0 / 1 / 2 = base / AVX2 / AVX-512 clone, -1 = this machine's. */
int ls_trng_stats(uint64_t* pairs, uint64_t* redone);
/* Long fills of the native stream start their generator threads from JUMPED mt19937 states (csrc/ls_mt_jump.h: t^J modulo the
 * characteristic polynomial, applied as an XOR of ~10 k windows of a 33-block expansion of the state) instead of behind one thread that
 * walks the whole stream.  ls_trng_set_jump(0) restores the sequential scout (returns the previous setting); ls_trng_jump_check compares
 * the two ways of reaching the state `words` (a multiple of 624) further on: 0 = identical. */
int ls_trng_set_jump(int on);
int ls_trng_jump_check(uint32_t seed, uint64_t words, int* support);
int ls_trng_pairs_debug(const uint32_t* words, int np, int isa, double* fast_c, double* fast_s, float* zc, float* zs, uint8_t* redo,
                        double* libm_c, double* libm_s);

/* ---- SAG decoder ---------------------------------------------------------------
 * Decoder_TRANSFORMER (scripts/model/motionclip_module.py:98-183), called as SAG.decoder(batch) at
 * scripts/test_LivelySpeaker_ted.py:88 to produce init_image for the RAG refine loop.  Separate handle: it is a
 * different network with its own checkpoint (SAG.pth, keys 'decoder.*' with the prefix stripped). */
typedef struct ls_sag ls_sag;
typedef struct ls_sag_config {
    int32_t njoints, nfeats, nframes;   /* 9, 3, 34                                   */
    int32_t latent_dim, ff_size;        /* 512, 1024                                  */
    int32_t num_layers, num_heads;      /* 3, 4                                       */
    int32_t n_pre_poses;                /* 4                                          */
    int32_t device;
    int32_t reserved;
} ls_sag_config;
int ls_sag_create(const ls_sag_config* cfg, ls_sag** out);
void ls_sag_destroy(ls_sag* h);
const char* ls_sag_last_error(const ls_sag* h);
int ls_sag_set_weight(ls_sag* h, const char* key, const float* data, size_t n);
int ls_sag_commit_weights(ls_sag* h);
/* batch['x'] [B,J,F,T], batch['z'] [B,latent] (CLIP text feature), batch['mask'] [B,T] bytes or NULL (all true)
 * -> batch['output'] [B,J,F,T] */
int ls_sag_decode(ls_sag* h, int batch, int on_device, const float* x, const float* z, const unsigned char* mask,
                  float* out);
/* The same, enqueued only (device pointers): returns without waiting for the GPU; `out` is complete once ls_sag_stream() has reached
 * this point (order consumers with ls_stream_order).  Lets a caller that iterates batches decode batch n + 1 while batch n is refined. */
int ls_sag_decode_async(ls_sag* h, int batch, const float* x, const float* z, const unsigned char* mask, float* out);
float ls_sag_last_decode_ms(const ls_sag* h);   /* GPU time of the last decode (HIP events on the handle's stream); waits for an asynchronous one */
void* ls_sag_stream(const ls_sag* h);

/* ---- SAG encoder -----------------------------------------------------------------------------------------
 * Encoder_TRANSFORMER (scripts/model/motionclip_module.py:33-95, eval mode), the other half of MOTIONCLIP
 * (scripts/model/motionclip.py:75-83): a motion clip -> the CLIP-aligned latent mu = z that the decoder consumes.
 * Separate handle, configured by the decoder's config struct; its n_pre_poses field is ignored.  Weight keys are the module's own
 * (muQuery, sigmaQuery, skelEmbedding.*, seqTransEncoder.layers.N.*; in SAG.pth they carry the prefix 'encoder.'); '*.pe' is ignored.
 * A missing or mis-sized key fails in the commit call with the key named. */
typedef struct ls_sag_enc ls_sag_enc;
int ls_sag_enc_create(const ls_sag_config* cfg, ls_sag_enc** out);
void ls_sag_enc_destroy(ls_sag_enc* h);
const char* ls_sag_enc_last_error(const ls_sag_enc* h);
int ls_sag_enc_set_weight(ls_sag_enc* h, const char* key, const float* data, size_t n);
int ls_sag_enc_commit_weights(ls_sag_enc* h);
/* batch['x'] [B,J,F,T], batch['mask'] [B,T] bytes (0 = padded frame: never attended to) or NULL (all true) -> mu [B,latent] */
int ls_sag_enc_encode(ls_sag_enc* h, int batch, int on_device, const float* x, const unsigned char* mask, float* mu_out);
/* The same, enqueued only (device pointers): `mu_out` is complete once ls_sag_enc_stream() has reached this point; a decoder handle
 * consumes it without a host round trip after ls_stream_order(device, ls_sag_enc_stream(enc), ls_sag_stream(dec)). */
int ls_sag_enc_encode_async(ls_sag_enc* h, int batch, const float* x, const unsigned char* mask, float* mu_out);
float ls_sag_enc_last_encode_ms(const ls_sag_enc* h);   /* GPU time of the last encode; waits for an asynchronous one */
void* ls_sag_enc_stream(const ls_sag_enc* h);

/* ---- CLIP text encoder -----------------------------------------------------------------------------------
 * clip_model.encode_text(text).float() of scripts/test_LivelySpeaker_ted.py:85-86 and scripts/model/motionclip.py:52-53: the text
 * tower of CLIP ViT-B/32 in fp32 -- token + positional embedding, `layers` pre-norm blocks (causal nn.MultiheadAttention, MLP with
 * QuickGELU), ln_final, the row at text.argmax(-1) times text_projection.  Tokens are what clip.tokenize returns: [B, context_length]
 * int64.  Weight keys are CLIP's own state-dict names (token_embedding.weight, positional_embedding, transformer.resblocks.N.*,
 * ln_final.*, text_projection); a missing or mis-sized key fails in the commit call with the key named.
 * Supported: width = embed_dim = 512, heads = 8, context_length 1..77, layers 1..24, vocab_size >= 1; anything else is
 * LS_EUNSUPPORTED, decided before the device is touched.
 * prune != 0: only rows 0 .. eot of every sample are computed, packed back to back (the mask is causal and only the EOT row is read
 * out, so this is exact); prune = 0 computes all context_length rows of every sample.  Both give the same bits. */
typedef struct ls_clip_text ls_clip_text;
typedef struct ls_clip_text_config {
    int32_t device;
    int32_t vocab_size, context_length;     /* 49408, 77 */
    int32_t width, heads, layers;           /* 512, 8, 12 */
    int32_t embed_dim;                      /* 512        */
} ls_clip_text_config;
int ls_clip_text_create(const ls_clip_text_config* cfg, ls_clip_text** out);
void ls_clip_text_destroy(ls_clip_text* h);
const char* ls_clip_text_last_error(const ls_clip_text* h);
int ls_clip_text_set_weight(ls_clip_text* h, const char* key, const float* data, size_t n);
int ls_clip_text_commit_weights(ls_clip_text* h);
/* tokens [B, context_length] int64 -> out [B, embed_dim] fp32.  on_device: 0 = tokens and out are host memory, 1 = both are device
 * memory, 2 = host tokens, device out.  Host tokens are planned on the host (no device round trip).  Device tokens are planned by a
 * small kernel whose B + 1 ints the host reads back, because the GEMM grids need the packed row count: that copy is the call's one
 * host wait, also in the asynchronous form.  A token id outside [0, vocab_size) is LS_EINVAL, found by the plan before any gather. */
int ls_clip_text_encode(ls_clip_text* h, int batch, int on_device, const int64_t* tokens, int prune, float* out);
/* The same, enqueued only (`out` is device memory; tokens_on_device says where the tokens are): `out` is complete once
 * ls_clip_text_stream() has reached this point; a SAG decoder handle consumes it after
 * ls_stream_order(device, ls_clip_text_stream(clip), ls_sag_stream(dec)). */
int ls_clip_text_encode_async(ls_clip_text* h, int batch, int tokens_on_device, const int64_t* tokens, int prune, float* out);
float ls_clip_text_last_encode_ms(const ls_clip_text* h);   /* GPU time of the last encode; waits for an asynchronous one */
void* ls_clip_text_stream(const ls_clip_text* h);
/* The plan alone, on the host (needs no GPU): eot_out[b] = first position of row b's maximum (torch.argmax), row0_out[b] = the sum
 * of eot + 1 over the rows before b, *total_out = the packed row count.  LS_EINVAL if an id lies outside [0, vocab_size). */
int ls_clip_text_plan(const int64_t* tokens, int batch, int context_length, int vocab_size, int32_t* eot_out, int32_t* row0_out,
                      int64_t* total_out);

/* ---- caller-side post-processing of sampled clips ---------------------------------
 * scripts/test_RAG_ted.py:84-111 (layout change, mean add, per-bone normalisation, joint-angle change curve, motion
 * beats) and convert_dir_vec_to_pose (scripts/utils/data_utils.py:77-97).  Stateless; dataset constants are passed in. */
typedef struct ls_post_config {
    int32_t njoints;            /* direction vectors per frame: 9 (TED)                          */
    int32_t n_pairs;            /* angle pairs: 4 (test_RAG_ted.py:24-29)                        */
    int32_t n_pose_joints;      /* 10                                                            */
    float thres;                /* 0.03 (:32)                                                    */
    int32_t pair_a[8], pair_b[8];
    float change_angle[8];      /* (:30)                                                         */
    int32_t bone_parent[16], bone_child[16];   /* dir_vec_pairs (data_utils.py:13-14)            */
    float bone_len[16];
    float mean_dir_vec[48];     /* (:22)                                                         */
} ls_post_config;
/* sample [B,J,3,34] -> aligned [B,34,J*3], pose [B,34,n_pose_joints,3], angle_diff [B,34], beat_mask [B,34] (bytes);
 * any output may be NULL.  Pointers are device pointers iff on_device.  LS_EINVAL without a HIP call (the one check the timeline
 * entries share): a NULL config or sample, batch < 1, njoints outside [1, 16], n_pairs outside [0, 8], n_pose_joints outside
 * [0, 17], a bone_parent or bone_child of the first njoints bones outside [0, 16], a pair index of the first n_pairs pairs outside
 * [0, njoints).  (Earlier versions passed an out-of-range bone or pair index on to the kernel.) */
int ls_ted_post(int device, int on_device, int batch, const ls_post_config* c, const float* sample, float* aligned,
                float* pose, float* angle_diff, unsigned char* beat_mask);

/* BEAT twin of the caller plumbing (scripts_beat/test_RAG_beat.py:86, 101): the sampled tensor [B,J,6,34] in the reference layout
 * -> decoded_motions [B,34,J*6] (`.permute(0, 3, 1, 2).reshape(tar_pose.shape)`) and pred_euler [B,34,J*3] in degrees
 * (`matrix_to_euler_angles(rotation_6d_to_matrix(.), "XYZ") / pi * 180`, scripts_beat/dataloaders/rot_utils.py:218-257, 513-534:
 * Gram-Schmidt on the two 3-vectors, then (atan2(-m12, m22), asin(m02), atan2(-m01, m00))).  Either output may be NULL. */
int ls_beat_post(int device, int on_device, int batch, int njoints, const float* sample, float* decoded, float* euler_deg);

/* The BEAT evaluation metrics of a batch (scripts_beat/utils/metric.py: SRGR.run :27-51, alignment.load_pose :76-98, GAHR and
 * calculate_align :162-193) on the Euler planes [B,34,J*3] in degrees that ls_beat_post writes; one workgroup per clip, every
 * per-clip sum a fixed tree, so a clip's numbers do not depend on the batch it travels in.
 *   success[B,34,J]   1 where sum_k |pred - target| < threshold
 *   srgr_sum[B]       sum over (frame, joint) of success * semantic[frame] * scale (semantic NULL: weight 1); the caller divides by
 *                     34 * J * B for SRGR.run's rate
 *   vel[B,6,33]       per series s, the norm of the frame-to-frame difference of the three angles of joint series_joint[s] (raw
 *                     degrees, no wrapping)
 *   beat_mask[B,6,33] strict local minima of vel as scipy.signal.argrelextrema(x, np.less, order) finds them in its default
 *                     mode='clip': x[i] < x[clip(i - k)] and x[i] < x[clip(i + k)] for k = 1..order (the end frames never are)
 *   align[B]          mean over the clip's onsets of exp(-min_m (onset - m / fps)^2 / (2 sigma^2)), m over the beats of series
 *                     align_series; 0 for a clip without a motion beat
 * pred is required; target, semantic and every output may be NULL (success and srgr_sum need target, align needs the onsets).
 * Tensor pointers are device pointers iff on_device; onset_offsets is read by the host in both modes.  LS_EINVAL without a launch:
 * NULL pred, batch < 1, order < 1, a series joint outside [0, njoints), onset_offsets not starting at 0 or a clip without an onset
 * when align is asked for. */
typedef struct ls_beat_metrics_args {
    int32_t batch;
    int32_t njoints;              /* J: 47 on BEAT                                                               */
    int32_t on_device;
    int32_t order;                /* argrelextrema order: 2 (test_RAG_beat.py:43)                                */
    int32_t align_series;         /* the series align reads: 2, the right wrist (metric.py:189)                  */
    int32_t reserved;
    int32_t series_joint[6];      /* right arm, right shoulder, right wrist, left arm, left shoulder, left wrist */
    float threshold;              /* 4 (test_LivelySpeaker_beat.py: SRGR(4, 47))                                 */
    float scale;                  /* 1 / 0.165 (metric.py:41)                                                    */
    float sigma;                  /* 0.3                                                                         */
    float fps;                    /* 15                                                                          */
    const float* pred;            /* [B,34,J*3]                                                                  */
    const float* target;          /* [B,34,J*3] or NULL                                                          */
    const float* semantic;        /* [B,34] or NULL                                                              */
    const float* onset_times;     /* flat, seconds; clip b owns [onset_offsets[b], onset_offsets[b+1])           */
    const int64_t* onset_offsets; /* [B+1] HOST                                                                  */
    unsigned char* success;
    float* srgr_sum;
    float* vel;
    unsigned char* beat_mask;
    float* align;
} ls_beat_metrics_args;
int ls_beat_metrics(int device, const ls_beat_metrics_args* a);

/* L1div.run (metric.py:12-24): *sum_out = sum over rows and columns of |x - column mean| of x [rows, dim].  The column means are
 * reduced in a fixed order and rounded to fp32 (np.mean of an fp32 array), |x - mean| is fp32, the total float64; x is only read
 * (the reference overwrites it).  x is a device pointer iff on_device, sum_out a host pointer.
 * The name spells "l1div" without its digit: exported names in this header are lower-case letters and underscores only, which
 * is what the export check of the test suite collects them by. */
int ls_beat_ldiv(int device, int on_device, int64_t rows, int dim, const float* x, double* sum_out);

/* ---- the same post-processing and scores on a stitched timeline of n_frames frames ---------------------------
 * ls_long_sample returns [B,J,F,N] with N = 34 + 30 (W - 1).  These are the loop bodies above with 34 replaced by N = n_frames and
 * 33 by N - 1 (no counterpart in the reference, which scores 34-frame clips): a timeline clip is ONE series, nothing resets at a
 * window seam.  The kernels run over (clip, tile of LS_TIMELINE_TILE frames) with a recomputed halo; a frame's numbers are those of
 * the 34-frame kernels' own per-frame functions and do not depend on the batch, the tile size or the tile the frame lands in, and at
 * n_frames = 34 every output equals ls_ted_post's / ls_beat_post's / ls_beat_metrics's bit for bit.
 *   ls_ted_post_timeline      timeline [B,J,3,N] -> aligned [B,N,J*3], pose [B,N,n_pose_joints,3], angle_diff [B,N] (0 at frame 0),
 *                             beat_mask [B,N] (bytes; beats at t in [2, N-2]); any output may be NULL
 *   ls_beat_post_timeline     timeline [B,J,6,N] -> decoded [B,N,J*6], euler_deg [B,N,J*3]; either may be NULL
 *   ls_beat_metrics_timeline  ls_beat_metrics_args with pred / target [B,N,J*3], semantic [B,N], success [B,N,J], vel and
 *                             beat_mask [B,6,N-1] (mode='clip' clamps at 0 and N-2; beat time m / fps), srgr_sum and align [B]
 *   ls_ted_beat_align         the TED beat-consistency sum of every clip (scripts/test_RAG_ted.py:113-123) in float64:
 *                             align_sum[b] = sum over the first onset_count[b] entries a = frame * hop / sr of row b of onset_frames
 *                             [B,onset_cols] (the slab ls_onsets writes) of exp(-min_m (a - m)^2 / (2 sigma^2)), m = t / fps over the
 *                             set frames t of beat_mask [B,N]; n_beats[b] = the number of set frames; a clip without one has
 *                             align_sum 0 (the caller leaves its onsets out of the running count, as the reference's `continue`
 *                             does).  fps, sigma and sr are doubles: the host loop this restates computes with Python floats.
 *                             Either output may be NULL.
 * Pointers are device pointers iff on_device (onset_offsets: host, as in ls_beat_metrics).  LS_EINVAL without a HIP call: a NULL
 * input, batch < 1, n_frames > LS_TIMELINE_MAX_FRAMES, n_frames < 4 (TED post and align), < 2 (BEAT post), < 2 order + 2 (BEAT
 * metrics), whatever ls_ted_post / ls_beat_metrics refuse, and for ls_ted_beat_align onset_cols < 1, a host onset_count entry
 * outside [0, onset_cols] (device-resident counts are clamped), fps, sigma or sr not positive, hop < 1.
 * ls_ted_beat_align needs no ragged twin: on a beat mask that is zero beyond each clip's valid frames (what
 * ls_ted_post_timeline_ragged writes) with per-clip onset counts, its sums and n_beats are those of the solo call at the clip's own
 * length, bit for bit -- a frame without a beat enters the minimum as +inf and changes nothing, and the onsets are partitioned over the
 * threads by their index alone.
 * Not built: timelines longer than LS_TIMELINE_MAX_FRAMES. */
#define LS_TIMELINE_MAX_FRAMES 4096
#define LS_TIMELINE_TILE 64
int ls_ted_post_timeline(int device, int on_device, int batch, int n_frames, const ls_post_config* c, const float* timeline,
                         float* aligned, float* pose, float* angle_diff, unsigned char* beat_mask);
int ls_beat_post_timeline(int device, int on_device, int batch, int njoints, int n_frames, const float* timeline, float* decoded,
                          float* euler_deg);
int ls_beat_metrics_timeline(int device, int n_frames, const ls_beat_metrics_args* a);
typedef struct ls_ted_align_args {
    int32_t batch;
    int32_t n_frames;
    int32_t on_device;
    int32_t onset_cols;                /* F: columns of the onset slab                                       */
    double fps;                        /* 15                                                                 */
    double sigma;                      /* 0.1 (test_RAG_ted.py:33)                                           */
    double sr;                         /* 16000                                                              */
    int32_t hop;                       /* 512                                                                */
    int32_t reserved;
    const unsigned char* beat_mask;    /* [B,N]                                                              */
    const int32_t* onset_frames;       /* [B,onset_cols]                                                     */
    const int32_t* onset_count;        /* [B]                                                                */
    double* align_sum;                 /* [B]                                                                */
    int32_t* n_beats;                  /* [B]                                                                */
} ls_ted_align_args;
int ls_ted_beat_align(int device, const ls_ted_align_args* a);

/* ---- clips of different lengths in one call ---------------------------------------------------------------
 * The timeline entries above for a padded batch: n_frames is the ROW STRIDE N_max of every tensor (vel and the BEAT beat_mask keep
 * row stride N_max - 1) and frames [B] (HOST, in both modes) holds each clip's valid frames.  On clip b's valid range every output
 * equals, bit for bit, what the equal-length entry returns for that clip alone (batch 1, n_frames = frames[b]); srgr_sum[b] and
 * align[b] are the clip's own.  Beyond the valid range the outputs are 0 and the inputs are never read.  Work follows the valid
 * frames: the per-frame kernels run over the tile table of ls_ragged_tiles.  LS_EINVAL without a HIP call: whatever the equal-length
 * entry refuses, a NULL frames, an entry above n_frames or below the entry's minimum (4 TED, 2 BEAT post, 2 order + 2 metrics).
 * Not built: device-resident length arrays. */
int ls_ted_post_timeline_ragged(int device, int on_device, int batch, int n_frames, const int32_t* frames, const ls_post_config* c,
                                const float* timeline, float* aligned, float* pose, float* angle_diff, unsigned char* beat_mask);
int ls_beat_post_timeline_ragged(int device, int on_device, int batch, int njoints, int n_frames, const int32_t* frames,
                                 const float* timeline, float* decoded, float* euler_deg);
int ls_beat_metrics_timeline_ragged(int device, int n_frames, const int32_t* frames, const ls_beat_metrics_args* a);
/* The launch plan of the per-frame timeline kernels, on the host (no device is touched): the (clip, first frame) of every tile of
 * `tile` frames that holds at least one valid frame, clip-major, into clip_out / start_out [cap]; *n_out receives their number.
 * The outputs may be NULL to ask for the count alone.  LS_EINVAL: batch < 1, a NULL frames, tile < 1, an entry < 1, cap too small. */
int ls_ragged_tiles(int batch, const int32_t* frames, int tile, int32_t* clip_out, int32_t* start_out, int32_t cap, int32_t* n_out);

/* ---- Post-processing stream: the timeline entries' outputs as frames arrive ----------------------------------
 * A handle of `capacity` SLOTS; each slot is one series of unbounded length that is fed in chunks (the frames ls_long_pool_push
 * returns, or any other source in its [S, J, F, K] layout).  A push post-processes the new frames of every slot and returns the motion
 * beats that have just become decidable; per slot, the outputs concatenated over the pushes and the finish are bit for bit what
 * ls_ted_post_timeline (TED), ls_beat_post_timeline and ls_beat_metrics_timeline's beat_mask (BEAT) give for the whole series, under
 * any chunking and beyond LS_TIMELINE_MAX_FRAMES.  The kernels call the timeline kernels' per-frame functions; what a frame needs from
 * its left is CARRIED per slot on the device and recomputed from there: TED keeps the last 3 raw frames (angle_diff[f] needs frame
 * f - 1, the beat at f needs angle_diff[f - 1 .. f + 1], so the beat output lags the frames by one), BEAT the last 2 order + 1 Euler
 * triples of the six series joints (v[f] = |e[f + 1] - e[f]|; the minimum at f is decided once v[f + order] exists, a lag of
 * order + 1 frames; mode='clip' clamps at 0 and, at the finish, at V - 1 = N - 2).
 *
 * ls_post_stream_plan (no handle, no GPU) is the one definition of the beat entries a push decides: with n_before frames in the
 * series and n_new more, entries [*beat_first, *beat_first + *beat_count) -- frames of beat_mask (TED, dataset 0) or velocity indices
 * (BEAT, dataset 1).  TED: [max(0, n - 1), N - 1) with N = n_before + n_new, and up to N when finishing (frame N - 1 is never a beat).
 * BEAT: [max(0, n - order - 1), max(0, N - order - 1)), and up to max(0, N - 1) when finishing.  Over the pushes and the finish the
 * ranges tile [0, N) (TED) or [0, N - 1) (BEAT) once, in order.  LS_EINVAL: dataset outside {0, 1}, BEAT order outside
 * [1, LS_POST_STREAM_MAX_ORDER], a negative count, a sum above 2^62, finishing a series without a frame, NULL outputs.
 * ls_post_stream_check (no handle, no GPU) is the check a push runs ahead of any launch, slot by slot on that plan: LS_EINVAL for a
 * NULL counts, capacity < 1, K outside [0, LS_POST_STREAM_MAX_CHUNK], counts[s] outside [0, K], beat_capacity below a slot's
 * beat_count; LS_ESTATE for finish on a slot with no frames.  beat_first / beat_count [capacity] may be NULL.
 *
 * ls_post_stream_open allocates everything for `capacity` slots and LS_POST_STREAM_MAX_CHUNK frames per push (the carries, the slot
 * table, and the staging of a host-side push); nothing grows afterwards.  cfg: the TED configuration (dataset 0; njoints comes from
 * it); njoints, order, series_joint: BEAT (dataset 1).  LS_EINVAL ahead of any HIP call: what the plan refuses, capacity < 1, what
 * ls_ted_post refuses of a configuration, njoints < 1, a series joint outside [0, njoints).
 * ls_post_stream_push: frames [S, J, F, K] (F = 3 TED, 6 BEAT; frame-innermost) holds counts[s] new frames of slot s in
 * frames[s, :, :, :counts[s]]; what lies behind counts[s] is never read.  Outputs, any of them NULL, rows behind counts[s] zeroed:
 * TED aligned [S,K,J*3], pose [S,K,n_pose_joints,3], angle_diff [S,K], beat_mask [S,beat_capacity]; BEAT decoded [S,K,J*6],
 * euler_deg [S,K,J*3], beat_mask [S,6,beat_capacity].  Entry q of slot s's beat_mask row is series entry beat_first[s] + q, for
 * q < beat_count[s]; the rest of the row is 0.  finish[s] != 0 ends slot s's series with this push (counts[s] may be 0): the pending
 * entries are emitted and the slot is free -- its next frames start a new series at frame 0.  A failed launch marks the handle failed
 * (LS_ESTATE from then on).  frames and the tensor outputs are device pointers iff on_device; counts, finish, beat_first and
 * beat_count are HOST arrays in both modes.
 * Audio onsets and the alignment scores: at the finish, score stream (ls_score_stream_*).  Not built: device-resident counts, chunks
 * above LS_POST_STREAM_MAX_CHUNK frames per push, SRGR (it needs targets). */
#define LS_POST_STREAM_MAX_CHUNK 256
#define LS_POST_STREAM_MAX_ORDER 8
typedef struct ls_post_stream ls_post_stream;
typedef struct ls_post_stream_push_args {
    int32_t on_device;
    int32_t K;                  /* row stride of frames and of the per-frame outputs: 0 .. LS_POST_STREAM_MAX_CHUNK   */
    int32_t beat_capacity;      /* row stride of beat_mask                                                            */
    int32_t reserved;
    const float* frames;        /* [S, J, F, K]; may be NULL when K == 0                                              */
    const int32_t* counts;      /* [S] HOST                                                                           */
    const int32_t* finish;      /* [S] HOST or NULL                                                                   */
    float* aligned;             /* TED                                                                                */
    float* pose;
    float* angle_diff;
    float* decoded;             /* BEAT                                                                               */
    float* euler_deg;
    unsigned char* beat_mask;
    int64_t* beat_first;        /* [S] HOST or NULL                                                                   */
    int32_t* beat_count;        /* [S] HOST or NULL                                                                   */
} ls_post_stream_push_args;
int ls_post_stream_plan(int32_t dataset, int32_t order, int64_t n_before, int64_t n_new, int32_t finishing, int64_t* beat_first,
                        int32_t* beat_count);
int ls_post_stream_check(int32_t dataset, int32_t order, int32_t capacity, const int64_t* frames_in, int32_t K, const int32_t* counts,
                         const int32_t* finish, int32_t beat_capacity, int64_t* beat_first, int32_t* beat_count);
int ls_post_stream_open(int device, int32_t dataset, int32_t capacity, const ls_post_config* cfg, int32_t njoints, int32_t order,
                        const int32_t* series_joint, ls_post_stream** out);
int ls_post_stream_push(ls_post_stream* h, const ls_post_stream_push_args* a);
/* frames_in [capacity] (nullable): the frames of each slot's running series; *device_bytes (nullable): what the handle holds */
int ls_post_stream_info(const ls_post_stream* h, int64_t* frames_in, int64_t* device_bytes);
void ls_post_stream_close(ls_post_stream* h);
const char* ls_post_stream_last_error(const ls_post_stream* h);

/* ---- audio onsets for the beat-alignment scores ------------------------------------------------------------
 * What the reference's scripts take from librosa 0.9.2 (scripts/test_RAG_ted.py:113 onset_detect(y, sr=16000, units='time');
 * scripts_beat/utils/metric.py:60-74 alignment.load_audio), for a batch of equally long clips (ls_onsets_ragged: of any lengths):
 *   frames     y padded by 1024 on both sides (pad_mode), n_fft 2048, hop 512, periodic Hann: F = 1 + length / 512 frames
 *   mel_db     10 log10(max(1e-10, W P)) with P the power spectrum and W 128 Slaney mel filters on [0, fmax], BEFORE the clip-wide
 *              clamp to (max - 80) that the envelope applies
 *   rms        librosa.feature.rms(S=|stft|): sqrt(2 sum_k P'[k] / 2048^2), P' = P with rows 0 and 1024 halved
 *   oenv       concat(zeros(3), mean over the mels of max(0, S[t+1] - S[t]))[:F], S the clamped mel_db
 *   onset_raw  util.peak_pick on (oenv - min) / (max + tiny) with onset_detect's default windows for sr_pick and hop 512, and delta
 *   onset_bt, onset_bt_rms   onset_backtrack(onset_raw, oenv) and (onset_raw, rms): the nearest minimum at or before each onset
 * Two kernels: one wave per frame for the spectrum (a 1024-point complex FFT in LDS, mel sums gathered per filter in a fixed
 * order), one workgroup per clip for everything after it; a clip's numbers do not depend on the batch it travels in.
 * With `envelope` instead of `audio`, `length` counts frames and the pick runs on the given envelope (onset_detect(onset_envelope=)).
 * The onset slabs are [B,F] int32 of which the first count[b] entries of row b are valid (the rest is -1).  Every output may be
 * NULL; kernel_ms is a HOST pointer in both modes.  LS_EINVAL without a launch: NULL args, neither or both inputs, batch < 1,
 * length < 1, reflect padding with length <= 1024, more than 4096 frames, an unknown pad_mode, fmax <= 0, sr <= 0, sr_pick <= 0,
 * and mel_db, rms or onset_bt_rms asked for with a given envelope. */
#define LS_ONSETS_PAD_CONSTANT 0
#define LS_ONSETS_PAD_REFLECT 1
#define LS_ONSETS_MAX_FRAMES 4096
typedef struct ls_onsets_args {
    int32_t batch;
    int32_t length;          /* samples per clip; frames per clip when envelope is given                         */
    int32_t on_device;
    int32_t pad_mode;        /* LS_ONSETS_PAD_CONSTANT (0.9.2's default) | LS_ONSETS_PAD_REFLECT                   */
    float sr;                /* of the audio: 16000                                                              */
    float sr_pick;           /* of the picking windows: 16000 on TED, 22050 on BEAT (load_audio passes no sr)    */
    float fmax;              /* 11025 in 0.9.x, sr / 2 from 0.10 on                                              */
    float delta;             /* 0.07                                                                             */
    const float* audio;      /* [B,length] or NULL                                                               */
    const float* envelope;   /* [B,length] or NULL                                                               */
    float* mel_db;           /* [B,F,128]                                                                        */
    float* rms;              /* [B,F]                                                                            */
    float* oenv;             /* [B,F]                                                                            */
    int32_t* count;          /* [B]                                                                              */
    int32_t* onset_raw;      /* [B,F]                                                                            */
    int32_t* onset_bt;       /* [B,F]                                                                            */
    int32_t* onset_bt_rms;   /* [B,F]                                                                            */
    float* kernel_ms;        /* HOST [2]: the spectrum and the pick kernel, timed with events (0 for one not run) */
} ls_onsets_args;
int ls_onsets(int device, const ls_onsets_args* a);
/* ls_onsets for clips of different lengths: a->length is the ROW STRIDE of audio (or envelope) and lengths [B] (HOST, in both modes)
 * holds each clip's valid samples (frames, with `envelope`), each in [1, a->length].  The outputs keep F = 1 + length / 512 columns
 * (length columns with `envelope`); clip b has F_b = 1 + lengths[b] / 512 frames (lengths[b] with `envelope`).  On its F_b frames
 * every output equals, bit for bit, what ls_onsets returns for that clip alone at its own length: the centre padding reflects or
 * zeroes at the clip's own last sample, the 80 dB clamp and the normalisation use the clip's own maximum, the windows are cut at
 * F_b.  Beyond them the float outputs are 0 and the onset slabs -1; input beyond a clip's valid length is never read.  The spectrum
 * runs one wave per valid frame (sum of F_b).  LS_EINVAL without a launch: a NULL lengths, an entry outside [1, length], reflect
 * padding with an entry <= 1024, and whatever ls_onsets refuses.  Not built: device-resident length arrays. */
int ls_onsets_ragged(int device, const ls_onsets_args* a, const int32_t* lengths);
/* ls_onsets for an equal-length batch of clips of ANY length (a talk of a quarter of an hour has 28 000 frames): the arguments and
 * the meaning of ls_onsets -- audio or a given envelope, every output nullable, kernel_ms -- without LS_ONSETS_MAX_FRAMES.  The
 * spectrum is ls_onsets' kernel.  What follows it runs over (clip, tile of LS_SCORE_TILE frames) with nothing in LDS sized by the
 * clip: tile partials and a combine for the clip maximum of mel_db and the envelope's extrema (exact in any order), the flux and
 * the detection flag per frame with the windows read from global memory, the flagged frames compacted per tile and walked by one
 * wave per clip (n > last + wait is sequential in the candidates, not the frames), one thread per onset searching left for both
 * backtracks.  Every float is a per-frame expression or an exact reduction: up to LS_ONSETS_MAX_FRAMES frames every output equals
 * ls_onsets' bit for bit.  kernel_ms[1] covers all launches of the pick.  Device memory beyond the outputs: mel_db (512 B per
 * frame) and 12 B per frame of candidates and slabs where the caller leaves them out.  LS_EINVAL without a launch: whatever
 * ls_onsets refuses except the frame count, length > 2^31 - 2048, and B * F frames beyond the grid (2^33 - 4).  Not built: the
 * ragged form. */
#define LS_SCORE_TILE 256
int ls_onsets_long(int device, const ls_onsets_args* a);

/* The tables ls_onsets computes with, built on the host in double and rounded to float32: window [n_fft] (periodic Hann), twiddle
 * [n_fft][2] (exp(-2 pi i n / n_fft)), and librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax, htk=False, norm='slaney') in CSR
 * form: mel_ptr [n_mels + 1], mel_col and mel_w [nnz] (weights that round to 0 are left out).  *nnz_out receives nnz; every
 * pointer may be NULL, so a first call can ask for nnz alone.  LS_EINVAL: n_fft no power of two, sr <= 0, fmax <= fmin, fmin < 0,
 * n_mels < 1, nnz_cap < nnz when the CSR arrays are asked for.  No device is touched. */
int ls_onsets_tables(float sr, int n_fft, int n_mels, float fmin, float fmax, float* window, float* twiddle, int32_t* mel_ptr,
                     int32_t* mel_col, float* mel_w, int32_t nnz_cap, int32_t* nnz_out);

/* ---- Score stream: audio onsets and the beat-alignment scores for series of any length -----------------------
 * Only two steps of librosa's onset chain need the whole signal -- the clamp at (max - 80 dB) and the envelope's min / max
 * normalisation -- and both are order-independent reductions.  The spectrum is causal.  So the chain splits: spectra as audio
 * arrives (ls_score_stream_push), the tiled pick of ls_onsets_long and the alignment sums when a series ends
 * (ls_score_stream_finish).  A handle has `capacity` SLOTS; a slot is one series (a talk).  Everything is allocated at open for
 * max_audio_frames and max_beat_entries per slot and nothing grows afterwards.  Per slot the handle keeps mel_db
 * [max_audio_frames, 128] and rms (516 B per audio frame: about 16 KB per second of 16 kHz audio), the motion-beat bytes
 * [max_beat_entries], an audio carry of the samples a pending frame still needs (below 2048 + 512; two copies, written in turn)
 * and the workspace of the finish (envelope, candidates and the three slabs: 20 B per audio frame; a beat list of 4 B per entry).
 *
 * ls_score_stream_plan (no handle, no GPU) is the one definition of the audio frames a push decides: with samples_before samples
 * in the series and n_new more, frames [*frame_first, *frame_first + *frame_count).  Frame f is decided once the series holds
 * 512 f + 1024 samples, and under reflect padding 1025; a finish decides every frame below 1 + L / 512 (L the total).  Over the
 * pushes and the finish the ranges tile [0, 1 + L / 512) once, in order.  LS_EINVAL: NULL outputs, an unknown pad_mode, a negative
 * count, a total above 2^31 - 2048, finishing an empty series, finishing with reflect padding and L <= 1024.
 *
 * ls_score_stream_open: dataset 0 (TED: the beat-consistency sum of ls_ted_beat_align) or 1 (BEAT: the align of
 * ls_beat_metrics_timeline).  LS_EINVAL ahead of any HIP call: a NULL config or out, dataset outside {0, 1}, capacity < 1,
 * max_audio_frames < 1 or above 2^22 - 3, max_beat_entries < 0, max_chunk < 1, what ls_onsets refuses of sr, sr_pick, pad_mode,
 * fmax, and fps, sigma, time_rate <= 0, hop < 1, onset_source outside {0, 1, 2}.
 * ls_score_stream_push: per slot s, lengths[s] new samples in audio[s, :lengths[s]] (row stride n_max <= max_chunk) and / or
 * beat_count[s] motion-beat bytes in beats[s, :beat_count[s]] (row stride beat_capacity) that continue the slot's entries at
 * beat_first[s] -- what ls_post_stream_push returns (TED: beat_mask; BEAT: the row of the series the alignment uses).  The spectrum
 * kernel runs over the (slot, frame) table of the newly decided frames, reads carry + chunk and stores the rows; the carries roll;
 * the bytes are appended.  Everything is refused ahead of any launch, slot by slot, and leaves the handle untouched: LS_EINVAL for
 * a NULL argument, n_max outside [0, max_chunk], a length outside [0, n_max], audio without lengths, a negative beat_count or one
 * above beat_capacity, beats without beat_first / beat_count; LS_ESTATE for a frame beyond max_audio_frames, an entry beyond
 * max_beat_entries, beat_first[s] different from the entries the slot holds (with beat_count[s] > 0).  A failed launch marks the
 * handle failed (LS_ESTATE from then on).
 * ls_score_stream_finish: for every slot with finish[s] != 0 the remaining frames are decided (end padding at the slot's own
 * last sample), the tiled pick runs on its F = 1 + L / 512 frames, the alignment sum runs against its beats, and the slot is free.
 * Outputs, any of them NULL: count [S], onset_raw, onset_bt, onset_bt_rms [S, cols] int32, oenv, rms [S, cols], mel_db
 * [S, cols, 128] -- row s holds the slot's F entries (for F <= LS_ONSETS_MAX_FRAMES bit for bit those of ls_onsets on the slot's
 * samples alone, under any chunking), the slabs -1 behind count[s]; what lies behind F and the rows of slots that do not finish
 * are not written.  TED: align_sum [S] double and n_beats [S] as ls_ted_beat_align forms them from onset_raw (up to
 * LS_TIMELINE_MAX_FRAMES entries bit for bit: onset i stays on thread i % 256, added in index order; the beats are compacted to
 * a sorted list and the nearest is found by binary search -- the minimum over the same set is the same value).  BEAT: align [S]
 * float as ls_beat_metrics_timeline forms it from the slab `onset_source` at frame * hop / time_rate (NaN for a slot without an
 * onset).  n_frames [S] (HOST) receives F, 0 for a slot that does not finish.  LS_EINVAL: NULL finish or outputs, cols below a
 * finishing slot's F; LS_ESTATE: a finishing slot without audio, or with too little for its padding (reflect, L <= 1024).
 * Lengths, counts, firsts and flags are HOST arrays in both modes; tensor arguments are device pointers iff on_device.
 * Not built: a causal approximation of the normalisation, SRGR online, device-resident lengths, growing a slot. */
#define LS_SCORE_STREAM_MAX_BEATS 4096   /* beat_capacity of a push, at most */
typedef struct ls_score_stream ls_score_stream;
typedef struct ls_score_config {
    float sr;                /* of the audio: 16000                                                              */
    float sr_pick;           /* of the picking windows: 16000 on TED, 22050 on BEAT                              */
    int32_t pad_mode;        /* LS_ONSETS_PAD_CONSTANT | LS_ONSETS_PAD_REFLECT                                   */
    float fmax;
    float delta;
    int32_t hop;             /* samples per onset frame in the scores' time axis: 512                            */
    int32_t onset_source;    /* BEAT: 0 onset_raw, 1 onset_bt, 2 onset_bt_rms (score_timeline's)                 */
    int32_t max_chunk;       /* samples per slot and push, at most: sizes the staging of host-side pushes        */
    double fps;              /* of the motion-beat entries: 15                                                   */
    double sigma;            /* TED 0.1 (beat consistency), BEAT 0.3                                             */
    double time_rate;        /* BEAT: onset time = frame * hop / time_rate, 22050 (librosa's default rate)       */
} ls_score_config;
typedef struct ls_score_stream_push_args {
    int32_t on_device;
    int32_t n_max;              /* row stride of audio                                                                */
    int32_t beat_capacity;      /* row stride of beats                                                                */
    int32_t reserved;
    const float* audio;         /* [S, n_max] or NULL                                                                 */
    const int32_t* lengths;     /* [S] HOST                                                                           */
    const unsigned char* beats; /* [S, beat_capacity] or NULL                                                         */
    const int64_t* beat_first;  /* [S] HOST                                                                           */
    const int32_t* beat_count;  /* [S] HOST                                                                           */
} ls_score_stream_push_args;
typedef struct ls_score_stream_outputs {
    int32_t on_device;
    int32_t cols;               /* row stride of the per-frame outputs                                                */
    int32_t* n_frames;          /* [S] HOST                                                                           */
    int32_t* count;             /* [S]                                                                                */
    int32_t* onset_raw;         /* [S, cols]                                                                          */
    int32_t* onset_bt;
    int32_t* onset_bt_rms;
    float* oenv;                /* [S, cols]                                                                          */
    float* mel_db;              /* [S, cols, 128]                                                                     */
    float* rms;                 /* [S, cols]                                                                          */
    double* align_sum;          /* [S] TED                                                                            */
    int32_t* n_beats;           /* [S] TED                                                                            */
    float* align;               /* [S] BEAT                                                                           */
} ls_score_stream_outputs;
int ls_score_stream_plan(int32_t pad_mode, int64_t samples_before, int64_t n_new, int32_t finishing, int64_t* frame_first,
                         int32_t* frame_count);
int ls_score_stream_open(int device, int32_t dataset, int32_t capacity, int32_t max_audio_frames, int32_t max_beat_entries,
                         const ls_score_config* cfg, ls_score_stream** out);
int ls_score_stream_push(ls_score_stream* h, const ls_score_stream_push_args* a);
int ls_score_stream_finish(ls_score_stream* h, const int32_t* finish, const ls_score_stream_outputs* out);
/* samples_in, frames_done, beats_in [capacity] (nullable): each slot's samples, decided audio frames and beat entries */
int ls_score_stream_info(const ls_score_stream* h, int64_t* samples_in, int64_t* frames_done, int64_t* beats_in, int64_t* device_bytes);
void ls_score_stream_close(ls_score_stream* h);
const char* ls_score_stream_last_error(const ls_score_stream* h);

/* ---- Audio front end: resample any integer rate to the model's rate on the device ---------------------------
 * A polyphase windowed-sinc resampler, one-shot (ls_resample) and streaming (ls_resample_stream_*), with the mixdown of interleaved
 * channels in front of the filter.  ONE DEFINITION: with g = gcd(in_sr, out_sr), up = out_sr / g, down = in_sr / g, q = max(up, down)
 * and half = zeros * q,
 *   h[i] = up * (rolloff / q) * sinc(rolloff * (i - half) / q) * kaiser(2 half + 1, beta)[i],   i = 0 .. 2 half
 * (sinc and kaiser as numpy defines them; computed in double on the host, rounded to float32 once), and output m of x[0 .. n) is
 *   y[m] = sum_k h[m down - k up + half] x[k],   m in [0, ceil(n up / down)),
 * over the k in [0, n) whose tap exists.  This is scipy.signal.resample_poly(x, up, down, window = h / up).  The sum of one output is
 * a chain of float32 fused multiply-adds in an order that depends on (up, down, half) alone -- not on the chunking, the slot, the
 * batch or the output's place in a launch -- and a tap whose sample does not exist contributes nothing, so the streaming form gives
 * bit for bit the whole-series call under any chunking.  in_sr == out_sr is a pass-through: the mixdown alone.
 * Mixdown: audio is mono [.., n] or interleaved [.., n, C], 1 <= C <= LS_RESAMPLE_MAX_CHANNELS.  float32: the float32 sum in channel
 * order times float(1 / C); int16: the exact int32 sum, converted, times float(1 / (32768 C)).
 *
 * ls_resample_ratio, ls_resample_plan and ls_resample_taps touch no device.
 * ls_resample_ratio: up, down, half, n_taps = 2 half + 1, taps_per_output = floor(2 half / up) + 1 and carry_len =
 * ceil((2 half + down) / up) + 1, the samples before a push that its outputs may read.  LS_EINVAL: a rate or zeros < 1, a NULL
 * output; LS_EUNSUPPORTED: n_taps above 2^22.
 * ls_resample_plan is the one definition of what a push emits: with n samples of a running series in, outputs [0, D(n)) are decided,
 * D(n) = max(0, floor((n up - 1 - half) / down) + 1), and D(n) = ceil(n up / down) at the finish; a push from n_before to
 * n_before + n_new emits [D(n_before), D(n_before + n_new)).  Over the pushes and the finish the ranges tile the whole-series output
 * once, in order.  A pass-through plans with half = 0.  LS_EINVAL: NULL outputs, up or down < 1, a negative half or count, counts or
 * products above 2^62, finishing a series without a sample.
 * ls_resample_taps: h64 and / or h32 [2 half + 1] (one of them may be NULL).  LS_EINVAL: both NULL, up, down or zeros < 1, beta < 0,
 * rolloff outside (0, 1]; LS_EUNSUPPORTED: more than 2^22 taps.
 *
 * ls_resample: audio [batch, row_stride] elements of dtype, clip b's lengths[b] frames of `channels` samples at its row's start;
 * out [batch, out_stride] receives clip b's ceil(lengths[b] up / down) outputs and 0 behind them; out_lengths (HOST, nullable) those
 * counts.  Nothing beyond a clip's own frames is read.  audio and out are device pointers iff on_device; lengths is a HOST array.
 * Every refusal sits ahead of any HIP call.  LS_EINVAL: NULL args, audio, lengths or out, batch outside [1, 65535], an unknown dtype,
 * channels outside [1, 8], a length outside [1, 2^31 - 1] or beyond row_stride / channels, out_stride below a clip's outputs, what
 * ls_resample_ratio and ls_resample_taps refuse; LS_EUNSUPPORTED as they do (ls_resample_stream_last_error(NULL) names the count).
 *
 * ls_resample_stream_open allocates everything for `capacity` slots and max_chunk frames per slot and push: the tap table, two mono
 * carries of carry_len + 3 samples per slot (written in turn; the 3: what a tap row padded to a multiple of 4 reaches), the slot table and the staging of host-side pushes.  Nothing grows
 * afterwards.  LS_EINVAL ahead of any HIP call: capacity < 1, max_chunk < 1, what ls_resample refuses of the rates, dtype, channels
 * and filter.
 * ls_resample_stream_push: audio [S, n_max (, C)], slot s's lengths[s] new frames at its row's start; finish[s] != 0 ends slot s's
 * series with this push (finish may be NULL).  out [S, out_capacity] receives slot s's new outputs from column 0 on; out_first and
 * out_count [S] (HOST, nullable) the plan's range, filled before anything is launched.  A slot that finishes is empty afterwards: its
 * next samples start a new series at sample 0.  Refused ahead of any launch, leaving the handle untouched -- LS_EINVAL: NULL args,
 * lengths, or audio / out where a slot has frames / outputs, n_max outside [0, max_chunk], a length outside [0, n_max], a push the
 * plan refuses (a finish on a slot without a sample), out_capacity below a slot's count; LS_ESTATE: a handle after a failed launch.
 * ls_resample_stream_reset drops slot's series without emitting what is pending (no samples in, no carry); idempotent.  LS_EINVAL:
 * a slot outside [0, capacity).
 * Not built: non-integer rates, time-varying rates, device-resident lengths. */
#define LS_RESAMPLE_F32 0
#define LS_RESAMPLE_I16 1
#define LS_RESAMPLE_MAX_CHANNELS 8
typedef struct ls_resample_stream ls_resample_stream;
typedef struct ls_resample_args {
    int32_t batch;
    int32_t on_device;
    int32_t dtype;              /* LS_RESAMPLE_F32 | LS_RESAMPLE_I16                                                  */
    int32_t channels;
    int64_t row_stride;         /* elements between the rows of audio                                                 */
    const void* audio;          /* [batch, row_stride]                                                                */
    const int64_t* lengths;     /* [batch] HOST: frames per clip                                                      */
    int32_t in_sr;
    int32_t out_sr;
    int32_t zeros;
    int32_t reserved;
    double beta;
    double rolloff;
    float* out;                 /* [batch, out_stride]                                                                */
    int64_t out_stride;
    int64_t* out_lengths;       /* [batch] HOST or NULL                                                               */
} ls_resample_args;
typedef struct ls_resample_stream_push_args {
    int32_t on_device;
    int32_t n_max;              /* frames per row of audio                                                            */
    int64_t out_capacity;       /* row stride of out                                                                  */
    const void* audio;          /* [S, n_max (, C)] or NULL when no slot has a frame                                  */
    const int32_t* lengths;     /* [S] HOST                                                                           */
    const int32_t* finish;      /* [S] HOST or NULL                                                                   */
    float* out;                 /* [S, out_capacity] or NULL when no slot has an output                               */
    int64_t* out_first;         /* [S] HOST or NULL                                                                   */
    int64_t* out_count;         /* [S] HOST or NULL                                                                   */
} ls_resample_stream_push_args;
int ls_resample_ratio(int32_t in_sr, int32_t out_sr, int32_t zeros, int64_t* up, int64_t* down, int64_t* half, int64_t* taps_per_output,
                      int64_t* carry_len, int64_t* n_taps);
int ls_resample_plan(int64_t up, int64_t down, int64_t half, int64_t n_before, int64_t n_new, int32_t finishing, int64_t* out_first,
                     int64_t* out_count);
int ls_resample_taps(int64_t up, int64_t down, int32_t zeros, double beta, double rolloff, double* h64, float* h32);
int ls_resample(int device, const ls_resample_args* a);
int ls_resample_stream_open(int device, int32_t capacity, int32_t in_sr, int32_t out_sr, int32_t channels, int32_t dtype, int32_t zeros,
                            double beta, double rolloff, int32_t max_chunk, ls_resample_stream** out);
int ls_resample_stream_push(ls_resample_stream* h, const ls_resample_stream_push_args* a);
int ls_resample_stream_reset(ls_resample_stream* h, int32_t slot);
/* samples_in, outputs_done [capacity] (nullable): each slot's input frames and outputs so far */
int ls_resample_stream_info(const ls_resample_stream* h, int64_t* samples_in, int64_t* outputs_done, int64_t* device_bytes);
void ls_resample_stream_close(ls_resample_stream* h);
const char* ls_resample_stream_last_error(const ls_resample_stream* h);

/* ---- dataset ingest: recorded poses and audio -> model inputs ----------------------------------------------
 * The forward direction of the pose transforms above, as the reference's offline pipeline computes it: TED
 * DataPreprocessor._sample_from_clip (scripts/data_loader/data_preprocessor.py:69-167) with resample_pose_seq,
 * convert_pose_seq_to_dir_vec and make_audio_fixed_length (scripts/utils/data_utils.py:46-120), MotionPreprocessor
 * (data_loader/motion_preprocessor.py) and the clipping of SpeechMotionDataset.__getitem__ (lmdb_data_loader.py:166-174); BEAT
 * CustomDataset._sample_from_clip (scripts_beat/dataloaders/beat.py:365-485) and scripts_beat/data_libs/process_cache.py:38-45.
 * A batch of recordings of different lengths goes in as concatenated arrays; every window comes out in the layouts the other entry
 * points take.  The plan is host-only and exact (double); the kernels read nothing beyond a recording's own frames and samples. */
#define LS_INGEST_PASS 0          /* verdicts, MotionPreprocessor's filtering_message */
#define LS_INGEST_POSE 1          /* "pose": mean |pose - mean_pose| < 0.02                                   */
#define LS_INGEST_SPINE 2         /* "spine angle": max > 30 degrees or mean > 20 degrees                     */
#define LS_INGEST_MOTION 3        /* "motion": both wrist variances < 0.0014                                  */
#define LS_INGEST_WORDS 4         /* fewer than two words in the window; the filter is then never evaluated   */
#define LS_INGEST_MAX_POSES 64    /* n_poses at most                                                          */
#define LS_INGEST_MAX_EXT 128     /* n_ext at most                                                            */
#define LS_INGEST_N_STATS 5       /* pose difference, spine max, spine mean (degrees), left and right wrist variance */
typedef struct ls_ingest_plan_args {
    int32_t batch;
    int32_t n_poses;            /* 34: frames of a sample                                                              */
    int32_t n_ext;              /* frames of a window: int(round(n_poses * 1.25)) = 42 for TED, n_poses for BEAT       */
    int32_t stride;             /* 10                                                                                  */
    int32_t beat;               /* 0: the TED arithmetic, 1: BEAT's (no resampling; times are whole seconds)           */
    int32_t frame_cap, window_cap; /* rows the frame and window arrays hold; 0 with NULL arrays asks for the counts alone */
    int32_t n_frames, n_windows;   /* OUT: rows of the two tables                                                      */
    int32_t reserved;
    double fps;                 /* 15                                                                                  */
    double sr;                  /* 16000                                                                               */
    const int32_t* n_raw;       /* [B] raw frames of each recording (>= 2)                                             */
    const double* start_time;   /* [B] seconds; BEAT: clip_s_t = clean_first_seconds                                   */
    const double* end_time;     /* [B] seconds; BEAT: clip_e_t = round_seconds - clean_final_seconds                   */
    const int64_t* audio_len;   /* [B] samples                                                                         */
    const int64_t* word_offsets;/* [B + 1] or NULL: rows of word_times of each recording; NULL: every window has words */
    const double* word_times;   /* [n_words][2] (start, end), sorted by start within a recording                       */
    int32_t* frame_offsets;     /* OUT [B + 1]: first row of each recording's resampled frames                         */
    int32_t* frame_clip;        /* OUT [n_frames]                                                                      */
    int32_t* frame_lo;          /* OUT [n_frames] raw frame below, within the recording                                */
    int32_t* frame_hi;          /* OUT [n_frames] lo + 1                                                               */
    float* frame_frac;          /* OUT [n_frames] x_new - lo, rounded to float once; 1 at whole positions, > 1 in the extrapolated tail */
    int32_t* window_offsets;    /* OUT [B + 1]                                                                         */
    int32_t* win_clip;          /* OUT [n_windows]                                                                     */
    int32_t* win_first;         /* OUT [n_windows] first frame within the recording (TED: resampled frames; BEAT: raw) */
    int64_t* win_audio_start;   /* OUT [n_windows] first sample within the recording                                   */
    int32_t* win_n_pad;         /* OUT [n_windows] samples np.pad(mode='symmetric') would append                       */
    unsigned char* win_has_words; /* OUT [n_windows] get_words_in_time_range found at least 2                          */
} ls_ingest_plan_args;
/* TED: the frame table restates np.arange(0, n, n / (duration * fps)) (length ceil(n / step), values i * step) and interp1d(
 * kind='linear', fill_value='extrapolate') (searchsorted left, clipped to [1, n - 1]); per recording floor((K - n_ext) / stride) + 1
 * windows (none for K < n_ext), audio_start = floor(start_idx / K * L), window length int(n_ext / fps * sr).  BEAT: beat.py:364-372,
 * 392-395.  Any OUT array may be NULL.  LS_EINVAL: a NULL input, batch < 1, n_poses outside [1, 64], n_ext outside [n_poses, 128],
 * stride < 1, fps or sr <= 0, n_raw < 2, end_time <= start_time (TED), a BEAT clip beyond its recording, an empty audio, a padding longer than the audio itself, unsorted
 * word offsets, a cap below the count when the arrays are given.  No device is touched. */
int ls_ingest_plan(ls_ingest_plan_args* a);

typedef struct ls_ted_ingest_args {
    int32_t batch, on_device;
    int32_t n_poses, n_ext;
    int32_t n_frames, n_windows;   /* rows of the plan's tables                                                        */
    int32_t audio_out_len;         /* int(round(n_poses / fps * sr)) = 36267                                           */
    int32_t reserved;
    const ls_post_config* cfg;     /* the bone table and mean_dir_vec; njoints 9 and n_pose_joints 10                  */
    const float* mean_pose;        /* [30], host                                                                       */
    /* the plan: host arrays in both modes */
    const int32_t* n_raw;
    const int64_t* audio_len;
    const int32_t* frame_offsets;
    const int32_t* frame_clip;
    const int32_t* frame_lo;
    const int32_t* frame_hi;
    const float* frame_frac;
    const int32_t* win_clip;
    const int32_t* win_first;
    const int64_t* win_audio_start;
    const unsigned char* win_has_words;
    /* the recordings, concatenated: device pointers iff on_device */
    const float* raw_poses;        /* [sum n_raw][10][3]                                                               */
    const float* audio;            /* [sum audio_len]                                                                  */
    /* outputs, device pointers iff on_device; any may be NULL */
    float* resampled;              /* [n_frames][30]                                                                   */
    float* dir_vec;                /* [n_frames][27] unit bone directions                                              */
    float* pose_seq;               /* [n_windows][n_poses][30]                                                         */
    float* vec_seq;                /* [n_windows][n_poses][27] directions minus mean_dir_vec                           */
    float* x;                      /* [n_windows][9][3][n_poses], the model's layout                                   */
    float* audio_out;              /* [n_windows][audio_out_len]                                                       */
    float* stats;                  /* [n_windows][LS_INGEST_N_STATS], over the window's n_ext frames                   */
    int32_t* verdict;              /* [n_windows] LS_INGEST_*                                                          */
} ls_ted_ingest_args;
/* The tables are checked on the host before anything is launched (LS_EINVAL): every frame row and window must lie inside its
 * recording, and the symmetric padding inside its audio.  n_windows == 0 or n_frames == 0 is legal. */
int ls_ted_ingest(int device, const ls_ted_ingest_args* a);

typedef struct ls_beat_ingest_args {
    int32_t batch, on_device;
    int32_t n_poses;               /* 1 .. 34                                                                          */
    int32_t njoints;               /* 1 .. 47                                                                          */
    int32_t n_windows;
    int32_t audio_out_len;         /* floor(n_poses / fps * sr) = 36266                                                */
    const float* mean_pose;        /* [njoints * 3] degrees, host                                                      */
    const float* std_pose;         /* [njoints * 3], host                                                              */
    const int32_t* n_raw;          /* host, like the window table                                                      */
    const int64_t* audio_len;
    const int32_t* win_clip;
    const int32_t* win_first;
    const int64_t* win_audio_start;
    const unsigned char* win_has_words;  /* the caller's per-window byte: 0 gives LS_INGEST_WORDS; NULL keeps every window */
    const float* poses;            /* [sum n_raw][njoints * 3] normalised Euler angles; device pointer iff on_device   */
    const float* audio;            /* [sum audio_len]                                                                  */
    float* rot6d;                  /* [n_windows][n_poses][njoints * 6]                                                */
    float* x;                      /* [n_windows][njoints][6][n_poses]                                                 */
    float* audio_out;              /* [n_windows][audio_out_len]                                                       */
    int32_t* verdict;              /* [n_windows] LS_INGEST_PASS or LS_INGEST_WORDS                                    */
} ls_beat_ingest_args;
int ls_beat_ingest(int device, const ls_beat_ingest_args* a);

/* ---- training step ----------------------------------------------------------------
 * One optimisation step of the RAG denoiser as TrainLoop.run_step runs it (scripts/train_utils/train_loop.py:146-186):
 *   x_t = q_sample(x_start, t, noise)                                  gaussian_diffusion.py:1281-1282
 *   out = RAG.forward(x_t, t, y) in training mode (mask_cond dropout)  scripts/model/RAG.py:79-133
 *   loss = huber(x_start, out) + lambda_vel * huber(velocities) + kld_weight * KLD(z_mu, z_logvar)
 *                                                                      gaussian_diffusion.py:1347-1396, train_loop.py:178
 *   backward through every parameter, then torch.optim.AdamW           train_loop.py:57-59, fp16_util.py:183-187
 * The trainer owns fp32 master parameters, gradients and Adam moments as FLAT device arrays with one layout
 * (ls_train_param_info); gradients are written to a caller-provided device array so that a data-parallel caller can
 * all-reduce it (RCCL) between ls_train_forward_backward and ls_train_adamw.  Random draws are inputs, in the
 * reference's order: t, noise = randn_like(x_start), drop = bernoulli(cond_mask_prob) [B], eps = randn_like(z_mu). */
typedef struct ls_trainer ls_trainer;
typedef struct ls_train_config {
    ls_config model;
    float lambda_vel;         /* 1.0  (parser_util.py:109)            */
    float kld_weight;         /* 0.01 (train_loop.py:178)             */
    int32_t diffusion_steps;  /* length of the q_sample tables        */
    int32_t reserved;
} ls_train_config;
typedef struct ls_train_batch {
    int32_t batch;
    int32_t on_device;            /* 1: tensor pointers below are device pointers (t stays a HOST pointer) */
    const float* x_start;         /* [B,J,F,T] motion                                            */
    const int64_t* t;             /* [B] HOST: diffusion timestep per sample (schedule_sampler)  */
    const float* noise;           /* [B,J,F,T]                                                   */
    const float* drop;            /* [B] 1.0 = drop the audio condition for this sample          */
    const float* eps;             /* [B,512]                                                     */
    const float* audio_input;     /* [B,audio_len]                                               */
    const float* origin_x;        /* [B,J,F,T]                                                   */
    const int64_t* vid_indices;   /* [B]                                                         */
    const int64_t* emo;           /* [B,T] or NULL (TED)                                         */
} ls_train_batch;
typedef struct ls_train_terms { float rot_mse, vel_mse, kld, loss, total; float fwd_ms, bwd_ms, reserved; } ls_train_terms;

int ls_train_create(const ls_train_config* cfg, ls_trainer** out);
void ls_train_destroy(ls_trainer* h);
const char* ls_train_last_error(const ls_trainer* h);
/* q_sample tables of GaussianDiffusion.__init__ (fp64, diffusion_steps entries) and _WrappedModel's timestep map */
int ls_train_set_schedule(ls_trainer* h, const double* sqrt_alphas_cumprod, const double* sqrt_one_minus_alphas_cumprod,
                          const int64_t* timestep_map);
/* parameter table: reference state-dict key, offset and element count inside the flat arrays */
int ls_train_param_count(const ls_trainer* h);
int64_t ls_train_flat_size(const ls_trainer* h);
int ls_train_param_info(const ls_trainer* h, int index, char* key, size_t key_cap, int64_t* offset, int64_t* numel);
int ls_train_set_weight(ls_trainer* h, const char* key, const float* data, size_t n);   /* host -> master params   */
int ls_train_get_weight(ls_trainer* h, const char* key, float* out, size_t n);           /* master params -> host   */
/* optimizer state for checkpoint / resume (opt%09d.pt, train_loop.py:222-227): which = 1 exp_avg, 2 exp_avg_sq */
int ls_train_get_moment(ls_trainer* h, int which, const char* key, float* out, size_t n);
int ls_train_set_moment(ls_trainer* h, int which, const char* key, const float* data, size_t n);
int64_t ls_train_get_step(const ls_trainer* h);
int ls_train_set_step(ls_trainer* h, int64_t step);
/* forward + loss + backward; grad: DEVICE array of ls_train_flat_size floats, overwritten */
int ls_train_forward_backward(ls_trainer* h, const ls_train_batch* b, float* grad, ls_train_terms* terms);
/* AdamW on the master parameters from a DEVICE gradient array; the step counter is the trainer's (starts at 1) */
int ls_train_adamw(ls_trainer* h, const float* grad, float lr, float beta1, float beta2, float eps, float weight_decay);
/* debug / test access to a named internal tensor of the last forward ("out" [B,T,JF], "x_t", "audio_feat" ...) */
int ls_train_read(ls_trainer* h, const char* what, float* out, size_t n);
void* ls_train_stream(const ls_trainer* h);

/* ---- FGD feature extractor -------------------------------------------------------
 * EmbeddingNet(...).pose_encoder in eval mode: poses [B, n_frames, pose_dim] -> latent mean [B, base]
 * (scripts/model/embedding_net.py:41-83, 261-270; BEAT HalfEmbeddingNet scripts_beat/model/motion_autoencoder.py:38-73,
 * 156-167).  Keys are the auto-encoder checkpoint's ('gen_dict'): pose_encoder.* are used, decoder.* / fc_logvar are
 * accepted and ignored.  Frechet distance / diversity on the features stay host code (ted_evaluator.py:61-152). */
typedef struct ls_eval ls_eval;
typedef struct ls_eval_config {
    int32_t pose_dim;   /* 27 TED                                   */
    int32_t n_frames;   /* 34                                       */
    int32_t base;       /* latent size: 32 TED | vae_length BEAT    */
    int32_t hidden1;    /* out_net widths: 256, 128 TED | 4*base, 2*base BEAT */
    int32_t hidden2;
    int32_t device;
} ls_eval_config;
int ls_eval_create(const ls_eval_config* cfg, ls_eval** out);
void ls_eval_destroy(ls_eval* h);
const char* ls_eval_last_error(const ls_eval* h);
int ls_eval_set_weight(ls_eval* h, const char* key, const float* data, size_t n);
int ls_eval_commit_weights(ls_eval* h);
int ls_eval_features(ls_eval* h, int batch, int on_device, const float* poses, float* feat);
void* ls_eval_stream(const ls_eval* h);

#ifdef __cplusplus
}
#endif
#endif /* LS_HIP_H */
