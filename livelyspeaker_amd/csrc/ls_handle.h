// Host-only declarations shared by the translation units behind the sampling ABI of include/ls_hip.h (ls_api.cpp: handle, weight commit,
// schedule, preparation -- the weight images themselves are built by ls_weights.cpp, which sees neither HIP nor this header; ls_plan.cpp: the step plan and the step launchers; ls_sample.cpp: the diffusion loop and the single-step
// entries; ls_chain_api.cpp: the chained windows of the long-form entries): the handle, copies between caller and internal buffers, and the guard of buffers a captured loop holds by address.
// The device buffer (DevBuf) and the error path (fail, HIPCHK) are those of every handle: ls_host.h.
#pragma once
#include "ls_hip.h"
#include "ls_host.h"
#include "ls_internal.h"

#include <map>
#include <string>
#include <vector>

namespace ls {

// one piece of a step plan: samples [first, first + n) of the prepared batch on one kernel family
// (0 fused: one workgroup per sample, 1 batch-level kernels, 2 sample-split kernel, 3 one workgroup per (sample, pass))
struct Seg { int path, first, n; };

}  // namespace ls
using ls::DevBuf; using ls::Seg;

struct ls_handle {
    ls_config cfg{};
    ls::Variant var = ls::kTED;
    int JF = 0, S = 0, R = 0, NOB = 0, KXQ = 0, MK = 0, KIN = 0;
    int T = ls::kT;             // frames; 34 = the reference's (fused step kernel), anything else = the long-sequence path (ls_long.hip)
    bool fused = true;      // the model HAS the fused kernel (34 frames)
    bool use_long = false;  // the prepared batch runs the batch-level kernels (always when !fused; small batches of a fused model)
    int path_mode = 0;      // ls_set_path: 0 auto, 1 one workgroup per sample (fused kernel), 2 batch-level kernels, 3 sample-split kernel, 4 one workgroup per (sample, pass)
    DevBuf pa_out, pa_cnt;  // CFG hand-off of the one-pass-per-workgroup kernel (ls_pass_kernel.h: two independent workgroups per CU): pass outputs [n][2][T][J*F], arrival tickets [n]
    int pass_n = 0;         // samples the hand-off buffers hold
    int pass_waves = 0;     // 0: 8-wave workgroups when the grid fits the chip once, 4-wave otherwise; 4: ls_set_path(5) forces the 4-wave form
    int pass_waves_env = 0; // LS_PASS_WAVES = 4 | 8 forces one (-DLS_DEBUG builds only)
    // the step plan of the prepared batch (decide_path): up to three pieces, e.g. 416 clips = 256 on the fused kernel + 128 on the
    // one-pass-per-workgroup kernel (one workgroup per CU) + 32 on the sample-split kernel (ls_coop_kernel.h: 16 workgroups per sample).
    int nseg = 1;
    Seg seg[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    bool plan_pair = false; // the plan assumed the single-pass form (every guidance scale 1)
    DevBuf wtok1_img;       // token-mix operand of one pass (sample-split kernel)
    DevBuf wtail;           // [L][S][4] token-mix weights of the ragged output rows 32 .. 35 (one-pass-per-workgroup kernel)
    DevBuf wtok1_hi_img, wtok1_lo_img;   // the same as bf16 hi / lo planes (one-pass-per-workgroup kernel, bf16x3)
    DevBuf co_x, co_part, co_gran, co_flag, co_err;      // its exchange workspaces (one launch's worth), granules / flags, timeout word
    unsigned coop_launches = 0;                        // launches since the granule words were zeroed: epoch = 64 * ordinal
    int n_cu = 256;         // compute units of the device (hipDeviceProp.multiProcessorCount): residency of the sample-split kernel, round sizes of the plans
    int max_thr_cu = 2048;  // hipDeviceProp.maxThreadsPerMultiProcessor: with n_cu, the geometry of torch's randn launches (LS_NOISE_TORCH_DEVICE)
    int coop_groups_max = ls::kCoopMaxGroups, coop_groups = 0;   // (sample, pass) groups per launch: cap of the 8-slice form (two workgroups per CU, eight per group), and what the workspaces hold
    int coop_ncb = 0;       // slicing of the sample-split kernel: 0 = by the step-time model; 1 | 2 | 4 = 8 | 4 | 2 slice workgroups per (sample, pass) (ls_set_path 8 | 6 | 7)
#ifndef LS_MIX_POSE_DEFAULT
#define LS_MIX_POSE_DEFAULT 1
#endif
#ifndef LS_COOP_XMAP_DEFAULT
#define LS_COOP_XMAP_DEFAULT -1
#endif
    int coop_xmap = LS_COOP_XMAP_DEFAULT;      // -1: by grid size (run_coop); otherwise the blockIdx -> (group, slice) mapping of the sample-split kernel (speed only; LS_COOP_XMAP in -DLS_DEBUG builds)
    int tokpad = 160;       // token axis of lw_wtp
    int JFP = 0;            // JF padded to a multiple of 32 (long path: K of the x_t projection)
    DevBuf lw_wt, lw_wtp, lw_bt, lw_wc, lw_bc, lw_wcf, lw_bcf, lw_wsum, lw_winx, lw_wout;     // long path: row-major weights (wtp: Wt zero-padded to 160 x 160 in k_long_tokmix's per-lane fragment order)
    DevBuf mx_wtok, mx_wch, mx_wpose, mx_pout, mx_xg, mx_gran;             // long-sequence mixer kernel (ls_mix_kernel.h): operand images, exchange workspace, granules
    bool mix_pose = LS_MIX_POSE_DEFAULT;                            // env LS_MIX_POSE=0: poseFinal as a GEMM behind the mixer (A/B runs)
    int mx_npt = 0;                                     // 16-column tiles of poseFinal inside the mixer; 0: poseFinal stays a GEMM
    int mix_cap = 0;                                    // (sample, pass) groups per mixer launch; 0: the model has no such kernel (or ls_set_path(2) asked for the batch-level kernels)
    DevBuf lx_proj, lx_X, lx_U, lx_OUT, lx_part1, lx_part2, lx_xpad;   // long path: workspaces (xpad: x_t rows padded to whole GEMM tiles)
    int convL[5] = {0, 0, 0, 0, 0};
    hipStream_t stream = nullptr;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};     // [0..3] sample / step timing, [4..5] ls_prepare, [6] host-input copies of ls_prepare_async
    // segmented TAPE mode (ls_sample_args.seg_count > 0): tapes arrive in pieces, uploaded on a second stream into two device slots
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_cs[2] = {nullptr, nullptr}, ev_cd[2] = {nullptr, nullptr}, ev_seg[2] = {nullptr, nullptr};   // upload start / done, steps done (per slot)
    bool slot_used[2] = {false, false}, upload_open[2] = {false, false};
    int seg_next = -1, seg_index = 0, seg_skip = 0, seg_sampler = 0;
    float seg_upload_ms = 0.f;
    bool prepare_pending = false;                                                  // ls_prepare_async enqueued, prepare_ms not read back yet
    std::string err;

    std::map<std::string, std::vector<float>> w;   // host copies under the reference's state-dict keys
    bool committed = false;
    unsigned weights_version = 0;

    // device weights
    DevBuf wch_hi_img, wch_lo_img, wch_lo2_img, ww_hi_img, ww_lo_img;
    DevBuf wch_img, bch, ln1a, ln1b, ln2a, ln2b, ww_img, btok_rows, winx_img, wout_img, wout_reg_img, bout, devw;
    DevBuf conv_img[4];     // MFMA operand images of the stride-6 conv layers (ls_conv.hip)
    DevBuf conv_w[4], conv_b[4], win_pre, win_aud, win_bias, spk_emb, ml_w, ml_b, emo_emb;
    int KPP = 0;            // prefix-pose + bit columns of input_mapping, padded to the GEMM's K tile
    DevBuf te_w0, te_b0, te_w2, te_b2, pe;

    // schedule
    bool have_sched = false;
    unsigned sched_version = 0;
    int n_steps = 0;
    std::vector<long long> tmap;
    std::vector<double> t_sac, t_s1mac, t_c1, t_c2, t_plv, t_ac, t_acp, t_srac, t_srm1ac;
    DevBuf temb, temb_tmp, tmap_dev;
    bool temb_valid = false;

    // per-call state
    int B = 0;              // prepared batch
    bool prepared = false;
    bool all_scale_one = false;   // every y['scale'] == 1: the CFG combination equals the cond output -> single-pass kernel
    DevBuf audio, origin_x, vid, emo, scale;
    DevBuf c1, c2, c3, c4, st1, st2, st3, feat_c, feat_u, static_c, static_u, z, z_ml, z_mu, z_logvar, z_std, emo_tok;
    DevBuf audio_feat, spart;
    DevBuf xa, xb, xtmp, xio, fwd_c, fwd_u, fwd_cfg, eps, noise, tfwd, tfwd_tmp, tidx, dump, trace, callp;
    DevBuf eps_tape, noise_tape;
    DevBuf inp_m8, inp_maskf, inp_motion, inp_tape;     // inpainting branch: mask bytes / mask as 0-1 floats and motion in the internal layout, q_sample noise tape
    DevBuf eps_slot[2], noise_slot[2], coef;
    DevBuf plms_buf;        // LS_SAMPLER_PLMS: five planes [B][T][JF] (each padded to whole 16-byte groups): a ring of four eps planes (step k
                            // writes plane k & 3 and reads the up to three before it) + mean_pred of the two-evaluation first step
    // LS_NOISE_TORCH_DEVICE: a ring of K steps' draws (eps [K][2][B][D], noise [K][B][J][F][T], inpainting re-noise [K][B][J][F][T]),
    // refilled by one generator launch per K steps inside the loop; K = what fits in trng_ring_bytes (ls_set_torch_ring_bytes)
    DevBuf trng_eps, trng_noise, trng_inz;
    size_t trng_ring_bytes = (size_t)256 << 20;
    // Philox keyed per row (ls_philox_rows.hip): row_gidx [n] uint64 on the device, the gidx every stream of row b draws at; a keyed
    // loop holds its address and fills the ring above from it.  rk_n: rows ls_set_row_keys set for ls_sample (0: none).  A keyed
    // session pool (pl_keyed) rewrites the table ahead of every round from pl_key [S], the slots' keys.
    DevBuf row_gidx;
    int rk_n = 0;
    // ls_bpd / ls_vb_terms: x_start, the column's q_sample noise and x_t (internal layout), the noise tape in the internal layout, the
    // per-index coefficient table of k_vb_terms (built for schedule bpd_coef_version) and the [3][B][n_steps] results
    DevBuf bpd_x0, bpd_nz, bpd_xt, bpd_tape, bpd_coef, bpd_out;
    unsigned bpd_coef_version = 0;
    bool bpd_coef_valid = false;
    std::string coef_key;   // (sampler, eta, schedule) the per-index coefficient table `coef` was built for

    // long-form synthesis (ls_chain_api.cpp: ls_long_prepare / ls_long_sample): lg_W chained windows of the prepared batch.  The zero-padded waveform [B][lg_L]
    // and one encoder chunk's clip-windows [chunk][audio_len]; per-call stores of the windows' audio features [W][B][T][256] and emotion
    // tokens [W][B][512]; the seed poses [B][JF][n_pre]; the call's tapes, text features, SAG output and outputs when the caller's are host memory
    int lg_W = 0;
    size_t lg_L = 0;
    bool lg_prepared = false;
    DevBuf lg_audio, lg_clips, lg_featc, lg_featp, lg_emo_ids, lg_emotok, lg_seed;
    DevBuf lg_x, lg_eps, lg_nz, lg_text, lg_init, lg_mask, lg_timeline, lg_windows;
    DevBuf lg_inz, lg_edit_range, lg_edit_chan;     // ls_long_edit: a host caller's re-noise tape; per clip [lo, hi) int32 [B][2] and the channel bytes [B][JF]
    DevBuf lg_edit_mask, lg_edit_flags, lg_edit_frames;     // an edit by element mask: a host caller's mask [B][JF][T_total], the pair flags [W][B] of k_edit_mask_pairs and the clips' frames [B]
    DevBuf lg_sag;          // ls_long_edit_sag: the SAG decoder's output [B][JF][T] of the window in flight (k_edit_start reads it)
    // a ragged long-form call (ls_long_prepare_ragged): clips held longest-first.  lg_bw[w] clips run window w (slots [0, lg_bw[w]) of
    // every per-clip buffer), lg_off[w] = sum of lg_bw[v], v < w, is window w's offset in the packed stores (lg_featc, the tapes);
    // lg_row [B] on the device maps slot -> the caller's clip; lg_scale_ones = leading slots whose guidance scale is 1.
    bool lg_ragged = false;
    std::vector<int> lg_bw, lg_off;
    int lg_scale_ones = 0;
    DevBuf lg_row, lg_table, lg_lens;
    // a compact timeline edit (ls_long_prepare_edit -> ls_long_edit_compact): clips in the caller's order.  The plan of
    // ls_long_edit_plan_compact: window lg_cw[e] runs the lg_cn[e] clips lg_crows[lg_coff[e] ..], and lg_coff[e] is its offset in the
    // packed stores (lg_featc, the tapes, the raw windows); lg_crows_dev holds the row tables on the device.  The arguments the plan
    // was made from (lg_clo / lg_chi as given, lg_cchan folded to 0 / 1; empty: every channel), which the edit must repeat.  The held
    // per-clip conditioning: lg_cvid / lg_cscale_dev [B], the scales on the host (a window's single-pass decision), the emotion
    // tokens in lg_emotok [W][B][512]; lg_ctext [B][512]: the text features of the window in flight, by row.
    bool lg_compact = false;
    std::vector<int32_t> lg_cw, lg_cn, lg_coff, lg_crows, lg_clo, lg_chi;
    std::vector<unsigned char> lg_cchan;
    // ... or, prepared by ls_long_prepare_edit_mask, the pair flags [W][B] of its mask (lg_clo / lg_chi / lg_cchan empty), which the
    // flags of the run's mask must repeat, and the clips' frames the flags were made with (empty: every clip has all W windows)
    std::vector<unsigned char> lg_cflags;
    std::vector<int32_t> lg_cframes;
    std::vector<float> lg_cscale;
    DevBuf lg_crows_dev, lg_cvid, lg_cscale_dev, lg_ctext;
    // Streaming sessions (ls_long_pool_open / _join / _push; ls_long_stream_open / _push): pl_S slots, each a stream of its own.  Per
    // slot on the device: the ring pl_ring [S][pl_R] (sample n of the slot at n % pl_R; the samples below audio_stride * pl_windows[s]
    // are dead), the hand-off poses pl_hand [S][JF][n_pre] (seed poses until the slot's window 0 has run), the held conditioning pl_vid /
    // pl_scale / pl_emotok [S][512] / pl_text [S][512]; per slot on the host: the counters, the scale and what is held.  A round gathers
    // its active slots into rows [0, A) of lg_clips, feat_u, origin_x, vid, scale, emo_tok and pl_ctext (k_pool_gather) by pl_table
    // [S][kPoolRow].  pl_state: kStreamNone, kStreamOpen, or why the session ended.  pl_rounds: rounds run since open (the PHILOX window
    // index).  pl_lockstep: the session was opened by ls_long_stream_open -- every slot joined there, all fed and closed together by
    // ls_long_stream_push; kLockstepClosed once its closing push has run.  pl_styled: the slots of the round prepare_style last ran for
    // (emptied by a join of one of them): a round of the same slots finds its speaker style in place.
    enum { kStreamNone = 0, kStreamOpen, kStreamReplaced, kStreamFailed };
    enum { kPool = 0, kLockstep, kLockstepClosed };
    int pl_state = kStreamNone, pl_lockstep = kPool;
    int pl_S = 0, pl_R = 0;
    long long pl_rounds = 0;
    std::vector<long long> pl_samples, pl_windows, pl_frames;
    std::vector<float> pl_scale_host;
    std::vector<char> pl_open, pl_have_emo, pl_have_text;
    std::vector<int32_t> pl_styled;
    bool pl_keyed = false;              // ls_long_pool_keyed: PHILOX draws at pl_key[slot] + (the slot's own window << 48)
    long long pl_joins = 0;             // joins since open: a keyed slot's default key
    std::vector<uint64_t> pl_key;
    DevBuf pl_ring, pl_hand, pl_vid, pl_scale, pl_emo_id, pl_emotok, pl_text, pl_ctext, pl_table;
    // Pinned poses of frames a slot has yet to return (ls_long_pool_pins / _pin / _unpin).  pl_pin_P == 0: the session has none and
    // holds nothing of the following.  Otherwise per slot a ring of pl_pin_P series frames, frame n at n % pl_pin_P: the values
    // pl_pin_val [S][P][JF] and one byte per element pl_pin_bit [S][P][JF] (1 = pinned).  pl_pin_frames [S]: the pending pinned frames
    // of each slot, ascending -- the host mirror the plan is made from (ls_long_pool_pin_plan); a frame leaves it when the window that
    // owns it has run (k_pool_pin_gather cleared its bytes), at ls_long_pool_unpin, and when its slot leaves or is joined.
    // pl_pin_poses / pl_pin_mask / pl_pin_pos: staging of one ls_long_pool_pin call (a host caller's arrays; the ring positions).
    // pl_pin_tape: the re-noise tape the next push's pinned calls read (ls_long_pool_pin_tape), taken by that push.
    int pl_pin_H = 0, pl_pin_P = 0;
    std::vector<std::vector<long long>> pl_pin_frames;
    DevBuf pl_pin_val, pl_pin_bit, pl_pin_poses, pl_pin_mask, pl_pin_pos;
    const float* pl_pin_tape = nullptr;
    long long pl_pin_tape_floats = 0;
    int pl_pin_tape_od = 0;
    // Cached graphs of the step loop, by loop key (ls_sample.cpp: loop_key holds everything a captured loop bakes in besides device
    // addresses, the batch and its step plan included).  At most kGraphCacheMax entries: a plain call whose key is missing drops them
    // all and captures its own (one entry, as before the cache); a ragged long-form call keeps one per window batch that serves two or
    // more windows, and never evicts while its own launches are in flight -- a key that does not fit runs as stream launches.
    // coop_launches: the sample-split launches the captured loop makes (a replay does not run the code that counts them).
    static constexpr int kGraphCacheMax = 8;
    struct CachedGraph { std::string key; hipGraph_t graph; hipGraphExec_t exec; unsigned coop_launches; };
    std::vector<CachedGraph> graphs;
    std::vector<int> graphs_for;      // the window batches (lg_bw) of the ragged call that last made room in the cache

    ls_timing timing{};
    ls::CallParams call_host{0, 0, 0, 0};
    unsigned tag_base = 0;  // sample-split kernel: base of the current call's hand-off tags (CallParams::tag_base)
    int precision = 0;      // LS_PRECISION_*: 0 fp32 (split-fp32 channel mixing in k_step), 1 bf16x3, 2 fp32 MFMA throughout (ls_set_precision)
#ifdef LS_DEBUG             // profiling variant of the library only (build_library(defines=['LS_DEBUG'])); never in the shipped .so
    DevBuf prof, wgt;       // wgt: [1024][2] start / end stamps of every workgroup of the last step launch
    bool prof_on = false;   // LS_PROF=<workgroup index>: in-kernel s_memtime phase stamps, read with ls_read("prof")
    int prof_wg = 0;
    int ablate = 0;         // LS_ABLATE (results are wrong when non-zero)
#endif
};

namespace ls {

// ---- defined in ls_api.cpp
int ensure_temb_table(ls_handle* h);
int build_temb_rows(ls_handle* h, const long long* idx_dev, int n, DevBuf& tmp, DevBuf& out);
void resolve_prepare_timing(ls_handle* h, bool block);
// the stages of ls_prepare that the long-form stages (ls_chain_api.cpp) run too, on the handle's stream
int prepare_scale(ls_handle* h, const float* scale, int B, int on_device, int* leading_ones = nullptr);     // leading_ones: clips ahead of the first scale != 1
int run_wav_encoder(ls_handle* h, const float* in, int B);
int prepare_style(ls_handle* h, int B);
int prepare_plan(ls_handle* h, int B);
int plan_workspaces(ls_handle* h);          // the workspaces of the CURRENT plan's kernel families (grow only; what prepare_plan does behind decide_path)
// ---- defined in ls_plan.cpp
int seg_n(const ls_handle* h, int path);
long long plan_code(const ls_handle* h);
int coop_cap(int n_cu, int ncb);
void decide_path(ls_handle* h);
void set_plan(ls_handle* h, int B);         // decide_path's plan for a batch of B, without touching the cached graphs (their keys hold the plan)
hipError_t run_step(ls_handle* h, StepArgs& s, int B, bool pair, hipStream_t st);
hipError_t coop_reset(ls_handle* h, hipStream_t st);
int advance_tags(ls_handle* h, hipStream_t st);
int coop_check(ls_handle* h, bool force = false);      // force: the call ran the sample-split kernel under a plan that is no longer current
void report_path(ls_handle* h, bool pair);
// ---- defined in ls_sample.cpp: what a chained window (ls_chain_api.cpp) runs of ls_sample
// What a loop whose key is not cached does to the graph cache: kReplace drops every cached graph and captures (every call but the ragged
// long-form one: the handle then holds one graph, as it always did); kKeep captures beside the others while the cache has room and runs
// stream launches when it has none; kReplayOnly never captures.  The last two never destroy a graph, so they are safe with replays in flight.
enum CachePolicy { kReplace, kKeep, kReplayOnly };
int check_sampler_args(ls_handle* h, const ls_sample_args* a);
// keyed: PHILOX rows draw at row_gidx (the caller wrote rows [0, B) in stream order) in place of sample_offset + b
int run_window_loop(ls_handle* h, const ls_sample_args* a, bool resident_inpaint, bool first, CachePolicy policy, int* graph_replayed, bool keyed = false);
// the ring of a keyed loop for batches up to B and loops up to n_exec steps, so that no loop at a smaller batch moves it;
// inp_noised: with the re-noise plane of the inpainting branch (a compact timeline edit of the TED tree)
int size_key_ring(ls_handle* h, int B, int n_exec, bool inp_noised = false);
inline float* x_plane(const ls_handle* h, int k) { return (k & 1) ? h->xb.f() : h->xa.f(); }      // x ahead of executed step k (xa / xb ping-pong)
// ---- defined in ls_chain_plan.cpp (host only): slot -> clip, windows per slot, clips per window of a ragged long-form call
void long_plan_drop(int B, int AL, const int64_t* lengths, std::vector<int>& row, std::vector<int>& wins, std::vector<int>& bw);
// ... the plan of a timeline edit from pair flags [W][B] (the one definition the range and the element-mask entries share), and the
// flags of a HOST element mask [B][JF][T + (W - 1)(T - n_pre)] (LS_EINVAL: a bad frames[b], a set byte at or beyond frames[b])
int edit_plan_of_flags(int B, int W, const unsigned char* flags, int32_t* windows, int32_t* counts, int32_t window_capacity, int32_t* rows,
                       int32_t row_capacity, int32_t* n_windows_run, int32_t* n_pairs);
int edit_mask_flags(int B, int W, int T, int n_pre, int JF, const unsigned char* mask, const int32_t* frames, std::vector<unsigned char>& flags);
// ... and the strided copies that feed a session's rings, five ints each: first slot, slots, ring position, offset into the take, samples
void feed_copies(int S, int R, const int* pos, const long long* from, const int* take, std::vector<int>& copies);

// copy a caller buffer (host or device) into an internal device buffer
inline int ingest(ls_handle* h, DevBuf& d, const void* src, size_t bytes, int on_device) {
    HIPCHK(h, d.ensure(bytes ? bytes : 4));
    if (bytes) HIPCHK(h, hipMemcpyAsync(d.p, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return LS_OK;
}
// the same from a host temporary: finished before it dies
inline int upload(ls_handle* h, DevBuf& d, const void* src, size_t bytes) {
    const int rc = ingest(h, d, src, bytes, 0);
    if (rc == LS_OK && bytes) HIPCHK(h, hipStreamSynchronize(h->stream));
    return rc;
}
inline int egress(ls_handle* h, void* dst, const void* src, size_t bytes, int on_device) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return LS_OK;
}

// a call that replaces the handle's prepared conditioning ends a running session, stream or pool (its next push reports LS_ESTATE)
inline void end_stream(ls_handle* h) {
    if (h->pl_state == ls_handle::kStreamOpen) h->pl_state = ls_handle::kStreamReplaced;
}
inline void end_chain(ls_handle* h) { h->lg_prepared = h->lg_compact = false; end_stream(h); }      // ls_prepare: a long-form call's conditioning goes too

inline void free_graph(ls_handle* h) {        // every cached graph: whatever invalidates one invalidates all
    for (auto& g : h->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    h->graphs.clear();
    h->graphs_for.clear();
}

// A captured loop holds raw device addresses.  Every buffer its launches can read or write grows through here: a buffer that moved
// drops the graph, so a replay never runs against freed memory.  *moved (optional): the memory is fresh.
inline int ensure_pinned(ls_handle* h, DevBuf& d, size_t bytes, bool* moved = nullptr) {
    const void* const was = d.p;
    HIPCHK(h, d.ensure(bytes));
    if (moved) *moved = was != d.p;
    if (was != d.p) free_graph(h);
    return LS_OK;
}
inline int ingest_pinned(ls_handle* h, DevBuf& d, const void* src, size_t bytes, int on_device) {
    const int rc = ensure_pinned(h, d, bytes ? bytes : 4);
    return rc != LS_OK ? rc : ingest(h, d, src, bytes, on_device);
}

// a caller tensor [B][J][F][T] -> the internal layout [B][T][JF] at dst (through xio), and back (through `stage`, xio unless given)
inline int ingest_internal(ls_handle* h, const float* src, float* dst, int B, int on_device) {
    const int rc = ingest(h, h->xio, src, (size_t)B * h->JF * h->T * sizeof(float), on_device);
    if (rc != LS_OK) return rc;
    HIPCHK(h, launch_to_internal(h->xio.f(), dst, B, h->JF, h->stream, h->T));
    return LS_OK;
}
inline int egress_internal(ls_handle* h, const float* src, float* dst, int B, int on_device, float* stage = nullptr) {
    if (!stage) stage = h->xio.f();
    HIPCHK(h, launch_from_internal(src, stage, B, h->JF, h->stream, h->T));
    return egress(h, dst, stage, (size_t)B * h->JF * h->T * sizeof(float), on_device);
}

// the cond / uncond pair of style eps of one model evaluation -> dst[0 .. B*kD), dst[B*kD .. 2*B*kD)
inline int ingest_eps_pair(ls_handle* h, float* dst, const float* eps_cond, const float* eps_uncond, int on_device) {
    const size_t ne = (size_t)h->B * kD;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPCHK(h, hipMemcpyAsync(dst, eps_cond, ne * sizeof(float), kind, h->stream));
    HIPCHK(h, hipMemcpyAsync(dst + ne, eps_uncond, ne * sizeof(float), kind, h->stream));
    return LS_OK;
}

// the single-pass form of a step (two samples' cond pass per workgroup): legal when every guidance scale is 1
inline bool single_pass(const ls_handle* h, int two_pass_always) { return h->fused && !h->use_long && h->all_scale_one && !two_pass_always; }

// the tail of a single-step entry: wait and check, unless the caller keeps everything on the device and asked not to
inline int sync_and_check(ls_handle* h, int no_sync, int on_device) {
    if (no_sync && on_device) return LS_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return coop_check(h);
}

}  // namespace ls
