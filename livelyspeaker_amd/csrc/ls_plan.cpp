// The step plan of a prepared batch and the launchers that run one diffusion step on it: step-time models of the four kernel
// families, plan_steps / decide_path (ls_plan_query exposes the plan without a GPU), run_step, and the hand-off state of the
// sample-split and one-pass-per-workgroup kernels that every call resets around its launches.
#include "ls_handle.h"

using namespace ls;

namespace {

// Step time of the sample-split kernel in ms, measured on MI355X (profiles/r06_split_variants.md): per launch base + per (sample, pass)
// group, for ncb = 1 | 2 | 4; [0] TED, [1] BEAT.  `g` groups cost the sum over the launches it takes.
struct CoopCost { float base, per_group; };
// [dataset][ncb 1 with up to one workgroup per CU (the slices of a group on one XCD) | ncb 1 two per CU | ncb 2 | ncb 4]
constexpr CoopCost kCoopCost[2][4] = {{{0.0909f, 0.000213f}, {0.0875f, 0.00096f}, {0.1397f, 0.0000958f}, {0.2297f, 0.00000625f}},
                                      {{0.0987f, 0.00028f}, {0.0963f, 0.00103f}, {0.1511f, 0.000156f}, {0.2610f, 0.0000115f}}};
// one launch of `gl` groups
float coop_launch_ms(bool ted, int ncb, int gl, int n_cu) {
    const CoopCost& c = kCoopCost[ted ? 0 : 1][ncb == 1 ? (gl * 8 <= n_cu ? 0 : 1) : ncb == 2 ? 2 : 3];
    return c.base + c.per_group * gl;
}

// `g` groups in launches of ONE slicing
float coop_ms_ncb(bool ted, int ncb, int g, int n_cu) {
    const int cap = coop_cap(n_cu, ncb);
    if (cap < 1) return 1e30f;
    float ms = 0.f;
    for (; g > 0; g -= cap) ms += coop_launch_ms(ted, ncb, g < cap ? g : cap, n_cu);
    return ms;
}

// `g` groups in the cheapest SEQUENCE of launches, each with its own slicing (80 clips = 64 on two slices + 16 on eight): the model time and
// the slicing of the first launch.  Launches hold whole samples (`np` groups each); ties go to more slices (shorter chains per workgroup).
struct CoopBest { float ms; int ncb; };
CoopBest coop_best(bool ted, int g, int n_cu, int np) {
    if (g < 1) return {0.f, 1};
    std::vector<float> cost((size_t)g + 1, 0.f);
    int first = 1;
    for (int k = np; k <= g; k += np) {
        float bm = 1e30f;
        int bn = 1;
        for (int ncb = 1; ncb <= 4; ncb *= 2) {
            const int cap = coop_cap(n_cu, ncb) / np * np;
            if (cap < np) continue;
            const int gl = k < cap ? k : cap;
            const float m = coop_launch_ms(ted, ncb, gl, n_cu) + cost[(size_t)(k - gl)];
            if (m < bm) { bm = m; bn = ncb; }
        }
        cost[(size_t)k] = bm;
        if (k == g) first = bn;
    }
    return {cost[(size_t)g], first};
}

// blockIdx -> (group, slice) mapping of a launch (speed only): a grid of up to one workgroup per CU keeps the slices of a group on one
// XCD (hand-offs through one L2: 13-16 % at 16 clips on 8 slices, 5-10 % on 4 / 2 slices), two per CU splits them 4 + 4 over two XCDs
int coop_xmap_for(int n_cu, int ncb, int groups) { return ncb != 1 || groups * 8 <= n_cu ? 1 : 2; }
// the slicing of the first launch of `g` groups
int coop_pick_ncb(bool ted, int g, int n_cu, int np) { return coop_best(ted, g, n_cu, np).ncb; }

// the sample-split kernel over samples [first, first + n): 8 / ncb workgroups per (sample, pass), as many samples per launch as are
// resident at once
hipError_t run_coop(ls_handle* h, const StepArgs& s, int first, int n, bool pair, hipStream_t st) {
    const int np = pair ? 1 : 2;
    for (int b0 = first; b0 < first + n;) {
        const int left = first + n - b0;
        const int ncb = h->coop_ncb ? h->coop_ncb : coop_pick_ncb(h->var == kTED, left * np, h->n_cu, np);     // per launch: the rest of the piece re-planned
        int cap = coop_cap(h->n_cu, ncb);
        if (cap > h->coop_groups) cap = h->coop_groups;
        const int per = cap / np;
        if (per < 1) return hipErrorInvalidValue;
        StepArgs c = s;
        c.cx = h->co_x.f(); c.cpart = h->co_part.f();
        c.cgran = static_cast<unsigned long long*>(h->co_gran.p); c.cflag = static_cast<unsigned long long*>(h->co_flag.p);
        c.cerr = static_cast<unsigned*>(h->co_err.p);
        c.epoch = (++h->coop_launches) * kCoopEpochStride;      // tags of one launch: epoch + 1 .. epoch + 2 * layers + 1 < the stride (checked in decide_path / ls_set_path)
        const int ns = left < per ? left : per;
        c.b0 = b0; c.npass = np; c.xmap = h->coop_xmap >= 0 ? h->coop_xmap : coop_xmap_for(h->n_cu, ncb, ns * np);
        b0 += ns;
        hipError_t e = launch_step_coop(h->var, ncb, c, ns, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// the one-pass-per-workgroup kernel over samples [first, first + n): 2 (CFG) or 1 (single pass) workgroups per sample, one launch
hipError_t run_pass(ls_handle* h, const StepArgs& s, int first, int n, bool pair, hipStream_t st) {
    StepArgs c = s;
    c.pf = h->pa_out.f(); c.pcnt = static_cast<unsigned*>(h->pa_cnt.p);
    c.b0 = first; c.npass = pair ? 1 : 2;
    // a grid that fits the chip once runs as 8-wave workgroups, one per CU (two waves per SIMD hide each other's round trips);
    // beyond that, 4-wave workgroups, two per CU
#ifdef LS_PASS_FORCE_WAVES
    const int waves = LS_PASS_FORCE_WAVES;          // A/B builds (tools/ab_variants.py)
#else
    const int forced = h->pass_waves_env ? h->pass_waves_env : h->pass_waves;
    const int waves = forced ? forced : (n * c.npass <= h->n_cu ? 8 : 4);
#endif
    return launch_step_pass(h->var, h->precision == 1 ? 1 : 0, waves, c, n, st);
}

// the batch-level kernels over samples [first, first + n): the same step from separate kernels over all rows (both passes always; exact fp32 only)
hipError_t run_long(ls_handle* h, const StepArgs& s, int first, int n, hipStream_t st) {
    LongStepArgs a{};
    const size_t ox = (size_t)first * h->T * h->JF, od = (size_t)first * kD, os = (size_t)first * h->T * kD;
    auto sh = [](auto* p, size_t o) { return p ? p + o : p; };
    a.tokpad = h->tokpad;
    a.B = n; a.b0 = first; a.T = h->T; a.S = h->S; a.npre = h->cfg.n_prefix_tokens; a.JF = h->JF; a.JFP = h->JFP; a.ldo = (h->JF + 127) / 128 * 128; a.layers = h->cfg.layers;
    a.x_in = s.x_in + ox; a.x_out = sh(s.x_out, ox); a.x0_out = sh(s.x0_out, ox); a.fwd_c = sh(s.fwd_c, ox); a.fwd_u = sh(s.fwd_u, ox);
    a.static_c = s.static_c + os; a.static_u = s.static_u + os; a.z_mu = s.z_mu + od; a.z_std = s.z_std + od; a.emo_tok = sh(s.emo_tok, od); a.scale = sh(s.scale, (size_t)first);
    a.temb = s.temb;
    a.xpad_ready = s.xpad_ready && first == 0 && n == h->B;
#ifdef LS_DEBUG
    a.prof = s.prof; a.prof_wg = s.prof_wg;
#endif
    a.eps_c = sh(s.eps_c, od); a.eps_u = sh(s.eps_u, od); a.noise = sh(s.noise, s.const_noise ? (size_t)0 : ox); a.const_noise = s.const_noise; a.call = s.call; a.step_id = s.step_id;
    a.winx = h->lw_winx.f(); a.ln1a = h->ln1a.f(); a.ln1b = h->ln1b.f(); a.ln2a = h->ln2a.f(); a.ln2b = h->ln2b.f();
    a.wt = h->lw_wt.f(); a.wtp = h->lw_wtp.f(); a.part1 = h->lx_part1.f(); a.part2 = h->lx_part2.f(); a.wcf = h->lw_wcf.f(); a.bcf = h->lw_bcf.f(); a.wsum = h->lw_wsum.f(); a.bt = h->lw_bt.f(); a.wc = h->lw_wc.f(); a.bc = h->lw_bc.f(); a.wout = h->lw_wout.f(); a.bout = h->bout.f();
    a.xproj = h->lx_proj.f(); a.xpad = h->lx_xpad.f(); a.X = h->lx_X.f(); a.U = h->lx_U.f(); a.OUT = h->lx_OUT.f();
    if (h->mix_cap > 0 && first == 0 && n == h->B && s.temb_stride == 0) {     // the one-launch mixer: whole prepared batch, uniform timestep (sampling)
        a.mix_cap = h->mix_cap; a.mix_wtok = h->mx_wtok.f(); a.mix_wch = h->mx_wch.f(); a.mix_xg = h->mx_xg.f();
        if (h->mx_npt > 0 && h->mx_pout.p && h->mix_pose) { a.mix_wpose = h->mx_wpose.f(); a.mix_pout = h->mx_pout.f(); a.mix_npt = h->mx_npt; }
        a.mix_gran = static_cast<unsigned long long*>(h->mx_gran.p); a.mix_err = static_cast<unsigned*>(h->co_err.p);
        a.mix_epoch0 = (h->coop_launches + 1) * kCoopEpochStride;
        h->coop_launches += (unsigned)((2 * n + h->mix_cap - 1) / h->mix_cap);
    }
    a.sampler = s.sampler; a.t_nonzero = s.t_nonzero; a.clip_denoised = s.clip_denoised;
    a.c0 = s.c0; a.c1 = s.c1; a.c2 = s.c2; a.c3 = s.c3; a.c4 = s.c4;
    return launch_step_long(a, st);
}

// precision 0 (fp32): split-fp32 channel mixing on the bf16 matrix cores (k_step<..,2>); 1: bf16x3 (k_step<..,1>); 2 (fp32_mfma):
// every contraction on the fp32 MFMA (k_step<..,0>).  The other step kernels have no split-fp32 form: modes 0 and 2 run them as fp32.
int step_prec(const ls_handle* h) { return h->precision == LS_PRECISION_BF16X3 ? 1 : h->precision == LS_PRECISION_FP32_MFMA ? 0 : 2; }
bool plan_applies(const ls_handle* h, const StepArgs& s, bool pair) {
    if (!h->fused) return true;                                        // batch-level kernels only
    if (s.trace) return false;                                         // the residual-stream trace exists in the fused kernel only
    if (h->nseg > 1 && pair != h->plan_pair) return false;             // a split plan was costed for the other form
    for (int i = 0; i < h->nseg; ++i)
        if (h->seg[i].path == 1 && s.temb_stride != 0) return false;   // per-sample timestep rows: every kernel but the batch-level ones
    return true;
}

// Which kernels the prepared batch runs on (34-frame models; other frame counts have only the batch-level kernels).
//   fused         one workgroup = one CU per sample: a step costs one CU's time for eight layers however small the batch, and a batch
//                 of 256 k + r samples pays k + 1 full rounds;
//   pass          one workgroup per (sample, CFG pass), two per CU (ls_pass_kernel.h): half-CU units, 128 samples fill the chip;
//   sample-split  16 workgroups per sample inside one launch (ls_coop_kernel.h), 32 samples per launch;
//   batch-level   every row of the batch through 21 launches per step that fill the chip (ls_long.hip).
// Step-time models in ms, measured on MI355X (profiles/r05_throughput_vs_batch.md): the plan is the cheapest of
//   all sample-split | all batch-level | all fused | all pass | full fused rounds + the remainder on sample-split, batch-level or pass.
// pass_round: two workgroups per CU; pass_single: one per CU, alone on the chip; pass_after: one per CU behind full rounds (they start
// as the faster workgroup of every CU finishes, inside the slower one's tail)
struct PathCost { float coop_base, coop_per_group, long_base, long_per_sample, fused_round, pass_round, pass_single, pass_after; };
constexpr PathCost kCostTed{0.0875f, 0.00096f, 0.175f, 0.0030f, 0.68f, 0.682f, 0.363f, 0.378f}, kCostBeat{0.0963f, 0.00103f, 0.166f, 0.0034f, 0.79f, 0.84f, 0.437f, 0.47f};
// bf16x3 (opt-in precision) exists in the fused and the one-pass-per-workgroup kernels only; measured on MI355X (tools/bf16x3_time.py)
constexpr PathCost kCostTedBf{1e30f, 1e30f, 1e30f, 1e30f, 0.289f, 0.321f, 0.193f, 0.2005f}, kCostBeatBf{1e30f, 1e30f, 1e30f, 1e30f, 0.391f, 0.462f, 0.28f, 0.302f};
// one-pass-per-workgroup kernel: two workgroups per CU are resident (pass_round each); up to one per CU left over run alone on their CU
float pass_ms(const PathCost& c, int n, int np, int n_cu) {
    const int wgs = n * np, full = wgs / (2 * n_cu), rem = wgs % (2 * n_cu);
    return c.pass_round * full + (rem == 0 ? 0.f : rem <= n_cu ? (full ? c.pass_after : c.pass_single) : c.pass_round);
}

// The plan as a pure function of what it depends on (also behind ls_plan_query, which needs no GPU: tests/test_host_logic.py).
struct PlanIn { bool ted, fused, have_long, pair; int B, precision, path_mode, n_cu, coop_groups_max, layers, coop_ncb; };
struct PlanOut { int nseg; Seg seg[3]; float ms; };
PlanOut plan_steps(const PlanIn& in) {
    PlanOut o{1, {{0, 0, in.B}, {0, 0, 0}, {0, 0, 0}}, 0.f};
    if (!in.fused) { o.seg[0].path = 1; return o; }
    if (in.path_mode == 1) return o;
    if (in.path_mode == 4) { o.seg[0].path = 3; return o; }
    if (in.precision == 1 && in.path_mode != 0) return o;
    if (in.path_mode == 2) { o.seg[0].path = in.have_long ? 1 : 0; return o; }
    if (in.path_mode == 3) { o.seg[0].path = 2; return o; }
    if (in.B <= 0) return o;
    const bool bf = in.precision == 1;      // bf16x3; the two fp32 modes share the exact-fp32 costs
    const PathCost& c = bf ? (in.ted ? kCostTedBf : kCostBeatBf) : (in.ted ? kCostTed : kCostBeat);
    const int B = in.B, np = in.pair ? 1 : 2, round = 2 * in.n_cu / np, unit = in.n_cu / np;     // round: samples of one fused round; unit: samples that put ONE pass workgroup on every CU
    const float thr = 256.0f / (float)in.n_cu;          // throughput-bound terms (measured on 256 CUs) on a smaller / larger device
    auto cost = [&](int path, int n) -> float {
        switch (path) {
        case 0: return c.fused_round * ((n + round - 1) / round);
        case 1: return in.have_long && !bf ? c.long_base + c.long_per_sample * thr * n : 1e30f;
        case 2: return bf || in.coop_groups_max < np || 2 * in.layers + 2 > (int)kCoopEpochStride ? 1e30f
                       : in.coop_ncb ? coop_ms_ncb(in.ted, in.coop_ncb, n * np, in.n_cu) : coop_best(in.ted, n * np, in.n_cu, np).ms;
        default: return pass_ms(c, n, np, in.n_cu);
        }
    };
    // head: the full fused rounds; the remainder r on one family, or -- beyond one pass workgroup per CU -- `unit` samples on the
    // one-pass-per-workgroup kernel and the rest on the sample-split / batch-level kernels (ties go to the earlier candidate)
    const int head = B >= round ? B / round * round : 0, r = B - head;
    float best = 0.f;
    Seg tail[2] = {{0, 0, 0}, {0, 0, 0}};
    int ntail = 0;
    if (r > 0) {
        best = 1e30f;
        for (int path = 0; path < 4; ++path) {
            const float t = cost(path, r);
            if (t < best) { best = t; ntail = 1; tail[0] = {path, head, r}; }
        }
        if (r > unit && !bf)
            for (int path = 1; path < 3; ++path) {
                const float t = cost(3, unit) + cost(path, r - unit);
                if (t < best) { best = t; ntail = 2; tail[0] = {3, head, unit}; tail[1] = {path, head + unit, r - unit}; }
            }
    }
    o.nseg = 0;
    if (head > 0) o.seg[o.nseg++] = {0, 0, head};
    for (int i = 0; i < ntail; ++i) {
        if (o.nseg > 0 && tail[i].path == 0 && o.seg[o.nseg - 1].path == 0) o.seg[o.nseg - 1].n += tail[i].n;      // one more fused round
        else o.seg[o.nseg++] = tail[i];
    }
    o.ms = c.fused_round * (head / round) + best;
    // ... or the whole batch on the one-pass-per-workgroup kernel: its later workgroups start as slots free up, so 384 clips
    // (768 workgroups) cost a round and a half, not two
    if (head > 0 && r > 0 && cost(3, B) < o.ms) { o.nseg = 1; o.seg[0] = {3, 0, B}; o.ms = cost(3, B); }
    return o;
}

}  // namespace

// samples of the plan's piece on kernel family `path` (0 if the plan has none)
int ls::seg_n(const ls_handle* h, int path) {
    for (int i = 0; i < h->nseg; ++i) if (h->seg[i].path == path) return h->seg[i].n;
    return 0;
}

// everything that identifies the plan (graph key, "did the plan change")
long long ls::plan_code(const ls_handle* h) {
    long long c = h->nseg;
    for (int i = 0; i < h->nseg; ++i) c = c * 8209 + h->seg[i].path + 4 * (long long)h->seg[i].n;
    return c;
}

// One diffusion step of the prepared batch on the kernels decide_path chose.
// pair: the single-pass variant (two samples' cond pass per workgroup), legal when every guidance scale is 1
hipError_t ls::run_step(ls_handle* h, StepArgs& s, int B, bool pair, hipStream_t st) {
    s.batch = B;
    if (!h->fused) return run_long(h, s, 0, B, st);
    if (!plan_applies(h, s, pair)) return launch_step(h->var, step_prec(h), pair ? 1 : 0, s, B, st);
    for (int i = 0; i < h->nseg; ++i) {
        const Seg& g = h->seg[i];
        const int n = h->nseg == 1 ? B : g.n;
        hipError_t e;
        switch (g.path) {
        case 0: s.batch = n; e = g.first == 0 ? launch_step(h->var, step_prec(h), pair ? 1 : 0, s, n, st) : hipErrorInvalidValue; s.batch = B; break;
        case 1: e = run_long(h, s, g.first, n, st); break;
        case 2: e = run_coop(h, s, g.first, n, pair, st); break;
        default: e = run_pass(h, s, g.first, n, pair, st); break;
        }
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// (sample, pass) groups of the sample-split kernel resident at once, by slicing: ncb = 1 (8 slices of 64 channels): two workgroups per CU;
// ncb = 2 / 4 (4 / 2 slices): one per CU (their registers).  The slices of a group wait for each other, so a launch never exceeds this.
int ls::coop_cap(int n_cu, int ncb) {
    const int cap = (ncb == 1 ? 2 : 1) * n_cu / (8 / ncb);
    return ncb == 1 && cap > kCoopMaxGroups ? kCoopMaxGroups : cap;
}

void ls::set_plan(ls_handle* h, int B) {
    h->plan_pair = h->all_scale_one;
    const PlanOut o = plan_steps(PlanIn{h->var == kTED, h->fused, h->lw_wtp.p != nullptr, h->plan_pair, B, h->precision, h->path_mode, h->n_cu,
                                        h->coop_groups_max, h->cfg.layers, h->coop_ncb});
    h->nseg = o.nseg;
    for (int i = 0; i < 3; ++i) h->seg[i] = o.seg[i];
    h->use_long = h->nseg == 1 && h->seg[0].path == 1;
}

void ls::decide_path(ls_handle* h) {
    const long long before = plan_code(h);
    set_plan(h, h->B);
    if (before != plan_code(h)) free_graph(h);
}

// zero the granule / flag words of the sample-split kernel (stream-ordered: a memset node when captured) and restart the epochs
hipError_t ls::coop_reset(ls_handle* h, hipStream_t st) {
    if (h->mix_cap > 0 && h->mx_gran.p) {
        h->coop_launches = 0;
        return hipMemsetAsync(h->mx_gran.p, 0, h->mx_gran.bytes, st);
    }
    if (seg_n(h, 2) == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(h->co_gran.p, 0, h->co_gran.bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(h->co_flag.p, 0, h->co_flag.bytes, st);
    h->coop_launches = 0;
    return e;
}

// A fresh range of hand-off tags for the call about to be enqueued (CallParams::tag_base, read by the sample-split kernel from device
// memory): advanced past everything the PREVIOUS call can have used -- 64 tags per launch it made (a forced sample-split path at a large
// batch makes many: 2048 clips x 1000 steps = 64 000 launches) -- and by at least 2^21, so that a granule an earlier call left behind can
// never pass for this call's whatever the zeroing ahead of the loop did.  (32-bit tags wrap after >= 2048 calls; every granule word is
// rewritten by every call that polls it, so a value that old no longer exists.)
// Arrival tickets of the one-pass-per-workgroup kernel: handed back at zero by every step's second arriver, and re-zeroed here ahead of
// every call by a plain stream memset (NOT a node of the captured loop: a replayed memset node was seen writing garbage,
// docs/DESIGN_NOTES_r5.md), so a launch that died between its two arrivals cannot leave an odd ticket behind for the next call.
static hipError_t pass_reset(ls_handle* h, hipStream_t st) {
    if (seg_n(h, 3) == 0 || !h->pa_cnt.p) return hipSuccess;
    return hipMemsetAsync(h->pa_cnt.p, 0, h->pa_cnt.bytes, st);
}

int ls::advance_tags(ls_handle* h, hipStream_t st) {
    HIPCHK(h, pass_reset(h, st));
    const unsigned long long span = ((unsigned long long)h->coop_launches + 2ull) * kCoopEpochStride;
    h->tag_base += span > (1ull << 21) ? (unsigned)span : (1u << 21);
    h->call_host.tag_base = h->tag_base;
    HIPCHK(h, hipMemcpyAsync(h->callp.p, &h->call_host, sizeof(CallParams), hipMemcpyHostToDevice, st));
    return LS_OK;
}

// after a stream synchronisation: did a hand-off spin of the sample-split kernel run out?  (Never observed; a result computed past a
// timeout is garbage, so the call fails loudly.)
int ls::coop_check(ls_handle* h, bool force) {
    if (!force && seg_n(h, 2) == 0 && h->mix_cap == 0) return LS_OK;
    unsigned v = 0;
    HIPCHK(h, hipMemcpy(&v, h->co_err.p, sizeof v, hipMemcpyDeviceToHost));
    if (!v) return LS_OK;
    HIPCHK(h, hipMemset(h->co_err.p, 0, sizeof v));
    return fail(h, LS_EHIP, "sample-split step kernel: an inter-workgroup hand-off timed out; the results of this call are invalid");
}

void ls::report_path(ls_handle* h, bool pair) {
    const bool split = h->nseg > 1 && pair == h->plan_pair;
    h->timing.step_path = (h->nseg == 1 || split) ? h->seg[0].path : 0;
    h->timing.tail_samples = split ? h->seg[1].n : 0;
    h->timing.tail_path = split ? h->seg[1].path : 0;
    h->timing.tail2_samples = split && h->nseg > 2 ? h->seg[2].n : 0;
    h->timing.tail2_path = split && h->nseg > 2 ? h->seg[2].path : 0;
    h->timing.coop_slices = !h->fused && h->mix_cap > 0 ? kMixSlices : 0;      // a long-sequence model: 4 = the one-launch mixer ran the blocks (step_path stays 1)
    if (h->fused && (h->nseg == 1 || split))
        for (int i = 0; i < h->nseg; ++i)
            if (h->seg[i].path == 2) {
                const int n = h->nseg == 1 ? h->B : h->seg[i].n, np = pair ? 1 : 2;
                h->timing.coop_slices = 8 / (h->coop_ncb ? h->coop_ncb : coop_pick_ncb(h->var == kTED, n * np, h->n_cu, np));      // of the first launch
            }
}

extern "C" {

int ls_set_precision(ls_handle* h, int mode) {
    if (!h) return LS_EINVAL;
    if (mode != LS_PRECISION_FP32 && mode != LS_PRECISION_BF16X3 && mode != LS_PRECISION_FP32_MFMA)
        return fail(h, LS_EINVAL, "unknown precision mode %d", mode);
    if (!h->fused && mode == LS_PRECISION_BF16X3) return fail(h, LS_EUNSUPPORTED, "the long-sequence path (nframes != %d) is exact fp32 only", kT);
    if (mode != h->precision) free_graph(h);
    h->precision = mode;
    if (h->prepared) {      // the plan may move to kernels whose workspaces the last ls_prepare did not allocate: prepare again then
        const long long was = plan_code(h);
        decide_path(h);
        if (was != plan_code(h)) h->prepared = false;
    }
    return LS_OK;
}

// The step plan `auto` would make (no handle, no GPU): out = {n pieces, then (path, first, count) per piece}, *ms = the model's step time.
int ls_plan_query(int beat, int batch, int single_pass, int precision, int n_cus, int* out10, float* ms) {
    if (!out10 || batch < 1 || n_cus < 8) return LS_EINVAL;
    const int gmax = 2 * n_cus / 8 < kCoopMaxGroups ? 2 * n_cus / 8 : kCoopMaxGroups;
    const PlanOut o = plan_steps(PlanIn{beat == 0, true, true, single_pass != 0, batch, precision, 0, n_cus, gmax, 8, 0});
    out10[0] = o.nseg;
    for (int i = 0; i < 3; ++i) { out10[1 + 3 * i] = o.seg[i].path; out10[2 + 3 * i] = o.seg[i].first; out10[3 + 3 * i] = o.seg[i].n; }
    if (ms) *ms = o.ms;
    return LS_OK;
}

// Slice workgroups per (sample, pass) the sample-split kernel would use for a piece of `groups` (sample, pass) groups (mode 3's choice).
int ls_plan_coop_slices(int beat, int groups, int n_cus) {
    if (groups < 1 || n_cus < 8) return LS_EINVAL;
    return 8 / coop_pick_ncb(beat == 0, groups, n_cus, 1);
}

int ls_set_path(ls_handle* h, int mode) {
    if (!h) return LS_EINVAL;
    if (mode < 0 || mode > 8) return fail(h, LS_EINVAL, "ls_set_path: mode %d (0 auto, 1 one workgroup per sample, 2 batch-level kernels, 3 sample-split kernel, 4 one workgroup per (sample, pass), 5 the same in its 4-wave / two-per-CU form at every grid size, 6 / 7 / 8 the sample-split kernel with 4 / 2 / 8 slices per (sample, pass))", mode);
    // modes 6 / 7 / 8 = mode 3 with the slicing forced (mode 3 picks it per piece from the step-time model): every slicing is pinned to the
    // reference's fixtures through these selectors (tests/test_gpu_coop.py)
    const int ncb = mode == 6 ? 2 : mode == 7 ? 4 : mode == 8 ? 1 : 0;
    if (mode >= 6) mode = 3;
    // mode 5 = mode 4 with the 4-wave form forced (mode 4 picks it only for grids beyond one workgroup per CU): the form the plans of a
    // device with fewer CUs reach at small batches, pinned to the reference's fixtures at B = 4 / 5 through this selector (tests/test_gpu_pass.py)
    const int waves = mode == 5 ? 4 : 0;
    if (mode == 5) mode = 4;
    if (mode == 3 && !h->fused && ncb == 0 && mix_supports(h->S)) {
        // a long-sequence model: mode 3 = its sample-split form, the one-launch mixer (ls_mix_kernel.h), at every batch size
        if (mode != h->path_mode) { h->path_mode = mode; h->prepared = false; free_graph(h); }
        return LS_OK;
    }
    if (mode >= 3 && !h->fused) return fail(h, LS_EUNSUPPORTED, "nframes != %d has neither the sample-split nor the one-pass-per-workgroup kernel", kT);
    if (mode == 3 && h->precision == LS_PRECISION_BF16X3) return fail(h, LS_EUNSUPPORTED, "the sample-split kernel is exact fp32 only");
    if (mode == 3 && 2 * h->cfg.layers + 2 > (int)kCoopEpochStride)
        return fail(h, LS_EUNSUPPORTED, "the sample-split kernel tags its hand-offs with %u values per launch: %d layers need %d", kCoopEpochStride, h->cfg.layers, 2 * h->cfg.layers + 2);
    if (mode == 3 && h->coop_groups_max < 2)
        return fail(h, LS_EUNSUPPORTED, "the sample-split kernel needs the 16 workgroups of a sample resident at once (two per CU): %d CUs are too few", h->n_cu);
    if (mode == 2 && h->fused && h->lw_wtp.p == nullptr && h->committed) return fail(h, LS_EUNSUPPORTED, "batch-level kernels need S <= 160");
    if (mode == 1 && !h->fused) return fail(h, LS_EUNSUPPORTED, "nframes != %d has no fused kernel", kT);
    if (mode != h->path_mode || waves != h->pass_waves || ncb != h->coop_ncb) { h->path_mode = mode; h->pass_waves = waves; h->coop_ncb = ncb; h->prepared = false; free_graph(h); }      // takes effect at the next ls_prepare (workspaces)
    return LS_OK;
}

}  // extern "C"
