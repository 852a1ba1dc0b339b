// Host side of the C-ABI declared in include/ls_hip.h: handle, weight images in MFMA operand order,
// once-per-call preparation, the diffusion loop (stream launches or a captured hipGraph) and read-back.
// No torch types here; the Python shim (livelyspeaker_amd/_lib.py) binds these symbols with ctypes.
#include "ls_hip.h"
#include "ls_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace ls;

namespace {

thread_local std::string g_create_error;     // message of this thread's last failed ls_create (handles may be created from several threads)

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    hipError_t ensure(size_t n) {
        if (n <= bytes) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; bytes = 0; }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    float* f() const { return static_cast<float*>(p); }
};

const int kConvCin[4] = {1, 32, 64, 128};
const int kConvCout[4] = {32, 64, 128, 256};
const int kConvStride[4] = {5, 6, 6, 6};
const int kConvPad[4] = {1600, 0, 0, 0};
const int kConvKey[4] = {0, 3, 6, 9};

// bf16 round-to-nearest-even, as v_cvt_pk_bf16_f32 does on the device side of the split
unsigned short f32_to_bf16(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
float bf16_to_f32(unsigned short h) {
    const unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

}  // namespace

// one piece of a step plan: samples [first, first + n) of the prepared batch on one kernel family
// (0 fused: one workgroup per sample, 1 batch-level kernels, 2 sample-split kernel, 3 one workgroup per (sample, pass))
struct Seg { int path, first, n; };

struct ls_handle {
    ls_config cfg{};
    Variant var = kTED;
    int JF = 0, S = 0, R = 0, NOB = 0, KXQ = 0, MK = 0, KIN = 0, KF = 0, KFP = 0;      // KFP: KF padded to the GEMM's K tile
    int T = kT;             // frames; 34 = the reference's (fused step kernel), anything else = the long-sequence path (ls_long.hip)
    bool fused = true;      // the model HAS the fused kernel (34 frames)
    bool use_long = false;  // the prepared batch runs the batch-level kernels (always when !fused; small batches of a fused model)
    int path_mode = 0;      // ls_set_path: 0 auto, 1 one workgroup per sample (fused kernel), 2 batch-level kernels, 3 sample-split kernel, 4 one workgroup per (sample, pass)
    bool use_pass = false;  // the prepared batch runs the one-pass-per-workgroup kernel (ls_pass_kernel.h: two independent workgroups per CU)
    DevBuf pa_out, pa_cnt;  // its CFG hand-off: pass outputs [n][2][T][J*F], arrival tickets [n]
    int pass_n = 0;         // samples the hand-off buffers hold
    int pass_waves = 0;     // 0: 8-wave workgroups when the grid fits the chip once, 4-wave otherwise; 4: ls_set_path(5) forces the 4-wave form
    int pass_waves_env = 0; // LS_PASS_WAVES = 4 | 8 forces one (-DLS_DEBUG builds only)
    bool use_coop = false;  // the prepared batch runs the sample-split kernel (ls_coop_kernel.h: 16 workgroups per sample)
    // the step plan of the prepared batch (decide_path): up to three pieces, e.g. 416 clips = 256 on the fused kernel + 128 on the
    // one-pass-per-workgroup kernel (one workgroup per CU) + 32 on the sample-split kernel.  use_long / use_coop / use_pass: the whole batch
    // is on that family (one piece).
    int nseg = 1;
    Seg seg[3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    bool plan_pair = false; // the plan assumed the single-pass form (every guidance scale 1)
    DevBuf wtok1_img;       // token-mix operand of one pass (sample-split kernel)
    DevBuf wtail;           // [L][S][4] token-mix weights of the ragged output rows 32 .. 35 (one-pass-per-workgroup kernel)
    DevBuf wtok1_hi_img, wtok1_lo_img;   // the same as bf16 hi / lo planes (one-pass-per-workgroup kernel, bf16x3)
    DevBuf co_x, co_part, co_gran, co_flag, co_err;      // its exchange workspaces (one launch's worth), granules / flags, timeout word
    unsigned coop_launches = 0;                        // launches since the granule words were zeroed: epoch = 64 * ordinal
    unsigned coop_err_host = 0;
    int n_cu = 256;         // compute units of the device (hipDeviceProp.multiProcessorCount): residency of the sample-split kernel, round sizes of the plans
    int max_thr_cu = 2048;  // hipDeviceProp.maxThreadsPerMultiProcessor: with n_cu, the geometry of torch's randn launches (LS_NOISE_TORCH_DEVICE)
    int coop_groups_max = kCoopMaxGroups, coop_groups = 0;   // (sample, pass) groups per launch: cap of the 8-slice form (two workgroups per CU, eight per group), and what the workspaces hold
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
    DevBuf conv_w[4], conv_b[4], win_full, win_pre, win_aud, win_bias, spk_emb, ml_w, ml_b, emo_emb;
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
    std::string coef_key;   // (sampler, eta, schedule) the per-index coefficient table `coef` was built for

    // cached graph of the step loop
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
    std::string graph_key;

    ls_timing timing{};
    CallParams call_host{0, 0, 0, 0};
    unsigned tag_base = 0;  // sample-split kernel: base of the current call's hand-off tags (CallParams::tag_base)
    int precision = 0;      // LS_PRECISION_*: 0 fp32 (split-fp32 channel mixing in k_step), 1 bf16x3, 2 fp32 MFMA throughout (ls_set_precision)
#ifdef LS_DEBUG             // profiling variant of the library only (build_library(defines=['LS_DEBUG'])); never in the shipped .so
    DevBuf prof, wgt;       // wgt: [1024][2] start / end stamps of every workgroup of the last step launch
    bool prof_on = false;   // LS_PROF=<workgroup index>: in-kernel s_memtime phase stamps, read with ls_read("prof")
    int prof_wg = 0;
    int ablate = 0;         // LS_ABLATE (results are wrong when non-zero)
#endif
};

namespace {

hipError_t run_step(ls_handle* h, StepArgs& s, int B, bool pair, hipStream_t st);
void resolve_prepare_timing(ls_handle* h, bool block);

int fail(ls_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(h, expr)                                                                         \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return fail((h), LS_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

int upload(ls_handle* h, DevBuf& d, const void* src, size_t bytes) {
    HIPCHK(h, d.ensure(bytes ? bytes : 4));
    if (bytes) {
        HIPCHK(h, hipMemcpyAsync(d.p, src, bytes, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));     // src is usually a temporary: finish before it dies
    }
    return LS_OK;
}

// copy a caller buffer (host or device) into an internal device buffer
int ingest(ls_handle* h, DevBuf& d, const void* src, size_t bytes, int on_device) {
    HIPCHK(h, d.ensure(bytes ? bytes : 4));
    HIPCHK(h, hipMemcpyAsync(d.p, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    return LS_OK;
}
int egress(ls_handle* h, void* dst, const void* src, size_t bytes, int on_device) {
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    return LS_OK;
}

const std::vector<float>* find_w(ls_handle* h, const std::string& key, size_t want) {
    auto it = h->w.find(key);
    if (it == h->w.end()) { fail(h, LS_ESTATE, "missing weight '%s'", key.c_str()); return nullptr; }
    if (it->second.size() != want) {
        fail(h, LS_EINVAL, "weight '%s' has %zu elements, expected %zu", key.c_str(), it->second.size(), want);
        return nullptr;
    }
    return &it->second;
}

void free_graph(ls_handle* h) {
    if (h->graph_exec) (void)hipGraphExecDestroy(h->graph_exec);
    if (h->graph) (void)hipGraphDestroy(h->graph);
    h->graph_exec = nullptr;
    h->graph = nullptr;
    h->graph_key.clear();
}

// Device images whose element order is the per-lane MFMA operand order of the fused step kernel (ls_step_kernel.h).
int build_fused_images(ls_handle* h) {
    const int L = h->cfg.layers, S = h->S, R = h->R, JF = h->JF, D = kD;
    const int MK = h->MK, KXQ = h->KXQ, NOB = h->NOB, KIN = h->KIN;
    std::vector<float> wch((size_t)L * D * D), bch((size_t)L * D), l1a((size_t)L * D), l1b((size_t)L * D),
        l2a((size_t)L * D), l2b((size_t)L * D), ww((size_t)L * kNT * MK * 64), bt((size_t)L * 80, 0.f);
    std::vector<unsigned short> wch_hi((size_t)L * D * D), wch_lo((size_t)L * D * D), wch_lo2((size_t)L * D * D);
    const int KS = (R + 31) / 32;
    const int MK1 = (S + 3) / 4;
    const int MQ1 = (MK1 + 3) / 4;
    std::vector<float> wt1((size_t)L * 3 * MQ1 * 256);
    std::vector<unsigned short> wwh((size_t)L * kNT * KS * 64 * 8), wwl((size_t)L * kNT * KS * 64 * 8);
    const int KS1 = (S + 31) / 32;
    std::vector<unsigned short> wt1h((size_t)L * 3 * KS1 * 64 * 8), wt1l((size_t)L * 3 * KS1 * 64 * 8);
    std::vector<float> wtl((size_t)L * S * 4, 0.f);
    char key[160];
    for (int l = 0; l < L; ++l) {
        auto K = [&](const char* suffix) { snprintf(key, sizeof key, "backbone.mlps.%d.%s", l, suffix); return std::string(key); };
        const auto* W = find_w(h, K("block2.1.weight"), (size_t)D * D);        // Linear(512,512) [out][in], mlp_module.py:58-60
        const auto* b2 = find_w(h, K("block2.1.bias"), D);
        const auto* Wt = find_w(h, K("block1.1.weight"), (size_t)S * S);       // Conv1d(S,S,1) [out tok][in tok][1], :51-55
        const auto* b1 = find_w(h, K("block1.1.bias"), S);
        const auto* a1 = find_w(h, K("block1.0.alpha"), D);
        const auto* be1 = find_w(h, K("block1.0.beta"), D);
        const auto* a2 = find_w(h, K("block2.0.alpha"), D);
        const auto* be2 = find_w(h, K("block2.0.beta"), D);
        if (!W || !b2 || !Wt || !b1 || !a1 || !be1 || !a2 || !be2) return LS_ESTATE;
        // wch_img[l][w][p][q][c2][lane][j] = W[n = 64w + 16(2p+c2) + (lane&15)][k = 16q + 4(lane>>4) + j]
        size_t o = (size_t)l * D * D;
        for (int w = 0; w < kWaves; ++w)
            for (int p = 0; p < 2; ++p)
                for (int q = 0; q < 32; ++q)
                    for (int c2 = 0; c2 < 2; ++c2)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 4; ++j) {
                                const int n = 64 * w + 16 * (2 * p + c2) + (lane & 15);
                                const int k = 16 * q + 4 * (lane >> 4) + j;
                                wch[o++] = (*W)[(size_t)n * D + k] * (*a2)[k];        // W' = W . diag(alpha2)
                            }
        // bf16 images, operand order of v_mfma_f32_16x16x32_bf16: [l][w][p][q16][c2][lane][8 k].  W' = hi + mid + lo exactly, each
        // round-to-nearest-even: hi = bf16(W'), mid = bf16(W' - hi), lo = bf16(W' - hi - mid) (both differences are exact in fp32).
        // bf16x3 uses hi and mid (its "lo" plane, wch_lo_img); split-fp32 (k_step PREC 2) all three.
        {
            size_t oh = (size_t)l * D * D;
            for (int w = 0; w < kWaves; ++w)
                for (int p = 0; p < 2; ++p)
                    for (int q = 0; q < 16; ++q)
                        for (int c2 = 0; c2 < 2; ++c2)
                            for (int lane = 0; lane < 64; ++lane)
                                for (int e = 0; e < 8; ++e) {
                                    const int n = 64 * w + 16 * (2 * p + c2) + (lane & 15);
                                    const int k = 32 * q + 8 * (lane >> 4) + e;
                                    const float v = (*W)[(size_t)n * D + k] * (*a2)[k];
                                    const unsigned short hi = f32_to_bf16(v);
                                    wch_hi[oh] = hi;
                                    const float r = v - bf16_to_f32(hi);
                                    wch_lo[oh] = f32_to_bf16(r);
                                    wch_lo2[oh] = f32_to_bf16(r - bf16_to_f32(wch_lo[oh]));
                                    ++oh;
                                }
        }
        for (int n = 0; n < D; ++n) {                                                    // b' = b + W . beta2
            double acc = (*b2)[n];
            for (int k = 0; k < D; ++k) acc += (double)(*W)[(size_t)n * D + k] * (double)(*be2)[k];
            bch[(size_t)l * D + n] = (float)acc;
        }
        memcpy(&l1a[(size_t)l * D], a1->data(), D * sizeof(float));
        memcpy(&l1b[(size_t)l * D], be1->data(), D * sizeof(float));
        memcpy(&l2a[(size_t)l * D], a2->data(), D * sizeof(float));
        memcpy(&l2b[(size_t)l * D], be2->data(), D * sizeof(float));
        // ww_img[l][t][m][lane] = WW[r = 16t + (lane&15)][r' = 4m + (lane>>4)], WW = blockdiag(Wt, Wt) on packed rows
        for (int t = 0; t < kNT; ++t)
            for (int m = 0; m < MK; ++m)
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = 16 * t + (lane & 15), rp = 4 * m + (lane >> 4);
                    float v = 0.f;
                    if (r < R && rp < R && r / S == rp / S) v = (*Wt)[(size_t)(r % S) * S + (rp % S)];
                    ww[(((size_t)l * kNT + t) * MK + m) * 64 + lane] = v;
                }
        // bf16x3 token-mix images: [l][t][ks][lane][e] = WW[r = 16t + (lane&15)][r' = 32ks + 8(lane>>4) + e]
        for (int t = 0; t < kNT; ++t)
            for (int ks = 0; ks < KS; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int r = 16 * t + (lane & 15), rp = 32 * ks + 8 * (lane >> 4) + e;
                        float v = 0.f;
                        if (r < R && rp < R && r / S == rp / S) v = (*Wt)[(size_t)(r % S) * S + (rp % S)];
                        const size_t o = ((((size_t)l * kNT + t) * KS + ks) * 64 + lane) * 8 + e;
                        wwh[o] = f32_to_bf16(v);
                        wwl[o] = f32_to_bf16(v - bf16_to_f32(wwh[o]));
                    }
        for (int r = 0; r < R; ++r) bt[(size_t)l * 80 + r] = (*b1)[r % S];
        // wtail[l][k][i] = Wt[32 + i][k] (zero beyond the last row): the A operand of the ragged rows' 4x4x1 MFMAs (ls_pass_kernel.h)
        for (int k = 0; k < S; ++k)
            for (int i = 0; i < 4; ++i)
                if (32 + i < S) wtl[((size_t)l * S + k) * 4 + i] = (*Wt)[(size_t)(32 + i) * S + k];
        // wtok1_hi / lo [l][t][ks][lane][e] = Wt[r = 16t + (lane&15)][r' = 32ks + 8(lane>>4) + e] of ONE pass as bf16 hi / lo planes (ls_pass_kernel.h)
        for (int t = 0; t < 3; ++t)
            for (int ks = 0; ks < KS1; ++ks)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int r = 16 * t + (lane & 15), rp = 32 * ks + 8 * (lane >> 4) + e;
                        const float v = (r < S && rp < S) ? (*Wt)[(size_t)r * S + rp] : 0.f;
                        const size_t o = ((((size_t)l * 3 + t) * KS1 + ks) * 64 + lane) * 8 + e;
                        wt1h[o] = f32_to_bf16(v);
                        wt1l[o] = f32_to_bf16(v - bf16_to_f32(wt1h[o]));
                    }
        // wtok1_img[l][t][mq][lane][j] = Wt[r = 16t + (lane&15)][r' = 4(4mq + j) + (lane>>4)] of ONE pass, zero outside S x S (ls_coop_kernel.h)
        for (int t = 0; t < 3; ++t)
            for (int m = 0; m < 4 * MQ1; ++m)
                for (int lane = 0; lane < 64; ++lane) {
                    const int r = 16 * t + (lane & 15), rp = 4 * m + (lane >> 4);
                    wt1[((((size_t)l * 3 + t) * MQ1 + (m >> 2)) * 64 + lane) * 4 + (m & 3)] = (r < S && rp < S) ? (*Wt)[(size_t)r * S + rp] : 0.f;
                }
    }
    const auto* Win = find_w(h, "input_mapping.weight", (size_t)D * KIN);        // RAG.py:62
    const auto* bin = find_w(h, "input_mapping.bias", D);
    const auto* Wout = find_w(h, "output_process.poseFinal.weight", (size_t)JF * D);   // RAG.py:203
    const auto* bo = find_w(h, "output_process.poseFinal.bias", JF);
    if (!Win || !bin || !Wout || !bo) return LS_ESTATE;
    std::vector<float> winx((size_t)kWaves * 2 * KXQ * 2 * 64 * 4), wout((size_t)NOB * 32 * 64 * 4), bout((size_t)NOB * 16, 0.f);
    {
        size_t o = 0;
        for (int w = 0; w < kWaves; ++w)
            for (int p = 0; p < 2; ++p)
                for (int q = 0; q < KXQ; ++q)
                    for (int c2 = 0; c2 < 2; ++c2)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 4; ++j) {
                                const int n = 64 * w + 16 * (2 * p + c2) + (lane & 15);
                                const int k = 16 * q + 4 * (lane >> 4) + j;
                                winx[o++] = k < JF ? (*Win)[(size_t)n * KIN + k] : 0.f;
                            }
        o = 0;
        for (int ob = 0; ob < NOB; ++ob)
            for (int q = 0; q < 32; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int c = 16 * ob + (lane & 15);
                        const int k = 16 * q + 4 * (lane >> 4) + j;
                        wout[o++] = c < JF ? (*Wout)[(size_t)c * D + k] : 0.f;
                    }
        for (int c = 0; c < JF; ++c) bout[c] = (*bo)[c];
    }
    // wout_reg_img[w][ob][cb][lane][j] = Wout[c = 16ob + (lane&15)][k = 64w + 16cb + 4(lane>>4) + j]: the k order in which
    // wave w's residual registers X[cb][.][j] present the hidden state as an MFMA B operand
    std::vector<float> woutr((size_t)kWaves * NOB * kCB * 64 * 4);
    {
        size_t o = 0;
        for (int w = 0; w < kWaves; ++w)
            for (int ob = 0; ob < NOB; ++ob)
                for (int cb = 0; cb < kCB; ++cb)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j) {
                            const int c = 16 * ob + (lane & 15);
                            const int k = 64 * w + 16 * cb + 4 * (lane >> 4) + j;
                            woutr[o++] = c < JF ? (*Wout)[(size_t)c * D + k] : 0.f;
                        }
    }
    int rc;
#define UP(buf, vec) if ((rc = upload(h, h->buf, (vec).data(), (vec).size() * sizeof(float))) != LS_OK) return rc
    if ((rc = upload(h, h->wch_hi_img, wch_hi.data(), wch_hi.size() * sizeof(unsigned short))) != LS_OK) return rc;
    if ((rc = upload(h, h->wch_lo_img, wch_lo.data(), wch_lo.size() * sizeof(unsigned short))) != LS_OK) return rc;
    if ((rc = upload(h, h->wch_lo2_img, wch_lo2.data(), wch_lo2.size() * sizeof(unsigned short))) != LS_OK) return rc;
    if ((rc = upload(h, h->ww_hi_img, wwh.data(), wwh.size() * sizeof(unsigned short))) != LS_OK) return rc;
    if ((rc = upload(h, h->ww_lo_img, wwl.data(), wwl.size() * sizeof(unsigned short))) != LS_OK) return rc;
    if ((rc = upload(h, h->wtok1_hi_img, wt1h.data(), wt1h.size() * sizeof(unsigned short))) != LS_OK) return rc;
    if ((rc = upload(h, h->wtok1_lo_img, wt1l.data(), wt1l.size() * sizeof(unsigned short))) != LS_OK) return rc;
    UP(wch_img, wch); UP(bch, bch); UP(ln1a, l1a); UP(ln1b, l1b); UP(ln2a, l2a); UP(ln2b, l2b);
    UP(wtail, wtl);
    UP(ww_img, ww); UP(wtok1_img, wt1); UP(btok_rows, bt); UP(winx_img, winx); UP(wout_img, wout); UP(wout_reg_img, woutr); UP(bout, bout);
#undef UP
    DevWeights dw{};
    dw.wch_img = h->wch_img.f(); dw.bch = h->bch.f(); dw.wsum = h->lw_wsum.f();
    dw.wch_hi_img = static_cast<const unsigned short*>(h->wch_hi_img.p);
    dw.wch_lo_img = static_cast<const unsigned short*>(h->wch_lo_img.p);
    dw.wch_lo2_img = static_cast<const unsigned short*>(h->wch_lo2_img.p);
    dw.ww_hi_img = static_cast<const unsigned short*>(h->ww_hi_img.p);
    dw.ww_lo_img = static_cast<const unsigned short*>(h->ww_lo_img.p);
    dw.ln1a = h->ln1a.f(); dw.ln1b = h->ln1b.f(); dw.ln2a = h->ln2a.f(); dw.ln2b = h->ln2b.f();
    dw.ww_img = h->ww_img.f(); dw.wtok1_img = h->wtok1_img.f(); dw.btok_rows = h->btok_rows.f();
    dw.wtail = h->wtail.f();
    dw.wtok1_hi_img = static_cast<const unsigned short*>(h->wtok1_hi_img.p); dw.wtok1_lo_img = static_cast<const unsigned short*>(h->wtok1_lo_img.p);
    dw.winx_img = h->winx_img.f(); dw.wout_img = h->wout_img.f(); dw.wout_reg_img = h->wout_reg_img.f(); dw.bout = h->bout.f();
    if ((rc = upload(h, h->devw, &dw, sizeof dw)) != LS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LS_OK;
}


// Weights of the once-per-call stage (audio encoder, static input projection, speaker style, timestep embedder): the same for the
// fused (34-frame) and the long-sequence path.
int build_shared_weights(ls_handle* h) {
    const int JF = h->JF, D = kD, KIN = h->KIN;
    char key[160];
    int rc;
    const auto* Win = find_w(h, "input_mapping.weight", (size_t)D * KIN);        // RAG.py:62
    const auto* bin = find_w(h, "input_mapping.bias", D);
    if (!Win || !bin) return LS_ESTATE;
#define UP(buf, vec) if ((rc = upload(h, h->buf, (vec).data(), (vec).size() * sizeof(float))) != LS_OK) return rc
    UP(win_full, *Win); UP(win_bias, *bin);
    {   // the static columns JF.. of input_mapping, split by the features they multiply: [prefix poses | bit] (shared by both CFG
        // passes; zero-padded to a whole number of K tiles so the projection takes the GEMM's fast path) and the 256 audio columns
        // (cond pass only)
        std::vector<float> wp((size_t)D * h->KPP, 0.f), wa((size_t)D * kAudioFeat);
        for (int n = 0; n < D; ++n) {
            for (int k = 0; k < JF + 1; ++k) wp[(size_t)n * h->KPP + k] = (*Win)[(size_t)n * KIN + JF + k];
            for (int k = 0; k < kAudioFeat; ++k) wa[(size_t)n * kAudioFeat + k] = (*Win)[(size_t)n * KIN + 2 * JF + 1 + k];
        }
        UP(win_pre, wp); UP(win_aud, wa);
    }
    // raw weights used by the once-per-call kernels
    for (int i = 0; i < 4; ++i) {
        snprintf(key, sizeof key, "audio_encoder.feat_extractor.%d.weight", kConvKey[i]);
        const auto* cw = find_w(h, key, (size_t)kConvCout[i] * kConvCin[i] * 15);   // audio_enc.py:9-20
        snprintf(key, sizeof key, "audio_encoder.feat_extractor.%d.bias", kConvKey[i]);
        const auto* cb = find_w(h, key, kConvCout[i]);
        if (!cw || !cb) return LS_ESTATE;
        UP(conv_w[i], *cw); UP(conv_b[i], *cb);
        if (i > 0) {
            // image [co tile][chunk][k][lane][cig]: W[co = 16*ct + (lane&15)][ci = 16*chunk + 4*cig + (lane>>4)][k]
            const int Cin = kConvCin[i], Cout = kConvCout[i], nchunk = Cin / 16;
            std::vector<float> img((size_t)Cout * Cin * 15 / 16 * 16);
            size_t o = 0;
            for (int ct = 0; ct < Cout / 16; ++ct)
                for (int ch = 0; ch < nchunk; ++ch)
                    for (int k = 0; k < 15; ++k)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int cig = 0; cig < 4; ++cig) {
                                const int co = 16 * ct + (lane & 15), ci = 16 * ch + 4 * cig + (lane >> 4);
                                img[o++] = (*cw)[((size_t)co * Cin + ci) * 15 + k];
                            }
            UP(conv_img[i], img);
        }
    }
    const auto* se = find_w(h, "speaker_embedding.weight", (size_t)h->cfg.n_speakers * 256);   // RAG.py:65-69
    const auto* mw = find_w(h, "speaker_mu.weight", (size_t)D * 256);
    const auto* mb = find_w(h, "speaker_mu.bias", D);
    const auto* lw = find_w(h, "speaker_logvar.weight", (size_t)D * 256);
    const auto* lb = find_w(h, "speaker_logvar.bias", D);
    const auto* t0w = find_w(h, "backbone.embed_timestep.time_embed.0.weight", (size_t)D * D);   // mlp_module.py:129-133
    const auto* t0b = find_w(h, "backbone.embed_timestep.time_embed.0.bias", D);
    const auto* t2w = find_w(h, "backbone.embed_timestep.time_embed.2.weight", (size_t)D * D);
    const auto* t2b = find_w(h, "backbone.embed_timestep.time_embed.2.bias", D);
    if (!se || !mw || !mb || !lw || !lb || !t0w || !t0b || !t2w || !t2b) return LS_ESTATE;
    UP(spk_emb, *se);
    {   // speaker_mu and speaker_logvar as ONE [1024][256] projection (rows 0..511 mu, 512..1023 logvar): one launch instead of three
        std::vector<float> w2(mw->begin(), mw->end()), b2(mb->begin(), mb->end());
        w2.insert(w2.end(), lw->begin(), lw->end());
        b2.insert(b2.end(), lb->begin(), lb->end());
        UP(ml_w, w2); UP(ml_b, b2);
    }
    UP(te_w0, *t0w); UP(te_b0, *t0b); UP(te_w2, *t2w); UP(te_b2, *t2b);
    if (h->cfg.n_emotions > 0) {
        const auto* ee = find_w(h, "emotion_embedding.weight", (size_t)h->cfg.n_emotions * D);   // scripts_beat/model/RAG.py:72
        if (!ee) return LS_ESTATE;
        UP(emo_emb, *ee);
    }
#undef UP
    // PositionalEncoding buffer (mlp_module.py:104-116), fp32 like the torch buffer
    {
        std::vector<float> pe((size_t)kPeRows * D);
        const float cexp = (float)(-std::log(10000.0) / D);
        for (int i = 0; i < D / 2; ++i) {
            const float div = expf((float)(2 * i) * cexp);
            for (int p = 0; p < kPeRows; ++p) {
                pe[(size_t)p * D + 2 * i] = sinf((float)p * div);
                pe[(size_t)p * D + 2 * i + 1] = cosf((float)p * div);
            }
        }
        if ((rc = upload(h, h->pe, pe.data(), pe.size() * sizeof(float))) != LS_OK) return rc;
    }
    return LS_OK;
}

// Long-sequence path (nframes != 34, ls_long.hip): plain row-major weights for the batch-level kernels.
int build_long_weights(ls_handle* h) {
    const int L = h->cfg.layers, S = h->S, JF = h->JF, D = kD, KIN = h->KIN, JFP = h->JFP;
    std::vector<float> wt((size_t)L * S * S), bt((size_t)L * S), wc((size_t)L * D * D), bc((size_t)L * D), l1a((size_t)L * D), l1b((size_t)L * D),
        l2a((size_t)L * D), l2b((size_t)L * D);
    char key[160];
    for (int l = 0; l < L; ++l) {
        auto K = [&](const char* suffix) { snprintf(key, sizeof key, "backbone.mlps.%d.%s", l, suffix); return std::string(key); };
        const auto* W = find_w(h, K("block2.1.weight"), (size_t)D * D);
        const auto* b2 = find_w(h, K("block2.1.bias"), D);
        const auto* Wt = find_w(h, K("block1.1.weight"), (size_t)S * S);
        const auto* b1 = find_w(h, K("block1.1.bias"), S);
        const auto* a1 = find_w(h, K("block1.0.alpha"), D);
        const auto* be1 = find_w(h, K("block1.0.beta"), D);
        const auto* a2 = find_w(h, K("block2.0.alpha"), D);
        const auto* be2 = find_w(h, K("block2.0.beta"), D);
        if (!W || !b2 || !Wt || !b1 || !a1 || !be1 || !a2 || !be2) return LS_ESTATE;
        memcpy(&wc[(size_t)l * D * D], W->data(), (size_t)D * D * sizeof(float));
        memcpy(&bc[(size_t)l * D], b2->data(), D * sizeof(float));
        memcpy(&wt[(size_t)l * S * S], Wt->data(), (size_t)S * S * sizeof(float));
        memcpy(&bt[(size_t)l * S], b1->data(), S * sizeof(float));
        memcpy(&l1a[(size_t)l * D], a1->data(), D * sizeof(float));
        memcpy(&l1b[(size_t)l * D], be1->data(), D * sizeof(float));
        memcpy(&l2a[(size_t)l * D], a2->data(), D * sizeof(float));
        memcpy(&l2b[(size_t)l * D], be2->data(), D * sizeof(float));
    }
    const auto* Win = find_w(h, "input_mapping.weight", (size_t)D * KIN);
    const auto* Wout = find_w(h, "output_process.poseFinal.weight", (size_t)JF * D);
    const auto* bo = find_w(h, "output_process.poseFinal.bias", JF);
    if (!Win || !Wout || !bo) return LS_ESTATE;
    std::vector<float> winx((size_t)D * JFP, 0.f);                                      // x_t columns, K padded to whole GEMM tiles
    for (int n = 0; n < D; ++n)
        for (int k = 0; k < JF; ++k) winx[(size_t)n * JFP + k] = (*Win)[(size_t)n * KIN + k];
    int rc;
#define UP(buf, vec) if ((rc = upload(h, h->buf, (vec).data(), (vec).size() * sizeof(float))) != LS_OK) return rc
    if (S <= 160) {                                                                     // operand image of the fused token-mixing kernel
        // per-lane fragment order: img[l][q][mt][lane = s16 + 16 g][e] = Wt[l][16 mt + s16][16 q + 4 g + e], zero beyond S; the token
        // axis is padded to 48 (three tiles: the reference's 35 / 36 tokens) or to 160
        const int P = S <= 48 ? 48 : 160, NT = P / 16;
        h->tokpad = P;
        std::vector<float> wtp((size_t)L * P * P, 0.f);
        for (int l = 0; l < L; ++l)
            for (int q = 0; q < NT; ++q)
                for (int mt = 0; mt < NT; ++mt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int r = 16 * mt + (lane & 15), k = 16 * q + 4 * (lane >> 4) + e;
                            if (r < S && k < S) wtp[(size_t)l * P * P + (((size_t)q * NT + mt) * 64 + lane) * 4 + e] = wt[((size_t)l * S + r) * S + k];
                        }
        UP(lw_wtp, wtp);
    } else {
        h->lw_wtp.release();
    }
    UP(lw_wt, wt); UP(lw_bt, bt); UP(lw_wc, wc); UP(lw_bc, bc); UP(ln1a, l1a); UP(ln1b, l1b); UP(ln2a, l2a); UP(ln2b, l2b);
    if (!h->fused && mix_supports(S)) {
        // operand images of the one-launch mixer (ls_mix_kernel.h).  wtok[l][q][mt][lane][e] = Wt[16 mt + s16][16 q + 4 e + g] (zero beyond S):
        // the four lane groups of an MFMA k step read four CONSECUTIVE rows of the LDS operand; wch[l][gb][q][lane][j] = W'[16 gb + s16][16 q + 4 g + j]
        std::vector<float> wtk((size_t)L * 100 * 256, 0.f), wch((size_t)L * D * D);
        for (int l = 0; l < L; ++l) {
            for (int q = 0; q < 10; ++q)
                for (int mt = 0; mt < 10; ++mt)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e) {
                            const int r = 16 * mt + (lane & 15), k = 16 * q + 4 * e + (lane >> 4);
                            if (r < S && k < S) wtk[(size_t)l * 25600 + (((size_t)q * 10 + mt) * 64 + lane) * 4 + e] = wt[((size_t)l * S + r) * S + k];
                        }
            for (int gb = 0; gb < 32; ++gb)
                for (int q = 0; q < 32; ++q)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j) {
                            const int n = 16 * gb + (lane & 15), k = 16 * q + 4 * (lane >> 4) + j;
                            wch[(size_t)l * D * D + (((size_t)gb * 32 + q) * 64 + lane) * 4 + j] = wc[((size_t)l * D + n) * D + k] * l2a[(size_t)l * D + k];
                        }
        }
        UP(mx_wtok, wtk); UP(mx_wch, wch);
    }
    if (S <= 160) {     // fused form: LayerNorm 2 folded around the channel-mixing product (ls_long.hip): W' = W diag(alpha2), bias' = b + W beta2,
                        // wsum[n] = sum_k W'[n][k] (the row's mean enters the epilogue as  - mean * wsum)
        std::vector<float> wcf((size_t)L * D * D), bcf((size_t)L * D), wsum((size_t)L * D);
        for (int l = 0; l < L; ++l)
            for (int n = 0; n < D; ++n) {
                double sb = bc[(size_t)l * D + n], sw = 0.0;
                for (int k = 0; k < D; ++k) {
                    const float wv = wc[((size_t)l * D + n) * D + k];
                    const float wf = wv * l2a[(size_t)l * D + k];
                    wcf[((size_t)l * D + n) * D + k] = wf;
                    sb += (double)wv * (double)l2b[(size_t)l * D + k];
                    sw += (double)wf;
                }
                bcf[(size_t)l * D + n] = (float)sb;
                wsum[(size_t)l * D + n] = (float)sw;
            }
        UP(lw_wcf, wcf); UP(lw_bcf, bcf); UP(lw_wsum, wsum);
    }
    // poseFinal rows padded with zero rows to whole 128-column GEMM tiles: N = 282 would send the product down the general staging
    // path (41 TFLOP/s at 9728 rows); as 384 columns it is a full-tile LDS-DMA product, the extra columns are never read
    const int JFN = (JF + 127) / 128 * 128;
    std::vector<float> woutp((size_t)JFN * D, 0.f);
    memcpy(woutp.data(), Wout->data(), (size_t)JF * D * sizeof(float));
    UP(lw_winx, winx); UP(lw_wout, woutp); UP(bout, *bo);
    h->mx_npt = 0;
    if (!h->fused && mix_supports(S) && (JF + 15) / 16 <= 20) {
        // poseFinal inside the mixer: wpose[nb][q][lane][j] = Wout[16 nb + s16][16 q + 4 g + j], zero rows beyond JF
        const int npt = (JF + 15) / 16;
        std::vector<float> wp((size_t)npt * 32 * 256, 0.f);
        for (int nb = 0; nb < npt; ++nb)
            for (int q = 0; q < 32; ++q)
                for (int lane = 0; lane < 64; ++lane)
                    for (int j = 0; j < 4; ++j) {
                        const int n = 16 * nb + (lane & 15), k = 16 * q + 4 * (lane >> 4) + j;
                        if (n < JF) wp[(((size_t)nb * 32 + q) * 64 + lane) * 4 + j] = (*Wout)[(size_t)n * D + k];
                    }
        UP(mx_wpose, wp);
        h->mx_npt = npt;
    }
#undef UP
    return LS_OK;
}

int build_images(ls_handle* h) {
    // a 34-frame model carries both forms: the fused kernel (one workgroup per sample) and the batch-level kernels small batches run on
    int rc = build_long_weights(h);
    if (rc != LS_OK) return rc;
    if (h->fused && (rc = build_fused_images(h)) != LS_OK) return rc;
    if ((rc = build_shared_weights(h)) != LS_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return LS_OK;
}

// temb[i] = time_embed(pe[timestep_map[i]])  (TimestepEmbedder, mlp_module.py:123-136), one row per schedule index
int build_temb_rows(ls_handle* h, const long long* idx_dev, int n, DevBuf& tmp, DevBuf& out) {
    HIPCHK(h, tmp.ensure((size_t)2 * n * kD * sizeof(float)));
    HIPCHK(h, out.ensure((size_t)n * kD * sizeof(float)));
    float* rows = tmp.f();
    float* hid = tmp.f() + (size_t)n * kD;
    HIPCHK(h, launch_gather_rows(h->pe.f(), reinterpret_cast<const int64_t*>(idx_dev), rows, n, kD, kPeRows, h->stream));
    HIPCHK(h, launch_gemm_nt(rows, kD, h->te_w0.f(), kD, h->te_b0.f(), nullptr, 0, hid, kD, n, kD, kD, 1, h->stream));
    HIPCHK(h, launch_gemm_nt(hid, kD, h->te_w2.f(), kD, h->te_b2.f(), nullptr, 0, out.f(), kD, n, kD, kD, 0, h->stream));
    return LS_OK;
}

int ensure_temb_table(ls_handle* h) {
    if (h->temb_valid) return LS_OK;
    int rc = upload(h, h->tmap_dev, h->tmap.data(), h->tmap.size() * sizeof(long long));
    if (rc != LS_OK) return rc;
    rc = build_temb_rows(h, static_cast<const long long*>(h->tmap_dev.p), h->n_steps, h->temb_tmp, h->temb);
    if (rc != LS_OK) return rc;
    h->temb_valid = true;
    return LS_OK;
}

// (sample, pass) groups of the sample-split kernel resident at once, by slicing: ncb = 1 (8 slices of 64 channels): two workgroups per CU;
// ncb = 2 / 4 (4 / 2 slices): one per CU (their registers).  The slices of a group wait for each other, so a launch never exceeds this.
int coop_cap(int n_cu, int ncb) {
    const int cap = (ncb == 1 ? 2 : 1) * n_cu / (8 / ncb);
    return ncb == 1 && cap > kCoopMaxGroups ? kCoopMaxGroups : cap;
}
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

// samples of the plan's piece on kernel family `path` (0 if the plan has none)
int seg_n(const ls_handle* h, int path) {
    for (int i = 0; i < h->nseg; ++i) if (h->seg[i].path == path) return h->seg[i].n;
    return 0;
}
// everything that identifies the plan (graph key, "did the plan change")
long long plan_code(const ls_handle* h) {
    long long c = h->nseg;
    for (int i = 0; i < h->nseg; ++i) c = c * 8209 + h->seg[i].path + 4 * (long long)h->seg[i].n;
    return c;
}

// One diffusion step of the prepared batch on the kernels decide_path chose.
// precision 0 (fp32): split-fp32 channel mixing on the bf16 matrix cores (k_step<..,2>); 1: bf16x3 (k_step<..,1>); 2 (fp32_mfma):
// every contraction on the fp32 MFMA (k_step<..,0>).  The other step kernels have no split-fp32 form: modes 0 and 2 run them as fp32.
// pair: the single-pass variant (two samples' cond pass per workgroup), legal when every guidance scale is 1
int step_prec(const ls_handle* h) { return h->precision == LS_PRECISION_BF16X3 ? 1 : h->precision == LS_PRECISION_FP32_MFMA ? 0 : 2; }
bool plan_applies(const ls_handle* h, const StepArgs& s, bool pair) {
    if (!h->fused) return true;                                        // batch-level kernels only
    if (s.trace) return false;                                         // the residual-stream trace exists in the fused kernel only
    if (h->nseg > 1 && pair != h->plan_pair) return false;             // a split plan was costed for the other form
    for (int i = 0; i < h->nseg; ++i)
        if (h->seg[i].path == 1 && s.temb_stride != 0) return false;   // per-sample timestep rows: every kernel but the batch-level ones
    return true;
}
hipError_t run_step(ls_handle* h, StepArgs& s, int B, bool pair, hipStream_t st) {
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


// prepare_ms of an ls_prepare_async whose work has finished (called behind every stream synchronisation; `block`: wait for it)
void resolve_prepare_timing(ls_handle* h, bool block) {
    if (!h->prepare_pending) return;
    if (block ? hipEventSynchronize(h->ev[5]) != hipSuccess : hipEventQuery(h->ev[5]) != hipSuccess) return;
    if (hipEventElapsedTime(&h->timing.prepare_ms, h->ev[4], h->ev[5]) == hipSuccess) h->prepare_pending = false;
}

// p_mean_variance's inpainting inputs (gaussian_diffusion.py:314-320) -> device, mask and motion in the internal [B][T][JF] layout
int stage_inpainting(ls_handle* h, const unsigned char* mask, const float* motion, const float* noise, size_t noise_elems, int on_device) {
    const int B = h->B, JF = h->JF;
    const size_t nelem = (size_t)B * JF * h->T, nx = nelem * sizeof(float);
    hipStream_t st = h->stream;
    const void* old[4] = {h->inp_m8.p, h->inp_maskf.p, h->inp_motion.p, h->inp_tape.p};
    int rc;
    if ((rc = ingest(h, h->inp_m8, mask, nelem, on_device)) != LS_OK) return rc;
    HIPCHK(h, h->xtmp.ensure(nx)); HIPCHK(h, h->xio.ensure(nx)); HIPCHK(h, h->inp_maskf.ensure(nx)); HIPCHK(h, h->inp_motion.ensure(nx));
    HIPCHK(h, launch_bytes_to_float(static_cast<const unsigned char*>(h->inp_m8.p), h->xio.f(), nelem, st));
    HIPCHK(h, launch_to_internal(h->xio.f(), h->inp_maskf.f(), B, JF, st, h->T));
    if ((rc = ingest(h, h->xio, motion, nx, on_device)) != LS_OK) return rc;
    HIPCHK(h, launch_to_internal(h->xio.f(), h->inp_motion.f(), B, JF, st, h->T));
    if (noise && (rc = ingest(h, h->inp_tape, noise, noise_elems * sizeof(float), on_device)) != LS_OK) return rc;
    if (old[0] != h->inp_m8.p || old[1] != h->inp_maskf.p || old[2] != h->inp_motion.p || old[3] != h->inp_tape.p) free_graph(h);
    return LS_OK;
}

// LS_SAMPLER_PLMS: the planes of plms_buf (stride in floats through *stride); a captured loop holds their addresses
int plms_planes(ls_handle* h, size_t nelem, size_t* stride) {
    const size_t ps = (nelem + 3) & ~(size_t)3;
    const void* old = h->plms_buf.p;
    HIPCHK(h, h->plms_buf.ensure(5 * ps * sizeof(float)));
    if (old != h->plms_buf.p) free_graph(h);
    *stride = ps;
    return LS_OK;
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

// the launch behind a denoiser launch with sampler = kNone: mix, clamp, update (coefficients as fill_sampler left them in `s`)
hipError_t run_inpaint_update(ls_handle* h, const StepArgs& s, int i, bool noised, const float* inoise, const float* noise, int const_noise,
                              float* x_out, float* dump, unsigned step_id, int clip, int B, hipStream_t st) {
    InpaintArgs ia{};
    ia.x_t = s.x_in; ia.x0 = h->fwd_cfg.f(); ia.maskf = h->inp_maskf.f(); ia.motion = h->inp_motion.f();
    ia.renoise = noised && i > 0;                                      // `if t[0] > 0` (:318)
    ia.inoise = ia.renoise ? inoise : nullptr;
    ia.noise = noise; ia.const_noise = const_noise; ia.out = x_out; ia.dump = dump;
    ia.call = s.call; ia.step_id = step_id;
    ia.JF = h->JF; ia.T = h->T; ia.sampler = s.sampler; ia.t_nonzero = s.t_nonzero; ia.clip = clip;
    if (i > 0) { ia.qa = (float)h->t_sac[i - 1]; ia.qb = (float)h->t_s1mac[i - 1]; }       // q_sample(., t - 1), cast like _extract_into_tensor
    ia.c0 = s.c0; ia.c1 = s.c1; ia.c2 = s.c2; ia.c3 = s.c3; ia.c4 = s.c4;
    return launch_inpaint_update(ia, B, st);
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

void decide_path(ls_handle* h) {
    const long long before = plan_code(h);
    h->plan_pair = h->all_scale_one;
    const PlanOut o = plan_steps(PlanIn{h->var == kTED, h->fused, h->lw_wtp.p != nullptr, h->plan_pair, h->B, h->precision, h->path_mode, h->n_cu,
                                        h->coop_groups_max, h->cfg.layers, h->coop_ncb});
    h->nseg = o.nseg;
    for (int i = 0; i < 3; ++i) h->seg[i] = o.seg[i];
    h->use_long = h->nseg == 1 && h->seg[0].path == 1;
    h->use_coop = h->nseg == 1 && h->seg[0].path == 2;
    h->use_pass = h->nseg == 1 && h->seg[0].path == 3;
    if (before != plan_code(h)) free_graph(h);
}

// zero the granule / flag words of the sample-split kernel (stream-ordered: a memset node when captured) and restart the epochs
hipError_t coop_reset(ls_handle* h, hipStream_t st) {
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
hipError_t pass_reset(ls_handle* h, hipStream_t st) {
    if (seg_n(h, 3) == 0 || !h->pa_cnt.p) return hipSuccess;
    return hipMemsetAsync(h->pa_cnt.p, 0, h->pa_cnt.bytes, st);
}

int advance_tags(ls_handle* h, hipStream_t st) {
    HIPCHK(h, pass_reset(h, st));
    const unsigned long long span = ((unsigned long long)h->coop_launches + 2ull) * kCoopEpochStride;
    h->tag_base += span > (1ull << 21) ? (unsigned)span : (1u << 21);
    h->call_host.tag_base = h->tag_base;
    HIPCHK(h, hipMemcpyAsync(h->callp.p, &h->call_host, sizeof(CallParams), hipMemcpyHostToDevice, st));
    return LS_OK;
}

// after a stream synchronisation: did a hand-off spin of the sample-split kernel run out?  (Never observed; a result computed past a
// timeout is garbage, so the call fails loudly.)
int coop_check(ls_handle* h) {
    if (seg_n(h, 2) == 0 && h->mix_cap == 0) return LS_OK;
    unsigned v = 0;
    HIPCHK(h, hipMemcpy(&v, h->co_err.p, sizeof v, hipMemcpyDeviceToHost));
    if (!v) return LS_OK;
    HIPCHK(h, hipMemset(h->co_err.p, 0, sizeof v));
    return fail(h, LS_EHIP, "sample-split step kernel: an inter-workgroup hand-off timed out; the results of this call are invalid");
}
void report_path(ls_handle* h, bool pair) {
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

// ls_sample with seg_count > 0: one piece of a TAPE-mode loop (see ls_sample_args in ls_hip.h)
int sample_segment(ls_handle* h, const ls_sample_args* a) {
    if (a->noise_mode != LS_NOISE_TAPE) return fail(h, LS_EINVAL, "segmented sampling is for TAPE mode (PHILOX needs no tapes)");
    if (a->inpaint_mask) return fail(h, LS_EUNSUPPORTED, "the inpainting branch is not combined with segmented tapes");
    if (!a->eps_tape || !a->noise_tape) return fail(h, LS_EINVAL, "segment needs eps_tape and noise_tape");
    if (a->n_dump > 0 && (a->sampler != LS_SAMPLER_DDPM || !a->dump_steps || !a->dump_out))
        return fail(h, LS_EINVAL, "dump_steps: DDPM only (ddim_sample_loop raises NotImplementedError, gaussian_diffusion.py:919-920)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, JF = h->JF, od = a->on_device;
    const int n_exec = h->n_steps - a->skip_timesteps;
    if (a->seg_begin < 0 || a->seg_begin + a->seg_count > n_exec) return fail(h, LS_EINVAL, "segment [%d, %d) outside the loop's %d steps", a->seg_begin, a->seg_begin + a->seg_count, n_exec);
    const bool last = a->seg_begin + a->seg_count == n_exec;
    if (last && !a->out) return fail(h, LS_EINVAL, "ls_sample: null out");
    const size_t nelem = (size_t)B * JF * h->T;
    const size_t nx = nelem * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    if (a->seg_begin == 0) {
        if (!a->x_init) return fail(h, LS_EINVAL, "TAPE mode needs x_init");
        HIPCHK(h, hipEventRecord(h->ev[0], st));
        HIPCHK(h, h->xa.ensure(nx)); HIPCHK(h, h->xb.ensure(nx)); HIPCHK(h, h->xtmp.ensure(nx)); HIPCHK(h, h->xio.ensure(nx));
        if ((rc = ingest(h, h->xio, a->x_init, nx, od)) != LS_OK) return rc;
        HIPCHK(h, launch_to_internal(h->xio.f(), h->xa.f(), B, JF, st, h->T));
        const int first_index = n_exec - 1;
        if (a->init_image || a->skip_timesteps > 0) {
            if (a->init_image) {
                if ((rc = ingest(h, h->xio, a->init_image, nx, od)) != LS_OK) return rc;
                HIPCHK(h, launch_to_internal(h->xio.f(), h->xtmp.f(), B, JF, st, h->T));
            } else {
                HIPCHK(h, hipMemsetAsync(h->xtmp.p, 0, nx, st));
            }
            HIPCHK(h, launch_q_sample(h->xtmp.f(), h->xa.f(), h->xa.f(), nelem, (float)h->t_sac[first_index], (float)h->t_s1mac[first_index], st));
        }
        if (a->n_dump > 0) {
            const void* old = h->dump.p;
            HIPCHK(h, h->dump.ensure((size_t)a->n_dump * nx));
            if (old != h->dump.p) free_graph(h);
        }
        if ((rc = advance_tags(h, st)) != LS_OK) return rc;
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
    if (od) {
        HIPCHK(h, hipMemcpyAsync(h->eps_slot[slot].p, a->eps_tape, eps_bytes, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, hipMemcpyAsync(h->noise_slot[slot].p, a->noise_tape, nz_bytes, hipMemcpyDeviceToDevice, st));
    } else {
        HIPCHK(h, hipEventRecord(h->ev_cs[slot], h->copy_stream));
        HIPCHK(h, hipMemcpyAsync(h->eps_slot[slot].p, a->eps_tape, eps_bytes, hipMemcpyHostToDevice, h->copy_stream));
        HIPCHK(h, hipMemcpyAsync(h->noise_slot[slot].p, a->noise_tape, nz_bytes, hipMemcpyHostToDevice, h->copy_stream));
        HIPCHK(h, hipEventRecord(h->ev_cd[slot], h->copy_stream));
        h->upload_open[slot] = true;
        HIPCHK(h, hipStreamWaitEvent(st, h->ev_cd[slot], 0));
        if ((rc = close_upload(h, slot ^ 1)) != LS_OK) return rc;              // the PREVIOUS segment's host buffers are free from here on
    }
    const bool pair = h->fused && !h->use_long && h->all_scale_one && !a->two_pass_always;
    for (int k = a->seg_begin; k < a->seg_begin + a->seg_count; ++k) {
        const int i = n_exec - 1 - k, r = k - a->seg_begin;
        StepArgs s;
        fill_common(h, s);
        fill_sampler(h, s, a->sampler, i, a->eta);
        s.clip_denoised = a->clip_denoised;
        s.x_in = (k & 1) ? h->xb.f() : h->xa.f();
        s.x_out = (k & 1) ? h->xa.f() : h->xb.f();
        s.temb = h->temb.f() + (size_t)i * kD; s.temb_stride = 0;
        s.step_id = (unsigned)k;
        s.eps_c = h->eps_slot[slot].f() + ((size_t)r * 2 + 0) * B * kD;
        s.eps_u = h->eps_slot[slot].f() + ((size_t)r * 2 + 1) * B * kD;
        s.noise = h->noise_slot[slot].f() + (size_t)r * nelem;
        s.const_noise = a->const_noise;
        for (int d = 0; d < a->n_dump; ++d)
            if (a->dump_steps[d] == k) s.x0_out = h->dump.f() + (size_t)d * nelem;
        HIPCHK(h, run_step(h, s, B, pair, st));
    }
    HIPCHK(h, hipEventRecord(h->ev_seg[slot], st));
    h->slot_used[slot] = true;
    h->seg_next = a->seg_begin + a->seg_count;
    h->seg_index++;
    if (!last) return LS_OK;
    HIPCHK(h, hipEventRecord(h->ev[2], st));
    const float* final_x = (n_exec & 1) ? h->xb.f() : h->xa.f();
    HIPCHK(h, launch_from_internal(final_x, h->xio.f(), B, JF, st, h->T));
    if ((rc = egress(h, a->out, h->xio.f(), nx, od)) != LS_OK) return rc;
    for (int d = 0; d < a->n_dump; ++d) {
        HIPCHK(h, launch_from_internal(h->dump.f() + (size_t)d * nelem, h->xio.f(), B, JF, st, h->T));
        if ((rc = egress(h, a->dump_out + (size_t)d * nelem, h->xio.f(), nx, od)) != LS_OK) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[3], st));
    HIPCHK(h, hipStreamSynchronize(st));
    resolve_prepare_timing(h, true);
    if ((rc = close_upload(h, 0)) != LS_OK || (rc = close_upload(h, 1)) != LS_OK) return rc;
    if ((rc = coop_check(h)) != LS_OK) return rc;
    report_path(h, pair);
    HIPCHK(h, hipEventElapsedTime(&h->timing.loop_ms, h->ev[1], h->ev[2]));
    HIPCHK(h, hipEventElapsedTime(&h->timing.total_ms, h->ev[0], h->ev[3]));
    h->timing.n_step_launches = n_exec;
    h->timing.single_pass = pair ? 1 : 0;
    h->timing.graph_replayed = 0;
    h->timing.tape_upload_ms = h->seg_upload_ms;
    h->timing.n_segments = h->seg_index;
    h->seg_next = -1;
    return LS_OK;
}

}  // namespace

extern "C" {

int ls_abi_version(void) { return LS_ABI_VERSION; }

const char* ls_last_error(const ls_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ls_create(const ls_config* cfg, ls_handle** out) {
    if (!cfg || !out) return fail(nullptr, LS_EINVAL, "ls_create: null argument");
    *out = nullptr;
    if (cfg->latent_dim != kD) return fail(nullptr, LS_EUNSUPPORTED, "latent_dim must be %d", kD);
    if (cfg->nframes < cfg->n_pre_seq || cfg->nframes < 1 || cfg->nframes > 4096) return fail(nullptr, LS_EINVAL, "nframes out of range");
    const int JF = cfg->njoints * cfg->nfeats;
    Variant var;
    if (JF == 27 && cfg->n_prefix_tokens == 1) var = kTED;
    else if (JF == 282 && cfg->n_prefix_tokens == 2) var = kBEAT;
    else return fail(nullptr, LS_EUNSUPPORTED, "unsupported shape: J*F=%d with %d prefix tokens (built: 27/1 TED, 282/2 BEAT)",
                     JF, cfg->n_prefix_tokens);
    if (cfg->layers < 1 || cfg->layers > 64) return fail(nullptr, LS_EINVAL, "layers out of range");
    if (cfg->n_prefix_tokens == 2 && cfg->n_emotions <= 0) return fail(nullptr, LS_EINVAL, "BEAT variant needs n_emotions > 0");
    int L = cfg->audio_len;
    int convL[5];
    convL[0] = L;
    for (int i = 0; i < 4; ++i) {
        L = (L + 2 * kConvPad[i] - 15) / kConvStride[i] + 1;
        convL[i + 1] = L;
    }
    if (L != cfg->nframes) return fail(nullptr, LS_EINVAL, "audio_len %d yields %d audio frames, need %d", cfg->audio_len, L, cfg->nframes);
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail(nullptr, LS_EHIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));
    ls_handle* h = new ls_handle();
    h->cfg = *cfg;
    {   // chip geometry: the step-time models were measured on 256 CUs; rounds, residency and the throughput-bound terms follow the device
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, cfg->device);
        if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "hipGetDeviceProperties(%d): %s", cfg->device, hipGetErrorString(e)); }
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
    h->var = var;
    h->JF = JF;
    h->T = cfg->nframes;
    h->fused = cfg->nframes == kT;          // the reference's 34 frames: fused step kernel; otherwise the long-sequence path
    h->JFP = (JF + 31) / 32 * 32;
    h->S = h->T + cfg->n_prefix_tokens;
    h->R = 2 * h->S;
    h->NOB = (JF + 15) / 16;
    h->KXQ = (JF + 15) / 16;
    h->MK = (h->R + 3) / 4;
    h->KIN = 2 * JF + 1 + kAudioFeat;
    h->KF = JF + 1 + kAudioFeat;
    h->KFP = (h->KF + 31) / 32 * 32;
    h->KPP = (JF + 1 + 31) / 32 * 32;
    memcpy(h->convL, convL, sizeof convL);
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    e = hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    for (auto& ev : h->ev) {
        e = hipEventCreate(&ev);
        if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "hipEventCreate: %s", hipGetErrorString(e)); }
    }
    for (int i = 0; i < 2; ++i) {
        hipEvent_t* evs[3] = {&h->ev_cs[i], &h->ev_cd[i], &h->ev_seg[i]};
        for (hipEvent_t* pe : evs) {
            e = hipEventCreate(pe);
            if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "hipEventCreate: %s", hipGetErrorString(e)); }
        }
    }
    e = init_step_kernels();
    if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "hipFuncSetAttribute(step kernel LDS): %s", hipGetErrorString(e)); }
    if (!h->fused && mix_supports(cfg->nframes + cfg->n_prefix_tokens)) {
        e = init_mix_kernels();
        if (e == hipSuccess) e = h->co_err.ensure(sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(h->co_err.p, 0, sizeof(unsigned), h->stream);
        if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "long-sequence mixer kernel setup: %s", hipGetErrorString(e)); }
    }
    if (h->fused) {         // sample-split kernel: LDS opt-in and one launch's worth of exchange workspaces (independent of the batch)
        e = init_coop_kernels();
        if (e == hipSuccess) e = init_pass_kernels();
        if (e == hipSuccess) e = h->co_err.ensure(sizeof(unsigned));
        if (e == hipSuccess) e = hipMemsetAsync(h->co_err.p, 0, sizeof(unsigned), h->stream);
        if (e != hipSuccess) { delete h; return fail(nullptr, LS_EHIP, "sample-split kernel setup: %s", hipGetErrorString(e)); }
    }
#ifdef LS_DEBUG
    if (h->prof_on) {
        std::vector<unsigned long long> z((size_t)kWaves * kProfPoints, 0ull);
        if (upload(h, h->prof, z.data(), z.size() * sizeof(unsigned long long)) != LS_OK) { g_create_error = h->err; delete h; return LS_EHIP; }
        std::vector<unsigned long long> zw(4096, 0ull);      // [1024][2] stamps | [2048] hardware ids (k_pass)
        if (upload(h, h->wgt, zw.data(), zw.size() * sizeof(unsigned long long)) != LS_OK) { g_create_error = h->err; delete h; return LS_EHIP; }
    }
#endif
    CallParams cp{0, 0, 0, 0};
    if (upload(h, h->callp, &cp, sizeof cp) != LS_OK) { g_create_error = h->err; delete h; return LS_EHIP; }
    *out = h;
    return LS_OK;
}

void ls_destroy(ls_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_graph(h);
    DevBuf* all[] = {&h->wch_hi_img, &h->wch_lo_img, &h->wch_lo2_img, &h->ww_hi_img, &h->ww_lo_img, &h->wch_img, &h->bch, &h->ln1a, &h->ln1b, &h->ln2a, &h->ln2b, &h->ww_img, &h->btok_rows, &h->winx_img,
                     &h->wout_img, &h->wout_reg_img, &h->bout, &h->devw, &h->win_full, &h->win_pre, &h->win_aud, &h->win_bias, &h->spk_emb, &h->ml_w, &h->ml_b,
                     &h->emo_emb, &h->te_w0, &h->te_b0, &h->te_w2, &h->te_b2, &h->pe, &h->temb, &h->temb_tmp,
                     &h->tmap_dev, &h->audio, &h->origin_x, &h->vid, &h->emo, &h->scale, &h->c1, &h->c2, &h->c3, &h->c4,
                     &h->st1, &h->st2, &h->st3, &h->feat_c, &h->feat_u, &h->static_c, &h->static_u, &h->z, &h->z_ml, &h->z_mu,
                     &h->z_logvar, &h->z_std, &h->emo_tok, &h->audio_feat, &h->spart, &h->xa, &h->xb, &h->xtmp, &h->xio, &h->fwd_c,
                     &h->fwd_u, &h->fwd_cfg, &h->eps, &h->noise, &h->tfwd, &h->tfwd_tmp, &h->tidx, &h->dump, &h->trace,
                     &h->callp, &h->eps_tape, &h->noise_tape, &h->lw_wt, &h->lw_wtp, &h->lx_part1, &h->lx_part2, &h->lw_bt, &h->lw_wc, &h->lw_bc, &h->lw_wcf, &h->lw_bcf, &h->lw_wsum, &h->lw_winx, &h->lw_wout,
                     &h->lx_proj, &h->lx_X, &h->lx_U, &h->lx_OUT, &h->lx_xpad, &h->mx_wtok, &h->mx_wch, &h->mx_wpose, &h->mx_pout, &h->mx_xg, &h->mx_gran, &h->wtok1_img, &h->co_x, &h->co_part, &h->co_gran, &h->co_flag, &h->co_err, &h->pa_out, &h->pa_cnt, &h->wtail, &h->wtok1_hi_img, &h->wtok1_lo_img};
    for (DevBuf* d : all) d->release();
#ifdef LS_DEBUG
    h->prof.release();
    h->wgt.release();
#endif
    for (int i = 0; i < 4; ++i) { h->conv_w[i].release(); h->conv_b[i].release(); h->conv_img[i].release(); }
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < 2; ++i) {
        h->eps_slot[i].release(); h->noise_slot[i].release();
        if (h->ev_cs[i]) (void)hipEventDestroy(h->ev_cs[i]);
        if (h->ev_cd[i]) (void)hipEventDestroy(h->ev_cd[i]);
        if (h->ev_seg[i]) (void)hipEventDestroy(h->ev_seg[i]);
    }
    h->coef.release();
    h->plms_buf.release();
    h->inp_m8.release(); h->inp_maskf.release(); h->inp_motion.release(); h->inp_tape.release();
    h->trng_eps.release(); h->trng_noise.release(); h->trng_inz.release();
    if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
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
    free_graph(h);
    return LS_OK;
}

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
    {   // guidance scale 1 for the whole batch (what the reference's callers run: test_RAG_ted.py:183): out_u + 1 * (out_c - out_u)
        // is out_c, so the sampling loop may skip the uncond pass (ls_sample_args.two_pass_always keeps both)
        std::vector<float> sc((size_t)B);
        if (od) {           // read back the ingested copy on the handle's own stream: ordered behind the caller's stream (ls_stream_order)
            HIPCHK(h, hipMemcpyAsync(sc.data(), h->scale.p, (size_t)B * sizeof(float), hipMemcpyDeviceToHost, st));
            HIPCHK(h, hipStreamSynchronize(st));
        } else {
            memcpy(sc.data(), c->scale, (size_t)B * sizeof(float));
        }
        h->all_scale_one = true;
        for (float v : sc) if (v != 1.0f) { h->all_scale_one = false; break; }
    }

    // ---- WavEncoder (audio_enc.py:6-25): conv -> [IN + LReLU fused into the next conv's staging] x3 -> conv
    const int* Lc = h->convL;
    DevBuf* outs[4] = {&h->c1, &h->c2, &h->c3, &h->c4};
    DevBuf* stats[3] = {&h->st1, &h->st2, &h->st3};
    const float* in = od ? static_cast<const float*>(c->audio_input) : h->audio.f();
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
    // ---- speaker style (RAG.py:116-119): z = Embedding[vid]; mu, logvar = Linear(z); std = exp(0.5*logvar)
    HIPCHK(h, h->z.ensure((size_t)B * 256 * sizeof(float)));
    HIPCHK(h, h->z_mu.ensure((size_t)B * kD * sizeof(float)));
    HIPCHK(h, h->z_logvar.ensure((size_t)B * kD * sizeof(float)));
    HIPCHK(h, h->z_std.ensure((size_t)B * kD * sizeof(float)));
    HIPCHK(h, launch_gather_rows(h->spk_emb.f(), static_cast<const int64_t*>(h->vid.p), h->z.f(), B, 256, h->cfg.n_speakers, st));
    HIPCHK(h, h->z_ml.ensure((size_t)B * 2 * kD * sizeof(float)));
    HIPCHK(h, launch_gemm_nt(h->z.f(), 256, h->ml_w.f(), 256, h->ml_b.f(), nullptr, 0, h->z_ml.f(), 2 * kD, B, 2 * kD, 256, 0, st));
    HIPCHK(h, launch_split_style(h->z_ml.f(), h->z_mu.f(), h->z_logvar.f(), h->z_std.f(), B, st));
    if (h->cfg.n_prefix_tokens == 2) {   // scripts_beat/model/RAG.py:125
        HIPCHK(h, h->emo_tok.ensure((size_t)B * kD * sizeof(float)));
        HIPCHK(h, launch_gather_rows(h->emo_emb.f(), static_cast<const int64_t*>(h->emo.p), h->emo_tok.f(), B, kD, h->cfg.n_emotions, st, h->T));   // y['emo'][:, 0]
    }
    { const int keepB = h->B; h->B = B; decide_path(h); h->B = keepB; }
    if (seg_n(h, 2) > 0) {      // exchange workspaces of the sample-split kernel: one launch's worth of (sample, pass) groups
        const int nco = seg_n(h, 2);
        int gcap = h->coop_groups_max;                  // the most groups any slicing keeps resident (LS_COOP_GROUPS caps all of them in -DLS_DEBUG builds)
        if (gcap == coop_cap(h->n_cu, 1))
            for (int ncb = 2; ncb <= 4; ncb *= 2) if (coop_cap(h->n_cu, ncb) > gcap) gcap = coop_cap(h->n_cu, ncb);
        const int groups = 2 * nco < gcap ? 2 * nco : gcap;
        const void* old[4] = {h->co_x.p, h->co_part.p, h->co_gran.p, h->co_flag.p};
        const size_t before = h->co_x.bytes;
        HIPCHK(h, h->co_x.ensure((size_t)groups * 36 * kD * sizeof(float)));
        if (h->co_x.bytes != before) HIPCHK(h, hipMemsetAsync(h->co_x.p, 0, h->co_x.bytes, st));     // rows a 35-row pass never writes are pulled into LDS (never read)
        HIPCHK(h, h->co_part.ensure((size_t)groups * 8 * 36 * (size_t)h->NOB * 16 * sizeof(float)));
        HIPCHK(h, h->co_gran.ensure((size_t)groups * 2 * 36 * 8 * 2 * sizeof(unsigned long long)));
        HIPCHK(h, h->co_flag.ensure((size_t)groups * 16 * sizeof(unsigned long long)));
        if (old[0] != h->co_x.p || old[1] != h->co_part.p || old[2] != h->co_gran.p || old[3] != h->co_flag.p) free_graph(h);
        h->coop_groups = groups;
    }
    if (seg_n(h, 3) > 0) {      // CFG hand-off of the one-pass-per-workgroup kernel: each pass's output, one ticket word per sample
        const int npa = seg_n(h, 3);
        const void* old[2] = {h->pa_out.p, h->pa_cnt.p};
        HIPCHK(h, h->pa_out.ensure((size_t)npa * 2 * h->T * h->JF * sizeof(float)));
        HIPCHK(h, h->pa_cnt.ensure((size_t)npa * sizeof(unsigned)));
        HIPCHK(h, hipMemsetAsync(h->pa_cnt.p, 0, h->pa_cnt.bytes, st));
        if (old[0] != h->pa_out.p || old[1] != h->pa_cnt.p) free_graph(h);
        h->pass_n = npa;
    }
    if (seg_n(h, 1) > 0) {      // workspaces of the batch-level path: token sequences of both passes (two buffers), row partials, poseFinal output
        const size_t nlo = seg_n(h, 1);
        const void* old[5] = {h->lx_proj.p, h->lx_X.p, h->lx_U.p, h->lx_OUT.p, h->lx_xpad.p};
        const size_t rows = ((size_t)2 * nlo * h->S + 127) / 128 * 128;      // whole 128-row GEMM tiles (the fused channel-mixing product runs over the pad rows too)
        const size_t mpad = ((size_t)nlo * h->T + 127) / 128 * 128;           // x_t projection on whole 128-row tiles (k_long_padx)
        HIPCHK(h, h->lx_proj.ensure(mpad * kD * sizeof(float)));
        HIPCHK(h, h->lx_xpad.ensure(mpad * h->JFP * sizeof(float)));
        { const size_t before = h->lx_X.bytes + h->lx_U.bytes;
          HIPCHK(h, h->lx_X.ensure(rows * kD * sizeof(float)));
          HIPCHK(h, h->lx_U.ensure(rows * kD * sizeof(float)));
          if (h->lx_X.bytes + h->lx_U.bytes != before) {                    // fresh memory: the pad rows must hold finite values (their products are computed and discarded)
              HIPCHK(h, hipMemsetAsync(h->lx_X.p, 0, h->lx_X.bytes, st)); HIPCHK(h, hipMemsetAsync(h->lx_U.p, 0, h->lx_U.bytes, st)); } }
        HIPCHK(h, h->lx_OUT.ensure(rows * (size_t)((h->JF + 127) / 128 * 128) * sizeof(float)));
        { const void* o1 = h->lx_part1.p; const void* o2 = h->lx_part2.p;
          HIPCHK(h, h->lx_part1.ensure(rows * 16 * sizeof(float))); HIPCHK(h, h->lx_part2.ensure(rows * 16 * sizeof(float)));
          if (o1 != h->lx_part1.p || o2 != h->lx_part2.p) {
              HIPCHK(h, hipMemsetAsync(h->lx_part1.p, 0, h->lx_part1.bytes, st)); HIPCHK(h, hipMemsetAsync(h->lx_part2.p, 0, h->lx_part2.bytes, st));
              free_graph(h); } }
        if (old[0] != h->lx_proj.p || old[1] != h->lx_X.p || old[2] != h->lx_U.p || old[3] != h->lx_OUT.p || old[4] != h->lx_xpad.p) free_graph(h);
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
                const void* o[2] = {h->mx_xg.p, h->mx_gran.p};
                HIPCHK(h, h->mx_xg.ensure((size_t)cap * 32 * kMixRows * 16 * sizeof(float)));
                HIPCHK(h, h->mx_gran.ensure((size_t)cap * (2 * kMixRows + 1) * kMixSlices * 2 * sizeof(unsigned long long)));
                if (o[0] != h->mx_xg.p) HIPCHK(h, hipMemsetAsync(h->mx_xg.p, 0, h->mx_xg.bytes, st));       // rows a pass never writes are pulled into LDS (finite, never used)
                if (h->mx_npt > 0) {      // partial poseFinal products of the whole batch: [2 B][4 slices][S][16 npt]
                    const void* op = h->mx_pout.p;
                    HIPCHK(h, h->mx_pout.ensure((size_t)2 * nlo * kMixSlices * h->S * 16 * h->mx_npt * sizeof(float)));
                    if (op != h->mx_pout.p) free_graph(h);
                }
                if (o[0] != h->mx_xg.p || o[1] != h->mx_gran.p) free_graph(h);
                h->mix_cap = cap;
            }
        }
        if (was_cap != h->mix_cap) free_graph(h);
    }
    HIPCHK(h, hipEventRecord(h->ev[5], st));
    if (wait) {
        HIPCHK(h, hipStreamSynchronize(st));
        HIPCHK(h, hipEventElapsedTime(&h->timing.prepare_ms, h->ev[4], h->ev[5]));
        h->prepare_pending = false;
    } else {
        h->timing.prepare_ms = -1.0f;          // until the work is known to be done (next synchronising call / ls_get_timing)
        h->prepare_pending = true;
    }
    if (h->B != B) free_graph(h);
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

int ls_forward(ls_handle* h, const ls_forward_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_forward: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_forward before ls_prepare");
    if (!a->x || !a->timesteps || !a->eps_cond || !a->eps_uncond) return fail(h, LS_EINVAL, "ls_forward: null input");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, JF = h->JF, od = a->on_device;
    const size_t nx = (size_t)B * JF * h->T * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ingest(h, h->xio, a->x, nx, od)) != LS_OK) return rc;
    HIPCHK(h, h->xa.ensure(nx));
    HIPCHK(h, launch_to_internal(h->xio.f(), h->xa.f(), B, JF, st, h->T));
    HIPCHK(h, h->eps.ensure((size_t)2 * B * kD * sizeof(float)));
    HIPCHK(h, hipMemcpyAsync(h->eps.f(), a->eps_cond, (size_t)B * kD * sizeof(float), od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->eps.f() + (size_t)B * kD, a->eps_uncond, (size_t)B * kD * sizeof(float), od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
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
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        HIPCHK(h, launch_from_internal(srcs[i], h->xio.f(), B, JF, st, h->T));
        if ((rc = egress(h, outs[i], h->xio.f(), nx, od)) != LS_OK) return rc;
    }
    if (a->trace && (rc = egress(h, a->trace, h->trace.f(), (size_t)B * (h->cfg.layers + 1) * h->R * kD * sizeof(float), od)) != LS_OK) return rc;
    if (!(a->no_sync && od)) { HIPCHK(h, hipStreamSynchronize(st)); if ((rc = coop_check(h)) != LS_OK) return rc; }
    return LS_OK;
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
    if ((rc = ingest(h, h->xio, a->x, nx, od)) != LS_OK) return rc;
    HIPCHK(h, h->xa.ensure(nx)); HIPCHK(h, h->xb.ensure(nx)); HIPCHK(h, h->fwd_cfg.ensure(nx));
    HIPCHK(h, launch_to_internal(h->xio.f(), h->xa.f(), B, JF, st, h->T));
    HIPCHK(h, h->eps.ensure((size_t)2 * B * kD * sizeof(float)));
    const hipMemcpyKind kind = od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPCHK(h, hipMemcpyAsync(h->eps.f(), a->eps_cond, (size_t)B * kD * sizeof(float), kind, st));
    HIPCHK(h, hipMemcpyAsync(h->eps.f() + (size_t)B * kD, a->eps_uncond, (size_t)B * kD * sizeof(float), kind, st));
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
    const bool pair = h->fused && !h->use_long && h->all_scale_one && !a->two_pass_always;
    if (inpaint) {
        if ((rc = stage_inpainting(h, a->inpaint_mask, a->inpainted_motion, a->inpaint_noise, (size_t)B * JF * h->T, od)) != LS_OK) return rc;
        fill_sampler(h, s, a->sampler, index, a->eta);
        s.noise = h->noise.f();
        s.temb = h->temb.f() + (size_t)index * kD; s.temb_stride = 0;
        StepArgs m = s;
        m.sampler = kNone; m.clip_denoised = 0; m.x_out = nullptr; m.noise = nullptr;
        HIPCHK(h, run_step(h, m, B, pair, st));
        HIPCHK(h, run_inpaint_update(h, s, index, a->inpaint_noise != nullptr, h->inp_tape.f(), s.noise, 0, h->xb.f(), nullptr, 0u,
                                     a->clip_denoised, B, st));
    } else if (!per_sample) {
        fill_sampler(h, s, a->sampler, index, a->eta);
        s.noise = h->noise.f();
        s.temb = h->temb.f() + (size_t)index * kD; s.temb_stride = 0;
        HIPCHK(h, run_step(h, s, B, pair, st));
    } else {
        // denoiser with one timestep-embedding row per sample (what ls_forward does), pred_xstart -> fwd_cfg; then the posterior /
        // DDIM update with per-sample coefficients as its own elementwise kernel, both driven by the index vector on the device
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
        HIPCHK(h, launch_sampler_update(h->xa.f(), h->fwd_cfg.f(), h->noise.f(), h->coef.f(), static_cast<const int64_t*>(h->tidx.p), h->n_steps,
                                        h->xb.f(), B, JF, h->T, a->sampler == LS_SAMPLER_DDPM ? kDDPM : kDDIM, st));
    }
    HIPCHK(h, launch_from_internal(h->xb.f(), h->xio.f(), B, JF, st, h->T));
    if ((rc = egress(h, a->sample, h->xio.f(), nx, od)) != LS_OK) return rc;
    if (a->pred_xstart) {
        HIPCHK(h, h->xtmp.ensure(nx));
        HIPCHK(h, launch_from_internal(h->fwd_cfg.f(), h->xtmp.f(), B, JF, st, h->T));
        if ((rc = egress(h, a->pred_xstart, h->xtmp.f(), nx, od)) != LS_OK) return rc;
    }
    if (!(a->no_sync && od)) { HIPCHK(h, hipStreamSynchronize(st)); if ((rc = coop_check(h)) != LS_OK) return rc; }
    return LS_OK;
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

int ls_sample(ls_handle* h, const ls_sample_args* a) {
    if (!h || !a) return fail(h, LS_EINVAL, "ls_sample: null argument");
    if (!h->prepared) return fail(h, LS_ESTATE, "ls_sample before ls_prepare");
    if (!h->have_sched) return fail(h, LS_ESTATE, "ls_sample before ls_set_schedule");
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
    if (a->seg_count > 0) return sample_segment(h, a);
    h->seg_next = -1;
    if (!a->out) return fail(h, LS_EINVAL, "ls_sample: null out");
    const bool tape = a->noise_mode == LS_NOISE_TAPE;
    const bool tdev = a->noise_mode == LS_NOISE_TORCH_DEVICE;
    if (tape && (!a->x_init || !a->eps_tape || (!a->noise_tape && !plms))) return fail(h, LS_EINVAL, "TAPE mode needs x_init, eps_tape and noise_tape");
    if (!tape && !tdev && a->const_noise) return fail(h, LS_EUNSUPPORTED, "const_noise is supported in TAPE and TORCH_DEVICE modes only");
    if (tdev && (a->sample_offset & 3)) return fail(h, LS_EINVAL, "TORCH_DEVICE: the generator offset %llu is not a multiple of 4", (unsigned long long)a->sample_offset);
    if (a->n_dump > 0 && (a->sampler != LS_SAMPLER_DDPM || !a->dump_steps || !a->dump_out))
        return fail(h, LS_EINVAL, "dump_steps: DDPM only (ddim_sample_loop raises NotImplementedError, gaussian_diffusion.py:919-920)");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int B = h->B, JF = h->JF, od = a->on_device;
    const int n_exec = h->n_steps - a->skip_timesteps;
    const int n_eval = n_exec + (plms ? 1 : 0);           // model evaluations = pairs of style eps
    const size_t nelem = (size_t)B * JF * h->T;
    const size_t nx = nelem * sizeof(float);
    hipStream_t st = h->stream;
    int rc;
    if ((rc = ensure_temb_table(h)) != LS_OK) return rc;
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    HIPCHK(h, h->xa.ensure(nx)); HIPCHK(h, h->xb.ensure(nx)); HIPCHK(h, h->xtmp.ensure(nx)); HIPCHK(h, h->xio.ensure(nx));
    h->call_host = CallParams{a->seed, a->sample_offset, h->tag_base, 0u};
    if ((rc = advance_tags(h, st)) != LS_OK) return rc;          // uploads call_host with this call's tag base

    // x_T (gaussian_diffusion.py:700-707 / :972-977)
    TorchDrawArgs tda{};            // TORCH_DEVICE: the per-step draws (filled in below), x_T's draw first when the call makes it
    tda.call = static_cast<const CallParams*>(h->callp.p);
    tda.B = B; tda.JF = JF; tda.T = h->T; tda.last_step = n_exec - 1;
    const unsigned long long x_adv = (tdev && !a->x_init) ? torch_randn_advance((long long)nelem, h->n_cu, h->max_thr_cu, nullptr) : 0ull;
    if (a->x_init) {
        if ((rc = ingest(h, h->xio, a->x_init, nx, od)) != LS_OK) return rc;
        HIPCHK(h, launch_to_internal(h->xio.f(), h->xa.f(), B, JF, st, h->T));
    } else if (tdev) {
        TorchDrawArgs xa = tda;     // randn(*shape) at the generator's offset, then (const_noise) [[0]].repeat(B, 1, 1, 1)
        xa.k0 = 0; xa.nsteps = 1; xa.ndraw = 1; xa.last_step = -1;
        xa.d[0] = torch_draw(h->xio.f(), 0, (long long)nelem, h->n_cu, h->max_thr_cu, 0, 0);
        HIPCHK(h, launch_torch_draws(xa, st));
        if (a->const_noise) HIPCHK(h, launch_bcast_first(h->xio.f(), B, JF * h->T, st));
        HIPCHK(h, launch_to_internal(h->xio.f(), h->xa.f(), B, JF, st, h->T));
    } else {
        HIPCHK(h, launch_randn_fill(h->xa.f(), B, JF, static_cast<const CallParams*>(h->callp.p), 0u, st, h->T));
    }
    // init_image -> q_sample at the first executed index (:709-716 / :979-986)
    const int first_index = n_exec - 1;
    if (a->init_image || a->skip_timesteps > 0) {
        if (a->init_image) {
            if ((rc = ingest(h, h->xio, a->init_image, nx, od)) != LS_OK) return rc;
            HIPCHK(h, launch_to_internal(h->xio.f(), h->xtmp.f(), B, JF, st, h->T));
        } else {
            HIPCHK(h, hipMemsetAsync(h->xtmp.p, 0, nx, st));
        }
        HIPCHK(h, launch_q_sample(h->xtmp.f(), h->xa.f(), h->xa.f(), nelem, (float)h->t_sac[first_index], (float)h->t_s1mac[first_index], st));
    }
    if (tape) {
        const void* old_e = h->eps_tape.p; const void* old_n = h->noise_tape.p;
        if ((rc = ingest(h, h->eps_tape, a->eps_tape, (size_t)n_eval * 2 * B * kD * sizeof(float), od)) != LS_OK) return rc;
        if (!plms && (rc = ingest(h, h->noise_tape, a->noise_tape, (size_t)n_exec * nx, od)) != LS_OK) return rc;
        if (old_e != h->eps_tape.p || old_n != h->noise_tape.p) free_graph(h);
    }
    size_t plms_stride = 0;
    if (plms) {
        if ((rc = plms_planes(h, nelem, &plms_stride)) != LS_OK) return rc;
        const void* oldc = h->fwd_cfg.p;
        HIPCHK(h, h->fwd_cfg.ensure(nx));
        if (oldc != h->fwd_cfg.p) free_graph(h);
    }
    if (a->n_dump > 0) {
        const void* old = h->dump.p;
        HIPCHK(h, h->dump.ensure((size_t)a->n_dump * nx));
        if (old != h->dump.p) free_graph(h);
    }
    const bool inpaint = a->inpaint_mask != nullptr;
    const bool inp_noised = inpaint && a->inpaint_noised;
    if (inpaint) {
        if (!a->inpainted_motion) return fail(h, LS_EINVAL, "inpaint_mask without inpainted_motion");
        if (tape && inp_noised && !a->inpaint_noise) return fail(h, LS_EINVAL, "TAPE mode with inpaint_noised needs inpaint_noise");
        if ((rc = stage_inpainting(h, a->inpaint_mask, a->inpainted_motion, (tape && inp_noised) ? a->inpaint_noise : nullptr,
                                   (size_t)n_exec * nelem, od)) != LS_OK) return rc;
        const void* oldc = h->fwd_cfg.p;
        HIPCHK(h, h->fwd_cfg.ensure(nx));
        if (oldc != h->fwd_cfg.p) free_graph(h);
    }
    int ring_k = 0;                 // TORCH_DEVICE: steps per ring refill
    if (tdev) {
        const size_t eps_step = (size_t)2 * B * kD;
        const size_t per_step = (eps_step + nelem * (inp_noised ? 2 : 1)) * sizeof(float);
        const size_t fit = h->trng_ring_bytes / per_step;
        ring_k = fit < 1 ? 1 : fit > (size_t)n_exec ? n_exec : (int)fit;
        const void* old[3] = {h->trng_eps.p, h->trng_noise.p, h->trng_inz.p};
        HIPCHK(h, h->trng_eps.ensure(eps_step * ring_k * sizeof(float)));
        HIPCHK(h, h->trng_noise.ensure(nx * ring_k));
        if (inp_noised) HIPCHK(h, h->trng_inz.ensure(nx * ring_k));
        if (old[0] != h->trng_eps.p || old[1] != h->trng_noise.p || old[2] != h->trng_inz.p) free_graph(h);
        // per step, in the reference's order: the style eps of the cond and the uncond pass (RAG.py:10-13, 120: randn_like of a
        // [B, 1, 512] std), the inpainting branch's q_sample re-noise while t > 0 (gaussian_diffusion.py:318), the step noise randn_like(x)
        // in x's memory order (:543 / :787; [T][B][J][F] from the second step on, _ref_strides in gaussian_diffusion.py)
        int nd = 0;
        tda.d[nd++] = torch_draw(h->trng_eps.f(), eps_step, (long long)B * kD, h->n_cu, h->max_thr_cu, 0, 0);
        tda.d[nd++] = torch_draw(h->trng_eps.f() + (size_t)B * kD, eps_step, (long long)B * kD, h->n_cu, h->max_thr_cu, 0, 0);
        if (inp_noised) tda.d[nd++] = torch_draw(h->trng_inz.f(), nelem, (long long)nelem, h->n_cu, h->max_thr_cu, 0, 1);
        tda.d[nd++] = torch_draw(h->trng_noise.f(), nelem, (long long)nelem, h->n_cu, h->max_thr_cu, 1, 0);
        tda.ndraw = nd;
        tda.step_adv = 0;
        for (int d = 0; d < nd; ++d) tda.step_adv += tda.d[d].adv;
    }

    // ---- the loop: for i = T-1-skip ... 0 (gaussian_diffusion.py:724-743 / :994-1014) ----------------
    const bool pair = h->fused && !h->use_long && h->all_scale_one && !a->two_pass_always;
    std::string key;
    {
        char keybuf[256];
        snprintf(keybuf, sizeof keybuf, "P%d B%d s%d e%a k%d n%d c%d cl%d w%u v%u p%d d%d L%lld", h->precision, B, a->sampler, (double)a->eta,
                 a->skip_timesteps, a->noise_mode, a->const_noise, a->clip_denoised, h->weights_version, h->sched_version, (int)pair, a->n_dump, plan_code(h));
        key = keybuf;
        if (inpaint) key += inp_noised ? " I2" : " I1";
        if (plms) key += " O" + std::to_string(a->plms_order);
        if (tdev) key += " R" + std::to_string(ring_k) + (a->x_init ? "x" : "X");
        for (int d = 0; d < a->n_dump; ++d) key += "," + std::to_string(a->dump_steps[d]);      // the whole list, however long
    }
    auto enqueue_loop = [&]() -> int {
        HIPCHK(h, coop_reset(h, st));              // a memset node at the head of the captured loop: replays start from zeroed granules
        for (int k = 0; k < n_exec; ++k) {
            const int i = n_exec - 1 - k;
            StepArgs s;
            fill_common(h, s);
            fill_sampler(h, s, a->sampler, i, a->eta);
            s.clip_denoised = a->clip_denoised;
            s.x_in = (k & 1) ? h->xb.f() : h->xa.f();
            s.x_out = (k & 1) ? h->xa.f() : h->xb.f();
            s.temb = h->temb.f() + (size_t)i * kD; s.temb_stride = 0;
            s.step_id = (unsigned)k;
            if (tape) {
                s.eps_c = h->eps_tape.f() + ((size_t)k * 2 + 0) * B * kD;
                s.eps_u = h->eps_tape.f() + ((size_t)k * 2 + 1) * B * kD;
                s.noise = h->noise_tape.f() + (size_t)k * nelem;
                s.const_noise = a->const_noise;
            }
            const int slot = tdev ? k % ring_k : 0;
            if (tdev) {
                if (slot == 0) {        // refill the ring with steps k .. k + K - 1 (stream order: the steps that read it before are done)
                    TorchDrawArgs g = tda;
                    g.k0 = k; g.nsteps = n_exec - k < ring_k ? n_exec - k : ring_k;
                    g.rel0 = x_adv + (unsigned long long)k * tda.step_adv;
                    HIPCHK(h, launch_torch_draws(g, st));
                }
                s.eps_c = h->trng_eps.f() + ((size_t)slot * 2 + 0) * B * kD;
                s.eps_u = h->trng_eps.f() + ((size_t)slot * 2 + 1) * B * kD;
                s.noise = h->trng_noise.f() + (size_t)slot * nelem;
                s.const_noise = a->const_noise;
            }
            float* dump_at = nullptr;
            for (int d = 0; d < a->n_dump; ++d)
                if (a->dump_steps[d] == k) dump_at = h->dump.f() + (size_t)d * nelem;
            if (inpaint) {
                // two launches: the denoiser alone (CFG-combined model output -> fwd_cfg), then mix + clamp + update
                StepArgs m = s;
                m.sampler = kNone; m.clip_denoised = 0; m.x0_out = h->fwd_cfg.f(); m.x_out = nullptr; m.noise = nullptr;
                HIPCHK(h, run_step(h, m, B, pair, st));
                const float* inz = tape ? h->inp_tape.f() + (size_t)k * nelem : tdev && inp_noised ? h->trng_inz.f() + (size_t)slot * nelem : nullptr;
                HIPCHK(h, run_inpaint_update(h, s, i, inp_noised, inz, s.noise, s.const_noise,
                                             s.x_out, dump_at, (unsigned)k, a->clip_denoised, B, st));
                continue;
            }
            if (dump_at) s.x0_out = dump_at;
            s.xpad_ready = k > 0;                      // long-sequence path: the previous step's update kernel wrote this step's padded x_t
            HIPCHK(h, run_step(h, s, B, pair, st));
        }
        return LS_OK;
    };
    // LS_SAMPLER_PLMS (:1016-1211): per executed step the denoiser alone (model output -> fwd_cfg) and k_plms_update; the first step
    // evaluates twice.  One linear chain on the handle's stream, like the loop above.
    auto enqueue_plms = [&]() -> int {
        HIPCHK(h, coop_reset(h, st));
        float* const ring = h->plms_buf.f();
        float* const mid = ring + 4 * plms_stride;
        unsigned e = 0;                                 // evaluation counter: index into eps_tape / Philox step_id
        auto denoise = [&](const float* x, int i) -> int {
            StepArgs m;
            fill_common(h, m);
            m.x_in = x; m.x0_out = h->fwd_cfg.f();
            m.temb = h->temb.f() + (size_t)i * kD; m.temb_stride = 0;     // model timestep timestep_map[i] (_WrappedModel)
            m.step_id = e;
            if (tape) {
                m.eps_c = h->eps_tape.f() + ((size_t)e * 2 + 0) * B * kD;
                m.eps_u = h->eps_tape.f() + ((size_t)e * 2 + 1) * B * kD;
            }
            ++e;
            HIPCHK(h, run_step(h, m, B, pair, st));
            return LS_OK;
        };
        for (int k = 0; k < n_exec; ++k) {
            const int i = n_exec - 1 - k;
            const float* x_in = (k & 1) ? h->xb.f() : h->xa.f();
            float* x_out = (k & 1) ? h->xa.f() : h->xb.f();
            float* plane = ring + (size_t)(k & 3) * plms_stride;
            int rc2;
            if ((rc2 = denoise(x_in, i)) != LS_OK) return rc2;
            if (k == 0) {
                HIPCHK(h, run_plms_update(h, kPlmsEulerA, i, 0, x_in, nullptr, nullptr, mid, plane, nullptr, a->clip_denoised, nelem, st));
                if ((rc2 = denoise(mid, i - 1)) != LS_OK) return rc2;
                const float* h1[3] = {plane, nullptr, nullptr};
                HIPCHK(h, run_plms_update(h, kPlmsEulerB, i, 1, x_in, mid, h1, x_out, nullptr, nullptr, a->clip_denoised, nelem, st));
                continue;
            }
            const int nh = (a->plms_order < k + 1 ? a->plms_order : k + 1) - 1;
            const float* hist[3] = {nullptr, nullptr, nullptr};
            for (int j = 0; j < nh; ++j) hist[j] = ring + (size_t)((k - 1 - j) & 3) * plms_stride;
            HIPCHK(h, run_plms_update(h, kPlmsMulti, i, nh, x_in, nullptr, hist, x_out, plane, nullptr, a->clip_denoised, nelem, st));
        }
        return LS_OK;
    };
    h->timing.graph_replayed = 0;
    HIPCHK(h, hipEventRecord(h->ev[1], st));
    if (a->use_graph) {
        if (!h->graph_exec || h->graph_key != key) {
            free_graph(h);
            HIPCHK(h, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            rc = plms ? enqueue_plms() : enqueue_loop();
            hipGraph_t g = nullptr;
            hipError_t e = hipStreamEndCapture(st, &g);
            if (rc != LS_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
            if (e != hipSuccess) return fail(h, LS_EHIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
            h->graph = g;
            HIPCHK(h, hipGraphInstantiate(&h->graph_exec, h->graph, nullptr, nullptr, 0));
            h->graph_key = key;
            HIPCHK(h, hipEventRecord(h->ev[1], st));    // exclude capture/instantiate from loop_ms
        } else {
            h->timing.graph_replayed = 1;
        }
        HIPCHK(h, hipGraphLaunch(h->graph_exec, st));
    } else {
        if ((rc = plms ? enqueue_plms() : enqueue_loop()) != LS_OK) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[2], st));
    const float* final_x = (n_exec & 1) ? h->xb.f() : h->xa.f();
    HIPCHK(h, launch_from_internal(final_x, h->xio.f(), B, JF, st, h->T));
    if ((rc = egress(h, a->out, h->xio.f(), nx, od)) != LS_OK) return rc;
    for (int d = 0; d < a->n_dump; ++d) {
        HIPCHK(h, launch_from_internal(h->dump.f() + (size_t)d * nelem, h->xio.f(), B, JF, st, h->T));
        if ((rc = egress(h, a->dump_out + (size_t)d * nelem, h->xio.f(), nx, od)) != LS_OK) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[3], st));
    HIPCHK(h, hipStreamSynchronize(st));
    resolve_prepare_timing(h, true);
    if ((rc = coop_check(h)) != LS_OK) return rc;
    report_path(h, pair);
    HIPCHK(h, hipEventElapsedTime(&h->timing.loop_ms, h->ev[1], h->ev[2]));
    HIPCHK(h, hipEventElapsedTime(&h->timing.total_ms, h->ev[0], h->ev[3]));
    h->timing.n_step_launches = n_eval;
    h->timing.single_pass = pair ? 1 : 0;
    h->timing.tape_upload_ms = 0.f;
    h->timing.n_segments = 1;
    return LS_OK;
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
    float* const mid = ring + 4 * ps;
    if ((rc = ingest(h, h->xio, a->x, nx, od)) != LS_OK) return rc;
    HIPCHK(h, launch_to_internal(h->xio.f(), h->xa.f(), B, JF, st, h->T));
    // old_eps, newest first, into planes 0 .. n_hist - 1; this step's eps goes to plane 3
    const int nh = (a->order < a->n_hist + 1 ? a->order : a->n_hist + 1) - 1;
    const float* hist[3] = {nullptr, nullptr, nullptr};
    for (int j = 0; j < nh; ++j) {
        if ((rc = ingest(h, h->xio, a->hist[a->n_hist - 1 - j], nx, od)) != LS_OK) return rc;
        HIPCHK(h, launch_to_internal(h->xio.f(), ring + (size_t)j * ps, B, JF, st, h->T));
        hist[j] = ring + (size_t)j * ps;
    }
    float* const plane = ring + 3 * ps;
    const hipMemcpyKind kind = od ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t ne = (size_t)B * kD;
    HIPCHK(h, h->eps.ensure(4 * ne * sizeof(float)));
    HIPCHK(h, hipMemcpyAsync(h->eps.f(), a->eps_cond, ne * sizeof(float), kind, st));
    HIPCHK(h, hipMemcpyAsync(h->eps.f() + ne, a->eps_uncond, ne * sizeof(float), kind, st));
    if (first) {
        HIPCHK(h, hipMemcpyAsync(h->eps.f() + 2 * ne, a->eps_cond2, ne * sizeof(float), kind, st));
        HIPCHK(h, hipMemcpyAsync(h->eps.f() + 3 * ne, a->eps_uncond2, ne * sizeof(float), kind, st));
    }
    if ((rc = advance_tags(h, st)) != LS_OK) return rc;
    HIPCHK(h, coop_reset(h, st));
    const bool pair = h->fused && !h->use_long && h->all_scale_one && !a->two_pass_always;
    auto denoise = [&](const float* x, int i, int e) -> int {
        StepArgs m;
        fill_common(h, m);
        m.x_in = x; m.x0_out = h->fwd_cfg.f();
        m.temb = h->temb.f() + (size_t)i * kD; m.temb_stride = 0;
        m.eps_c = h->eps.f() + (size_t)(2 * e) * ne; m.eps_u = h->eps.f() + (size_t)(2 * e + 1) * ne;
        HIPCHK(h, run_step(h, m, B, pair, st));
        return LS_OK;
    };
    float* const pred = h->xtmp.f();                  // pred_xstart of the FIRST evaluation (clamped), internal layout
    if ((rc = denoise(h->xa.f(), a->index, 0)) != LS_OK) return rc;
    if (first) {
        HIPCHK(h, run_plms_update(h, kPlmsEulerA, a->index, 0, h->xa.f(), nullptr, nullptr, mid, plane, pred, a->clip_denoised, nelem, st));
        if ((rc = denoise(mid, a->index - 1, 1)) != LS_OK) return rc;
        const float* h1[3] = {plane, nullptr, nullptr};
        HIPCHK(h, run_plms_update(h, kPlmsEulerB, a->index, 1, h->xa.f(), mid, h1, h->xb.f(), nullptr, nullptr, a->clip_denoised, nelem, st));
    } else {
        HIPCHK(h, run_plms_update(h, kPlmsMulti, a->index, nh, h->xa.f(), nullptr, hist, h->xb.f(), plane, pred, a->clip_denoised, nelem, st));
    }
    HIPCHK(h, launch_from_internal(h->xb.f(), h->xio.f(), B, JF, st, h->T));
    if ((rc = egress(h, a->sample, h->xio.f(), nx, od)) != LS_OK) return rc;
    if (a->pred_xstart) {
        HIPCHK(h, launch_from_internal(pred, h->xio.f(), B, JF, st, h->T));
        if ((rc = egress(h, a->pred_xstart, h->xio.f(), nx, od)) != LS_OK) return rc;
    }
    if (a->eps_out) {
        HIPCHK(h, launch_from_internal(plane, h->xio.f(), B, JF, st, h->T));
        if ((rc = egress(h, a->eps_out, h->xio.f(), nx, od)) != LS_OK) return rc;
    }
    if (!(a->no_sync && od)) { HIPCHK(h, hipStreamSynchronize(st)); if ((rc = coop_check(h)) != LS_OK) return rc; }
    return LS_OK;
}

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
    HIPCHK(h, launch_from_internal(h->xtmp.f(), h->xio.f(), batch, h->JF, h->stream, h->T));
    int rc = egress(h, out, h->xio.f(), nx, on_device);
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
    if (n == "prof") {
        if (!h->prof_on) return fail(h, LS_ESTATE, "LS_PROF not set");
        cnt = (size_t)kWaves * kProfPoints * 2;     // 64-bit stamps as pairs of 32-bit words
        if (cnt > capacity) return fail(h, LS_EINVAL, "capacity");
        HIPCHK(h, hipMemcpy(host_out, h->prof.p, cnt * sizeof(float), hipMemcpyDeviceToHost));
        return (long long)cnt;
    }
#endif
#ifdef LS_DEBUG
    if (n == "wgt") {
        if (!h->prof_on) return fail(h, LS_ESTATE, "LS_PROF not set");
        cnt = 2048 * 2;
        if (cnt > capacity) return fail(h, LS_EINVAL, "capacity");
        HIPCHK(h, hipMemcpy(host_out, h->wgt.p, cnt * sizeof(float), hipMemcpyDeviceToHost));
        return (long long)cnt;
    }
    if (n == "wgt_hw") {       // k_pass: HW_ID | XCC_ID << 32 of every workgroup's wave 0
        if (!h->prof_on) return fail(h, LS_ESTATE, "LS_PROF not set");
        cnt = 2048 * 2;
        if (cnt > capacity) return fail(h, LS_EINVAL, "capacity");
        HIPCHK(h, hipMemcpy(host_out, static_cast<unsigned long long*>(h->wgt.p) + 2048, cnt * sizeof(float), hipMemcpyDeviceToHost));
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
