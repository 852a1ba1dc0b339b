// Post-processing and scoring of a stitched timeline (long_form.sample_long): the reference's loop bodies of ls_post.hip and
// ls_beat_metrics.hip with the clip length 34 replaced by N frames, N up to LS_TIMELINE_MAX_FRAMES.  A timeline clip is ONE series:
// nothing resets at a window seam.
//   k_ted_timeline           grid (frame tile, clip): layout change, mean add, bone normalisation, change curve, beats, pose
//   k_beat_post_timeline     grid (frame tile, joint chunk, clip): layout change, rot6d -> Euler
//   k_beat_metrics_timeline  grid (frame tile, clip): SRGR success, the six velocity series and their minima
//   k_beat_reduce_timeline   one workgroup per clip: srgr_sum and align from the masks in global memory
//   k_ted_align              one workgroup per clip: the TED beat-consistency sum of a clip, in float64
// A tile is LS_TIMELINE_TILE frames plus a halo that is RECOMPUTED, never exchanged: TED stages two frames to the left and one to the
// right (angle_diff needs the frame before it, the beat test one angle_diff on either side); the BEAT minima stage `order` velocities
// on either side.  Every frame's numbers come from the functions of ls_post_frame.h (or, for the metrics, k_beat_metrics's expressions
// under the same contraction setting) on the same inputs, so they do not depend on the tile a frame lands in, the tile size or the batch.
// The input is frame-innermost ([B,J,F,N]): it is read with consecutive lanes on consecutive frames and transposed through LDS with
// an odd row stride (ds_write banks are (a/4) % 32: 32 lanes at an odd stride touch 32 banks), as k_chain_window does; every output
// leaves along its own innermost axis.  Sums are fixed trees (per-thread stride order, wave butterfly, four wave partials in order).
// Algorithmic bytes per clip (fp32): TED reads 108 N and writes 108 N + 120 N + 5 N; BEAT post reads 1128 N and writes 1692 N.
// Ragged batches (the *_ragged entries): clip b holds frames[b] valid frames in rows of stride N_max.  The per-frame kernels are the
// same bodies instantiated with kRagged: a 1-D grid over the (clip, first frame) table of ls_ragged_tiles, so work follows the valid
// frames, and every clamp, halo and beat range uses the clip's own N_b; only the addresses use the stride.  What lies beyond a clip's
// valid range is never read and is zeroed by a memset ahead of the launch.
#include "ls_hip.h"
#include "ls_post_frame.h"
#include "ls_staging.h"

namespace ls {
namespace {

constexpr int kTile = LS_TIMELINE_TILE, kMaxN = LS_TIMELINE_MAX_FRAMES;
constexpr int kStage = kTile + 3;                 // TED: frames t0 - 2 .. t0 + kTile
constexpr int kLd = (kMaxBones + 1) * 3 + 2;      // 53: odd row stride that holds a frame's vectors and a frame's pose
constexpr int kJChunk = 16;                       // BEAT post: joints per workgroup
constexpr int kLd6 = kJChunk * 6 + 1, kLd3 = kJChunk * 3 + 1;
constexpr int kSeries = 6;

static_assert(kLd % 2 == 1 && kLd6 % 2 == 1 && kLd3 % 2 == 1, "odd LDS row strides");
static_assert(kTile <= 256, "one thread per frame of a tile");

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// device arrays of a ragged call: the clips' valid frames [B] and the tile table [grid] (all NULL in an equal-length call)
struct RaggedPlan {
    const int *frames, *tile_clip, *tile_start;
};

// the workgroup's clip, first frame and the clip's frame count; `stride` is the row stride in frames (equal lengths: the count itself)
template <bool kRagged>
__device__ __forceinline__ void tile_of(const RaggedPlan& r, int dense_clip, int stride, int& b, int& t0, int& N) {
    if (kRagged) {
        b = r.tile_clip[blockIdx.x];
        t0 = r.tile_start[blockIdx.x];
        N = r.frames[b];
    } else {
        b = dense_clip;
        t0 = blockIdx.x * kTile;
        N = stride;
    }
}

}  // namespace

template <bool kRagged>
__global__ __launch_bounds__(256) void k_ted_timeline(const float* __restrict__ sample, PostParams p, int NS, RaggedPlan rp,
                                                      float* __restrict__ aligned, float* __restrict__ pose,
                                                      float* __restrict__ angle_diff, unsigned char* __restrict__ beat_mask) {
    __shared__ float sv[kStage][kLd];           // raw, then aligned + mean (un-normalised)
    __shared__ float sn[kStage][kLd];           // per-bone unit vectors, later the tile's poses
    __shared__ float sang[kMaxPairs][kStage];
    __shared__ float sdiff[kStage];
    int b, t0, N;                                                       // N: the clip's own frames; NS: the row stride
    tile_of<kRagged>(rp, blockIdx.y, NS, b, t0, N);
    const int tid = threadIdx.x;
    const int JF = p.njoints * 3, f_lo = t0 - 2;                       // staged row l holds frame f_lo + l
    for (int i = tid; i < JF * kStage; i += 256) {                      // lanes along the frame axis
        const int c = i / kStage, l = i - c * kStage, f = f_lo + l;
        if (f >= 0 && f < N) sv[l][c] = sample[((size_t)b * JF + c) * NS + f];
    }
    __syncthreads();
    for (int i = tid; i < kStage * JF; i += 256) {                      // [B,J,F,N] -> [B,N,J*F]: lanes along the channel axis
        const int l = i / JF, c = i - l * JF, f = f_lo + l;
        if (f < 0 || f >= N) continue;
        const float v = sv[l][c];
        if (aligned && l >= 2 && l < 2 + kTile) aligned[((size_t)b * NS + f) * JF + c] = v;
        sv[l][c] = v + p.mean_dir_vec[c];
    }
    __syncthreads();
    for (int i = tid; i < kStage * p.njoints; i += 256) {
        const int l = i / p.njoints, j = i - l * p.njoints, f = f_lo + l;
        if (f >= 0 && f < N) ted_unit(&sv[l][3 * j], &sn[l][3 * j]);
    }
    __syncthreads();
    for (int i = tid; i < kStage * p.n_pairs; i += 256) {
        const int k = i / kStage, l = i - k * kStage, f = f_lo + l;
        if (f >= 0 && f < N) sang[k][l] = ted_pair_angle(&sn[l][3 * p.pair_a[k]], &sn[l][3 * p.pair_b[k]]);
    }
    __syncthreads();
    if (tid >= 1 && tid < kStage) {                                     // the curve at frames t0 - 1 .. t0 + kTile; frame 0 holds 0
        const int l = tid, f = f_lo + l;
        if (f >= 0 && f < N) {
            const float d = f > 0 ? ted_angle_change(p, &sang[0][l], &sang[0][l - 1], kStage) : 0.f;
            sdiff[l] = d;
            if (angle_diff && l >= 2 && l < 2 + kTile) angle_diff[(size_t)b * NS + f] = d;
        }
    }
    __syncthreads();
    if (beat_mask && tid < kTile && t0 + tid < N) {                     // local minima of the change curve, t in [2, N - 2]
        const int l = tid + 2, f = t0 + tid;
        bool beat = false;
        if (f >= 2 && f <= N - 2) beat = ted_is_beat(sdiff[l], sdiff[l - 1], sdiff[l + 1], p.thres);
        beat_mask[(size_t)b * NS + f] = beat ? 1 : 0;
    }
    if (!pose) return;
    if (tid < kTile && t0 + tid < N) ted_pose_frame(p, sv[tid + 2], sn[tid + 2]);      // sn: every reader is past the barrier above
    __syncthreads();
    const int PJ = p.n_pose_joints * 3;
    for (int i = tid; i < kTile * PJ; i += 256) {
        const int l = i / PJ, c = i - l * PJ, f = t0 + l;
        if (f < N) pose[((size_t)b * NS + f) * PJ + c] = sn[l + 2][c];
    }
}

template <bool kRagged>
__global__ __launch_bounds__(256) void k_beat_post_timeline(const float* __restrict__ sample, float* __restrict__ decoded,
                                                            float* __restrict__ euler, int J, int NS, RaggedPlan rp) {
    __shared__ float s6[kTile][kLd6];
    __shared__ float s3[kTile][kLd3];
    int b, t0, N;
    tile_of<kRagged>(rp, blockIdx.z, NS, b, t0, N);
    const int j0 = blockIdx.y * kJChunk, tid = threadIdx.x;
    const int nj = J - j0 < kJChunk ? J - j0 : kJChunk, C = nj * 6, E = nj * 3;
    for (int i = tid; i < C * kTile; i += 256) {                        // lanes along the frame axis
        const int c = i / kTile, l = i - c * kTile, f = t0 + l;
        if (f < N) s6[l][c] = sample[(((size_t)b * J + j0) * 6 + c) * NS + f];
    }
    __syncthreads();
    if (decoded) {
        for (int i = tid; i < kTile * C; i += 256) {
            const int l = i / C, c = i - l * C, f = t0 + l;
            if (f < N) decoded[(((size_t)b * NS + f) * J + j0) * 6 + c] = s6[l][c];
        }
    }
    if (!euler) return;
    for (int i = tid; i < kTile * nj; i += 256) {
        const int l = i / nj, j = i - l * nj;
        if (t0 + l >= N) continue;
        float d6[6], o[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) d6[k] = s6[l][6 * j + k];
        beat_rot6d_to_euler(d6, o);
        s3[l][3 * j] = o[0]; s3[l][3 * j + 1] = o[1]; s3[l][3 * j + 2] = o[2];
    }
    __syncthreads();
    for (int i = tid; i < kTile * E; i += 256) {
        const int l = i / E, c = i - l * E, f = t0 + l;
        if (f < N) euler[(((size_t)b * NS + f) * J + j0) * 3 + c] = s3[l][c];
    }
}

namespace {

struct TimelineMetricsParams {
    int J, N, order, align_series;
    int joint[kSeries];
    float threshold, scale, sigma, fps;
    const float *pred, *target, *semantic, *onset_times;
    const long long* onset_offsets;
    unsigned char *success, *beat_mask;
    float *srgr_sum, *vel, *align;
    RaggedPlan rp;              // N is the row stride of a ragged call
};

struct TedAlignParams {
    int N, onset_cols, hop;
    double fps, sigma, sr;
    const unsigned char* beat_mask;
    const int *onset_frames, *onset_count;
    double* align_sum;
    int* n_beats;
};

}  // namespace

// k_beat_metrics's per-entry expressions on frames [t0, t0 + kTile) of clip b; the velocities of a series are staged with `order`
// neighbours on either side of the tile, clamped to the clip as argrelextrema's mode='clip' clamps them
template <bool kRagged>
__global__ __launch_bounds__(256) void k_beat_metrics_timeline(const TimelineMetricsParams p) {
#pragma clang fp contract(off)
    __shared__ float svel[kTile + kMaxN];
    int b, t0, N;
    tile_of<kRagged>(p.rp, blockIdx.y, p.N, b, t0, N);
    const int tid = threadIdx.x;
    const int NS = p.N, VS = NS - 1, V = N - 1, JC = p.J * 3;
    const float* pred = p.pred + (size_t)b * NS * JC;
    if (p.target && p.success) {
        const float* tar = p.target + (size_t)b * NS * JC;
        const int e1 = (t0 + kTile < N ? t0 + kTile : N) * p.J;
        for (int e = t0 * p.J + tid; e < e1; e += 256) {
            const float* a = pred + (size_t)e * 3;
            const float* t = tar + (size_t)e * 3;
            const float diff = (fabsf(a[0] - t[0]) + fabsf(a[1] - t[1])) + fabsf(a[2] - t[2]);
            p.success[(size_t)b * NS * p.J + e] = diff < p.threshold ? 1 : 0;
        }
    }
    if ((!p.vel && !p.beat_mask) || t0 >= V) return;
    const int lo = t0 - p.order > 0 ? t0 - p.order : 0;
    const int hi = t0 + kTile + p.order < V ? t0 + kTile + p.order : V;        // staged velocities [lo, hi): at most kTile + 2 * order
    for (int s = 0; s < kSeries; ++s) {
        for (int i = tid; i < hi - lo; i += 256) {
            const int f = lo + i;
            const float* a = pred + (size_t)f * JC + p.joint[s] * 3;
            const float* c = a + JC;
            const float dx = c[0] - a[0], dy = c[1] - a[1], dz = c[2] - a[2];
            const float v = sqrtf((dx * dx + dy * dy) + dz * dz);
            svel[i] = v;
            if (p.vel && f >= t0 && f < t0 + kTile) p.vel[((size_t)b * kSeries + s) * VS + f] = v;
        }
        __syncthreads();
        if (p.beat_mask && tid < kTile && t0 + tid < V) {
            const int f = t0 + tid;
            const float x = svel[f - lo];
            bool beat = true;
            for (int k = 1; k <= p.order && beat; ++k) {
                const int l = f - k < 0 ? 0 : f - k, h = f + k > V - 1 ? V - 1 : f + k;
                beat = x < svel[l - lo] && x < svel[h - lo];
            }
            p.beat_mask[((size_t)b * kSeries + s) * VS + f] = beat ? 1 : 0;
        }
        __syncthreads();
    }
}

// the clip's two sums, in k_beat_metrics's order, from the masks k_beat_metrics_timeline left in global memory
template <bool kRagged>
__global__ __launch_bounds__(256) void k_beat_reduce_timeline(const TimelineMetricsParams p) {
#pragma clang fp contract(off)
    __shared__ float sbeat[kMaxN];              // the time of a beat of the series the alignment uses, +inf where there is none
    __shared__ float part[4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
    const int NS = p.N, VS = NS - 1, N = kRagged ? p.rp.frames[b] : NS, V = N - 1;
    if (p.srgr_sum) {
        const unsigned char* ok = p.success + (size_t)b * NS * p.J;
        float s = 0.f;
        for (int e = tid; e < N * p.J; e += 256)
            if (ok[e]) s += (p.semantic ? p.semantic[(size_t)b * NS + e / p.J] : 1.0f) * p.scale;
        s = wave_sum(s);
        if ((tid & 63) == 0) part[wave] = s;
        __syncthreads();
        if (tid == 0) p.srgr_sum[b] = ((part[0] + part[1]) + part[2]) + part[3];
        __syncthreads();
    }
    if (!p.align) return;
    for (int i = tid; i < V; i += 256)
        sbeat[i] = p.beat_mask[((size_t)b * kSeries + p.align_series) * VS + i] ? (float)i / p.fps : INFINITY;
    __syncthreads();
    const long long o0 = p.onset_offsets[b], o1 = p.onset_offsets[b + 1];
    const float two_var = 2.0f * (p.sigma * p.sigma);
    float s = 0.f;
    for (long long i = o0 + tid; i < o1; i += 256) {
        const float t = p.onset_times[i];
        float dmin = INFINITY;
        for (int m = 0; m < V; ++m) dmin = fminf(dmin, fabsf(sbeat[m] - t));      // |inf - t| = inf: a frame without a beat changes nothing
        s += expf(-(dmin * dmin) / two_var);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) p.align[b] = (((part[0] + part[1]) + part[2]) + part[3]) / (float)(o1 - o0);
}

// BeatConsistency.push's clip body in its float64 operations: sum over the clip's onsets a = frame * hop / sr of
// exp(-min_m (a - m)^2 / (2 sigma^2)), m = t / fps over the set frames t of the clip's beat mask; 0 for a clip without a beat
__global__ __launch_bounds__(256) void k_ted_align(const TedAlignParams p) {
#pragma clang fp contract(off)
    __shared__ double sm[kMaxN];                // the time of a motion beat, +inf at a frame without one
    __shared__ double dpart[4];
    __shared__ int ipart[4];
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, N = p.N;
    int nb = 0;
    for (int i = tid; i < N; i += 256) {
        const int m = p.beat_mask[(size_t)b * N + i] ? 1 : 0;
        sm[i] = m ? (double)i / p.fps : (double)INFINITY;
        nb += m;
    }
    nb = wave_sum(nb);
    if ((tid & 63) == 0) ipart[wave] = nb;
    __syncthreads();
    const int beats = ipart[0] + ipart[1] + ipart[2] + ipart[3];
    if (tid == 0 && p.n_beats) p.n_beats[b] = beats;
    if (!p.align_sum) return;
    if (beats == 0) {
        if (tid == 0) p.align_sum[b] = 0.0;
        return;
    }
    int cnt = p.onset_count[b];
    cnt = cnt < 0 ? 0 : (cnt > p.onset_cols ? p.onset_cols : cnt);      // device-resident counts cannot be refused by the host
    const double two_var = (2.0 * p.sigma) * p.sigma;
    double s = 0.0;
    for (int i = tid; i < cnt; i += 256) {
        const double a = (double)((long long)p.onset_frames[(size_t)b * p.onset_cols + i] * (long long)p.hop) / p.sr;
        double dmin = INFINITY;
        for (int t = 0; t < N; ++t) {
            const double d = a - sm[t];               // -inf at a frame without a beat: its square changes nothing
            dmin = fmin(dmin, d * d);
        }
        s += exp(-dmin / two_var);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) dpart[wave] = s;
    __syncthreads();
    if (tid == 0) p.align_sum[b] = ((dpart[0] + dpart[1]) + dpart[2]) + dpart[3];
}

namespace {

inline unsigned tiles_of(int n_frames) { return (unsigned)((n_frames + kTile - 1) / kTile); }

// the launch plan of a ragged call: frames[b] in [least, stride] is checked by the caller; the table is ls_ragged_tiles's
struct TilePlan {
    std::vector<int32_t> table;                   // frames [B], then the tiles' clips [n] and first frames [n]: one upload
    size_t n = 0;
    RaggedPlan dev{};
    bool build(int batch, const int32_t* frames) {
        int32_t count = 0;
        if (ls_ragged_tiles(batch, frames, kTile, nullptr, nullptr, 0, &count) != LS_OK) return false;
        n = (size_t)count;
        table.assign(frames, frames + batch);
        table.resize((size_t)batch + 2 * n);
        return ls_ragged_tiles(batch, frames, kTile, table.data() + batch, table.data() + batch + n, count, &count) == LS_OK;
    }
    void upload(Staging& st, int batch) {         // lengths are host data in both modes
        dev.frames = st.upload(table.data(), table.size());
        dev.tile_clip = dev.frames + batch;
        dev.tile_start = dev.tile_clip + n;
    }
    unsigned tiles() const { return (unsigned)n; }
};

inline bool frames_within(int batch, const int32_t* frames, long long least, int stride) {
    if (!frames) return false;
    for (int b = 0; b < batch; ++b)
        if (frames[b] < least || frames[b] > stride) return false;
    return true;
}

int ted_post_timeline(int device, int on_device, int batch, int n_frames, const int32_t* frames, bool ragged, const ls_post_config* c,
                      const float* timeline, float* aligned, float* pose, float* angle_diff, unsigned char* beat_mask) {
    PostParams p;
    if (!timeline || batch < 1 || n_frames < 4 || n_frames > kMaxN || !post_params(c, &p)) return LS_EINVAL;
    TilePlan plan;
    if (ragged && (!frames_within(batch, frames, 4, n_frames) || !plan.build(batch, frames))) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    const size_t n_in = (size_t)batch * c->njoints * 3 * n_frames, n_t = (size_t)batch * n_frames;
    Staging st(on_device != 0);
    const float* d_in = st.in(timeline, n_in);
    float* d_al = st.out(aligned, n_in);
    float* d_pose = st.out(pose, n_t * c->n_pose_joints * 3);
    float* d_diff = st.out(angle_diff, n_t);
    unsigned char* d_mask = st.out(beat_mask, n_t);
    if (ragged) {
        plan.upload(st, batch);
        st.fill(d_al, 0, n_in * 4);
        st.fill(d_pose, 0, n_t * c->n_pose_joints * 3 * 4);
        st.fill(d_diff, 0, n_t * 4);
        st.fill(d_mask, 0, n_t);
        if (st.e == hipSuccess)
            hipLaunchKernelGGL(k_ted_timeline<true>, dim3(plan.tiles()), dim3(256), 0, 0, d_in, p, n_frames, plan.dev, d_al, d_pose, d_diff, d_mask);
    } else if (st.e == hipSuccess) {
        hipLaunchKernelGGL(k_ted_timeline<false>, dim3(tiles_of(n_frames), batch), dim3(256), 0, 0, d_in, p, n_frames, RaggedPlan{}, d_al, d_pose,
                           d_diff, d_mask);
    }
    return st.finish();
}

int beat_post_timeline(int device, int on_device, int batch, int njoints, int n_frames, const int32_t* frames, bool ragged,
                       const float* timeline, float* decoded, float* euler_deg) {
    if (!timeline || batch < 1 || njoints < 1 || n_frames < 2 || n_frames > kMaxN) return LS_EINVAL;
    const unsigned chunks = (unsigned)((njoints + kJChunk - 1) / kJChunk);
    if (chunks > 65535u || batch > 65535) return LS_EINVAL;              // grid dimensions y and z
    TilePlan plan;
    if (ragged && (!frames_within(batch, frames, 2, n_frames) || !plan.build(batch, frames))) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    const size_t n_in = (size_t)batch * njoints * 6 * n_frames;
    Staging st(on_device != 0);
    const float* d_in = st.in(timeline, n_in);
    float* d_dec = st.out(decoded, n_in);
    float* d_eu = st.out(euler_deg, n_in / 2);
    if (ragged) {
        plan.upload(st, batch);
        st.fill(d_dec, 0, n_in * 4);
        st.fill(d_eu, 0, n_in / 2 * 4);
        if (st.e == hipSuccess)
            hipLaunchKernelGGL(k_beat_post_timeline<true>, dim3(plan.tiles(), chunks), dim3(256), 0, 0, d_in, d_dec, d_eu, njoints, n_frames, plan.dev);
    } else if (st.e == hipSuccess) {
        hipLaunchKernelGGL(k_beat_post_timeline<false>, dim3(tiles_of(n_frames), chunks, batch), dim3(256), 0, 0, d_in, d_dec, d_eu, njoints, n_frames,
                           RaggedPlan{});
    }
    return st.finish();
}

int beat_metrics_timeline(int device, int n_frames, const int32_t* frames, bool ragged, const ls_beat_metrics_args* a) {
    bool motion;
    long long n_onsets;
    if (!beat_metrics_args_ok(a, &motion, &n_onsets)) return LS_EINVAL;
    if (n_frames > kMaxN || (long long)n_frames < 2LL * a->order + 2) return LS_EINVAL;
    const int B = a->batch, N = n_frames, V = N - 1;
    if (B > 65535) return LS_EINVAL;                                           // grid dimension y
    TilePlan plan;
    if (ragged && (!frames_within(B, frames, 2LL * a->order + 2, N) || !plan.build(B, frames))) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    const size_t n_eu = (size_t)B * N * a->njoints * 3, n_tj = (size_t)B * N * a->njoints, n_v = (size_t)B * kSeries * V;
    TimelineMetricsParams p{};
    p.J = a->njoints; p.N = N; p.order = a->order; p.align_series = a->align_series;
    for (int s = 0; s < kSeries; ++s) p.joint[s] = motion ? a->series_joint[s] : 0;
    p.threshold = a->threshold; p.scale = a->scale; p.sigma = a->sigma; p.fps = a->fps;
    Staging st(a->on_device != 0);
    p.pred = st.in(a->pred, n_eu);
    p.target = st.in(a->target, n_eu);
    p.semantic = a->target ? st.in(a->semantic, (size_t)B * N) : nullptr;
    if (a->align) {
        p.onset_offsets = reinterpret_cast<const long long*>(st.upload(a->onset_offsets, (size_t)B + 1));       // host data in both modes
        p.onset_times = st.in(a->onset_times, (size_t)n_onsets);
    }
    p.success = st.out(a->success, n_tj, a->srgr_sum != nullptr);              // the reduction reads both masks from global memory
    p.srgr_sum = st.out(a->srgr_sum, (size_t)B);
    p.vel = st.out(a->vel, n_v);
    p.beat_mask = st.out(a->beat_mask, n_v, a->align != nullptr);
    p.align = st.out(a->align, (size_t)B);
    const bool frame_pass = (p.target && p.success) || p.vel || p.beat_mask, reduce = p.srgr_sum || p.align;
    if (ragged) {
        plan.upload(st, B);
        p.rp = plan.dev;
        st.fill(p.success, 0, n_tj);
        st.fill(p.vel, 0, n_v * 4);
        st.fill(p.beat_mask, 0, n_v);
        if (st.e == hipSuccess && frame_pass) hipLaunchKernelGGL(k_beat_metrics_timeline<true>, dim3(plan.tiles()), dim3(256), 0, 0, p);
        if (st.e == hipSuccess && reduce) hipLaunchKernelGGL(k_beat_reduce_timeline<true>, dim3(B), dim3(256), 0, 0, p);
    } else {
        if (st.e == hipSuccess && frame_pass) hipLaunchKernelGGL(k_beat_metrics_timeline<false>, dim3(tiles_of(N), B), dim3(256), 0, 0, p);
        if (st.e == hipSuccess && reduce) hipLaunchKernelGGL(k_beat_reduce_timeline<false>, dim3(B), dim3(256), 0, 0, p);
    }
    return st.finish();
}

}  // namespace
}  // namespace ls

extern "C" int ls_ragged_tiles(int batch, const int32_t* frames, int tile, int32_t* clip_out, int32_t* start_out, int32_t cap,
                               int32_t* n_out) {
    if (batch < 1 || !frames || tile < 1) return LS_EINVAL;
    long long n = 0;
    for (int b = 0; b < batch; ++b) {
        if (frames[b] < 1) return LS_EINVAL;
        n += ((long long)frames[b] + tile - 1) / tile;
    }
    if (n > 0x7fffffffLL) return LS_EINVAL;
    if (clip_out || start_out) {
        if ((long long)cap < n) return LS_EINVAL;
        long long i = 0;
        for (int b = 0; b < batch; ++b)
            for (long long t0 = 0; t0 < frames[b]; t0 += tile, ++i) {
                if (clip_out) clip_out[i] = b;
                if (start_out) start_out[i] = (int32_t)t0;
            }
    }
    if (n_out) *n_out = (int32_t)n;
    return LS_OK;
}

extern "C" int ls_ted_post_timeline(int device, int on_device, int batch, int n_frames, const ls_post_config* c, const float* timeline,
                                    float* aligned, float* pose, float* angle_diff, unsigned char* beat_mask) {
    return ls::ted_post_timeline(device, on_device, batch, n_frames, nullptr, false, c, timeline, aligned, pose, angle_diff, beat_mask);
}

extern "C" int ls_ted_post_timeline_ragged(int device, int on_device, int batch, int n_frames, const int32_t* frames,
                                           const ls_post_config* c, const float* timeline, float* aligned, float* pose, float* angle_diff,
                                           unsigned char* beat_mask) {
    return ls::ted_post_timeline(device, on_device, batch, n_frames, frames, true, c, timeline, aligned, pose, angle_diff, beat_mask);
}

extern "C" int ls_beat_post_timeline(int device, int on_device, int batch, int njoints, int n_frames, const float* timeline,
                                     float* decoded, float* euler_deg) {
    return ls::beat_post_timeline(device, on_device, batch, njoints, n_frames, nullptr, false, timeline, decoded, euler_deg);
}

extern "C" int ls_beat_post_timeline_ragged(int device, int on_device, int batch, int njoints, int n_frames, const int32_t* frames,
                                            const float* timeline, float* decoded, float* euler_deg) {
    return ls::beat_post_timeline(device, on_device, batch, njoints, n_frames, frames, true, timeline, decoded, euler_deg);
}

extern "C" int ls_beat_metrics_timeline(int device, int n_frames, const ls_beat_metrics_args* a) {
    return ls::beat_metrics_timeline(device, n_frames, nullptr, false, a);
}

extern "C" int ls_beat_metrics_timeline_ragged(int device, int n_frames, const int32_t* frames, const ls_beat_metrics_args* a) {
    return ls::beat_metrics_timeline(device, n_frames, frames, true, a);
}

extern "C" int ls_ted_beat_align(int device, const ls_ted_align_args* a) {
    using namespace ls;
    if (!a || !a->beat_mask || !a->onset_frames || !a->onset_count || a->batch < 1 || a->n_frames < 4 || a->n_frames > kMaxN ||
        a->onset_cols < 1)
        return LS_EINVAL;
    if (!(a->fps > 0.0) || !(a->sigma > 0.0) || !(a->sr > 0.0) || a->hop < 1) return LS_EINVAL;
    const int B = a->batch;
    if (!a->on_device)
        for (int b = 0; b < B; ++b)
            if (a->onset_count[b] < 0 || a->onset_count[b] > a->onset_cols) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    TedAlignParams p{};
    p.N = a->n_frames; p.onset_cols = a->onset_cols; p.hop = a->hop; p.fps = a->fps; p.sigma = a->sigma; p.sr = a->sr;
    Staging st(a->on_device != 0);
    p.beat_mask = st.in(a->beat_mask, (size_t)B * a->n_frames);
    p.onset_frames = st.in(a->onset_frames, (size_t)B * a->onset_cols);
    p.onset_count = st.in(a->onset_count, (size_t)B);
    p.align_sum = st.out(a->align_sum, (size_t)B);
    p.n_beats = st.out(a->n_beats, (size_t)B);
    if (st.e == hipSuccess && (p.align_sum || p.n_beats)) hipLaunchKernelGGL(k_ted_align, dim3(B), dim3(256), 0, 0, p);
    return st.finish();
}
