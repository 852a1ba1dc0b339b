// The post-processing stream's kernels: ls_timeline.hip's per-frame outputs for the frames a push brings, with the left halo taken
// from a per-slot CARRY in place of the input.
//   k_ted_post_stream   grid (tile of new frames): layout change, mean add, bone normalisation, change curve, pose, and the beat of
//                       the frame BEFORE each new frame (the beat at f needs angle_diff[f + 1])
//   k_beat_post_stream  grid (tile, joint chunk | series): layout change and rot6d -> Euler per joint chunk; the last y index stages the
//                       six series joints' Euler triples, forms the velocities and decides the minima that lag order + 1 frames
// Slot s holds n frames so far and gets k new ones; a tile is kPsTile units of the slot (new frames; for BEAT also beat entries) from
// the (slot, first unit) table the host builds, so work follows what arrived.  The halo is RECOMPUTED from raw carried values with the
// functions of ls_post_frame.h, exactly as the timeline kernels recompute theirs from the input: TED carries the slot's last 3 raw
// frames (the beat at n - 1 needs angle_diff[n - 2 .. n], hence frames n - 3 .. n), BEAT the last 2 order + 1 Euler triples of the six
// series joints (the oldest undecided minimum, n - order - 1, looks `order` velocities to its left).  Only a slot's tile 0 can reach
// behind frame n, so tile 0 alone reads the carry and, past a barrier, rewrites it: from the input where the new frames suffice and
// from the old carry it has staged where they do not (chunks of 1 or 2 frames).  Input behind a slot's k frames is never read; the
// host zeroes every output ahead of the launch, which is also what TED's one pending entry at the finish is (frame N - 1 is never a
// beat).  LDS rows keep ls_timeline.hip's odd strides.
// Bytes per new frame (fp32): TED reads 108 and writes 108 + 120 + 5; BEAT (J = 47) reads 1128 + 144 and writes 1692 + 6.
#include "ls_post_stream.h"

namespace ls {
namespace {

constexpr int kTile = kPsTile, kSeries = kPsSeries;
constexpr int kHalo = kPsTedCarry;                // TED: frames n + t0 - 3 .. n + t0 + kTile - 1
constexpr int kStage = kTile + kHalo;
constexpr int kLd = (kMaxBones + 1) * 3 + 2;      // 53, as k_ted_timeline
constexpr int kJChunk = 16;
constexpr int kLd6 = kJChunk * 6 + 1, kLd3 = kJChunk * 3 + 1;
constexpr int kRows = kTile + kPsBeatCarry;       // BEAT series: frames bf + t0 - order .. bf + t0 + kTile + order
constexpr int kLdRaw = kSeries * 6 + 1, kLdEu = kPsBeatRow + 1;

static_assert(kLd % 2 == 1 && kLd6 % 2 == 1 && kLd3 % 2 == 1 && kLdRaw % 2 == 1 && kLdEu % 2 == 1, "odd LDS row strides");
static_assert(kTile <= 256, "one thread per unit of a tile");

}  // namespace

__global__ __launch_bounds__(256) void k_ted_post_stream(PostParams p, TedStreamArgs a) {
    __shared__ float sv[kStage][kLd];           // raw, then aligned + mean (un-normalised)
    __shared__ float sn[kStage][kLd];           // per-bone unit vectors, later the tile's poses
    __shared__ float sang[kMaxPairs][kStage];
    __shared__ float sdiff[kStage];
    const int s = a.t.tile_slot[blockIdx.x], t0 = a.t.tile_start[blockIdx.x], k = a.t.k[s], tid = threadIdx.x;
    const long long n = a.t.n[s], N = n + k, f_lo = n + t0 - kHalo;            // staged row l holds the series' frame f_lo + l
    const int JF = p.njoints * 3;
    const float* in = a.frames + (size_t)s * JF * a.K;
    float* carry = a.carry + (size_t)s * JF * kHalo;
    for (int i = tid; i < JF * kStage; i += 256) {                      // lanes along the frame axis
        const int c = i / kStage, l = i - c * kStage;
        const long long f = f_lo + l;
        if (f < 0 || f >= N) continue;
        sv[l][c] = f >= n ? in[(size_t)c * a.K + (int)(f - n)] : carry[c * kHalo + (int)(f - (n - kHalo))];
    }
    __syncthreads();
    if (t0 == 0) {                                                      // the carry of the next push: frames N - 3 .. N - 1
        for (int i = tid; i < JF * kHalo; i += 256) {
            const int c = i / kHalo, r = i - c * kHalo;
            const long long f = N - kHalo + r;
            if (f < 0) continue;
            carry[c * kHalo + r] = f >= n ? in[(size_t)c * a.K + (int)(f - n)] : sv[(int)(f - f_lo)][c];
        }
        __syncthreads();
    }
    for (int i = tid; i < kStage * JF; i += 256) {                      // [S,J,3,K] -> [S,K,J*3]: lanes along the channel axis
        const int l = i / JF, c = i - l * JF;
        const long long f = f_lo + l;
        if (f < 0 || f >= N) continue;
        const float v = sv[l][c];
        if (a.aligned && l >= kHalo) a.aligned[((size_t)s * a.K + (t0 + l - kHalo)) * JF + c] = v;
        sv[l][c] = v + p.mean_dir_vec[c];
    }
    __syncthreads();
    for (int i = tid; i < kStage * p.njoints; i += 256) {
        const int l = i / p.njoints, j = i - l * p.njoints;
        const long long f = f_lo + l;
        if (f >= 0 && f < N) ted_unit(&sv[l][3 * j], &sn[l][3 * j]);
    }
    __syncthreads();
    for (int i = tid; i < kStage * p.n_pairs; i += 256) {
        const int q = i / kStage, l = i - q * kStage;
        const long long f = f_lo + l;
        if (f >= 0 && f < N) sang[q][l] = ted_pair_angle(&sn[l][3 * p.pair_a[q]], &sn[l][3 * p.pair_b[q]]);
    }
    __syncthreads();
    if (tid >= 1 && tid < kStage) {                                     // the curve at frames f_lo + 1 ..; the series' frame 0 holds 0
        const int l = tid;
        const long long f = f_lo + l;
        if (f >= 0 && f < N) {
            const float d = f > 0 ? ted_angle_change(p, &sang[0][l], &sang[0][l - 1], kStage) : 0.f;
            sdiff[l] = d;
            if (a.angle_diff && l >= kHalo) a.angle_diff[(size_t)s * a.K + (t0 + l - kHalo)] = d;
        }
    }
    __syncthreads();
    if (a.beat_mask && tid < kTile && t0 + tid < k) {                   // new frame g decides the beat at g - 1: a minimum at t >= 2
        const int l = tid + kHalo;
        const long long e = n + t0 + tid - 1, first = n > 0 ? n - 1 : 0;
        if (e >= 0) {
            bool beat = false;
            if (e >= 2) beat = ted_is_beat(sdiff[l - 1], sdiff[l - 2], sdiff[l], p.thres);
            a.beat_mask[(size_t)s * a.Kb + (int)(e - first)] = beat ? 1 : 0;
        }
    }
    if (!a.pose) return;
    if (tid < kTile && t0 + tid < k) ted_pose_frame(p, sv[tid + kHalo], sn[tid + kHalo]);       // sn: every reader is past the barrier above
    __syncthreads();
    const int PJ = p.n_pose_joints * 3;
    for (int i = tid; i < kTile * PJ; i += 256) {
        const int l = i / PJ, c = i - l * PJ;
        if (t0 + l < k) a.pose[((size_t)s * a.K + t0 + l) * PJ + c] = sn[l + kHalo][c];
    }
}

namespace {

// k_beat_post_timeline's body on the new frames [t0, t0 + kTile) of slot s and the joints [j0, j0 + kJChunk)
__device__ __forceinline__ void beat_frames_tile(const BeatStreamArgs& a, int s, int t0, int k, int j0) {
    __shared__ float s6[kTile][kLd6];
    __shared__ float s3[kTile][kLd3];
    const int tid = threadIdx.x, J = a.J;
    const int nj = J - j0 < kJChunk ? J - j0 : kJChunk, C = nj * 6, E = nj * 3;
    for (int i = tid; i < C * kTile; i += 256) {                        // lanes along the frame axis
        const int c = i / kTile, l = i - c * kTile;
        if (t0 + l < k) s6[l][c] = a.frames[(((size_t)s * J + j0) * 6 + c) * a.K + t0 + l];
    }
    __syncthreads();
    if (a.decoded) {
        for (int i = tid; i < kTile * C; i += 256) {
            const int l = i / C, c = i - l * C;
            if (t0 + l < k) a.decoded[(((size_t)s * a.K + t0 + l) * J + j0) * 6 + c] = s6[l][c];
        }
    }
    if (!a.euler) return;
    for (int i = tid; i < kTile * nj; i += 256) {
        const int l = i / nj, j = i - l * nj;
        if (t0 + l >= k) continue;
        float d6[6], o[3];
#pragma unroll
        for (int q = 0; q < 6; ++q) d6[q] = s6[l][6 * j + q];
        beat_rot6d_to_euler(d6, o);
        s3[l][3 * j] = o[0]; s3[l][3 * j + 1] = o[1]; s3[l][3 * j + 2] = o[2];
    }
    __syncthreads();
    for (int i = tid; i < kTile * E; i += 256) {
        const int l = i / E, c = i - l * E;
        if (t0 + l < k) a.euler[(((size_t)s * a.K + t0 + l) * J + j0) * 3 + c] = s3[l][c];
    }
}

// the beat entries [t0, t0 + kTile) of the ones this push decides for slot s, in k_beat_metrics_timeline's expressions; tile 0 also
// rewrites the slot's carry
__device__ __forceinline__ void beat_series_tile(const BeatStreamArgs& a, int s, int t0, int k, long long n, int fin) {
#pragma clang fp contract(off)
    __shared__ float sraw[kRows][kLdRaw];       // the six series joints' rot6d of the staged new frames
    __shared__ float se[kRows][kLdEu];          // their Euler triples: new frames computed, older ones from the carry
    __shared__ float svel[kSeries][kRows];
    const int tid = threadIdx.x, order = a.order, live = 2 * order + 1;
    const long long N = n + k, V = N - 1;
    const long long first = n - order - 1 > 0 ? n - order - 1 : 0;                 // ls_post_stream_plan's range
    const long long decided = N - order - 1 > 0 ? N - order - 1 : 0;
    const int count = (int)((fin ? (V > 0 ? V : 0) : decided) - first);
    const long long f_lo = first + t0 - order;                                    // staged row l holds the series' frame f_lo + l
    float* carry = a.carry + (size_t)s * kPsBeatCarry * kPsBeatRow;                // row r: frame n - live + r
    for (int i = tid; i < kSeries * 6 * kRows; i += 256) {                          // lanes along the frame axis
        const int c = i / kRows, l = i - c * kRows;
        const long long f = f_lo + l;
        if (f < n || f >= N) continue;
        sraw[l][c] = a.frames[(((size_t)s * a.J + a.joint[c / 6]) * 6 + c % 6) * a.K + (int)(f - n)];
    }
    for (int i = tid; i < kRows * kPsBeatRow; i += 256) {
        const int l = i / kPsBeatRow, c = i - l * kPsBeatRow;
        const long long f = f_lo + l, r = f - (n - live);
        if (f >= 0 && f < n && r >= 0) se[l][c] = carry[(int)r * kPsBeatRow + c];
    }
    __syncthreads();
    for (int i = tid; i < kRows * kSeries; i += 256) {
        const int l = i / kSeries, j = i - l * kSeries;
        const long long f = f_lo + l;
        if (f < n || f >= N) continue;
        float d6[6], o[3];
#pragma unroll
        for (int q = 0; q < 6; ++q) d6[q] = sraw[l][6 * j + q];
        beat_rot6d_to_euler(d6, o);
        se[l][3 * j] = o[0]; se[l][3 * j + 1] = o[1]; se[l][3 * j + 2] = o[2];
    }
    __syncthreads();
    if (t0 == 0 && k > 0) {                                                       // the carry of the next push: frames N - live .. N - 1
        for (int i = tid; i < live * kSeries; i += 256) {
            const int r = i / kSeries, j = i - r * kSeries;
            const long long f = N - live + r;                                     // >= f_lo: f_lo is n - live, or below 0
            if (f < 0) continue;
            float o[3];
            if (f - f_lo < kRows) {
                const int l = (int)(f - f_lo);
                o[0] = se[l][3 * j]; o[1] = se[l][3 * j + 1]; o[2] = se[l][3 * j + 2];
            } else {                                                              // a new frame beyond this tile's rows
                float d6[6];
#pragma unroll
                for (int q = 0; q < 6; ++q) d6[q] = a.frames[(((size_t)s * a.J + a.joint[j]) * 6 + q) * a.K + (int)(f - n)];
                beat_rot6d_to_euler(d6, o);
            }
            carry[r * kPsBeatRow + 3 * j] = o[0]; carry[r * kPsBeatRow + 3 * j + 1] = o[1]; carry[r * kPsBeatRow + 3 * j + 2] = o[2];
        }
    }
    if (!a.beat_mask || t0 >= count) return;
    for (int i = tid; i < kSeries * (kRows - 1); i += 256) {                        // v[f] = |e[f + 1] - e[f]| for f in [0, V)
        const int j = i / (kRows - 1), l = i - j * (kRows - 1);
        const long long f = f_lo + l;
        if (f < 0 || f >= V) continue;
        const float* p0 = &se[l][3 * j];
        const float* p1 = &se[l + 1][3 * j];
        const float dx = p1[0] - p0[0], dy = p1[1] - p0[1], dz = p1[2] - p0[2];
        svel[j][l] = sqrtf((dx * dx + dy * dy) + dz * dz);
    }
    __syncthreads();
    if (tid < kTile && t0 + tid < count) {
        const long long f = first + t0 + tid;
        for (int j = 0; j < kSeries; ++j) {
            const float x = svel[j][(int)(f - f_lo)];
            bool beat = true;
            for (int q = 1; q <= order && beat; ++q) {
                const long long l = f - q < 0 ? 0 : f - q, h = f + q > V - 1 ? V - 1 : f + q;
                beat = x < svel[j][(int)(l - f_lo)] && x < svel[j][(int)(h - f_lo)];
            }
            a.beat_mask[((size_t)s * kSeries + j) * a.Kb + t0 + tid] = beat ? 1 : 0;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(256) void k_beat_post_stream(BeatStreamArgs a) {
    const int s = a.t.tile_slot[blockIdx.x], t0 = a.t.tile_start[blockIdx.x], k = a.t.k[s];
    if (blockIdx.y + 1 == gridDim.y) {
        beat_series_tile(a, s, t0, k, a.t.n[s], a.t.fin[s]);
    } else if (t0 < k) {
        beat_frames_tile(a, s, t0, k, (int)blockIdx.y * kJChunk);
    }
}

hipError_t launch_ted_post_stream(const PostParams& p, const TedStreamArgs& a, unsigned tiles, hipStream_t stream) {
    hipLaunchKernelGGL(k_ted_post_stream, dim3(tiles), dim3(256), 0, stream, p, a);
    return hipGetLastError();
}

hipError_t launch_beat_post_stream(const BeatStreamArgs& a, unsigned tiles, hipStream_t stream) {
    const unsigned chunks = (unsigned)((a.J + kJChunk - 1) / kJChunk);
    hipLaunchKernelGGL(k_beat_post_stream, dim3(tiles, chunks + 1), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace ls
