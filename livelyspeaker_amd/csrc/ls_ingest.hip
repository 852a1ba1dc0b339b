// Dataset ingest on the device: recorded poses and audio -> the tensors the model, the evaluators and the trainer take.
//   k_ingest_resample_dirvec   resample_pose_seq + convert_pose_seq_to_dir_vec, once per resampled frame (scripts/utils/data_utils.py:46-56,
//                              101-120): overlapping windows (stride 10 of 42) share their frames, so nothing is interpolated twice
//   k_ted_ingest_window        one workgroup per window: MotionPreprocessor's three statistics and verdict (motion_preprocessor.py),
//                              the [:n_poses] clipping (lmdb_data_loader.py:166-174), the model's [9,3,T] layout and the audio window
//   k_beat_ingest_window       one workgroup per window: `* std + mean`, Euler XYZ -> rot6d (scripts_beat/data_libs/process_cache.py:38-45)
// Latency-bound gathers and a few hundred flops per frame; what they buy is that a recording crosses to the device once, as recorded,
// and every window is cut there.  The audio windows are read straight from the recording, np.pad(mode='symmetric') as index
// arithmetic; every per-window sum is a fixed tree, so a window's numbers do not depend on the batch it travels in.
#include "ls_hip.h"
#include "ls_ingest.h"
#include "ls_ingest_frame.h"

namespace ls {
namespace {

constexpr int kFramesPerBlock = 16;
constexpr int kWinThreads = 256;

// sum over the workgroup's 256 values as a fixed binary tree in LDS; every thread receives it
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kWinThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float block_max(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = kWinThreads / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// the window's samples of np.pad(recording, (0, n_pad), mode='symmetric'): index k >= L reads L - 1 - (k - L).  The entry has
// checked 0 <= start and start + out_len <= 2 L, so one reflection is all there is and no index leaves the recording.
__device__ __forceinline__ void audio_window(const IngestAudio& au, int w, int clip) {
    if (!au.out) return;
    const int64_t L = au.len[clip], s = au.win_start[w];
    const float* src = au.audio + au.off[clip];
    float* dst = au.out + (size_t)w * au.out_len;
    for (int i = threadIdx.x; i < au.out_len; i += kWinThreads) {
        int64_t k = s + i;
        if (k >= L) k = 2 * L - 1 - k;
        dst[i] = src[k];
    }
}

}  // namespace

__global__ __launch_bounds__(64) void k_ingest_resample_dirvec(IngestFrameArgs a) {
    __shared__ float sp[kFramesPerBlock * kIngestPose];
    __shared__ float sd[kFramesPerBlock * kIngestDir];
    const int f0 = blockIdx.x * kFramesPerBlock, tid = threadIdx.x;
    const int nf = min(kFramesPerBlock, a.n_frames - f0);
    for (int i = tid; i < nf * kIngestPose; i += 64) {
        const int f = i / kIngestPose, c = i - f * kIngestPose, row = f0 + f;
        const float* rec = a.raw + a.raw_off[a.clip[row]] * kIngestPose;
        const float v = ingest_lerp(rec[(size_t)a.lo[row] * kIngestPose + c], rec[(size_t)a.hi[row] * kIngestPose + c], a.frac[row]);
        sp[i] = v;
        if (a.resampled) a.resampled[(size_t)f0 * kIngestPose + i] = v;
    }
    __syncthreads();
    for (int i = tid; i < nf * kIngestBones; i += 64) {
        const int f = i / kIngestBones, j = i - f * kIngestBones;
        ingest_bone_dir(&sp[f * kIngestPose + 3 * a.bone_child[j]], &sp[f * kIngestPose + 3 * a.bone_parent[j]], &sd[f * kIngestDir + 3 * j]);
    }
    __syncthreads();
    for (int i = tid; i < nf * kIngestDir; i += 64) a.dir_vec[(size_t)f0 * kIngestDir + i] = sd[i];
}

__global__ __launch_bounds__(kWinThreads) void k_ted_ingest_window(TedWindowArgs a) {
    __shared__ float sp[LS_INGEST_MAX_EXT * kIngestPose];      // the window's n_ext poses, [T][30]
    // [T][27] with the row stride left at 27: the transposed read below has consecutive lanes on consecutive frames, and 27 is
    // coprime to the 32 banks of a ds_read_b32, so the 32 lanes of a half-wave fall on 32 different banks (a padded stride of 28
    // would put them on 8)
    __shared__ float sv[LS_INGEST_MAX_POSES * kIngestDir];
    __shared__ float red[kWinThreads];
    __shared__ float smean[kIngestPose + kIngestDir];
    __shared__ float svar[6];
    const int w = blockIdx.x, tid = threadIdx.x;
    const int clip = a.win_clip[w];
    const size_t row0 = (size_t)a.frame_off[clip] + a.win_first[w];
    const int n_in = a.n_ext * kIngestPose, n_pose = a.n_poses * kIngestPose, n_vec = a.n_poses * kIngestDir;
    if (tid < kIngestPose) smean[tid] = a.mean_pose[tid];
    else if (tid < kIngestPose + kIngestDir) smean[tid] = a.mean_dir_vec[tid - kIngestPose];
    __syncthreads();
    for (int i = tid; i < n_in; i += kWinThreads) {
        const float v = a.resampled[row0 * kIngestPose + i];
        sp[i] = v;
        if (a.pose_seq && i < n_pose) a.pose_seq[(size_t)w * n_pose + i] = v;
    }
    for (int i = tid; i < n_vec; i += kWinThreads) {
        const float v = a.dir_vec[row0 * kIngestDir + i] - smean[kIngestPose + i % kIngestDir];      // normalize_dir_vec
        sv[i] = v;
        if (a.vec_seq) a.vec_seq[(size_t)w * n_vec + i] = v;
    }
    __syncthreads();
    if (a.x) {
        for (int i = tid; i < n_vec; i += kWinThreads) {                   // [T][JF] -> [JF][T]
            const int c = i / a.n_poses, t = i - c * a.n_poses;
            a.x[(size_t)w * n_vec + i] = sv[t * kIngestDir + c];
        }
    }
    // MotionPreprocessor over the n_ext frames.  check_pose_diff: mean |pose - mean_pose|
    float part = 0.f;
    for (int i = tid; i < n_in; i += kWinThreads) part += fabsf(sp[i] - smean[i % kIngestPose]);
    const float pose_diff = block_sum(part, red) / (float)n_in;
    // check_spine_angle: max and mean over the frames
    const float ang = tid < a.n_ext ? ingest_spine_angle_deg(&sp[tid * kIngestPose], &sp[tid * kIngestPose + 3]) : 0.f;
    const float spine_mean = block_sum(ang, red) / (float)a.n_ext;
    const float spine_max = block_max(tid < a.n_ext ? ang : -INFINITY, red);
    // check_static_motion: np.var (two passes, / n) of the three coordinates of joints 6 and 9, one thread per coordinate, in frame order
    if (tid < 6) {
        const int col = tid < 3 ? 6 * 3 + tid : 9 * 3 + tid - 3;
        float m = 0.f, v = 0.f;
        for (int t = 0; t < a.n_ext; ++t) m += sp[t * kIngestPose + col];
        m /= (float)a.n_ext;
        for (int t = 0; t < a.n_ext; ++t) { const float d = sp[t * kIngestPose + col] - m; v += d * d; }
        svar[tid] = v / (float)a.n_ext;
    }
    __syncthreads();
    if (tid == 0) {
        const float left = svar[0] + svar[1] + svar[2], right = svar[3] + svar[4] + svar[5];
        int verdict = LS_INGEST_PASS;
        if (!a.win_has_words[w]) verdict = LS_INGEST_WORDS;
        else if (pose_diff < 0.02f) verdict = LS_INGEST_POSE;
        else if (spine_max > 30.f || spine_mean > 20.f) verdict = LS_INGEST_SPINE;
        else if (left < 0.0014f && right < 0.0014f) verdict = LS_INGEST_MOTION;
        if (a.verdict) a.verdict[w] = verdict;
        if (a.stats) {
            float* s = a.stats + (size_t)w * LS_INGEST_N_STATS;
            s[0] = pose_diff; s[1] = spine_max; s[2] = spine_mean; s[3] = left; s[4] = right;
        }
    }
    audio_window(a.au, w, clip);
}

constexpr int kBeatRows = 34, kBeatJoints = 47;       // the entry refuses more
constexpr int kBeatStride = kBeatJoints * 6 + 1;      // odd: the transposed read of the [T][J*6] tile is conflict-free, as in k_ted_ingest_window

__global__ __launch_bounds__(kWinThreads) void k_beat_ingest_window(BeatWindowArgs a) {
    __shared__ float tile[kBeatRows * kBeatStride];
    const int w = blockIdx.x, tid = threadIdx.x;
    const int clip = a.win_clip[w];
    const int J = a.njoints, J3 = J * 3, J6 = J * 6;
    const float* rec = a.poses + ((size_t)a.pose_off[clip] + a.win_first[w]) * J3;
    for (int i = tid; i < a.n_poses * J; i += kWinThreads) {
        const int t = i / J, j = i - t * J;
        float o[6];
        beat_euler_to_rot6d(rec + (size_t)t * J3 + 3 * j, a.mean + 3 * j, a.std + 3 * j, o);
#pragma unroll
        for (int f = 0; f < 6; ++f) tile[t * kBeatStride + 6 * j + f] = o[f];
    }
    __syncthreads();
    const int n_out = a.n_poses * J6;
    if (a.rot6d) {
        for (int i = tid; i < n_out; i += kWinThreads) {
            const int t = i / J6, c = i - t * J6;
            a.rot6d[(size_t)w * n_out + i] = tile[t * kBeatStride + c];
        }
    }
    if (a.x) {
        for (int i = tid; i < n_out; i += kWinThreads) {                   // [T][J*6] -> [J][6][T]
            const int c = i / a.n_poses, t = i - c * a.n_poses;
            a.x[(size_t)w * n_out + i] = tile[t * kBeatStride + c];
        }
    }
    if (a.verdict && tid == 0) a.verdict[w] = a.win_has_words && !a.win_has_words[w] ? LS_INGEST_WORDS : LS_INGEST_PASS;
    audio_window(a.au, w, clip);
}

hipError_t launch_ingest_frames(const IngestFrameArgs& a, hipStream_t st) {
    if (a.n_frames < 1) return hipSuccess;
    hipLaunchKernelGGL(k_ingest_resample_dirvec, dim3((a.n_frames + kFramesPerBlock - 1) / kFramesPerBlock), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_ted_ingest_windows(const TedWindowArgs& a, int n_windows, hipStream_t st) {
    if (n_windows < 1) return hipSuccess;
    hipLaunchKernelGGL(k_ted_ingest_window, dim3(n_windows), dim3(kWinThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_beat_ingest_windows(const BeatWindowArgs& a, int n_windows, hipStream_t st) {
    if (n_windows < 1) return hipSuccess;
    hipLaunchKernelGGL(k_beat_ingest_window, dim3(n_windows), dim3(kWinThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace ls
