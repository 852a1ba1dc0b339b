// Caller-side post-processing of a sampled batch, one workgroup per clip:
//   aligned_motions = sample.permute(0,3,1,2).reshape(B,34,27)                      scripts/test_RAG_ted.py:84
//   beat_vec = normalize(aligned + mean_dir_vec);  joint-angle change curve;  motion beats   :88-111
//   convert_dir_vec_to_pose(aligned + mean_dir_vec)                                scripts/utils/data_utils.py:77-97
// Tiny and latency-bound (918 floats per clip); it exists so the sampled tensor never has to leave the GPU in the
// reference's [B,J,F,T] layout just to be transposed and scanned on the host.
#include "ls_hip.h"
#include "ls_internal.h"
#include "ls_post_frame.h"
#include "ls_staging.h"

namespace ls {

__global__ __launch_bounds__(64) void k_ted_post(const float* __restrict__ sample, PostParams p, float* __restrict__ aligned,
                                                 float* __restrict__ pose, float* __restrict__ angle_diff,
                                                 unsigned char* __restrict__ beat_mask) {
    __shared__ float sv[kT][kMaxBones * 3];     // aligned + mean (un-normalised)
    __shared__ float sn[kT][kMaxBones * 3];     // per-bone unit vectors
    __shared__ float sang[kMaxPairs][kT];
    __shared__ float sdiff[kT];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int JF = p.njoints * 3;
    for (int i = tid; i < kT * JF; i += 64) {
        const int f = i / JF, c = i - f * JF;
        const float v = sample[((size_t)b * JF + c) * kT + f];          // [B,J,F,T] -> [B,T,J*F]
        if (aligned) aligned[(size_t)b * kT * JF + i] = v;
        sv[f][c] = v + p.mean_dir_vec[c];
    }
    __syncthreads();
    for (int i = tid; i < kT * p.njoints; i += 64) {                    // F.normalize(dim=-1): x / max(||x||, 1e-12)
        const int f = i / p.njoints, j = i - f * p.njoints;
        ted_unit(&sv[f][3 * j], &sn[f][3 * j]);
    }
    __syncthreads();
    for (int i = tid; i < kT * p.n_pairs; i += 64) {                    // angle between the two bones of each pair
        const int k = i / kT, f = i - k * kT;
        sang[k][f] = ted_pair_angle(&sn[f][3 * p.pair_a[k]], &sn[f][3 * p.pair_b[k]]);
    }
    __syncthreads();
    if (tid < kT) {
        const float d = tid > 0 ? ted_angle_change(p, &sang[0][tid], &sang[0][tid - 1], kT) : 0.f;
        sdiff[tid] = d;
        if (angle_diff) angle_diff[(size_t)b * kT + tid] = d;
    }
    __syncthreads();
    if (beat_mask && tid < kT) {                                        // local minima of the change curve, t in [2, 32]
        bool beat = false;
        if (tid >= 2 && tid <= kT - 2) beat = ted_is_beat(sdiff[tid], sdiff[tid - 1], sdiff[tid + 1], p.thres);
        beat_mask[(size_t)b * kT + tid] = beat ? 1 : 0;
    }
    if (pose) {                                                         // joint positions along the bone tree
        for (int f = tid; f < kT; f += 64) ted_pose_frame(p, sv[f], pose + ((size_t)b * kT + f) * p.n_pose_joints * 3);
    }
}

}  // namespace ls

extern "C" int ls_ted_post(int device, int on_device, int batch, const ls_post_config* c, const float* sample,
                           float* aligned, float* pose, float* angle_diff, unsigned char* beat_mask) {
    using namespace ls;
    PostParams p;
    if (!sample || batch < 1 || !post_params(c, &p)) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    const size_t n_in = (size_t)batch * p.njoints * 3 * kT, n_t = (size_t)batch * kT;
    Staging st(on_device != 0);
    const float* d_in = st.in(sample, n_in);
    float* d_al = st.out(aligned, n_in);
    float* d_pose = st.out(pose, n_t * p.n_pose_joints * 3);
    float* d_diff = st.out(angle_diff, n_t);
    unsigned char* d_mask = st.out(beat_mask, n_t);
    if (st.e == hipSuccess) hipLaunchKernelGGL(k_ted_post, dim3(batch), dim3(64), 0, 0, d_in, p, d_al, d_pose, d_diff, d_mask);
    return st.finish();
}

// ---- BEAT: rot6d -> rotation matrix -> Euler XYZ (degrees), plus the [B,J,6,T] -> [B,T,J*6] layout change --------------------
namespace ls {

__global__ __launch_bounds__(256) void k_beat_post(const float* __restrict__ sample, float* __restrict__ decoded, float* __restrict__ euler,
                                                   int J, size_t total) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;          // one thread per (b, t, joint)
    if (i >= total) return;
    const int j = (int)(i % J);
    const size_t bt = i / J;
    const int t = (int)(bt % kT);
    const size_t b = bt / kT;
    float d6[6];
#pragma unroll
    for (int f = 0; f < 6; ++f) d6[f] = sample[((b * J + j) * 6 + f) * kT + t];
    if (decoded) {
#pragma unroll
        for (int f = 0; f < 6; ++f) decoded[(bt * J + j) * 6 + f] = d6[f];
    }
    if (!euler) return;
    beat_rot6d_to_euler(d6, euler + (bt * J + j) * 3);
}

}  // namespace ls

extern "C" int ls_beat_post(int device, int on_device, int batch, int njoints, const float* sample, float* decoded, float* euler_deg) {
    using namespace ls;
    if (!sample || batch < 1 || njoints < 1) return LS_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return LS_EHIP;
    const size_t n_in = (size_t)batch * njoints * 6 * kT, total = (size_t)batch * kT * njoints;
    Staging st(on_device != 0);
    const float* d_in = st.in(sample, n_in);
    float* d_dec = st.out(decoded, n_in);
    float* d_eu = st.out(euler_deg, total * 3);
    if (st.e == hipSuccess)
        hipLaunchKernelGGL(k_beat_post, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, d_in, d_dec, d_eu, njoints, total);
    return st.finish();
}
