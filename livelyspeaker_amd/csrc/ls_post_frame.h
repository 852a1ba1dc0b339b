// The per-frame arithmetic of the caller-side post-processing, stated once: the 34-frame kernels (ls_post.hip) and the timeline
// kernels (ls_timeline.hip) call these, so a frame's numbers do not depend on which kernel computed them.  Every function takes and
// returns values; loads, stores and the staging in LDS belong to the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "ls_hip.h"

namespace ls {

constexpr int kMaxBones = 16, kMaxPairs = 8;

struct PostParams {
    int njoints;                       // bones (direction vectors), 9 for TED
    int n_pairs;
    int pair_a[kMaxPairs], pair_b[kMaxPairs];
    float change_angle[kMaxPairs];
    float thres;
    int n_pose_joints;                 // 10
    int bone_parent[kMaxBones], bone_child[kMaxBones];
    float bone_len[kMaxBones];
    float mean_dir_vec[kMaxBones * 3];
};

// host: the one check and copy of a caller's configuration (ls_ted_post and the timeline entries).  false, and LS_EINVAL from the
// entry, for what would index outside a frame: the bone tree indexes ted_pose_frame's kMaxBones + 1 joints, a pair the frame's bones
inline bool post_params(const ls_post_config* c, PostParams* p) {
    if (!c || c->njoints < 1 || c->njoints > kMaxBones || c->n_pairs < 0 || c->n_pairs > kMaxPairs || c->n_pose_joints < 0 ||
        c->n_pose_joints > kMaxBones + 1)
        return false;
    for (int j = 0; j < c->njoints; ++j)
        if (c->bone_parent[j] < 0 || c->bone_parent[j] > kMaxBones || c->bone_child[j] < 0 || c->bone_child[j] > kMaxBones) return false;
    for (int k = 0; k < c->n_pairs; ++k)
        if (c->pair_a[k] < 0 || c->pair_a[k] >= c->njoints || c->pair_b[k] < 0 || c->pair_b[k] >= c->njoints) return false;
    *p = PostParams{};
    p->njoints = c->njoints; p->n_pairs = c->n_pairs; p->thres = c->thres; p->n_pose_joints = c->n_pose_joints;
    for (int k = 0; k < c->n_pairs; ++k) { p->pair_a[k] = c->pair_a[k]; p->pair_b[k] = c->pair_b[k]; p->change_angle[k] = c->change_angle[k]; }
    for (int j = 0; j < c->njoints; ++j) { p->bone_parent[j] = c->bone_parent[j]; p->bone_child[j] = c->bone_child[j]; p->bone_len[j] = c->bone_len[j]; }
    for (int j = 0; j < c->njoints * 3; ++j) p->mean_dir_vec[j] = c->mean_dir_vec[j];
    return true;
}

// F.normalize(dim=-1) of one bone: x / max(||x||, 1e-12); in: the un-normalised vector, out: the unit vector
__device__ __forceinline__ void ted_unit(const float* in, float* out) {
    const float x = in[0], y = in[1], z = in[2];
    const float inv = 1.0f / fmaxf(sqrtf(x * x + y * y + z * z), 1e-12f);
    out[0] = x * inv; out[1] = y * inv; out[2] = z * inv;
}

// angle between two unit bones, in units of pi
__device__ __forceinline__ float ted_pair_angle(const float* u, const float* v) {
    float ip = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
    ip = fminf(fmaxf(ip, -1.0f), 1.0f);
    return acosf(ip) * 0.3183098861837907f;
}

// one frame of the joint-angle change curve: ang and prev hold the pair angles of the frame and of the one before it, `stride`
// floats apart per pair
__device__ __forceinline__ float ted_angle_change(const PostParams& p, const float* ang, const float* prev, int stride) {
    float d = 0.f;
    for (int k = 0; k < p.n_pairs; ++k)
        d += fabsf(ang[k * stride] - prev[k * stride]) / p.change_angle[k] / (float)p.n_pairs;
    return d;
}

// a motion beat: a strict local minimum of the change curve that lies at least thres below one neighbour
__device__ __forceinline__ bool ted_is_beat(float c, float l, float r, float thres) {
    return (c < l && c < r) && (l - c >= thres || r - c >= thres);
}

// convert_dir_vec_to_pose of one frame: sv holds its njoints * 3 un-normalised direction vectors, o receives n_pose_joints * 3
__device__ __forceinline__ void ted_pose_frame(const PostParams& p, const float* sv, float* o) {
    float jp[kMaxBones + 1][3];
    for (int j = 0; j < p.n_pose_joints; ++j) jp[j][0] = jp[j][1] = jp[j][2] = 0.f;
    for (int j = 0; j < p.njoints; ++j)
        for (int e = 0; e < 3; ++e) jp[p.bone_child[j]][e] = jp[p.bone_parent[j]][e] + p.bone_len[j] * sv[3 * j + e];
    for (int j = 0; j < p.n_pose_joints; ++j)
        for (int e = 0; e < 3; ++e) o[3 * j + e] = jp[j][e];
}

// rot6d -> Euler XYZ in degrees of one joint.  rotation_6d_to_matrix (rot_utils.py:529-534): b1 = normalize(a1),
// b2 = normalize(a2 - (b1.a2) b1), b3 = b1 x b2; rows of M.  matrix_to_euler_angles(M, "XYZ") (rot_utils.py:238-257):
// (atan2(-m12, m22), asin(m02), atan2(-m01, m00))
__device__ __forceinline__ void beat_rot6d_to_euler(const float* d6, float* o) {
    const float n1 = fmaxf(sqrtf(d6[0] * d6[0] + d6[1] * d6[1] + d6[2] * d6[2]), 1e-12f);      // F.normalize: x / max(|x|, eps)
    const float b1x = d6[0] / n1, b1y = d6[1] / n1, b1z = d6[2] / n1;
    const float dt = b1x * d6[3] + b1y * d6[4] + b1z * d6[5];
    float b2x = d6[3] - dt * b1x, b2y = d6[4] - dt * b1y, b2z = d6[5] - dt * b1z;
    const float n2 = fmaxf(sqrtf(b2x * b2x + b2y * b2y + b2z * b2z), 1e-12f);
    b2x /= n2; b2y /= n2; b2z /= n2;
    const float b3z = b1x * b2y - b1y * b2x;                           // only m22 of the third row is needed
    const float k = 57.29577951308232f;                                // / pi * 180
    o[0] = atan2f(-b2z, b3z) * k;
    o[1] = asinf(b1z) * k;
    o[2] = atan2f(-b1y, b1x) * k;
}

}  // namespace ls
