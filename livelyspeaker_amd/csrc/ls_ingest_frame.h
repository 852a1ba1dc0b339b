// The per-frame arithmetic of the dataset ingest (ls_ingest.hip), stated once beside ls_post_frame.h, whose inverse it is: values in,
// values out; loads, stores and the staging in LDS belong to the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "ls_hip.h"

namespace ls {

// interp1d(kind='linear') between two raw frames (utils/data_utils.py:46-56): y_lo + (y_hi - y_lo) * frac, each step rounded to
// float32 (no contraction into an fma, so the number does not depend on the compiler's choice); frac > 1 extrapolates
__device__ __forceinline__ float ingest_lerp(float y_lo, float y_hi, float frac) {
    return __fadd_rn(y_lo, __fmul_rn(__fsub_rn(y_hi, y_lo), frac));
}

// one bone of convert_pose_seq_to_dir_vec (utils/data_utils.py:101-120): child - parent, divided by its norm as
// sklearn.preprocessing.normalize does, where a zero norm divides by 1 and the direction stays zero (not NaN)
__device__ __forceinline__ void ingest_bone_dir(const float* child, const float* parent, float* out) {
    const float x = child[0] - parent[0], y = child[1] - parent[1], z = child[2] - parent[2];
    float n = sqrtf(x * x + y * y + z * z);
    if (n == 0.f) n = 1.f;
    out[0] = x / n; out[1] = y / n; out[2] = z / n;
}

// MotionPreprocessor.check_spine_angle's angle of one frame (motion_preprocessor.py:67-77), in degrees: between joint 1 - joint 0
// and (0, -1, 0), the cosine clipped to [-1, 1].  A zero spine gives NaN in the reference (0 / 0) and here.
__device__ __forceinline__ float ingest_spine_angle_deg(const float* j0, const float* j1) {
    const float x = j1[0] - j0[0], y = j1[1] - j0[1], z = j1[2] - j0[2];
    const float c = -y / sqrtf(x * x + y * y + z * z);
    return acosf(fminf(fmaxf(c, -1.0f), 1.0f)) * 57.29577951308232f;
}

// one BEAT joint (scripts_beat/data_libs/process_cache.py:38-45): normalised Euler degrees -> `* std + mean` -> radians (/ 180, then
// * pi, as the float32 tensor is scaled there) -> euler_angles_to_matrix(., "XYZ") = Rx Ry Rz -> matrix_to_rotation_6d, the first two
// rows.  Every product is rounded on its own, as torch.matmul's 3x3 products of float32 are not contracted with the sum in any fixed
// way; the entries with a structural zero or one are exact either way.
__device__ __forceinline__ void beat_euler_to_rot6d(const float* e_norm, const float* mean, const float* std, float* o) {
    float s[3], c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float deg = __fadd_rn(__fmul_rn(e_norm[k], std[k]), mean[k]);
        const float rad = __fmul_rn(deg / 180.0f, 3.14159265358979323846f);
        s[k] = sinf(rad);
        c[k] = cosf(rad);
    }
    // Rx Ry = [[cy, 0, sy], [sx sy, cx, -sx cy], [-cx sy, sx, cx cy]];  (Rx Ry) Rz, rows 0 and 1
    const float sxsy = __fmul_rn(s[0], s[1]), sxcy = __fmul_rn(s[0], c[1]);
    o[0] = __fmul_rn(c[1], c[2]);
    o[1] = -__fmul_rn(c[1], s[2]);
    o[2] = s[1];
    o[3] = __fadd_rn(__fmul_rn(sxsy, c[2]), __fmul_rn(c[0], s[2]));
    o[4] = __fadd_rn(-__fmul_rn(sxsy, s[2]), __fmul_rn(c[0], c[2]));
    o[5] = -sxcy;
}

}  // namespace ls
