// Philox draws keyed per ROW (ls_set_row_keys, a keyed session pool): row b draws every stream at gidx = table[b] in place of
// CallParams::sample_offset + b.  The step kernels do not learn about the table: the draws of a stretch of executed steps are written to
// device tapes in the layouts the LS_NOISE_TORCH_DEVICE ring has (eps [K][2][B][D], noise and inpainting re-noise [K][B][J][F][T]) and the loop reads them as
// it reads that ring.  The counters and the Box-Muller arithmetic are ls_philox.h's, unchanged, so a tape element is the bits the
// in-kernel draw of the same (seed, gidx, step, stream, element) would have been.  The table sits at a fixed device address and is
// rewritten in stream order ahead of a loop; no key is a launch argument, so a captured loop replays under other keys.
#include "ls_philox.h"

namespace ls {

// x_T of row b in the internal layout [B][T][JF]: stream 0 of step id 0xFFFFFF, element c * T + f (k_randn_fill's).  One Philox
// block per thread; the row's last block may be partial (TED: J*F*T = 918 = 229 * 4 + 2).
__global__ void k_row_xt(const RowDrawArgs a) {
    const int b = blockIdx.y, n = a.JF * a.T;
    const unsigned blk = blockIdx.x * blockDim.x + threadIdx.x;
    if (4u * blk >= (unsigned)n) return;
    float z[4];
    philox_normal4(a.call, a.gidx[b], 0xFFFFFFu, 0u, blk, z);
    float* const row = a.x + (size_t)b * n;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = (int)(4u * blk) + j;
        if (e < n) { const int c = e / a.T, f = e - c * a.T; row[f * a.JF + c] = z[j]; }
    }
}

// The draws of executed steps k0 .. k0 + nsteps - 1 into slots 0 .. nsteps - 1 of the ring.  grid (blocks, B, nsteps); one Philox
// block per thread: threads [0, D / 2) of a (row, step) draw the style eps of the cond and the uncond pass (streams 1 and 2, D / 4
// blocks each: whole float4 groups, D = 512), the threads behind them the step noise (stream 3), which the loop's last step does not
// read and which is not drawn there.  With a.inz as many threads again draw the inpainting branch's re-noise of the kept motion
// (stream 4, element c * T + f of the reference layout: the draw k_inpaint_update makes itself where it is given no tape), under
// the same rule for the last step (t == 0 re-noises nothing).  A noise row starts 8-byte aligned at best (918 floats), hence
// scalar stores there.
__global__ void k_row_draws(const RowDrawArgs a) {
    const int b = blockIdx.y, r = blockIdx.z, k = a.k0 + r, n = a.JF * a.T;
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long gidx = a.gidx[b];
    float z[4];
    if (t < (unsigned)(kD / 2)) {
        const unsigned p = t / (kD / 4), blk = t - p * (kD / 4);
        philox_normal4(a.call, gidx, (unsigned)k, 1u + p, blk, z);
        float* const row = a.eps + (((size_t)r * 2 + p) * a.B + b) * kD;
        *reinterpret_cast<float4*>(row + 4 * blk) = make_float4(z[0], z[1], z[2], z[3]);
        return;
    }
    if (k == a.last_step) return;
    const unsigned nblk = ((unsigned)n + 3u) / 4u;
    unsigned blk = t - (unsigned)(kD / 2);
    const bool renoise = a.inz && blk >= nblk;      // the threads behind the step noise's: stream 4, same element order
    if (renoise) blk -= nblk;
    if (blk >= nblk) return;
    philox_normal4(a.call, gidx, (unsigned)k, renoise ? 4u : 3u, blk, z);
    float* const row = (renoise ? a.inz : a.noise) + ((size_t)r * a.B + b) * n;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((int)(4u * blk) + j < n) row[4 * blk + j] = z[j];
}

hipError_t launch_row_xt(const RowDrawArgs& a, hipStream_t st) {
    const int blocks = (a.JF * a.T + 3) / 4;
    hipLaunchKernelGGL(k_row_xt, dim3((blocks + 255) / 256, a.B), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_row_draws(const RowDrawArgs& a, hipStream_t st) {
    const int threads = kD / 2 + (a.JF * a.T + 3) / 4 * (a.inz ? 2 : 1);
    hipLaunchKernelGGL(k_row_draws, dim3((threads + 255) / 256, a.B, a.nsteps), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace ls
