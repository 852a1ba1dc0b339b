// torch's DEVICE normal stream, restated (LS_NOISE_TORCH_DEVICE): what torch.randn / randn_like draw on a ROCm GPU, so that a loop
// whose callers run the reference on the GPU (scripts/test_RAG_ted.py:21, device = cuda:0) gets the reference's noise bit for bit.
//
// torch (ATen/native/hip/DistributionTemplates.h: calc_execution_policy, distribution_elementwise_grid_stride_kernel,
// normal_and_transform) fills a float32 tensor of n elements with generator state (seed, offset) as follows: G = min(ceil(n / 256),
// CUs * (maxThreadsPerMultiProcessor / 256)) blocks of 256 threads, S = 256 G threads; thread idx owns a Philox4x32-10 state whose
// counter is (offset / 4 + r, idx) (64-bit words 0-1, 64-bit words 2-3) and whose key is the seed; its r-th hiprand_normal4 gives the
// elements li = (4 r + ii) S + idx, ii = 0..3, in memory order (TensorIterator walks a dense tensor in memory order).  The offset then
// advances by 4 ceil(n / (4 S)).  hiprand_normal4 = rocrand's normal_distribution4: Box-Muller on (r0, r1) and (r2, r3) with the SINE
// in the first output (rocrand/rocrand_normal.h box_muller) -- not the transform of ls_philox.h's box_muller.  The expressions below
// are rocrand's, compiled with the same defaults (FP contraction on: the two uniform conversions become FMAs; __sincosf =
// v_sin_f32 / v_cos_f32), except logf, whose expansion is spelled out in the rounding torch's kernel uses (torch_logf); the tests
// compare the result with torch itself.
#include "ls_philox.h"

namespace ls {

// logf of u in [2^-32, 1] (normal numbers: no denormal scaling) as torch's kernel evaluates it: log2 on v_log_f32, then times ln2 in
// two parts -- the rounded product with the high part, plus (its exact residual and the product with the low part, by FMAs) -- added
// in a SEPARATE rounding.  A compiler that expands logf itself may fuse that last add into an FMA (one ulp apart in ~10 % of the
// draws), so the expansion is written out with contraction off.
__device__ __forceinline__ float torch_logf(float u) {
#pragma clang fp contract(off)
    const float l2 = __builtin_amdgcn_logf(u);
    const float hi = l2 * 0x1.62e42ep-1f;                           // ln2 high part (0x3f317217)
    float lo = __builtin_fmaf(l2, 0x1.62e42ep-1f, -hi);
    lo = __builtin_fmaf(l2, 0x1.efa39ep-25f, lo);                   // ln2 low part (0x3377d1cf)
    return hi + lo;
}

__device__ __forceinline__ void torch_box_muller(unsigned x, unsigned y, float& first, float& second) {
    const float u = 2.3283064e-10f + (x * 2.3283064e-10f);          // ROCRAND_2POW32_INV
    const float v = 1.46291807e-09f + (y * 1.46291807e-09f);        // ROCRAND_2POW32_INV_2PI
    const float s = sqrtf(-2.0f * torch_logf(u));                   // sqrtf: correctly rounded, as in torch's build
    __sincosf(v, &first, &second);
    first *= s;
    second *= s;
}

// one rocrand Philox block at counter (ctr, idx) under the 64-bit key `seed`: four normals
__device__ __forceinline__ void torch_normal4(unsigned long long seed, unsigned long long ctr, unsigned long long idx, float z[4]) {
    unsigned c[4] = {(unsigned)ctr, (unsigned)(ctr >> 32), (unsigned)idx, (unsigned)(idx >> 32)};
    philox4x32(c, (unsigned)seed, (unsigned)(seed >> 32));
    torch_box_muller(c[0], c[1], z[0], z[1]);
    torch_box_muller(c[2], c[3], z[2], z[3]);
}

// element li of a draw alone: its Philox block and the one Box-Muller output it takes
__device__ __forceinline__ float torch_normal1(unsigned long long seed, unsigned long long off4, unsigned li, unsigned S) {
    const unsigned idx = li % S, j = li / S;
    unsigned c[4] = {(unsigned)(off4 + (j >> 2)), (unsigned)((off4 + (j >> 2)) >> 32), idx, 0u};
    philox4x32(c, (unsigned)seed, (unsigned)(seed >> 32));
    float first, second;
    torch_box_muller((j & 2) ? c[2] : c[0], (j & 2) ? c[3] : c[1], first, second);
    return (j & 1) ? second : first;
}

// blockIdx.y = (step r of the launch, draw d).  Plain draws: a thread computes one Philox block -- torch's thread idx = w mod S, its
// round w / S -- and stores the four elements that block feeds (S apart: coalesced across the wave).  Draws in x's [T][B][J][F] memory
// order (perm) would scatter those stores T floats apart into the [B][J][F][T] tape, so there a thread owns one TAPE element
// o = (b J F + jf) T + t instead and evaluates its block for that element alone (li = t B J F + b J F + jf; li = o at the first step).
__global__ __launch_bounds__(256) void k_torch_draws(TorchDrawArgs a) {
    const int r = blockIdx.y / a.ndraw, di = blockIdx.y - r * a.ndraw;
    const TorchDraw& d = a.d[di];
    const unsigned w = blockIdx.x * 256u + threadIdx.x;
    if (w >= d.work) return;
    const int k = a.k0 + r;
    if (d.skip_last && k == a.last_step) return;
    unsigned long long rel = a.rel0 + (unsigned long long)r * a.step_adv;
    for (int e = 0; e < di; ++e)
        if (!(a.d[e].skip_last && k == a.last_step)) rel += a.d[e].adv;
    const unsigned long long off = a.call->sample_offset + rel;
    float* dst = d.dst + (size_t)r * d.dst_stride;
    if (d.perm) {
        unsigned li = w;
        if (k > 0) {
            const unsigned c = w / a.T, t = w - c * a.T;
            li = t * ((unsigned)a.B * a.JF) + c;
        }
        dst[w] = torch_normal1(a.call->seed, off / 4, li, d.S) + 0.0f;
        return;
    }
    const unsigned S = d.S, idx = w % S, rr = w / S;
    float z[4];
    torch_normal4(a.call->seed, off / 4 + rr, idx, z);
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) {
        const unsigned long long li = (4ull * rr + ii) * S + idx;
        if (li < d.n) dst[li] = z[ii] + 0.0f;      // torch's transformation::normal, mean 0, std 1: fma(1, z, 0) (-0 becomes +0)
    }
}

hipError_t launch_torch_draws(const TorchDrawArgs& a, hipStream_t st) {
    if (a.nsteps < 1 || a.ndraw < 1 || a.ndraw > 4) return hipErrorInvalidValue;
    unsigned long long wmax = 0;
    for (int d = 0; d < a.ndraw; ++d) {
        if (a.d[d].n >= (1ull << 31) || a.d[d].work >= (1ull << 32) - 256) return hipErrorInvalidValue;   // 32-bit element indices, as torch's launch
        if (a.d[d].work > wmax) wmax = a.d[d].work;
    }
    const unsigned long long gy = (unsigned long long)a.nsteps * a.ndraw;
    if (gy > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_torch_draws, dim3((unsigned)((wmax + 255) / 256), (unsigned)gy), dim3(256), 0, st, a);
    return hipGetLastError();
}

// torch's launch geometry for n elements: threads of the grid-stride loop (*S) and the generator offset advance
unsigned long long torch_randn_advance(long long n, int n_cu, int max_threads_per_cu, unsigned* S) {
    if (S) *S = 0;
    if (n <= 0 || n_cu <= 0 || max_threads_per_cu < 256) return 0;
    const unsigned long long blocks = ((unsigned long long)n + 255) / 256;
    const unsigned long long cap = (unsigned long long)n_cu * (unsigned)(max_threads_per_cu / 256);
    const unsigned long long threads = 256ull * (blocks < cap ? blocks : cap);
    if (S) *S = (unsigned)threads;
    return (((unsigned long long)n - 1) / (threads * 4) + 1) * 4;
}

TorchDraw torch_draw(float* dst, size_t dst_stride, long long n, int n_cu, int max_threads_per_cu, int perm, int skip_last) {
    TorchDraw d{};
    d.dst = dst; d.dst_stride = dst_stride; d.n = (unsigned long long)n;
    d.adv = torch_randn_advance(n, n_cu, max_threads_per_cu, &d.S);
    d.work = perm ? (unsigned long long)n : (unsigned long long)d.S * (d.adv / 4);     // perm: one thread per element
    d.perm = perm; d.skip_last = skip_last;
    return d;
}

// const_noise's x_T: every sample becomes sample 0 (x_init[[0]].repeat(B, 1, 1, 1))
__global__ void k_bcast_first(float* __restrict__ x, int B, int per) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= per) return;
    const float v = x[i];
    for (int b = 1; b < B; ++b) x[(size_t)b * per + i] = v;
}
hipError_t launch_bcast_first(float* x, int B, int per, hipStream_t st) {
    if (B > 1) hipLaunchKernelGGL(k_bcast_first, dim3((per + 255) / 256), dim3(256), 0, st, x, B, per);
    return hipGetLastError();
}

}  // namespace ls
