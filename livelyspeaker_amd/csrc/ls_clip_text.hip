// CLIP text encoder (ViT-B/32's text tower: 12 pre-norm blocks, width 512, 8 heads of 64, context 77): what is the tower's own --
// the token plan, the embedding gather into packed rows, the causal attention and the EOT-row gather.  The linears run on the fp32
// LDS-DMA GEMM (ls_gemm.hip, QuickGELU = activation 4), the LayerNorms on k_layernorm512 (ls_sag.hip); ls_clip_text_api.cpp chains them.
//
// Packing.  The mask is causal and only the row at the EOT token is read out, so rows behind EOT cannot reach the result: sample b
// contributes its rows 0 .. eot[b] only (len[b] = eot[b] + 1), stored back to back from row0[b] = sum of the lengths before it.  The
// full form (prune = 0) is the same code with len[b] = context and row0[b] = context * b.
#include "ls_internal.h"
#include "ls_lanes.h"

namespace ls {

typedef float f4 __attribute__((ext_vector_type(4)));

// Device tokens: plan[b] = first position of the row maximum (torch.argmax; EOT is the largest id), plan[B] = number of ids outside
// [0, vocab).  One wave per sample, lane = positions lane and lane + 64.  The host reads the B + 1 ints back and builds row0 / len.
__global__ __launch_bounds__(256) void k_clip_plan(const long long* __restrict__ tok, int* __restrict__ plan, int B, int ctx, int vocab) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    long long best = -1;             // below every valid id; an invalid row is an error whatever its argmax
    int pos = ctx, bad = 0;
    for (int t = lane; t < ctx; t += 64) {
        const long long v = tok[(size_t)b * ctx + t];
        if (v < 0 || v >= vocab) ++bad;
        if (v > best) { best = v; pos = t; }              // ascending t: the first position of this lane's maximum
    }
    // the wave's maximum, ties to the smaller position
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long long ob = __shfl_xor(best, off);
        const int op = __shfl_xor(pos, off);
        bad += __shfl_xor(bad, off);
        if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
    }
    if (lane == 0) {
        plan[b] = pos;
        if (bad) atomicAdd(&plan[B], bad);
    }
}

// x[row0[b] + t] = token_embedding[tok[b][t]] + positional_embedding[t] for t < len[b].  Workgroup = one sample, two rows at a time
// (128 float4 per row).  Token ids were range-checked by the plan (on the host or by k_clip_plan) before this kernel is launched.
__global__ __launch_bounds__(256) void k_clip_embed(const long long* __restrict__ tok, const int* __restrict__ row0, const int* __restrict__ len,
                                                    const float* __restrict__ temb, const float* __restrict__ pemb, float* __restrict__ x, int ctx) {
    const int b = blockIdx.x, half = threadIdx.x >> 7, c = threadIdx.x & 127;
    const int n = len[b], r0 = row0[b];
    for (int t = half; t < n; t += 2) {
        const long long id = tok[(size_t)b * ctx + t];
        const f4 v = reinterpret_cast<const f4*>(temb + (size_t)id * kD)[c] + reinterpret_cast<const f4*>(pemb + (size_t)t * kD)[c];
        reinterpret_cast<f4*>(x + (size_t)(r0 + t) * kD)[c] = v;
    }
}

// e[b] = x[row0[b] + eot[b]]: the B rows that leave the tower
__global__ __launch_bounds__(128) void k_clip_gather_eot(const float* __restrict__ x, const int* __restrict__ row0, const int* __restrict__ eot,
                                                         float* __restrict__ e) {
    const int b = blockIdx.x;
    reinterpret_cast<f4*>(e + (size_t)b * kD)[threadIdx.x] = reinterpret_cast<const f4*>(x + (size_t)(row0[b] + eot[b]) * kD)[threadIdx.x];
}

// nn.MultiheadAttention self-attention under the causal mask (-inf strictly above the diagonal) of one sample's S = len[b] <= 80 rows.
// qkv rows are [q | k | v] of width 3*D (packed in_proj), packed per sample from row0[b].  Workgroup = one sample, 4 waves, looping
// over its heads with the NEXT head's Q / K / V in flight in registers, as k_sag_attention (ls_sag.hip) does.  S is padded to
// NT = ceil(S / 16) <= 5 tiles of 16 on v_mfma_f32_16x16x4_f32; the tiles wholly above the diagonal or beyond S are never computed:
//   scores = Q K^T : the NT (NT + 1) / 2 tiles (mt, nt <= mt), dealt round-robin to the waves; K-dim = HD in the k-permuted float4 order
//   softmax        : one wave per query row a, lane = keys lane and lane + 64; a key beyond a is -inf before the row maximum, so its
//                    probability is exactly 0, and it is written as 0 up to the end of the row's diagonal tile (P.V's K padding)
//   out = P V      : wave = one of the HD / 16 = 4 feature tiles, all NT row tiles; row tile mt contracts keys 0 .. 16 (mt + 1) - 1
// A row's result depends on its own index a and its own keys alone: the wave-wide max / sum run over all 64 lanes in a fixed pattern
// (masked keys enter as -inf / 0) and P.V sums keys in ascending groups of four up to the end of a's diagonal tile.  Neither len[b]
// nor the other samples enter, which is what makes the pruned and the full form, and any batch composition, agree bitwise.
// LDS is sized by the launch for SP = 16 * (the batch's largest NT) rows: Q (pre-scaled), K, V [SP][HD + 4] and scores / P [SP][81].
// Rows S .. 16 NT - 1 of Q / K / V hold copies of row S - 1 (finite; they only meet masked scores and zero probabilities).
template <int HD>
__global__ __launch_bounds__(256) void k_clip_attention(const float* __restrict__ qkv, float* __restrict__ out, const int* __restrict__ row0,
                                                        const int* __restrict__ len, int D, int heads, int SP) {
    static_assert(HD == 64, "one P.V feature tile per wave; 16 float4 per row");
    constexpr int LQ = HD + 4, LP = kClipLP, MAXT = 5;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sq = smem;
    float* sk = sq + SP * LQ;
    float* sv = sk + SP * LQ;
    float* sp = sv + SP * LQ;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int s16 = lane & 15, g = lane >> 4;
    const int S = __builtin_amdgcn_readfirstlane(len[b]), r0 = __builtin_amdgcn_readfirstlane(row0[b]);
    const int NT = (S + 15) >> 4;                                 // <= SP / 16 <= MAXT (checked by the launcher's caller)
    const float scale = rsqrtf((float)HD);
    f4 vq[MAXT], vk[MAXT], vv[MAXT];
    // this thread's share of one head's Q / K / V: chunk j = the 16 rows of tile j (thread = (row in tile, float4 of the row))
    const int tr = tid >> 4, d4 = tid & 15;
    auto fetch = [&](int h) {
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
            if (j < NT) {
                const float* row = qkv + (size_t)(r0 + min(16 * j + tr, S - 1)) * 3 * D + h * HD + 4 * d4;
                vq[j] = *reinterpret_cast<const f4*>(row);
                vk[j] = *reinterpret_cast<const f4*>(row + D);
                vv[j] = *reinterpret_cast<const f4*>(row + 2 * D);
            }
        }
    };
    fetch(0);
    for (int h = 0; h < heads; ++h) {
        if (h) __syncthreads();                                   // the previous head's P.V is done reading sv / sp
#pragma unroll
        for (int j = 0; j < MAXT; ++j) {
            if (j < NT) {
                const int o = (16 * j + tr) * LQ + 4 * d4;
                *reinterpret_cast<f4*>(&sq[o]) = vq[j] * scale;   // torch scales q before q.k^T
                *reinterpret_cast<f4*>(&sk[o]) = vk[j];
                *reinterpret_cast<f4*>(&sv[o]) = vv[j];
            }
        }
        __syncthreads();
        if (h + 1 < heads) fetch(h + 1);                          // in flight during this head's scores / softmax / P.V
        // ---- scores: lane holds S[a = 16 mt + 4 g + r][c = 16 nt + s16]
        int tile = 0;
        for (int mt = 0; mt < NT; ++mt)
            for (int nt = 0; nt <= mt; ++nt, ++tile) {
                if ((tile & 3) != w) continue;
                const float* qa = sq + (16 * mt + s16) * LQ + 4 * g;
                const float* kb = sk + (16 * nt + s16) * LQ + 4 * g;
                f4 acc = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < HD / 16; ++q) {
                    const f4 av = *reinterpret_cast<const f4*>(qa + 16 * q), bv = *reinterpret_cast<const f4*>(kb + 16 * q);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], bv[e], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) sp[(16 * mt + 4 * g + r) * LP + 16 * nt + s16] = acc[r];
            }
        __syncthreads();
        // ---- softmax of query row a over keys 0 .. a: one wave per row
        for (int a = w; a < S; a += 4) {
            const int k1 = lane + 64, kend = 16 * (a / 16 + 1);   // keys a + 1 .. kend - 1: zero (the diagonal tile's upper part)
            const float v0 = lane <= a ? sp[a * LP + lane] : -INFINITY;
            const float v1 = k1 <= a ? sp[a * LP + k1] : -INFINITY;
            const float m = wave_max(fmaxf(v0, v1));
            const float e0 = lane <= a ? expf(v0 - m) : 0.f;
            const float e1 = k1 <= a ? expf(v1 - m) : 0.f;
            const float inv = 1.0f / wave_sum(e0 + e1);
            if (lane < kend) sp[a * LP + lane] = e0 * inv;
            if (k1 < kend) sp[a * LP + k1] = e1 * inv;
        }
        __syncthreads();
        // ---- out = P V: wave w owns feature tile w; lane holds O[a = 16 mt + 4 g + r][d = 16 w + s16]
        f4 acc[MAXT];
#pragma unroll
        for (int mt = 0; mt < MAXT; ++mt) acc[mt] = (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < MAXT; ++kt) {
            if (kt < NT) {
#pragma unroll
                for (int kq = 0; kq < 4; ++kq) {
                    const int key = 16 * kt + 4 * kq + g;
                    const float bv = sv[key * LQ + 16 * w + s16];
#pragma unroll
                    for (int mt = kt; mt < MAXT; ++mt) {
                        if (mt < NT) {
                            const float av = sp[min(16 * mt + s16, S - 1) * LP + key];      // rows S .. : clamped, never stored
                            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[mt], 0, 0, 0);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < MAXT; ++mt) {
            if (mt < NT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int a = 16 * mt + 4 * g + r;
                    if (a < S) out[(size_t)(r0 + a) * D + h * HD + 16 * w + s16] = acc[mt][r];
                }
            }
        }
    }
}

hipError_t launch_clip_plan(const long long* tok, int* plan, int B, int ctx, int vocab, hipStream_t st) {
    hipError_t e = hipMemsetAsync(plan + B, 0, sizeof(int), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_clip_plan, dim3((B + 3) / 4), dim3(256), 0, st, tok, plan, B, ctx, vocab);
    return hipGetLastError();
}
hipError_t launch_clip_embed(const long long* tok, const int* row0, const int* len, const float* temb, const float* pemb, float* x, int B,
                             int ctx, hipStream_t st) {
    hipLaunchKernelGGL(k_clip_embed, dim3(B), dim3(256), 0, st, tok, row0, len, temb, pemb, x, ctx);
    return hipGetLastError();
}
hipError_t launch_clip_gather_eot(const float* x, const int* row0, const int* eot, float* e, int B, hipStream_t st) {
    hipLaunchKernelGGL(k_clip_gather_eot, dim3(B), dim3(128), 0, st, x, row0, eot, e);
    return hipGetLastError();
}
// max_len: the largest len[b] of the batch (<= 80); it sizes the workgroup's LDS, nothing else
hipError_t launch_clip_attention(const float* qkv, float* out, const int* row0, const int* len, int B, int heads, int D, int max_len,
                                 hipStream_t st) {
    if (D / heads != 64 || max_len < 1 || max_len > 80) return hipErrorInvalidValue;
    const int SP = (max_len + 15) / 16 * 16;
    const size_t lds = (size_t)SP * (3 * (64 + 4) + kClipLP) * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_clip_attention<64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((k_clip_attention<64>), dim3(B), dim3(256), lds, st, qkv, out, row0, len, D, heads, SP);
    return hipGetLastError();
}

}  // namespace ls
