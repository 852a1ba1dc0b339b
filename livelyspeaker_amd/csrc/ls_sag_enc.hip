// SAG encoder: Encoder_TRANSFORMER.forward, scripts/model/motionclip_module.py:33-95 (eval mode) --
// xseq = [muQuery | sigmaQuery | skelEmbedding(frames)] + pe[0:36]; 3 x nn.TransformerEncoderLayer (post-norm, 4 heads x 128, FFN
// 512-1024-512 with exact GELU) under src_key_padding_mask = ~[1, 1, mask]; mu = token 0 of the last layer.
// The linears run on the fp32 MFMA GEMM (ls_gemm.hip), the 36-token self-attention is ls_sag.hip's kernel instantiated for S = 36 with
// a key mask; this file holds what is the encoder's own: the token builder's staging kernel and the last layer's one-query attention.
#include "ls_internal.h"
#include "ls_lanes.h"

namespace ls {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));

// Workgroup = one sample.  x[b] ([JF][T], frames contiguous) is read coalesced into LDS (row stride T + 1: the transposed read below
// walks c at a fixed f) and leaves as the GEMM operand xt[b*T + f][0..KP) = x[b, :, f], zero beyond JF (KP = JF rounded up to the
// GEMM's K tile, so the skelEmbedding product stays on the full-tile path; BEAT's K = 282 is a real contraction).  The token rows
// are seeded with what the product is added onto: pe[f + 2] for the frames, query + pe for the two learned tokens (:81-84).
__global__ __launch_bounds__(256) void k_sag_enc_prepare(const float* __restrict__ x, const unsigned char* __restrict__ mask,
                                                         const float* __restrict__ mu_q, const float* __restrict__ sigma_q,
                                                         const float* __restrict__ pe, float* __restrict__ tok, float* __restrict__ xt,
                                                         unsigned char* __restrict__ kmask, int JF, int KP) {
    extern __shared__ float sx[];                                 // [JF][T + 1]
    constexpr int S = kSagEncS, LX = kT + 1;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xb = x + (size_t)b * JF * kT;
    for (int i = tid; i < JF * kT; i += 256) sx[(i / kT) * LX + i % kT] = xb[i];
    if (tid < S) kmask[b * S + tid] = tid < 2 ? 1 : (mask ? (mask[b * kT + tid - 2] != 0) : 1);
    f4* tb = reinterpret_cast<f4*>(tok + (size_t)b * S * kD);
    const f4* pv = reinterpret_cast<const f4*>(pe);
    for (int i = tid; i < S * kD / 4; i += 256) {
        f4 v = pv[i];
        if (i < kD / 4) v += reinterpret_cast<const f4*>(mu_q)[i];
        else if (i < 2 * kD / 4) v += reinterpret_cast<const f4*>(sigma_q)[i - kD / 4];
        tb[i] = v;
    }
    __syncthreads();
    float* xo = xt + (size_t)b * kT * KP;
    for (int i = tid; i < kT * KP; i += 256) {
        const int f = i / KP, c = i - f * KP;
        xo[i] = c < JF ? sx[c * LX + f] : 0.f;
    }
}

// Last layer, token 0 only (the encoder returns final[0]): one query against the 36 keys of its sample, per head.  Workgroup = one
// sample, wave = head, lane = two of the head's 128 features: every K / V row segment is one coalesced 512-byte read straight into
// registers (all 72 issued together), a score is a wave-wide sum, the softmax runs on wave-uniform scalars in the order of
// k_sag_attention (max, exp, sum, e * 1/sum; a masked key is -inf before the max), and P.V is lane-local.
template <int HD>
__global__ __launch_bounds__(256) void k_sag_enc_attention_row0(const float* __restrict__ q0, const float* __restrict__ kv,
                                                                const unsigned char* __restrict__ kmask, float* __restrict__ out, int D,
                                                                int heads) {
    static_assert(HD == 128, "lane = two features of a 128-wide head");
    constexpr int S = kSagEncS;
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float scale = rsqrtf((float)HD);
    for (int h = w; h < heads; h += 4) {
        const float* kb = kv + (size_t)b * S * 2 * D + h * HD + 2 * lane;
        f2 k[S], v[S];
#pragma unroll
        for (int j = 0; j < S; ++j) {
            k[j] = *reinterpret_cast<const f2*>(kb + (size_t)j * 2 * D);
            v[j] = *reinterpret_cast<const f2*>(kb + (size_t)j * 2 * D + D);
        }
        const f2 q = *reinterpret_cast<const f2*>(q0 + (size_t)b * D + h * HD + 2 * lane) * scale;      // torch scales q before q.k^T
        float s[S], m = -INFINITY;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            s[j] = wave_sum(fmaf(q[0], k[j][0], q[1] * k[j][1]));
            if (kmask[b * S + j] == 0) s[j] = -INFINITY;
            m = fmaxf(m, s[j]);
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < S; ++j) { s[j] = expf(s[j] - m); sum += s[j]; }
        const float inv = 1.0f / sum;
        f2 o = (f2){0.f, 0.f};
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const float p = s[j] * inv;
            o[0] = fmaf(p, v[j][0], o[0]);
            o[1] = fmaf(p, v[j][1], o[1]);
        }
        *reinterpret_cast<f2*>(out + (size_t)b * D + h * HD + 2 * lane) = o;
    }
}

hipError_t launch_sag_enc_prepare(const float* x, const unsigned char* mask, const float* mu_q, const float* sigma_q, const float* pe,
                                  float* tok, float* xt, unsigned char* kmask, int B, int JF, int KP, hipStream_t st) {
    const size_t lds = (size_t)JF * (kT + 1) * sizeof(float);
    if (KP < JF || lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sag_enc_prepare, dim3(B), dim3(256), lds, st, x, mask, mu_q, sigma_q, pe, tok, xt, kmask, JF, KP);
    return hipGetLastError();
}
hipError_t launch_sag_enc_attention_row0(const float* q0, const float* kv, const unsigned char* kmask, float* out, int B, int heads, int D,
                                         hipStream_t st) {
    if (D / heads != 128 || !kmask) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_sag_enc_attention_row0<128>), dim3(B), dim3(256), 0, st, q0, kv, kmask, out, D, heads);
    return hipGetLastError();
}

}  // namespace ls
