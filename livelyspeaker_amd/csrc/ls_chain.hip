// Window hand-off of long-form synthesis (ls_long_sample, ls_sample.cpp): the model continues a 34-frame clip by conditioning the next
// one on its last n_pre_seq poses (origin_x[..., :n_pre_seq], RAG.py:110-112).  k_chain_window does everything of that hand-off that
// touches device memory, so the host copies nothing from the device and does not synchronise between two windows:
//   * the n_pre rows per clip of feat_u that change with the window ([poses | 1 | 0 pad]: exactly what k_build_feats writes for them;
//     the rows of the frames n_pre.. are zero and stay so from the call's first window),
//   * the prefix columns of origin_x in the reference layout [B][JF][T] (the rest stays zero; in the LivelySpeaker chain this is also
//     the SAG decoder's `x`, which reads those columns only),
//   * the finished window's new frames into the stitched timeline [B][JF][T_total], and the raw window [B][JF][T] when asked for.
// One workgroup per clip.  The previous window's sample arrives in the internal layout [T][JF] and leaves transposed, so it is staged
// through LDS once (row stride JF | 1: odd, the transposed reads touch every bank once) and every global store runs along the frame axis.
// Algorithmic bytes per clip (fp32): read T*JF (window 0: n_pre*JF seed poses), write n_pre*(KPP + JF) + (T - n_pre)*JF (+ T*JF raw
// window; window 0 writes all T frames): 7.9 KB TED, 81 KB BEAT.
#include "ls_internal.h"

namespace ls {

__global__ __launch_bounds__(256) void k_chain_window(const ChainArgs a) {
    extern __shared__ float tile[];                 // [T][JF | 1]
    const int b = blockIdx.x, tid = threadIdx.x, JF = a.JF, T = a.T, ld = JF | 1, npre = a.n_pre;
    if (a.prev) {
        const float* src = a.prev + (size_t)b * T * JF;
        for (int i = tid; i < T * JF; i += 256) tile[(i / JF) * ld + i % JF] = src[i];
        __syncthreads();
    }
    if (a.feat_u) {
        // prefix pose j of the coming window: frame T - n_pre + j of the previous one, or the caller's seed pose j
        float* fu = a.feat_u + (size_t)b * T * a.KPP;
        for (int i = tid; i < npre * a.KPP; i += 256) {
            const int j = i / a.KPP, c = i - j * a.KPP;
            float v = c == JF ? 1.f : 0.f;
            if (c < JF) v = a.prev ? tile[(T - npre + j) * ld + c] : a.seed[((size_t)b * JF + c) * npre + j];
            fu[i] = v;
        }
        float* ox = a.origin_x + (size_t)b * JF * T;
        for (int i = tid; i < JF * npre; i += 256) {
            const int c = i / npre, j = i - c * npre;
            ox[(size_t)c * T + j] = a.prev ? tile[(T - npre + j) * ld + c] : a.seed[((size_t)b * JF + c) * npre + j];
        }
    }
    if (!a.prev) return;
    if (a.timeline) {                               // frames f0 .. T-1 of the finished window -> timeline frames t_off ..
        const int nf = T - a.f0;
        float* tl = a.timeline + (size_t)b * JF * a.T_total + a.t_off;
        for (int i = tid; i < JF * nf; i += 256) {
            const int c = i / nf, f = i - c * nf;
            tl[(size_t)c * a.T_total + f] = tile[(a.f0 + f) * ld + c];
        }
    }
    if (a.window) {
        float* wd = a.window + (size_t)b * JF * T;
        for (int i = tid; i < JF * T; i += 256) wd[i] = tile[(i % T) * ld + i / T];
    }
}

hipError_t launch_chain_window(const ChainArgs& a, int B, hipStream_t st) {
    const size_t lds = (size_t)a.T * (a.JF | 1) * sizeof(float);
    if (lds > 64 * 1024 || a.n_pre > a.T || a.f0 < 0 || a.f0 > a.T || a.t_off < 0 || a.t_off + (a.T - a.f0) > a.T_total) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chain_window, dim3(B), dim3(256), lds, st, a);
    return hipGetLastError();
}

}  // namespace ls
