// Window hand-off of long-form synthesis (ls_long_sample, ls_sample.cpp): the model continues a 34-frame clip by conditioning the next
// one on its last n_pre_seq poses (origin_x[..., :n_pre_seq], RAG.py:110-112).  k_chain_window does everything of that hand-off that
// touches device memory, so the host copies nothing from the device and does not synchronise between two windows:
//   * the n_pre rows per clip of feat_u that change with the window ([poses | 1 | 0 pad]: exactly what k_build_feats writes for them;
//     the rows of the frames n_pre.. are zero and stay so from the call's first window),
//   * the prefix columns of origin_x in the reference layout [B][JF][T] (the rest stays zero; in the LivelySpeaker chain this is also
//     the SAG decoder's `x`, which reads those columns only),
//   * the finished window's new frames into the stitched timeline [B][JF][T_total], and the raw window [B][JF][T] when asked for.
// One workgroup per clip (a ragged call: per slot of the longest-first order, see ChainArgs::row).  The previous window's sample arrives in the internal layout [T][JF] and leaves transposed, so it is staged
// through LDS once (row stride JF | 1: odd, the transposed reads touch every bank once) and every global store runs along the frame axis.
// Algorithmic bytes per clip (fp32): read T*JF (window 0: n_pre*JF seed poses), write n_pre*(KPP + JF) + (T - n_pre)*JF (+ T*JF raw
// window; window 0 writes all T frames): 7.9 KB TED, 81 KB BEAT.
#include "ls_internal.h"

namespace ls {

__global__ __launch_bounds__(256) void k_chain_window(const ChainArgs a) {
    extern __shared__ float tile[];                 // [T][JF | 1]
    const int b = blockIdx.x, tid = threadIdx.x, JF = a.JF, T = a.T, ld = JF | 1, npre = a.n_pre;
    const int r = a.row ? a.row[b] : b;             // the caller's clip behind slot b (ragged call; otherwise the slot itself)
    const bool next = !a.row || b < a.n_next;       // this clip runs the coming window
    if (a.prev) {
        const float* src = a.prev + (size_t)b * T * JF;
        for (int i = tid; i < T * JF; i += 256) tile[(i / JF) * ld + i % JF] = src[i];
        __syncthreads();
    }
    if (a.feat_u && next) {
        // prefix pose j of the coming window: frame T - n_pre + j of the previous one, or the caller's seed pose j
        float* fu = a.feat_u + (size_t)b * T * a.KPP;
        for (int i = tid; i < npre * a.KPP; i += 256) {
            const int j = i / a.KPP, c = i - j * a.KPP;
            float v = c == JF ? 1.f : 0.f;
            if (c < JF) v = a.prev ? tile[(T - npre + j) * ld + c] : a.seed[((size_t)r * JF + c) * npre + j];
            fu[i] = v;
        }
        float* ox = a.origin_x + (size_t)b * JF * T;
        for (int i = tid; i < JF * npre; i += 256) {
            const int c = i / npre, j = i - c * npre;
            ox[(size_t)c * T + j] = a.prev ? tile[(T - npre + j) * ld + c] : a.seed[((size_t)r * JF + c) * npre + j];
        }
    }
    if (!a.prev) return;
    if (a.timeline) {                               // frames f0 .. T-1 of the finished window -> timeline frames t_off ..
        const int nf = T - a.f0;
        float* tl = a.timeline + (size_t)r * JF * a.T_total + a.t_off;
        for (int i = tid; i < JF * nf; i += 256) {
            const int c = i / nf, f = i - c * nf;
            tl[(size_t)c * a.T_total + f] = tile[(a.f0 + f) * ld + c];
        }
    }
    if (a.window) {
        float* wd = a.window + (size_t)r * JF * T;
        for (int i = tid; i < JF * T; i += 256) wd[i] = tile[(i % T) * ld + i / T];
    }
}

hipError_t launch_chain_window(const ChainArgs& a, int B, hipStream_t st) {
    const size_t lds = (size_t)a.T * (a.JF | 1) * sizeof(float);
    if (lds > 64 * 1024 || a.n_pre > a.T || a.f0 < 0 || a.f0 > a.T || a.t_off < 0 || a.t_off + (a.T - a.f0) > a.T_total) return hipErrorInvalidValue;
    if (B < 1 || (a.row && (a.n_next < 0 || a.n_next > B))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_chain_window, dim3(B), dim3(256), lds, st, a);
    return hipGetLastError();
}

// The WavEncoder input of a ragged long-form call: workgroup (x, p) fills 1024 samples of clip-window p = (row, w) of the chunk's table
// from the caller's waveform, zero from the clip's own length on.  Each thread owns four consecutive samples of the destination, shifted
// so that its store is one 16-byte access (clips come from hipMalloc; a clip starts at p * AL floats); the up to three samples ahead of
// the first aligned one and the tail behind the last whole group are scalar.  The load is a float4 too when the source address is
// 16-byte aligned and all four samples are valid, four guarded scalar loads otherwise.  Bytes: reads and writes n * AL floats once.
__global__ __launch_bounds__(256) void k_long_gather_clips(const float* __restrict__ audio, const int* __restrict__ table, const int* __restrict__ lengths,
                                                           float* __restrict__ clips, int AL, long long L, int stride) {
    const int p = blockIdx.y, row = table[2 * p], w = table[2 * p + 1];
    const long long len = lengths[row], lo = (long long)w * stride;      // sample i of the clip-window is sample lo + i of the clip
    const float* src = audio + (size_t)row * (size_t)L + (size_t)lo;
    float* dst = clips + (size_t)p * AL;
    const int to_aligned = (int)((4 - ((size_t)p * AL & 3)) & 3), head = to_aligned < AL ? to_aligned : AL;
    const int nvec = (AL - head) / 4;
    auto at = [&](int i) { return lo + i < len ? src[i] : 0.f; };
    if (blockIdx.x == 0) {                          // scalar head and tail (at most three samples each)
        const int t = threadIdx.x;
        if (t < head) dst[t] = at(t);
        const int tail0 = head + 4 * nvec;
        if (t >= 4 && t < 4 + (AL - tail0)) dst[tail0 + (t - 4)] = at(tail0 + (t - 4));
    }
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nvec) return;
    const int i = head + 4 * g;
    float4 v;
    if (lo + i + 3 < len && ((size_t)(src + i) & 15) == 0) {
        v = *reinterpret_cast<const float4*>(src + i);
    } else {
        v.x = at(i); v.y = at(i + 1); v.z = at(i + 2); v.w = at(i + 3);
    }
    *reinterpret_cast<float4*>(dst + i) = v;
}

hipError_t launch_long_gather_clips(const float* audio, const int* table, const int* lengths, float* clips, int n, int AL, long long L,
                                    int stride, hipStream_t st) {
    if (n < 1 || n > 65535 || AL < 1 || L < 1 || stride < 1 || ((size_t)clips & 15)) return hipErrorInvalidValue;
    const int gx = (AL / 4 + 255) / 256;             // >= the float4 groups of a clip, whatever its head
    hipLaunchKernelGGL(k_long_gather_clips, dim3(gx > 0 ? gx : 1, n), dim3(256), 0, st, audio, table, lengths, clips, AL, L, stride);
    return hipGetLastError();
}

}  // namespace ls
