// Window hand-off of long-form synthesis (ls_long_sample, ls_chain_api.cpp): the model continues a 34-frame clip by conditioning the next
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
// k_edit_gather / k_edit_scatter (further down) are the same cut and stitch for a timeline EDIT (ls_long_edit): a window's frames leave
// the timeline as the loop's inpainting inputs and its editable elements return.  Algorithmic bytes per clip (fp32): gather 15.7 KB TED,
// 163 KB BEAT (with the init plane); scatter at most 11.0 KB TED, 115 KB BEAT (with the raw window); the terms are spelled out at the kernels.
// k_edit_start puts the SAG decoder's output under the editable elements of the init plane (ls_long_edit_sag): at most 7.4 KB TED, 77 KB BEAT.
// The COMPACT edit (ls_long_edit_compact) runs the same three kernels on the rows of a table, one per clip that has an editable element
// in the window, and k_cond_gather moves those clips' held conditioning into the rows.
// An edit by ELEMENT MASK (ls_long_edit_mask and its kin) runs the same three kernels again: "editable" is read from a byte per element of
// the timeline (EditArgs::emask) in place of the clip's rectangle, through the one rule edit_editable; k_edit_mask_pairs reduces a mask
// that lives on the device to one flag per (clip, window), which is all of it the host's plan needs.
// A streaming SESSION (ls_long_pool_push; ls_long_stream_push: the pool whose slots move together) keeps the hand-off per slot:
// k_pool_gather and k_pool_scatter (at the end) move one round's active slots -- a window of audio out of each slot's circular ring,
// its hand-off poses, its held conditioning -- into and out of the compact rows a sampling call at that batch reads.
// PINNED POSES of frames a slot has yet to return (ls_long_pool_pin) live in a ring per slot: k_pool_pin_store / k_pool_pin_clear
// write it, k_pool_pin_gather turns it into the inpainting planes of the rows of a pinned call (at the end).
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

// One window of a timeline edit (ls_long_edit, ls_chain_api.cpp; EditArgs in ls_internal.h): the loop's inpainting inputs are cut out of the
// timeline on the device and its result goes back the same way, so a window costs two launches beside its loop and no host round trip.
// Stream order makes the next window's gather see this window's scatter.  One workgroup per clip, the tile of k_chain_window (row stride
// JF | 1); the timeline, the init plane and the raw window are walked along the frame axis, the internal-layout planes along the channels,
// the seed poses along their n_pre axis (window 0 stages them in n_pre more tile rows).  No atomics: every element has one writer.
// With a row table (EditArgs::rows; the COMPACT edit, ls_long_edit_compact) workgroup r serves clip rows[r]: the timeline, the ranges,
// the channel bytes and the seed poses are the clip's, every compact plane is row r's.  One body for both: a null table is the
// identity, so the dense edit runs the code it always ran, and the rows of a table are distinct clips, so every element keeps one
// writer.  The table costs 4 bytes per row on top of the bytes below, which hold per ROW as they held per clip.
// Algorithmic bytes per clip (fp32), k_edit_gather: read T*JF (+ n_pre*JF seed poses in window 0) + JF channel bytes + 8, write 2*T*JF
// (motion, mask) + n_pre*(KPP + JF) (+ T*JF init plane with skip_timesteps > 0): 15.7 KB TED, 163 KB BEAT with the init plane.
// k_edit_scatter: read T*JF + JF bytes + 8, write the editable elements (at most (T - n_pre)*JF, window 0: T*JF) (+ T*JF raw window): at
// most 11.0 KB TED, 115 KB BEAT.
// "Editable" is DATA: with an element mask (EditArgs::emask, bytes [clips][JF][T_total] in the timeline's own layout; ls_long_edit_mask)
// element (c, f) of window w is editable iff its byte is set and w owns the frame; without one the rule is the rectangle it always was
// (the clip's range times its channel bytes).  One rule for the three kernels below in both of their forms; the mask, like the ranges,
// belongs to the CLIP (rows[r]), not to the row.  A mask costs JF * T byte loads per clip in place of JF + 8 bytes.
struct EditRule { const unsigned char* em; const unsigned char* ch; int lo, hi; };
__device__ __forceinline__ EditRule edit_rule(const EditArgs& a, int b) {
    if (a.emask) return {a.emask + (size_t)b * a.JF * a.T_total + a.w * (a.T - a.n_pre), nullptr, 0, 0};
    return {nullptr, a.chan + (size_t)b * a.JF, a.range[2 * b], a.range[2 * b + 1]};
}
__device__ __forceinline__ bool edit_editable(const EditArgs& a, const EditRule& r, int c, int f) {
    if (a.w != 0 && f < a.n_pre) return false;      // the frame is owned by the window before
    if (r.em) return r.em[(size_t)c * a.T_total + f] != 0;
    const int t = a.w * (a.T - a.n_pre) + f;
    return r.ch[c] != 0 && t >= r.lo && t < r.hi;
}

__global__ __launch_bounds__(256) void k_edit_gather(const EditArgs a) {
    extern __shared__ float tile[];                 // [T (+ n_pre in window 0)][JF | 1]
    const int r = blockIdx.x, tid = threadIdx.x, JF = a.JF, T = a.T, ld = JF | 1, npre = a.n_pre;
    const int b = a.rows ? a.rows[r] : r;           // the clip behind row r (a uniform load; the dense edit: the row itself)
    const float* tl = a.timeline + (size_t)b * JF * a.T_total + a.w * (T - npre);
    float* init = a.init ? a.init + (size_t)r * JF * T : nullptr;
    for (int i = tid; i < JF * T; i += 256) {
        const int c = i / T, f = i - c * T;
        const float v = tl[(size_t)c * a.T_total + f];
        tile[f * ld + c] = v;
        if (init) init[i] = v;
    }
    const float* pre = tile;                        // prefix pose j of channel c: pre[j * ld + c]; the slice's own first frames, or the seed poses
    if (a.w == 0) {
        float* sp = tile + T * ld;
        const float* seed = a.seed + (size_t)b * JF * npre;
        for (int i = tid; i < JF * npre; i += 256) sp[(i % npre) * ld + i / npre] = seed[i];
        pre = sp;
    }
    __syncthreads();
    const EditRule rule = edit_rule(a, b);
    float* mo = a.motion + (size_t)r * T * JF;
    float* mk = a.maskf + (size_t)r * T * JF;
    for (int i = tid; i < T * JF; i += 256) {
        const int f = i / JF, c = i - f * JF;
        mo[i] = tile[f * ld + c];
        mk[i] = edit_editable(a, rule, c, f) ? 0.f : 1.f;      // inpainting_mask: true = keep the given motion
    }
    float* fu = a.feat_u + (size_t)r * T * a.KPP;
    for (int i = tid; i < npre * a.KPP; i += 256) {
        const int j = i / a.KPP, c = i - j * a.KPP;
        fu[i] = c < JF ? pre[j * ld + c] : c == JF ? 1.f : 0.f;
    }
    float* ox = a.origin_x + (size_t)r * JF * T;
    for (int i = tid; i < JF * npre; i += 256) {
        const int c = i / npre, j = i - c * npre;
        ox[(size_t)c * T + j] = pre[j * ld + c];
    }
}

__global__ __launch_bounds__(256) void k_edit_scatter(const EditArgs a) {
    extern __shared__ float tile[];                 // [T][JF | 1]
    const int r = blockIdx.x, tid = threadIdx.x, JF = a.JF, T = a.T, ld = JF | 1;
    const int b = a.rows ? a.rows[r] : r;
    const float* src = a.sample + (size_t)r * T * JF;
    for (int i = tid; i < T * JF; i += 256) tile[(i / JF) * ld + i % JF] = src[i];
    __syncthreads();
    const EditRule rule = edit_rule(a, b);
    float* tl = a.timeline + (size_t)b * JF * a.T_total + a.w * (T - a.n_pre);
    float* wd = a.window ? a.window + (size_t)r * JF * T : nullptr;
    for (int i = tid; i < JF * T; i += 256) {
        const int c = i / T, f = i - c * T;
        const float v = tile[f * ld + c];
        if (wd) wd[i] = v;
        if (edit_editable(a, rule, c, f)) tl[(size_t)c * a.T_total + f] = v;
    }
}

// The start of a SCRIPTED edit window (ls_long_edit_sag): init = where(keep, slice, decoder output).  k_edit_gather has left the slice
// in init; this stores sag_out over it exactly on the editable elements, so a kept element is never touched.  Both planes are in the
// reference layout [B][JF][T]: no tile, the frame axis innermost in both, one writer per element, no atomics.
// Algorithmic bytes per clip (fp32): read and write the editable elements (at most (T - n_pre)*JF each, window 0: T*JF) + JF channel
// bytes + 8: at most 7.4 KB TED, 77 KB BEAT.
__global__ __launch_bounds__(256) void k_edit_start(const EditArgs a, const float* __restrict__ sag_out) {
    const int r = blockIdx.x, tid = threadIdx.x, JF = a.JF, T = a.T;
    const int b = a.rows ? a.rows[r] : r;
    const EditRule rule = edit_rule(a, b);
    const float* src = sag_out + (size_t)r * JF * T;
    float* init = a.init + (size_t)r * JF * T;
    for (int i = tid; i < JF * T; i += 256) {
        const int c = i / T, f = i - c * T;
        if (edit_editable(a, rule, c, f)) init[i] = src[i];
    }
}

static bool edit_args_ok(const EditArgs& a, int B, int rows) {
    const size_t lds = (size_t)rows * (a.JF | 1) * sizeof(float);
    return B >= 1 && lds <= 64 * 1024 && a.n_pre >= 1 && a.n_pre <= a.T && a.w >= 0 && (long long)a.w * (a.T - a.n_pre) + a.T <= a.T_total &&
           a.timeline && (a.emask || (a.range && a.chan));
}
hipError_t launch_edit_gather(const EditArgs& a, int B, hipStream_t st) {
    const int rows = a.T + (a.w == 0 ? a.n_pre : 0);
    if (!edit_args_ok(a, B, rows) || a.KPP <= a.JF || !a.motion || !a.maskf || !a.feat_u || !a.origin_x || (a.w == 0 && !a.seed)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_edit_gather, dim3(B), dim3(256), (size_t)rows * (a.JF | 1) * sizeof(float), st, a);
    return hipGetLastError();
}
hipError_t launch_edit_start(const EditArgs& a, const float* sag_out, int B, hipStream_t st) {
    if (!edit_args_ok(a, B, 0) || a.JF < 1 || a.T < 1 || !a.init || !sag_out || sag_out == a.init) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_edit_start, dim3(B), dim3(256), 0, st, a, sag_out);
    return hipGetLastError();
}
hipError_t launch_edit_scatter(const EditArgs& a, int B, hipStream_t st) {
    if (!edit_args_ok(a, B, a.T) || !a.sample) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_edit_scatter, dim3(B), dim3(256), (size_t)a.T * (a.JF | 1) * sizeof(float), st, a);
    return hipGetLastError();
}

// The pair flags of an element mask that lives on the device (ls_long_edit_mask and its kin): flags[w][b] = 1 iff clip b has a set byte
// on a frame window w OWNS ([0, T) for w = 0, [w S + n_pre, w S + T) otherwise), any of the JF channels.  With frames [B] (a ragged
// batch) clip b has the windows w < W_b = (frames[b] - T) / S + 1 only; a set byte on a frame a later window owns is the caller's
// error and is reported as 2, never dropped.  Only these W * B bytes cross to the host; the plan is made from them there
// (edit_plan_of_flags, ls_chain_plan.cpp).  One workgroup per (clip, window): thread i walks the owned frames of a channel, so a wave
// reads consecutive bytes along N; the OR goes through one ballot per wave and four LDS words, one thread stores the byte.  Reads
// JF * (T - n_pre) bytes per pair (window 0: JF * T), writes one; not measured.
__global__ __launch_bounds__(256) void k_edit_mask_pairs(const unsigned char* __restrict__ mask, const int* __restrict__ frames,
                                                         unsigned char* __restrict__ flags, int B, int JF, int T, int n_pre, int T_total) {
    __shared__ int any_wave[4];
    const int b = blockIdx.x, w = blockIdx.y, tid = threadIdx.x, S = T - n_pre;
    const int f0 = w ? n_pre : 0, nf = T - f0;
    const unsigned char* m = mask + (size_t)b * JF * T_total + w * S + f0;
    int any = 0;
    for (int i = tid; i < JF * nf; i += 256) {
        const int c = i / nf, f = i - c * nf;
        any |= m[(size_t)c * T_total + f];
    }
    const unsigned long long vote = __ballot(any != 0);
    if ((tid & 63) == 0) any_wave[tid >> 6] = vote != 0ull;
    __syncthreads();
    if (tid == 0) {
        const bool set = (any_wave[0] | any_wave[1] | any_wave[2] | any_wave[3]) != 0;
        const bool has = !frames || w < (frames[b] - T) / S + 1;
        flags[(size_t)w * B + b] = set ? (has ? 1 : 2) : 0;
    }
}
hipError_t launch_edit_mask_pairs(const unsigned char* mask, const int* frames, unsigned char* flags, int B, int W, int JF, int T, int n_pre, hipStream_t st) {
    if (!mask || !flags || B < 1 || W < 1 || W > 65535 || JF < 1 || n_pre < 1 || T <= n_pre) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_edit_mask_pairs, dim3(B, W), dim3(256), 0, st, mask, frames, flags, B, JF, T, n_pre, T + (W - 1) * (T - n_pre));
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

// The WavEncoder input of one window of a streaming SESSION's slot: its audio_len samples from the slot's circular ring [R] (sample s
// of the slot sits at s % R; the window's first sample at pos0 = (w * stride) % R), zero from the slot's last sample on (n_valid
// samples of the window exist; fewer than AL only in the closing call).  AL <= R, so a window wraps at most once.  The destination
// layout, the float4 store per thread and the scalar head and tail are k_long_gather_clips'; the load is a float4 when all four samples
// exist, the ring position is a multiple of four (R is one, and a slot's ring starts 16-byte aligned) and the group does not cross the
// ring's end, four guarded scalar loads otherwise.  Bytes: reads at most and writes exactly AL floats per row.
// Workgroup x of the row whose source ring is src and whose destination is clips row `row` at dst (k_pool_gather)
__device__ __forceinline__ void gather_ring_window(const float* __restrict__ src, float* __restrict__ dst, int row, int AL, int R, int pos0, int n_valid) {
    const int to_aligned = (int)((4 - ((size_t)row * AL & 3)) & 3), head = to_aligned < AL ? to_aligned : AL;
    const int nvec = (AL - head) / 4;
    auto pos = [&](int i) { const int q = pos0 + i; return q >= R ? q - R : q; };      // pos0 < R and i < AL <= R: one wrap at most
    auto at = [&](int i) { return i < n_valid ? src[pos(i)] : 0.f; };
    if (blockIdx.x == 0) {                          // scalar head and tail (at most three samples each)
        const int t = threadIdx.x;
        if (t < head) dst[t] = at(t);
        const int tail0 = head + 4 * nvec;
        if (t >= 4 && t < 4 + (AL - tail0)) dst[tail0 + (t - 4)] = at(tail0 + (t - 4));
    }
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= nvec) return;
    const int i = head + 4 * g, q = pos(i);
    float4 v;
    if (i + 3 < n_valid && (q & 3) == 0 && q + 3 < R) {
        v = *reinterpret_cast<const float4*>(src + q);
    } else {
        v.x = at(i); v.y = at(i + 1); v.z = at(i + 2); v.w = at(i + 3);
    }
    *reinterpret_cast<float4*>(dst + i) = v;
}

// The held conditioning of source row `from` (a session's slot, a compact edit's clip) into compact row r: speaker id and guidance
// scale by thread 0, the emotion token and the text features as float4 by 128 threads each (512-float rows: every row starts
// 2 KB-aligned).  emo_tok / text null: that row is not moved.  256 threads.
__device__ __forceinline__ void gather_cond_row(int r, int from, const int64_t* __restrict__ vid_s, const float* __restrict__ scale_s,
                                                const float* __restrict__ emo_tok_s, const float* __restrict__ text_s, int64_t* __restrict__ vid,
                                                float* __restrict__ scale, float* __restrict__ emo_tok, float* __restrict__ text) {
    const int tid = threadIdx.x;
    if (tid == 0) { vid[r] = vid_s[from]; scale[r] = scale_s[from]; }
    if (emo_tok && tid < kD / 4)
        reinterpret_cast<float4*>(emo_tok + (size_t)r * kD)[tid] = reinterpret_cast<const float4*>(emo_tok_s + (size_t)from * kD)[tid];
    if (text && tid >= 128 && tid < 128 + kD / 4)
        reinterpret_cast<float4*>(text + (size_t)r * kD)[tid - 128] = reinterpret_cast<const float4*>(text_s + (size_t)from * kD)[tid - 128];
}

// One round of a streaming SESSION (ls_long_pool_push, ls_long_stream_push; PoolArgs in ls_internal.h): the A active slots of the round,
// in ascending slot order, become the rows 0 .. A-1 of every buffer a sampling call at batch A reads.  Workgroup (x, r) reads its table
// row once (a uniform load; no other load depends on a loaded value) and, for x below the audio workgroups, is gather_ring_window on
// slot table[r][0]'s ring at that slot's own position and valid count.  The one workgroup behind them (x == gridDim.x - 1) moves the slot's conditioning: its
// hand-off poses into the prefix rows of feat_u ([poses | 1 | 0 pad]) and the prefix columns of origin_x -- what k_chain_window
// writes for a next window; everything outside the prefix is zero from ls_long_pool_open on -- and its speaker id, guidance scale,
// emotion token and text features into compact row r (512-float rows as float4: every row starts 2 KB-aligned).
// Bytes per row (fp32): reads at most and writes AL samples; reads JF*n_pre poses, writes n_pre*(KPP + JF); 12 + 2 * 2 KB conditioning.
__global__ __launch_bounds__(256) void k_pool_gather(const PoolArgs a) {
    const int r = blockIdx.y, tid = threadIdx.x;
    const int* row = a.table + (size_t)r * kPoolRow;
    const int slot = row[0];
    if (blockIdx.x + 1 < gridDim.x) {
        gather_ring_window(a.ring + (size_t)slot * a.R, a.clips + (size_t)r * a.AL, r, a.AL, a.R, row[1], row[2]);
        return;
    }
    const int JF = a.JF, T = a.T, npre = a.n_pre;
    const float* hand = a.hand + (size_t)slot * JF * npre;          // [JF][n_pre]
    float* fu = a.feat_u + (size_t)r * T * a.KPP;
    for (int i = tid; i < npre * a.KPP; i += 256) {
        const int j = i / a.KPP, c = i - j * a.KPP;
        fu[i] = c < JF ? hand[c * npre + j] : c == JF ? 1.f : 0.f;
    }
    float* ox = a.origin_x + (size_t)r * JF * T;
    for (int i = tid; i < JF * npre; i += 256) {
        const int c = i / npre, j = i - c * npre;
        ox[(size_t)c * T + j] = hand[i];
    }
    gather_cond_row(r, slot, a.vid_s, a.scale_s, a.emo_tok_s, a.text_s, a.vid, a.scale, a.emo_tok, a.text);
}

// One window of a COMPACT timeline edit (ls_long_edit_compact): the held conditioning of clip rows[r] into compact row r, one
// workgroup per row -- gather_cond_row with clips in place of slots.  Bytes per row: 4 (table) + 12 + 2 KB per 512-float row moved.
__global__ __launch_bounds__(256) void k_cond_gather(const CondGatherArgs a) {
    const int r = blockIdx.x;
    gather_cond_row(r, a.rows[r], a.vid_c, a.scale_c, a.emo_tok_c, a.text_c, a.vid, a.scale, a.emo_tok, a.text);
}

// ... and the way back: one workgroup per row, k_chain_window's tile (row stride JF | 1: the transposed reads touch every bank once).
// Row r's frames f0 .. T-1 go to frames[slot] at the slot's own frame offset in this call (stores along the frame axis), its last n_pre
// poses into the slot's hand-off store, where the gather of the slot's next window -- in this call or a later one -- finds them.
// Bytes per row (fp32): reads T*JF, writes (T - f0)*JF + n_pre*JF.
__global__ __launch_bounds__(256) void k_pool_scatter(const PoolArgs a) {
    extern __shared__ float tile[];                 // [T][JF | 1]
    const int r = blockIdx.x, tid = threadIdx.x, JF = a.JF, T = a.T, ld = JF | 1, npre = a.n_pre;
    const int* row = a.table + (size_t)r * kPoolRow;
    const int slot = row[0], f0 = row[3], t_off = row[4];
    const float* src = a.prev + (size_t)r * T * JF;
    for (int i = tid; i < T * JF; i += 256) tile[(i / JF) * ld + i % JF] = src[i];
    __syncthreads();
    const int nf = T - f0;
    float* fr = a.frames + (size_t)slot * JF * a.T_total + t_off;
    for (int i = tid; i < JF * nf; i += 256) {
        const int c = i / nf, f = i - c * nf;
        fr[(size_t)c * a.T_total + f] = tile[(f0 + f) * ld + c];
    }
    float* hand = a.hand + (size_t)slot * JF * npre;
    for (int i = tid; i < JF * npre; i += 256) {
        const int c = i / npre, j = i - c * npre;
        hand[i] = tile[(T - npre + j) * ld + c];
    }
}

static bool pool_args_ok(const PoolArgs& a, int A) {
    return A >= 1 && A <= a.S && a.S <= 65535 && a.table && a.hand && a.JF >= 1 && a.T >= 1 && a.n_pre >= 1 && a.n_pre <= a.T;
}
hipError_t launch_pool_gather(const PoolArgs& a, int A, hipStream_t st) {
    if (!pool_args_ok(a, A) || a.AL < 1 || a.R < a.AL || (a.R & 3) || a.KPP <= a.JF) return hipErrorInvalidValue;
    if (!a.ring || !a.clips || !a.feat_u || !a.origin_x || !a.vid_s || !a.scale_s || !a.vid || !a.scale) return hipErrorInvalidValue;
    if (((size_t)a.clips & 15) || ((size_t)a.ring & 15) || (a.emo_tok && (!a.emo_tok_s || (((size_t)a.emo_tok | (size_t)a.emo_tok_s) & 15))) ||
        (a.text && (!a.text_s || (((size_t)a.text | (size_t)a.text_s) & 15)))) return hipErrorInvalidValue;
    const int gx = (a.AL / 4 + 255) / 256;           // >= the float4 groups of a clip, whatever its head
    hipLaunchKernelGGL(k_pool_gather, dim3((gx > 0 ? gx : 1) + 1, A), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_cond_gather(const CondGatherArgs& a, int A, hipStream_t st) {
    if (A < 1 || A > 65535 || !a.rows || !a.vid_c || !a.scale_c || !a.vid || !a.scale) return hipErrorInvalidValue;
    if ((a.emo_tok && (!a.emo_tok_c || (((size_t)a.emo_tok | (size_t)a.emo_tok_c) & 15))) ||
        (a.text && (!a.text_c || (((size_t)a.text | (size_t)a.text_c) & 15)))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_cond_gather, dim3(A), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_pool_scatter(const PoolArgs& a, int A, hipStream_t st) {
    const size_t lds = (size_t)a.T * (a.JF | 1) * sizeof(float);
    if (!pool_args_ok(a, A) || lds > 64 * 1024 || !a.prev || !a.frames || a.T_total < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_scatter, dim3(A), dim3(256), lds, st, a);
    return hipGetLastError();
}

// Pinned poses of a session's slots (ls_long_pool_pin; PinArgs in ls_internal.h): a ring of P series frames per slot, frame n at
// n % P, values and one byte per element, both [S][P][JF] -- JF innermost, so the store's writes and both sides of the gather run
// along the channels, as the internal-layout planes [A][T][JF] do.
// k_pool_pin_store: one workgroup per frame k of the call.  The caller's [J, F, K] layout is transposed on the way in: the reads of
// poses / mask walk a column (stride K), the writes a row of the ring.  An element the mask leaves out is not touched.
// Algorithmic bytes per frame (fp32, whole pose): reads 4 + 4 JF (+ JF mask bytes), writes 5 JF: 0.25 KB TED, 2.5 KB BEAT; not measured.
__global__ __launch_bounds__(256) void k_pool_pin_store(const PinArgs a) {
    const int k = blockIdx.x, JF = a.JF, K = a.K;
    const size_t at = ((size_t)a.slot * a.P + a.pos[k]) * JF;
    for (int c = threadIdx.x; c < JF; c += 256) {
        if (a.mask && !a.mask[(size_t)c * K + k]) continue;
        a.val[at + c] = a.poses[(size_t)c * K + k];
        a.bit[at + c] = 1;
    }
}
// The un-pin: the bytes of the K frames at pos (null: of frames 0 .. K-1 = the whole ring of the slot) become 0; the values stay, no
// byte names them.  Writes JF bytes per frame; not measured.
__global__ __launch_bounds__(256) void k_pool_pin_clear(const PinArgs a) {
    const int k = blockIdx.x, JF = a.JF;
    const size_t at = ((size_t)a.slot * a.P + (a.pos ? a.pos[k] : k)) * JF;
    for (int c = threadIdx.x; c < JF; c += 256) a.bit[at + c] = 0;
}
// One workgroup per row of a pinned call.  It reads its table row once (slot, f0 and the ring position of the window's frame 0: uniform
// loads, nothing else depends on a loaded value but the byte that selects), and writes the row's motion and maskf planes: for the
// frames f0 .. T-1 the window owns, the pinned value and 1 where the ring's byte is set, 0 and 0 elsewhere -- the prefix frames of a
// window w > 0 are never kept.  A byte it found set is cleared, so the position is free for frame n + P.  T <= P: the window's frames
// wrap at most once and sit at distinct positions, the rows of a call are distinct slots, so every element has one writer; no atomics.
// Algorithmic bytes per row (fp32): reads 32 (table) + (T - f0) JF bytes + 4 per pinned element, writes 2 * 4 T JF (the planes) + 1
// per pinned element: at most 8.3 KB TED, 86 KB BEAT; not measured.
__global__ __launch_bounds__(256) void k_pool_pin_gather(const PinArgs a) {
    const int r = blockIdx.x, JF = a.JF, T = a.T, P = a.P;
    const int* row = a.table + (size_t)r * kPoolRow;
    const int slot = row[0], f0 = row[3], p0 = row[5];
    float* mo = a.motion + (size_t)r * T * JF;
    float* mk = a.maskf + (size_t)r * T * JF;
    const size_t base = (size_t)slot * P;
    for (int i = threadIdx.x; i < T * JF; i += 256) {
        const int f = i / JF, c = i - f * JF;
        float v = 0.f, m = 0.f;
        if (f >= f0) {
            const int p = p0 + f >= P ? p0 + f - P : p0 + f;
            const size_t at = (base + p) * JF + c;
            if (a.bit[at]) { v = a.val[at]; m = 1.f; a.bit[at] = 0; }
        }
        mo[i] = v;
        mk[i] = m;                                      // inpainting_mask: true = keep the given motion
    }
}

static bool pin_args_ok(const PinArgs& a) {
    return a.val && a.bit && a.S >= 1 && a.S <= 65535 && a.JF >= 1 && a.T >= 1 && a.P >= a.T && (a.P & 3) == 0;
}
hipError_t launch_pool_pin_store(const PinArgs& a, hipStream_t st) {
    if (!pin_args_ok(a) || a.slot < 0 || a.slot >= a.S || a.K < 1 || a.K > a.P || !a.poses || !a.pos) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_pin_store, dim3(a.K), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_pool_pin_clear(const PinArgs& a, hipStream_t st) {
    if (!pin_args_ok(a) || a.slot < 0 || a.slot >= a.S || a.K < 1 || a.K > a.P || (!a.pos && a.K != a.P)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_pin_clear, dim3(a.K), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_pool_pin_gather(const PinArgs& a, int A, hipStream_t st) {
    if (!pin_args_ok(a) || A < 1 || A > a.S || !a.table || !a.motion || !a.maskf) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_pool_pin_gather, dim3(A), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace ls
