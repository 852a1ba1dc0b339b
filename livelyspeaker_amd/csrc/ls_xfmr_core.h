// What the three transformer handles share (ls_sag_api.cpp: SAG decoder, ls_sag_enc_api.cpp: SAG encoder, ls_clip_text_api.cpp: CLIP text
// encoder): the head of the handle (XfmrCore), its creation and teardown, the weight maps and the commit that resolves each tower's weight
// table to device pointers once, the post-norm feed-forward tail, the event-timed tail of a call.  SagBase: what only the SAG handles have.
#pragma once
#include <map>

#include "ls_host.h"
#include "ls_internal.h"

namespace ls {

// device pointers of one layer's weights, named by role: each tower's table maps its own state-dict names onto them
struct Layer {
    const float *in_w, *in_b, *out_w, *out_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;      // the attention's packed q / k / v and output projections; the feed-forward
    const float *ln_att_w, *ln_att_b, *ln_ffn_w, *ln_ffn_b, *ln_cross_w, *ln_cross_b;      // the norms of the attention / feed-forward / cross-attention blocks
};

// one row of a tower's per-layer weight table: key suffix, element count n + n_ff * (feed-forward width), slot (null: checked and uploaded only)
struct LayerRow { const char* key; size_t n, n_ff; const float* Layer::*slot; };

struct XfmrCore {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::string, std::vector<float>> w;
    std::map<std::string, DevBuf> dw;      // device copies under the same keys
    std::vector<Layer> layer;              // valid while `committed`
    bool committed = false;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0.f;
    bool pending_ms = false;   // an *_async call is enqueued: last_ms is read from the events when asked for
};

// a new handle on `device` with its stream and the two timing events
template <class Handle>
int xfmr_open(int device, Handle** out, void (*destroy)(Handle*)) {
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail<Handle>(nullptr, LS_EHIP, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    Handle* h = new Handle();
    h->device = device;
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return abandon(h, destroy, fail<Handle>(nullptr, LS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    for (auto& ev : h->ev)
        if (hipEventCreate(&ev) != hipSuccess) return abandon(h, destroy, fail<Handle>(nullptr, LS_EHIP, "hipEventCreate failed"));
    *out = h;
    return LS_OK;
}

// what every *_destroy does: the handle's device becomes current (its DevBufs free on it), the stream drains, events, stream and handle go
template <class Handle>
void xfmr_close(Handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

template <class Handle>
int xfmr_set_weight(Handle* h, const char* who, const char* key, const float* data, size_t n) {
    if (!h || !key || (!data && n)) return fail(h, LS_EINVAL, "%s: null argument", who);
    const std::string k(key);
    if (k.size() >= 3 && k.compare(k.size() - 3, 3, ".pe") == 0) return LS_OK;
    h->w[k].assign(data, data + n);
    h->committed = false;
    return LS_OK;
}

// One *_commit_weights.  need() checks and uploads weight by weight, in the order of the calls (the first missing key is the one
// reported); done() hands every device pointer to its slot once all uploads have succeeded, and only then is the handle committed.
template <class Handle>
struct Commit {
    Handle* h;
    std::vector<std::pair<const float**, const DevBuf*>> slots;
    explicit Commit(Handle* handle) : h(handle) { h->committed = false; }
    // the host weight `key` must hold `want` floats; it goes to the device under the same key
    int need(const std::string& key, size_t want, const float** slot) {
        auto it = h->w.find(key);
        if (it == h->w.end()) return fail(h, LS_ESTATE, "missing weight '%s'", key.c_str());
        if (it->second.size() != want) return fail(h, LS_EINVAL, "weight '%s' has %zu elements, expected %zu", key.c_str(), it->second.size(), want);
        DevBuf& b = h->dw[key];
        HIPCHK(h, b.ensure(want * sizeof(float)));
        HIPCHK(h, hipMemcpy(b.p, it->second.data(), want * sizeof(float), hipMemcpyHostToDevice));
        if (slot) slots.emplace_back(slot, &b);
        return LS_OK;
    }
    // the tower's table, once per layer: the keys are <prefix><layer>.<the row's suffix>
    template <size_t N>
    int layers(const char* prefix, int L, size_t FF, const LayerRow (&rows)[N]) {
        h->layer.assign(L, Layer{});
        char key[160];
        for (int l = 0; l < L; ++l)
            for (const LayerRow& r : rows) {
                snprintf(key, sizeof key, "%s%d.%s", prefix, l, r.key);
                if (const int rc = need(key, r.n + r.n_ff * FF, r.slot ? &(h->layer[l].*r.slot) : nullptr)) return rc;
            }
        return LS_OK;
    }
    int done() {
        for (auto& s : slots) *s.first = s.second->f();
        h->committed = true;
        return LS_OK;
    }
};

// the post-norm feed-forward tail of a layer on `rows` rows: hid = GELU(linear1(x)); t = linear2(hid) + x; y = LN(t)
template <class Handle>
int xfmr_ffn_postnorm(Handle* h, const Layer& w, const float* x, float* hid, float* t, float* y, int rows, int FF) {
    HIPCHK(h, launch_gemm_nt(x, kD, w.fc1_w, kD, w.fc1_b, nullptr, 0, hid, FF, rows, FF, kD, 3, h->stream));
    HIPCHK(h, launch_gemm_nt(hid, FF, w.fc2_w, FF, w.fc2_b, x, kD, t, kD, rows, kD, FF, 0, h->stream));
    HIPCHK(h, launch_layernorm512(t, nullptr, 0, w.ln_ffn_w, w.ln_ffn_b, y, rows, h->stream));
    return LS_OK;
}

// the tail of a decode / encode: close the timed span, copy the result out, then wait and read the span -- or leave that to xfmr_last_ms
// (the caller orders consumers behind the handle's stream: ls_stream_order)
template <class Handle>
int xfmr_finish(Handle* h, void* dst, const void* src, size_t bytes, int on_device, bool wait) {
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (!wait) { h->pending_ms = true; return LS_OK; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
    h->pending_ms = false;
    return LS_OK;
}

inline float xfmr_last_ms(const XfmrCore* h) {
    if (!h) return -1.f;
    if (h->pending_ms) {           // an asynchronous call: its span is read once it has finished (waits for it)
        XfmrCore* m = const_cast<XfmrCore*>(h);
        if (hipEventSynchronize(m->ev[1]) == hipSuccess && hipEventElapsedTime(&m->last_ms, m->ev[0], m->ev[1]) == hipSuccess) m->pending_ms = false;
    }
    return h->last_ms;
}

inline void* xfmr_stream(const XfmrCore* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

// what the two SAG handles add: their configuration and the PositionalEncoding table on the device
struct SagBase : XfmrCore { ls_sag_config cfg{}; int JF = 0; DevBuf pe; };

// the configuration checks both SAG handles make, in front of their own
template <class Handle>
int sag_check_config(const ls_sag_config* cfg, Handle** out, const char* who) {
    if (!cfg || !out) return fail<Handle>(nullptr, LS_EINVAL, "%s: null argument", who);
    *out = nullptr;
    if (cfg->latent_dim != kD) return fail<Handle>(nullptr, LS_EUNSUPPORTED, "latent_dim must be %d", kD);
    if (cfg->nframes != kT) return fail<Handle>(nullptr, LS_EUNSUPPORTED, "nframes must be %d", kT);
    if (cfg->num_heads < 1 || cfg->latent_dim / cfg->num_heads != 128)
        return fail<Handle>(nullptr, LS_EUNSUPPORTED, "head dim must be 128 (latent 512, 4 heads)");
    if (cfg->num_layers < 1 || cfg->ff_size < 1 || cfg->njoints < 1 || cfg->nfeats < 1) return fail<Handle>(nullptr, LS_EINVAL, "bad SAG config");
    return LS_OK;
}

// the SAG handle of a checked configuration: xfmr_open, then PositionalEncoding rows 0 .. pe_rows-1 on the device
template <class Handle>
int sag_open(const ls_sag_config* cfg, Handle** out, int pe_rows, void (*destroy)(Handle*)) {
    Handle* h = nullptr;
    const int rc = xfmr_open(cfg->device, &h, destroy);
    if (rc != LS_OK) return rc;
    h->cfg = *cfg;
    h->JF = cfg->njoints * cfg->nfeats;
    const std::vector<float> pe = pe_table(pe_rows, kD);
    if (h->pe.ensure(pe.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(h->pe.p, pe.data(), pe.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return abandon(h, destroy, fail<Handle>(nullptr, LS_EHIP, "pe upload failed"));
    *out = h;
    return LS_OK;
}

}  // namespace ls
