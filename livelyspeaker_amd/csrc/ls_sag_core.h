// What the two SAG handles share (ls_sag_api.cpp: decoder, ls_sag_enc_api.cpp: encoder): the head of the handle, its creation and
// teardown, the host / device weight maps and the event-timed tail of a call.  Handle is ls_sag or ls_sag_enc, both derived from SagCore.
#pragma once
#include <map>

#include "ls_host.h"
#include "ls_internal.h"

namespace ls {

struct SagCore {
    ls_sag_config cfg{};
    int JF = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::string, std::vector<float>> w;
    std::map<std::string, DevBuf> dw;      // device copies under the same keys
    bool committed = false;
    DevBuf pe;
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0.f;
    bool pending_ms = false;   // an *_async call is enqueued: last_ms is read from the events when asked for
};

// the configuration checks both handles make, in front of their own
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

// the handle of a checked configuration: stream, the two timing events and PositionalEncoding rows 0 .. pe_rows-1 on the device
template <class Handle>
int sag_open(const ls_sag_config* cfg, Handle** out, int pe_rows, void (*destroy)(Handle*)) {
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail<Handle>(nullptr, LS_EHIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));
    Handle* h = new Handle();
    h->cfg = *cfg;
    h->JF = cfg->njoints * cfg->nfeats;
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) return abandon(h, destroy, fail<Handle>(nullptr, LS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)));
    for (auto& ev : h->ev)
        if (hipEventCreate(&ev) != hipSuccess) return abandon(h, destroy, fail<Handle>(nullptr, LS_EHIP, "hipEventCreate failed"));
    const std::vector<float> pe = pe_table(pe_rows, kD);
    if (h->pe.ensure(pe.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(h->pe.p, pe.data(), pe.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
        return abandon(h, destroy, fail<Handle>(nullptr, LS_EHIP, "pe upload failed"));
    *out = h;
    return LS_OK;
}

// the handle's device becomes current (its DevBufs free on it), the stream drains, events and stream go; the caller deletes the handle
inline void sag_close(SagCore* h) {
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

template <class Handle>
int sag_set_weight(Handle* h, const char* who, const char* key, const float* data, size_t n) {
    if (!h || !key || (!data && n)) return fail(h, LS_EINVAL, "%s: null argument", who);
    const std::string k(key);
    if (k.size() >= 3 && k.compare(k.size() - 3, 3, ".pe") == 0) return LS_OK;
    h->w[k].assign(data, data + n);
    h->committed = false;
    return LS_OK;
}

// one step of *_commit_weights: the host weight `key` must hold `want` floats; it goes to the device under the same key
template <class Handle>
int sag_need(Handle* h, const std::string& key, size_t want) {
    auto it = h->w.find(key);
    if (it == h->w.end()) return fail(h, LS_ESTATE, "missing weight '%s'", key.c_str());
    if (it->second.size() != want) return fail(h, LS_EINVAL, "weight '%s' has %zu elements, expected %zu", key.c_str(), it->second.size(), want);
    DevBuf& b = h->dw[key];
    HIPCHK(h, b.ensure(want * sizeof(float)));
    HIPCHK(h, hipMemcpy(b.p, it->second.data(), want * sizeof(float), hipMemcpyHostToDevice));
    return LS_OK;
}

// the tail of a decode / encode: close the timed span, copy the result out, then wait and read the span -- or leave that to sag_last_ms
// (the caller orders consumers behind the handle's stream: ls_stream_order)
template <class Handle>
int sag_finish(Handle* h, void* dst, const void* src, size_t bytes, int on_device, bool wait) {
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    if (!wait) { h->pending_ms = true; return LS_OK; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
    h->pending_ms = false;
    return LS_OK;
}

inline float sag_last_ms(const SagCore* h) {
    if (!h) return -1.f;
    if (h->pending_ms) {           // an asynchronous call: its span is read once it has finished (waits for it)
        SagCore* m = const_cast<SagCore*>(h);
        if (hipEventSynchronize(m->ev[1]) == hipSuccess && hipEventElapsedTime(&m->last_ms, m->ev[0], m->ev[1]) == hipSuccess) m->pending_ms = false;
    }
    return h->last_ms;
}

inline void* sag_stream(const SagCore* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

}  // namespace ls
