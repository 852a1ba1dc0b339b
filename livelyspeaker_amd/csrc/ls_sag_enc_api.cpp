// C-ABI of the SAG encoder (include/ls_hip.h, "ls_sag_enc_*"): replaces SAG.encoder(batch) = Encoder_TRANSFORMER.forward
// (scripts/model/motionclip_module.py:70-95), the first half of MOTIONCLIP.forward (scripts/model/motionclip.py:75-83).
#include "ls_hip.h"
#include "ls_internal.h"
#include "ls_sag_host.h"
#include "ls_train.h"      // GemmArgs / op_rows / launch_gemm_tr: the skelEmbedding product needs the two-level output rows launch_gemm_nt does not expose

#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace ls;

namespace {
std::string g_enc_create_error;
constexpr int kS = kSagEncS;
}  // namespace

struct ls_sag_enc {
    ls_sag_config cfg{};
    int JF = 0, KP = 0;        // KP: skelEmbedding's fan-in rounded up to the GEMM's K tile kGemmTileK (27 -> 32, 282 -> 288)
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::string, std::vector<float>> w;
    std::map<std::string, DeviceBuf> dw;      // device copies under the same keys
    bool committed = false;
    DeviceBuf pe, wemb, xin, maskin, kmask, xt, tok, qkv, attn, t1, x2, hid, t3;
    DeviceBuf x0, q0, a0, t1c, x2c, hidc, t3c, mu;      // the last layer's token-0 rows, [B][...]
    hipEvent_t ev[2] = {nullptr, nullptr};
    float last_ms = 0.f;
    bool pending_ms = false;   // ls_sag_enc_encode_async enqueued: last_ms is read from the events when asked for
};

namespace {
int efail(ls_sag_enc* h, int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    const int rc = sag_fail(h, g_enc_create_error, code, fmt, ap);
    va_end(ap);
    return rc;
}
#define ECHK(h, expr) LS_SAG_CHK(efail, h, expr)
}  // namespace

extern "C" {

const char* ls_sag_enc_last_error(const ls_sag_enc* h) { return h ? h->err.c_str() : g_enc_create_error.c_str(); }

int ls_sag_enc_create(const ls_sag_config* cfg, ls_sag_enc** out) {
    if (!cfg || !out) return efail(nullptr, LS_EINVAL, "ls_sag_enc_create: null argument");
    *out = nullptr;
    if (cfg->latent_dim != kD) return efail(nullptr, LS_EUNSUPPORTED, "latent_dim must be %d", kD);
    if (cfg->nframes != kT) return efail(nullptr, LS_EUNSUPPORTED, "nframes must be %d", kT);
    if (cfg->num_heads < 1 || cfg->latent_dim / cfg->num_heads != 128)
        return efail(nullptr, LS_EUNSUPPORTED, "head dim must be 128 (latent 512, 4 heads)");
    if (cfg->num_layers < 1 || cfg->ff_size < 1 || cfg->njoints < 1 || cfg->nfeats < 1) return efail(nullptr, LS_EINVAL, "bad SAG config");
    if ((size_t)cfg->njoints * cfg->nfeats * (kT + 1) * sizeof(float) > 64 * 1024)
        return efail(nullptr, LS_EUNSUPPORTED, "njoints * nfeats = %d is too wide for the token builder", cfg->njoints * cfg->nfeats);
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return efail(nullptr, LS_EHIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));
    ls_sag_enc* h = new ls_sag_enc();
    h->cfg = *cfg;
    h->JF = cfg->njoints * cfg->nfeats;
    h->KP = (h->JF + kGemmTileK - 1) / kGemmTileK * kGemmTileK;
    e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return efail(nullptr, LS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    for (auto& ev : h->ev)
        if (hipEventCreate(&ev) != hipSuccess) { ls_sag_enc_destroy(h); return efail(nullptr, LS_EHIP, "hipEventCreate failed"); }
    // PositionalEncoding rows 0..35 (motionclip_module.py:12-29), fp32 like the torch buffer: the same table as ls_sag_create's, two rows longer
    std::vector<float> pe((size_t)kS * kD);
    const float cexp = (float)(-std::log(10000.0) / kD);
    for (int i = 0; i < kD / 2; ++i) {
        const float div = expf((float)(2 * i) * cexp);
        for (int p = 0; p < kS; ++p) {
            pe[(size_t)p * kD + 2 * i] = sinf((float)p * div);
            pe[(size_t)p * kD + 2 * i + 1] = cosf((float)p * div);
        }
    }
    if (h->pe.ensure(pe.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(h->pe.p, pe.data(), pe.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        ls_sag_enc_destroy(h);
        return efail(nullptr, LS_EHIP, "pe upload failed");
    }
    *out = h;
    return LS_OK;
}

void ls_sag_enc_destroy(ls_sag_enc* h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (auto& kv : h->dw) kv.second.release();
    DeviceBuf* all[] = {&h->pe, &h->wemb, &h->xin, &h->maskin, &h->kmask, &h->xt, &h->tok, &h->qkv, &h->attn, &h->t1, &h->x2, &h->hid, &h->t3,
                  &h->x0, &h->q0, &h->a0, &h->t1c, &h->x2c, &h->hidc, &h->t3c, &h->mu};
    for (DeviceBuf* b : all) b->release();
    for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int ls_sag_enc_set_weight(ls_sag_enc* h, const char* key, const float* data, size_t n) {
    if (!h || !key || (!data && n)) return efail(h, LS_EINVAL, "ls_sag_enc_set_weight: null argument");
    const std::string k(key);
    if (k.size() >= 3 && k.compare(k.size() - 3, 3, ".pe") == 0) return LS_OK;
    h->w[k].assign(data, data + n);
    h->committed = false;
    return LS_OK;
}

int ls_sag_enc_commit_weights(ls_sag_enc* h) {
    if (!h) return LS_EINVAL;
    ECHK(h, hipSetDevice(h->cfg.device));
    h->committed = false;
    const int D = kD, FF = h->cfg.ff_size, JF = h->JF, KP = h->KP;
    auto need = [&](const std::string& key, size_t want) -> int {
        auto it = h->w.find(key);
        if (it == h->w.end()) return efail(h, LS_ESTATE, "missing weight '%s'", key.c_str());
        if (it->second.size() != want) return efail(h, LS_EINVAL, "weight '%s' has %zu elements, expected %zu", key.c_str(), it->second.size(), want);
        DeviceBuf& b = h->dw[key];
        ECHK(h, b.ensure(want * sizeof(float)));
        ECHK(h, hipMemcpy(b.p, it->second.data(), want * sizeof(float), hipMemcpyHostToDevice));
        return LS_OK;
    };
    int rc;
    char key[160];
    if ((rc = need("muQuery", D)) != LS_OK) return rc;                               // :56-58
    if ((rc = need("sigmaQuery", D)) != LS_OK) return rc;
    if ((rc = need("skelEmbedding.weight", (size_t)D * JF)) != LS_OK) return rc;
    if ((rc = need("skelEmbedding.bias", D)) != LS_OK) return rc;
    for (int l = 0; l < h->cfg.num_layers; ++l) {       // nn.TransformerEncoderLayer parameters (:62-68)
        struct { const char* s; size_t n; } items[] = {
            {"self_attn.in_proj_weight", (size_t)3 * D * D}, {"self_attn.in_proj_bias", (size_t)3 * D},
            {"self_attn.out_proj.weight", (size_t)D * D}, {"self_attn.out_proj.bias", (size_t)D},
            {"linear1.weight", (size_t)FF * D}, {"linear1.bias", (size_t)FF}, {"linear2.weight", (size_t)D * FF}, {"linear2.bias", (size_t)D},
            {"norm1.weight", (size_t)D}, {"norm1.bias", (size_t)D}, {"norm2.weight", (size_t)D}, {"norm2.bias", (size_t)D}};
        for (auto& it : items) {
            snprintf(key, sizeof key, "seqTransEncoder.layers.%d.%s", l, it.s);
            if ((rc = need(key, it.n)) != LS_OK) return rc;
        }
    }
    {   // skelEmbedding's weight with its rows zero-padded to KP columns: the operand xt is padded alike (k_sag_enc_prepare)
        const std::vector<float>& wsrc = h->w["skelEmbedding.weight"];
        std::vector<float> wp((size_t)D * KP, 0.f);
        for (int d = 0; d < D; ++d) std::memcpy(&wp[(size_t)d * KP], &wsrc[(size_t)d * JF], (size_t)JF * sizeof(float));
        ECHK(h, h->wemb.ensure(wp.size() * sizeof(float)));
        ECHK(h, hipMemcpy(h->wemb.p, wp.data(), wp.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    h->committed = true;
    return LS_OK;
}

static int sag_enc_encode_impl(ls_sag_enc* h, int batch, int on_device, const float* x, const unsigned char* mask, float* mu_out, bool wait) {
    if (!h || !x || !mu_out) return efail(h, LS_EINVAL, "ls_sag_enc_encode: null argument");
    if (!h->committed) return efail(h, LS_ESTATE, "ls_sag_enc_encode before ls_sag_enc_commit_weights");
    if (batch < 1) return efail(h, LS_EINVAL, "batch must be >= 1");
    if ((long long)batch * kS * (3 * kD > h->cfg.ff_size ? 3 * kD : h->cfg.ff_size) >= (1ll << 31))      // row * width stays an int
        return efail(h, LS_EINVAL, "batch %d is too large for one encode", batch);
    ECHK(h, hipSetDevice(h->cfg.device));
    const int B = batch, D = kD, FF = h->cfg.ff_size, JF = h->JF, KP = h->KP, M = B * kS, H = h->cfg.num_heads, L = h->cfg.num_layers;
    hipStream_t st = h->stream;
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t nx = (size_t)B * JF * kT * sizeof(float), nm = (size_t)M * D * sizeof(float), nb = (size_t)B * D * sizeof(float);
    ECHK(h, h->xin.ensure(nx)); ECHK(h, h->kmask.ensure((size_t)M)); ECHK(h, h->xt.ensure((size_t)B * kT * KP * sizeof(float)));
    ECHK(h, h->tok.ensure(nm)); ECHK(h, h->qkv.ensure(3 * nm)); ECHK(h, h->attn.ensure(nm)); ECHK(h, h->t1.ensure(nm));
    ECHK(h, h->x2.ensure(nm)); ECHK(h, h->t3.ensure(nm)); ECHK(h, h->hid.ensure((size_t)M * FF * sizeof(float)));
    ECHK(h, h->x0.ensure(nb)); ECHK(h, h->q0.ensure(nb)); ECHK(h, h->a0.ensure(nb)); ECHK(h, h->t1c.ensure(nb)); ECHK(h, h->x2c.ensure(nb));
    ECHK(h, h->t3c.ensure(nb)); ECHK(h, h->mu.ensure(nb)); ECHK(h, h->hidc.ensure((size_t)B * FF * sizeof(float)));
    ECHK(h, hipMemcpyAsync(h->xin.p, x, nx, in, st));
    const unsigned char* dmask = nullptr;
    if (mask) {
        ECHK(h, h->maskin.ensure((size_t)B * kT));
        ECHK(h, hipMemcpyAsync(h->maskin.p, mask, (size_t)B * kT, in, st));
        dmask = static_cast<const unsigned char*>(h->maskin.p);
    }
    auto W = [&](const std::string& k) { return h->dw[k].f(); };
    unsigned char* kmask = static_cast<unsigned char*>(h->kmask.p);
    ECHK(h, hipEventRecord(h->ev[0], st));
    // tokens: the two learned queries and pe are written by the staging kernel; skelEmbedding(frames) + bias is added onto rows 2.. of
    // every sample by one GEMM whose output rows skip the two query rows (two-level row index: 34 rows per 36-row sample)
    ECHK(h, launch_sag_enc_prepare(h->xin.f(), dmask, W("muQuery"), W("sigmaQuery"), h->pe.f(), h->tok.f(), h->xt.f(), kmask, B, JF, KP, st));
    {
        GemmArgs a{};
        a.A = op_rows(h->xt.f(), KP, B * kT, KP);
        a.B = op_rows(h->wemb.f(), KP, D, KP);
        a.C = h->tok.f() + (size_t)2 * D;
        a.cri = kT; a.cro = (long long)kS * D; a.crs = D; a.cns = 1;
        a.bias = W("skelEmbedding.bias"); a.R = a.C; a.act = 0;
        a.M = B * kT; a.N = D; a.K = KP;
        ECHK(h, launch_gemm_tr(a, true, true, 1, st));
    }
    float* xcur = h->tok.f();
    char pre[96];
#ifdef LS_SAG_ENC_FULL_LAST      // A/B build only (tools/sag_time.py): the last layer over all 36 rows, as the reference computes it
    const int nfull = L;
#else
    const int nfull = L - 1;
#endif
    for (int l = 0; l < nfull; ++l) {
        snprintf(pre, sizeof pre, "seqTransEncoder.layers.%d.", l);
        const std::string P(pre);
        // self-attention block: x = norm1(x + out_proj(softmax(q k^T / sqrt(128) + key mask) v))
        ECHK(h, launch_gemm_nt(xcur, D, W(P + "self_attn.in_proj_weight"), D, W(P + "self_attn.in_proj_bias"), nullptr, 0, h->qkv.f(), 3 * D, M, 3 * D, D, 0, st));
        ECHK(h, launch_sag_enc_attention(h->qkv.f(), kmask, h->attn.f(), B, H, D, st));
        ECHK(h, launch_gemm_nt(h->attn.f(), D, W(P + "self_attn.out_proj.weight"), D, W(P + "self_attn.out_proj.bias"), xcur, D, h->t1.f(), D, M, D, D, 0, st));
        ECHK(h, launch_layernorm512(h->t1.f(), nullptr, 0, W(P + "norm1.weight"), W(P + "norm1.bias"), h->x2.f(), M, st));
        // feed-forward: x = norm2(x + linear2(gelu(linear1(x))))
        ECHK(h, launch_gemm_nt(h->x2.f(), D, W(P + "linear1.weight"), D, W(P + "linear1.bias"), nullptr, 0, h->hid.f(), FF, M, FF, D, 3, st));
        ECHK(h, launch_gemm_nt(h->hid.f(), FF, W(P + "linear2.weight"), FF, W(P + "linear2.bias"), h->x2.f(), D, h->t3.f(), D, M, D, FF, 0, st));
        ECHK(h, launch_layernorm512(h->t3.f(), nullptr, 0, W(P + "norm2.weight"), W(P + "norm2.bias"), h->tok.f(), M, st));
    }
    const size_t rowb = (size_t)D * sizeof(float);
    if (nfull < L) {
        // Last layer: only token 0 leaves the encoder (:92), so K and V are projected for all 36 rows of a sample (rows D..3D of the packed
        // in_proj, one N = 2D GEMM) while Q, out_proj + residual, norm1, the FFN and norm2 run on the B token-0 rows, copied out first.
        snprintf(pre, sizeof pre, "seqTransEncoder.layers.%d.", L - 1);
        const std::string P(pre);
        const float* wi = W(P + "self_attn.in_proj_weight");
        const float* bi = W(P + "self_attn.in_proj_bias");
        ECHK(h, hipMemcpy2DAsync(h->x0.p, rowb, xcur, (size_t)kS * rowb, rowb, B, hipMemcpyDeviceToDevice, st));
        ECHK(h, launch_gemm_nt(xcur, D, wi + (size_t)D * D, D, bi + D, nullptr, 0, h->qkv.f(), 2 * D, M, 2 * D, D, 0, st));
        ECHK(h, launch_gemm_nt(h->x0.f(), D, wi, D, bi, nullptr, 0, h->q0.f(), D, B, D, D, 0, st));
        ECHK(h, launch_sag_enc_attention_row0(h->q0.f(), h->qkv.f(), kmask, h->a0.f(), B, H, D, st));
        ECHK(h, launch_gemm_nt(h->a0.f(), D, W(P + "self_attn.out_proj.weight"), D, W(P + "self_attn.out_proj.bias"), h->x0.f(), D, h->t1c.f(), D, B, D, D, 0, st));
        ECHK(h, launch_layernorm512(h->t1c.f(), nullptr, 0, W(P + "norm1.weight"), W(P + "norm1.bias"), h->x2c.f(), B, st));
        ECHK(h, launch_gemm_nt(h->x2c.f(), D, W(P + "linear1.weight"), D, W(P + "linear1.bias"), nullptr, 0, h->hidc.f(), FF, B, FF, D, 3, st));
        ECHK(h, launch_gemm_nt(h->hidc.f(), FF, W(P + "linear2.weight"), FF, W(P + "linear2.bias"), h->x2c.f(), D, h->t3c.f(), D, B, D, FF, 0, st));
        ECHK(h, launch_layernorm512(h->t3c.f(), nullptr, 0, W(P + "norm2.weight"), W(P + "norm2.bias"), h->mu.f(), B, st));
    } else {
        ECHK(h, hipMemcpy2DAsync(h->mu.p, rowb, xcur, (size_t)kS * rowb, rowb, B, hipMemcpyDeviceToDevice, st));
    }
    ECHK(h, hipEventRecord(h->ev[1], st));
    ECHK(h, hipMemcpyAsync(mu_out, h->mu.p, nb, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
    if (!wait) { h->pending_ms = true; return LS_OK; }      // the caller orders consumers behind ls_sag_enc_stream (ls_stream_order)
    ECHK(h, hipStreamSynchronize(st));
    ECHK(h, hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
    h->pending_ms = false;
    return LS_OK;
}

int ls_sag_enc_encode(ls_sag_enc* h, int batch, int on_device, const float* x, const unsigned char* mask, float* mu_out) {
    return sag_enc_encode_impl(h, batch, on_device, x, mask, mu_out, true);
}

// The same encode, enqueued only (device pointers): `mu_out` is complete once ls_sag_enc_stream() has reached this point, so a decoder
// handle consumes it after ls_stream_order(device, ls_sag_enc_stream(enc), ls_sag_stream(dec)) without a host round trip.
int ls_sag_enc_encode_async(ls_sag_enc* h, int batch, const float* x, const unsigned char* mask, float* mu_out) {
    return sag_enc_encode_impl(h, batch, 1, x, mask, mu_out, false);
}

float ls_sag_enc_last_encode_ms(const ls_sag_enc* h) {
    if (!h) return -1.f;
    if (h->pending_ms) {           // an asynchronous encode: its span is read once it has finished (waits for it)
        ls_sag_enc* m = const_cast<ls_sag_enc*>(h);
        if (hipEventSynchronize(m->ev[1]) == hipSuccess && hipEventElapsedTime(&m->last_ms, m->ev[0], m->ev[1]) == hipSuccess) m->pending_ms = false;
    }
    return h->last_ms;
}

void* ls_sag_enc_stream(const ls_sag_enc* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

}  // extern "C"
