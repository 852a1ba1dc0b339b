// C-ABI of the SAG encoder (include/ls_hip.h, "ls_sag_enc_*"): replaces SAG.encoder(batch) = Encoder_TRANSFORMER.forward
// (scripts/model/motionclip_module.py:70-95), the first half of MOTIONCLIP.forward (scripts/model/motionclip.py:75-83).
#include "ls_xfmr_core.h"
#include "ls_train.h"      // GemmArgs / op_rows / launch_gemm_tr: the skelEmbedding product needs the two-level output rows launch_gemm_nt does not expose

#include <cstring>

using namespace ls;

static constexpr int kS = kSagEncS;

// nn.TransformerEncoderLayer parameters (motionclip_module.py:62-68), in the order they are checked
static const LayerRow kSagEncRows[] = {
    {"self_attn.in_proj_weight", (size_t)3 * kD * kD, 0, &Layer::in_w}, {"self_attn.in_proj_bias", (size_t)3 * kD, 0, &Layer::in_b},
    {"self_attn.out_proj.weight", (size_t)kD * kD, 0, &Layer::out_w}, {"self_attn.out_proj.bias", kD, 0, &Layer::out_b},
    {"linear1.weight", 0, kD, &Layer::fc1_w}, {"linear1.bias", 0, 1, &Layer::fc1_b}, {"linear2.weight", 0, kD, &Layer::fc2_w}, {"linear2.bias", kD, 0, &Layer::fc2_b},
    {"norm1.weight", kD, 0, &Layer::ln_att_w}, {"norm1.bias", kD, 0, &Layer::ln_att_b}, {"norm2.weight", kD, 0, &Layer::ln_ffn_w}, {"norm2.bias", kD, 0, &Layer::ln_ffn_b}};

struct ls_sag_enc : SagBase {
    const float *mu_q = nullptr, *sigma_q = nullptr, *emb_b = nullptr;      // muQuery, sigmaQuery, skelEmbedding.bias on the device
    int KP = 0;                // skelEmbedding's fan-in rounded up to the GEMM's K tile kGemmTileK (27 -> 32, 282 -> 288)
    DevBuf wemb, xin, maskin, kmask, xt, tok, qkv, attn, t1, x2, hid, t3;
    DevBuf x0, q0, a0, t1c, x2c, hidc, t3c, mu;      // the last layer's token-0 rows, [B][...]
};

extern "C" {

const char* ls_sag_enc_last_error(const ls_sag_enc* h) { return last_error(h); }

int ls_sag_enc_create(const ls_sag_config* cfg, ls_sag_enc** out) {
    int rc = sag_check_config(cfg, out, "ls_sag_enc_create");
    if (rc != LS_OK) return rc;
    if ((size_t)cfg->njoints * cfg->nfeats * (kT + 1) * sizeof(float) > 64 * 1024)
        return fail<ls_sag_enc>(nullptr, LS_EUNSUPPORTED, "njoints * nfeats = %d is too wide for the token builder", cfg->njoints * cfg->nfeats);
    // PositionalEncoding rows 0..35: the same table as the decoder's, two rows longer
    if ((rc = sag_open(cfg, out, kS, ls_sag_enc_destroy)) != LS_OK) return rc;
    (*out)->KP = ((*out)->JF + kGemmTileK - 1) / kGemmTileK * kGemmTileK;
    return LS_OK;
}

void ls_sag_enc_destroy(ls_sag_enc* h) { xfmr_close(h); }

int ls_sag_enc_set_weight(ls_sag_enc* h, const char* key, const float* data, size_t n) { return xfmr_set_weight(h, "ls_sag_enc_set_weight", key, data, n); }

int ls_sag_enc_commit_weights(ls_sag_enc* h) {
    if (!h) return LS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    const int D = kD, JF = h->JF, KP = h->KP;
    Commit<ls_sag_enc> c(h);
    if (const int rc = c.need("muQuery", D, &h->mu_q)) return rc;                               // :56-58
    if (const int rc = c.need("sigmaQuery", D, &h->sigma_q)) return rc;
    if (const int rc = c.need("skelEmbedding.weight", (size_t)D * JF, nullptr)) return rc;      // the device reads its padded copy, wemb
    if (const int rc = c.need("skelEmbedding.bias", D, &h->emb_b)) return rc;
    if (const int rc = c.layers("seqTransEncoder.layers.", h->cfg.num_layers, h->cfg.ff_size, kSagEncRows)) return rc;
    {   // skelEmbedding's weight with its rows zero-padded to KP columns: the operand xt is padded alike (k_sag_enc_prepare)
        const std::vector<float>& wsrc = h->w.at("skelEmbedding.weight");
        std::vector<float> wp((size_t)D * KP, 0.f);
        for (int d = 0; d < D; ++d) std::memcpy(&wp[(size_t)d * KP], &wsrc[(size_t)d * JF], (size_t)JF * sizeof(float));
        HIPCHK(h, h->wemb.ensure(wp.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(h->wemb.p, wp.data(), wp.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return c.done();
}

static int sag_enc_encode_impl(ls_sag_enc* h, int batch, int on_device, const float* x, const unsigned char* mask, float* mu_out, bool wait) {
    if (!h || !x || !mu_out) return fail(h, LS_EINVAL, "ls_sag_enc_encode: null argument");
    if (!h->committed) return fail(h, LS_ESTATE, "ls_sag_enc_encode before ls_sag_enc_commit_weights");
    if (batch < 1) return fail(h, LS_EINVAL, "batch must be >= 1");
    if ((long long)batch * kS * (3 * kD > h->cfg.ff_size ? 3 * kD : h->cfg.ff_size) >= (1ll << 31))      // row * width stays an int
        return fail(h, LS_EINVAL, "batch %d is too large for one encode", batch);
    HIPCHK(h, hipSetDevice(h->device));
    const int B = batch, D = kD, FF = h->cfg.ff_size, JF = h->JF, KP = h->KP, M = B * kS, H = h->cfg.num_heads, L = h->cfg.num_layers;
    hipStream_t st = h->stream;
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t nx = (size_t)B * JF * kT * sizeof(float), nm = (size_t)M * D * sizeof(float), nb = (size_t)B * D * sizeof(float);
    HIPCHK(h, h->xin.ensure(nx)); HIPCHK(h, h->kmask.ensure((size_t)M)); HIPCHK(h, h->xt.ensure((size_t)B * kT * KP * sizeof(float)));
    HIPCHK(h, h->tok.ensure(nm)); HIPCHK(h, h->qkv.ensure(3 * nm)); HIPCHK(h, h->attn.ensure(nm)); HIPCHK(h, h->t1.ensure(nm));
    HIPCHK(h, h->x2.ensure(nm)); HIPCHK(h, h->t3.ensure(nm)); HIPCHK(h, h->hid.ensure((size_t)M * FF * sizeof(float)));
    HIPCHK(h, h->x0.ensure(nb)); HIPCHK(h, h->q0.ensure(nb)); HIPCHK(h, h->a0.ensure(nb)); HIPCHK(h, h->t1c.ensure(nb)); HIPCHK(h, h->x2c.ensure(nb));
    HIPCHK(h, h->t3c.ensure(nb)); HIPCHK(h, h->mu.ensure(nb)); HIPCHK(h, h->hidc.ensure((size_t)B * FF * sizeof(float)));
    HIPCHK(h, hipMemcpyAsync(h->xin.p, x, nx, in, st));
    const unsigned char* dmask = nullptr;
    if (mask) {
        HIPCHK(h, h->maskin.ensure((size_t)B * kT));
        HIPCHK(h, hipMemcpyAsync(h->maskin.p, mask, (size_t)B * kT, in, st));
        dmask = static_cast<const unsigned char*>(h->maskin.p);
    }
    unsigned char* kmask = static_cast<unsigned char*>(h->kmask.p);
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    // tokens: the two learned queries and pe are written by the staging kernel; skelEmbedding(frames) + bias is added onto rows 2.. of
    // every sample by one GEMM whose output rows skip the two query rows (two-level row index: 34 rows per 36-row sample)
    HIPCHK(h, launch_sag_enc_prepare(h->xin.f(), dmask, h->mu_q, h->sigma_q, h->pe.f(), h->tok.f(), h->xt.f(), kmask, B, JF, KP, st));
    {
        GemmArgs a{};
        a.A = op_rows(h->xt.f(), KP, B * kT, KP);
        a.B = op_rows(h->wemb.f(), KP, D, KP);
        a.C = h->tok.f() + (size_t)2 * D;
        a.cri = kT; a.cro = (long long)kS * D; a.crs = D; a.cns = 1;
        a.bias = h->emb_b; a.R = a.C; a.act = 0;
        a.M = B * kT; a.N = D; a.K = KP;
        HIPCHK(h, launch_gemm_tr(a, true, true, 1, st));
    }
    float* xcur = h->tok.f();
#ifdef LS_SAG_ENC_FULL_LAST      // A/B build only (tools/sag_time.py): the last layer over all 36 rows, as the reference computes it
    const int nfull = L;
#else
    const int nfull = L - 1;
#endif
    for (int l = 0; l < nfull; ++l) {
        const Layer& w = h->layer[l];
        // self-attention block: x = norm1(x + out_proj(softmax(q k^T / sqrt(128) + key mask) v))
        HIPCHK(h, launch_gemm_nt(xcur, D, w.in_w, D, w.in_b, nullptr, 0, h->qkv.f(), 3 * D, M, 3 * D, D, 0, st));
        HIPCHK(h, launch_sag_enc_attention(h->qkv.f(), kmask, h->attn.f(), B, H, D, st));
        HIPCHK(h, launch_gemm_nt(h->attn.f(), D, w.out_w, D, w.out_b, xcur, D, h->t1.f(), D, M, D, D, 0, st));
        HIPCHK(h, launch_layernorm512(h->t1.f(), nullptr, 0, w.ln_att_w, w.ln_att_b, h->x2.f(), M, st));
        // feed-forward: x = norm2(x + linear2(gelu(linear1(x))))
        if (const int rc = xfmr_ffn_postnorm(h, w, h->x2.f(), h->hid.f(), h->t3.f(), h->tok.f(), M, FF)) return rc;
    }
    const size_t rowb = (size_t)D * sizeof(float);
    if (nfull < L) {
        // Last layer: only token 0 leaves the encoder (:92), so K and V are projected for all 36 rows of a sample (rows D..3D of the packed
        // in_proj, one N = 2D GEMM) while Q, out_proj + residual, norm1, the FFN and norm2 run on the B token-0 rows, copied out first.
        const Layer& w = h->layer[L - 1];
        HIPCHK(h, hipMemcpy2DAsync(h->x0.p, rowb, xcur, (size_t)kS * rowb, rowb, B, hipMemcpyDeviceToDevice, st));
        HIPCHK(h, launch_gemm_nt(xcur, D, w.in_w + (size_t)D * D, D, w.in_b + D, nullptr, 0, h->qkv.f(), 2 * D, M, 2 * D, D, 0, st));
        HIPCHK(h, launch_gemm_nt(h->x0.f(), D, w.in_w, D, w.in_b, nullptr, 0, h->q0.f(), D, B, D, D, 0, st));
        HIPCHK(h, launch_sag_enc_attention_row0(h->q0.f(), h->qkv.f(), kmask, h->a0.f(), B, H, D, st));
        HIPCHK(h, launch_gemm_nt(h->a0.f(), D, w.out_w, D, w.out_b, h->x0.f(), D, h->t1c.f(), D, B, D, D, 0, st));
        HIPCHK(h, launch_layernorm512(h->t1c.f(), nullptr, 0, w.ln_att_w, w.ln_att_b, h->x2c.f(), B, st));
        if (const int rc = xfmr_ffn_postnorm(h, w, h->x2c.f(), h->hidc.f(), h->t3c.f(), h->mu.f(), B, FF)) return rc;
    } else {
        HIPCHK(h, hipMemcpy2DAsync(h->mu.p, rowb, xcur, (size_t)kS * rowb, rowb, B, hipMemcpyDeviceToDevice, st));
    }
    return xfmr_finish(h, mu_out, h->mu.p, nb, on_device, wait);
}

int ls_sag_enc_encode(ls_sag_enc* h, int batch, int on_device, const float* x, const unsigned char* mask, float* mu_out) {
    return sag_enc_encode_impl(h, batch, on_device, x, mask, mu_out, true);
}

// The same encode, enqueued only (device pointers): `mu_out` is complete once ls_sag_enc_stream() has reached this point, so a decoder
// handle consumes it after ls_stream_order(device, ls_sag_enc_stream(enc), ls_sag_stream(dec)) without a host round trip.
int ls_sag_enc_encode_async(ls_sag_enc* h, int batch, const float* x, const unsigned char* mask, float* mu_out) {
    return sag_enc_encode_impl(h, batch, 1, x, mask, mu_out, false);
}

float ls_sag_enc_last_encode_ms(const ls_sag_enc* h) { return xfmr_last_ms(h); }

void* ls_sag_enc_stream(const ls_sag_enc* h) { return xfmr_stream(h); }

}  // extern "C"
