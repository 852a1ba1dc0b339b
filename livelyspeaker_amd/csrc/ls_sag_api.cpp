// C-ABI of the SAG decoder (include/ls_hip.h, "ls_sag_*"): replaces SAG.decoder(batch) of
// scripts/test_LivelySpeaker_ted.py:88 = Decoder_TRANSFORMER.forward (scripts/model/motionclip_module.py:138-183).
#include "ls_xfmr_core.h"

using namespace ls;

struct ls_sag : SagBase {
    const float *map_w = nullptr, *map_b = nullptr, *final_w = nullptr, *final_b = nullptr;      // mapping.*, finallayer.* on the device
    DevBuf xin, zin, mask, q, qc, qkv, attn, t1, ca, x2, hid, t3, out;
    DevBuf wcross, bcross;      // cross-attention of ALL layers as one [L*D][D] matrix (see ls_sag_commit_weights)
};

// nn.TransformerDecoderLayer parameters (motionclip_module.py:122-128) in the order they are checked; the device reads multihead_attn.* as wcross / bcross
static const LayerRow kSagDecRows[] = {
    {"self_attn.in_proj_weight", (size_t)3 * kD * kD, 0, &Layer::in_w}, {"self_attn.in_proj_bias", (size_t)3 * kD, 0, &Layer::in_b},
    {"self_attn.out_proj.weight", (size_t)kD * kD, 0, &Layer::out_w}, {"self_attn.out_proj.bias", kD, 0, &Layer::out_b},
    {"multihead_attn.in_proj_weight", (size_t)3 * kD * kD, 0, nullptr}, {"multihead_attn.in_proj_bias", (size_t)3 * kD, 0, nullptr},
    {"multihead_attn.out_proj.weight", (size_t)kD * kD, 0, nullptr}, {"multihead_attn.out_proj.bias", kD, 0, nullptr},
    {"linear1.weight", 0, kD, &Layer::fc1_w}, {"linear1.bias", 0, 1, &Layer::fc1_b}, {"linear2.weight", 0, kD, &Layer::fc2_w}, {"linear2.bias", kD, 0, &Layer::fc2_b},
    {"norm1.weight", kD, 0, &Layer::ln_att_w}, {"norm1.bias", kD, 0, &Layer::ln_att_b}, {"norm2.weight", kD, 0, &Layer::ln_cross_w}, {"norm2.bias", kD, 0, &Layer::ln_cross_b},
    {"norm3.weight", kD, 0, &Layer::ln_ffn_w}, {"norm3.bias", kD, 0, &Layer::ln_ffn_b}};

extern "C" {

const char* ls_sag_last_error(const ls_sag* h) { return last_error(h); }

int ls_sag_create(const ls_sag_config* cfg, ls_sag** out) {
    const int rc = sag_check_config(cfg, out, "ls_sag_create");
    if (rc != LS_OK) return rc;
    if (cfg->n_pre_poses < 0 || cfg->n_pre_poses > kT) return fail<ls_sag>(nullptr, LS_EINVAL, "bad SAG config");
    return sag_open(cfg, out, kT, ls_sag_destroy);
}

void ls_sag_destroy(ls_sag* h) { xfmr_close(h); }

int ls_sag_set_weight(ls_sag* h, const char* key, const float* data, size_t n) { return xfmr_set_weight(h, "ls_sag_set_weight", key, data, n); }

int ls_sag_commit_weights(ls_sag* h) {
    if (!h) return LS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    const int D = kD, JF = h->JF;
    Commit<ls_sag> c(h);
    if (const int rc = c.layers("seqTransDecoder.layers.", h->cfg.num_layers, h->cfg.ff_size, kSagDecRows)) return rc;
    if (const int rc = c.need("finallayer.weight", (size_t)JF * D, &h->final_w)) return rc;      // :131
    if (const int rc = c.need("finallayer.bias", JF, &h->final_b)) return rc;
    if (const int rc = c.need("mapping.weight", (size_t)D * (JF + 1), &h->map_w)) return rc;   // :133  Linear(28,512)
    if (const int rc = c.need("mapping.bias", D, &h->map_b)) return rc;
    {   // Cross-attention to a memory of length 1 (the CLIP text feature): softmax over one key is 1, so every layer adds
        //     out_proj(v_proj(z)) = (W_out W_v) z + (W_out b_v + b_out)
        // to each of its rows -- a per-sample vector that depends on z only.  The products W_out W_v are formed here once (in double),
        // for all layers stacked as one [L*D][D] matrix, so a decode needs ONE small GEMM instead of two per layer.
        const int L = h->cfg.num_layers;
        std::vector<float> wc((size_t)L * D * D), bc((size_t)L * D);
        std::vector<double> row(D);
        for (int l = 0; l < L; ++l) {
            const std::string P = "seqTransDecoder.layers." + std::to_string(l) + ".multihead_attn.";
            const float* Wv = h->w.at(P + "in_proj_weight").data() + (size_t)2 * D * D;     // rows 2D..3D of in_proj: v_proj
            const float* bv = h->w.at(P + "in_proj_bias").data() + 2 * D;
            const float* Wo = h->w.at(P + "out_proj.weight").data();
            const float* bo = h->w.at(P + "out_proj.bias").data();
            for (int i = 0; i < D; ++i) {
                std::fill(row.begin(), row.end(), 0.0);
                double bacc = bo[i];
                for (int j = 0; j < D; ++j) {
                    const double wij = Wo[(size_t)i * D + j];
                    const float* wvj = Wv + (size_t)j * D;
                    for (int k = 0; k < D; ++k) row[k] += wij * (double)wvj[k];
                    bacc += wij * (double)bv[j];
                }
                for (int k = 0; k < D; ++k) wc[((size_t)l * D + i) * D + k] = (float)row[k];
                bc[(size_t)l * D + i] = (float)bacc;
            }
        }
        HIPCHK(h, h->wcross.ensure(wc.size() * sizeof(float)));
        HIPCHK(h, h->bcross.ensure(bc.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(h->wcross.p, wc.data(), wc.size() * sizeof(float), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(h->bcross.p, bc.data(), bc.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return c.done();
}

static int sag_decode_impl(ls_sag* h, int batch, int on_device, const float* x, const float* z, const unsigned char* mask, float* out, bool wait) {
    if (!h || !x || !z || !out) return fail(h, LS_EINVAL, "ls_sag_decode: null argument");
    if (!h->committed) return fail(h, LS_ESTATE, "ls_sag_decode before ls_sag_commit_weights");
    if (batch < 1) return fail(h, LS_EINVAL, "batch must be >= 1");
    HIPCHK(h, hipSetDevice(h->device));
    const int B = batch, D = kD, FF = h->cfg.ff_size, JF = h->JF, M = B * kT, H = h->cfg.num_heads;
    hipStream_t st = h->stream;
    const hipMemcpyKind in = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const size_t nx = (size_t)B * JF * kT * sizeof(float);
    HIPCHK(h, h->xin.ensure(nx)); HIPCHK(h, h->zin.ensure((size_t)B * D * sizeof(float))); HIPCHK(h, h->out.ensure(nx));
    HIPCHK(h, hipMemcpyAsync(h->xin.p, x, nx, in, st));
    HIPCHK(h, hipMemcpyAsync(h->zin.p, z, (size_t)B * D * sizeof(float), in, st));
    const unsigned char* dmask = nullptr;
    if (mask) {
        HIPCHK(h, h->mask.ensure((size_t)M));
        HIPCHK(h, hipMemcpyAsync(h->mask.p, mask, (size_t)M, in, st));
        dmask = static_cast<const unsigned char*>(h->mask.p);
    }
    const size_t nm = (size_t)M * D * sizeof(float);
    HIPCHK(h, h->q.ensure(nm));
    HIPCHK(h, h->qkv.ensure(3 * (nm + (size_t)128 * D * sizeof(float))));      // + the compact first layer's tile padding
    HIPCHK(h, h->attn.ensure(nm)); HIPCHK(h, h->t1.ensure(nm)); HIPCHK(h, h->x2.ensure(nm)); HIPCHK(h, h->t3.ensure(nm));
    HIPCHK(h, h->hid.ensure((size_t)M * FF * sizeof(float)));
    const int LD = h->cfg.num_layers * D;
    HIPCHK(h, h->ca.ensure((size_t)B * LD * sizeof(float)));
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    // cross-attention terms of all layers: ca[b][l*D + i] = (W_out_l W_v_l) z_b + (W_out_l b_v_l + b_out_l)
    HIPCHK(h, launch_gemm_nt(h->zin.f(), D, h->wcross.f(), D, h->bcross.f(), nullptr, 0, h->ca.f(), LD, B, LD, D, 0, st));
    // First layer: the query rows of frames f >= n_pre are b_map + pe[f] for EVERY sample, so their q / k / v projections are too.  Its
    // packed in_proj runs over the distinct rows only (B * n_pre + T - n_pre instead of B * T: 12 % of them at T = 34, n_pre = 4),
    // padded to whole 128-row tiles so that it stays on the GEMM's full-tile path; the attention kernel maps (sample, frame) to them.
    const int npre = h->cfg.n_pre_poses;
    const bool compact = npre > 0 && npre < kT;
    const int Mc = compact ? (B * npre + (kT - npre) + 127) / 128 * 128 : 0;
    if (compact) {
        const void* old = h->qc.p;
        HIPCHK(h, h->qc.ensure((size_t)Mc * D * sizeof(float)));
        if (old != h->qc.p) HIPCHK(h, hipMemsetAsync(h->qc.p, 0, (size_t)Mc * D * sizeof(float), st));       // pad rows: finite inputs
    }
    HIPCHK(h, launch_sag_queries(h->xin.f(), h->map_w, h->map_b, h->pe.f(), h->q.f(), compact ? h->qc.f() : nullptr, B, JF, npre, D, st));
    float* const xcur = h->q.f();      // every layer reads and writes q
    for (int l = 0; l < h->cfg.num_layers; ++l) {
        const Layer& w = h->layer[l];
        // self-attention block: x = norm1(x + out_proj(softmax(q k^T / sqrt(128)) v))
        const bool lc = compact && l == 0;
        HIPCHK(h, launch_gemm_nt(lc ? h->qc.f() : xcur, D, w.in_w, D, w.in_b, nullptr, 0, h->qkv.f(), 3 * D,
                               lc ? Mc : M, 3 * D, D, 0, st));
        HIPCHK(h, launch_sag_attention(h->qkv.f(), h->attn.f(), B, H, D, lc ? npre : 0, st));
        HIPCHK(h, launch_gemm_nt(h->attn.f(), D, w.out_w, D, w.out_b, xcur, D, h->t1.f(), D, M, D, D, 0, st));
        // ... norm1, then the cross-attention block x = norm2(x + ca_l[b]) (the per-sample vector computed above), in one pass
        HIPCHK(h, launch_layernorm512x2(h->t1.f(), w.ln_att_w, w.ln_att_b, h->ca.f() + (size_t)l * D, LD, w.ln_cross_w, w.ln_cross_b, h->x2.f(), M, st));
        // feed-forward: x = norm3(x + linear2(gelu(linear1(x))))
        if (const int rc = xfmr_ffn_postnorm(h, w, h->x2.f(), h->hid.f(), h->t3.f(), h->q.f(), M, FF)) return rc;
    }
    HIPCHK(h, launch_sag_final(xcur, h->final_w, h->final_b, dmask, h->out.f(), B, JF, D, st));
    return xfmr_finish(h, out, h->out.p, nx, on_device, wait);
}

int ls_sag_decode(ls_sag* h, int batch, int on_device, const float* x, const float* z, const unsigned char* mask, float* out) {
    return sag_decode_impl(h, batch, on_device, x, z, mask, out, true);
}

// The same decode, enqueued only (device pointers): returns without waiting for the GPU, so a caller that iterates batches can decode
// batch n + 1 on this handle's stream while batch n is refined on another handle's (scripts/test_LivelySpeaker_ted.py:57-113 runs them
// back to back).  `out` is complete once ls_sag_stream() has reached this point: order its consumers with ls_stream_order.  The
// handle's staging buffers are reused by the next decode on the same (in-order) stream.
int ls_sag_decode_async(ls_sag* h, int batch, const float* x, const float* z, const unsigned char* mask, float* out) {
    return sag_decode_impl(h, batch, 1, x, z, mask, out, false);
}

float ls_sag_last_decode_ms(const ls_sag* h) { return xfmr_last_ms(h); }

void* ls_sag_stream(const ls_sag* h) { return xfmr_stream(h); }

}  // extern "C"
