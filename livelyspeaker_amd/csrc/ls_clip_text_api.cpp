// C-ABI of the CLIP text encoder (include/ls_hip.h, "ls_clip_text_*"): replaces clip_model.encode_text(text).float()
// (scripts/test_LivelySpeaker_ted.py:85-86, scripts/model/motionclip.py:52-53).  The handle is an XfmrCore (ls_xfmr_core.h):
// stream, timing events, weight maps resolved to pointers at commit, error path.  Kernels: ls_clip_text.hip; linears: ls_gemm.hip; LayerNorm: ls_sag.hip.
#include "ls_xfmr_core.h"

using namespace ls;

namespace {

constexpr int kRowTile = 128;       // packed rows are padded to whole GEMM tiles so that every linear runs the LDS-DMA kernel, whose
                                    // result for a row does not depend on where the row sits (the bitwise tests rest on this)
inline int pad_rows(long long r) { return (int)((r + kRowTile - 1) / kRowTile * kRowTile); }

// first position of the row maximum, for every row; false if an id lies outside [0, vocab)
bool plan_rows(const int64_t* tok, int B, int ctx, int vocab, int* eot) {
    bool ok = true;
    for (int b = 0; b < B; ++b) {
        const int64_t* row = tok + (size_t)b * ctx;
        int pos = 0;
        for (int t = 0; t < ctx; ++t) {
            if (row[t] < 0 || row[t] >= vocab) ok = false;
            if (row[t] > row[pos]) pos = t;
        }
        eot[b] = pos;
    }
    return ok;
}

// ResidualAttentionBlock parameters, in the order they are checked (pre-norm: ln_1 in front of the attention, ln_2 in front of the MLP)
const LayerRow kClipRows[] = {
    {"ln_1.weight", kD, 0, &Layer::ln_att_w}, {"ln_1.bias", kD, 0, &Layer::ln_att_b}, {"attn.in_proj_weight", (size_t)3 * kD * kD, 0, &Layer::in_w},
    {"attn.in_proj_bias", (size_t)3 * kD, 0, &Layer::in_b}, {"attn.out_proj.weight", (size_t)kD * kD, 0, &Layer::out_w}, {"attn.out_proj.bias", kD, 0, &Layer::out_b},
    {"ln_2.weight", kD, 0, &Layer::ln_ffn_w}, {"ln_2.bias", kD, 0, &Layer::ln_ffn_b}, {"mlp.c_fc.weight", 0, kD, &Layer::fc1_w}, {"mlp.c_fc.bias", 0, 1, &Layer::fc1_b},
    {"mlp.c_proj.weight", 0, kD, &Layer::fc2_w}, {"mlp.c_proj.bias", kD, 0, &Layer::fc2_b}};

}  // namespace

struct ls_clip_text : XfmrCore {
    ls_clip_text_config cfg{};
    const float *tok_emb = nullptr, *pos_emb = nullptr, *lnf_w = nullptr, *lnf_b = nullptr;      // token_embedding.weight, positional_embedding, ln_final.*
    DevBuf proj_t;                        // text_projection transposed: [embed][width], the GEMM's W[n][k]
    DevBuf tok, plan;                     // tokens [B][ctx] int64; plan [3][B] ints: eot, row0, len (device tokens: k_clip_plan's [B + 1] first)
    DevBuf x, ln, qkv, attn, hid;         // packed rows, padded to whole GEMM tiles
    DevBuf e, eln, feat;                  // the B EOT rows, padded alike
    std::vector<int> hplan;               // host copy of the plan (stays alive under the asynchronous upload)
    std::vector<int64_t> htok;
};

extern "C" {

const char* ls_clip_text_last_error(const ls_clip_text* h) { return last_error(h); }

int ls_clip_text_plan(const int64_t* tokens, int batch, int context_length, int vocab_size, int32_t* eot_out, int32_t* row0_out,
                      int64_t* total_out) {
    if (!tokens || !eot_out || !row0_out || !total_out || batch < 1 || context_length < 1 || vocab_size < 1) return LS_EINVAL;
    if (!plan_rows(tokens, batch, context_length, vocab_size, eot_out)) return LS_EINVAL;
    int64_t r = 0;
    for (int b = 0; b < batch; ++b) { row0_out[b] = (int32_t)r; r += eot_out[b] + 1; }
    *total_out = r;
    return LS_OK;
}

int ls_clip_text_create(const ls_clip_text_config* cfg, ls_clip_text** out) {
    if (!cfg || !out) return fail<ls_clip_text>(nullptr, LS_EINVAL, "ls_clip_text_create: null argument");
    *out = nullptr;
    if (cfg->width != kD || cfg->embed_dim != kD) return fail<ls_clip_text>(nullptr, LS_EUNSUPPORTED, "width and embed_dim must be %d", kD);
    if (cfg->heads != 8) return fail<ls_clip_text>(nullptr, LS_EUNSUPPORTED, "heads must be 8 (head dim 64)");
    if (cfg->context_length < 1 || cfg->context_length > kClipCtx)
        return fail<ls_clip_text>(nullptr, LS_EUNSUPPORTED, "context_length must be 1..%d", kClipCtx);
    if (cfg->layers < 1 || cfg->layers > 24) return fail<ls_clip_text>(nullptr, LS_EUNSUPPORTED, "layers must be 1..24");
    if (cfg->vocab_size < 1) return fail<ls_clip_text>(nullptr, LS_EINVAL, "vocab_size must be >= 1");
    const int rc = xfmr_open(cfg->device, out, ls_clip_text_destroy);
    if (rc == LS_OK) (*out)->cfg = *cfg;
    return rc;
}

void ls_clip_text_destroy(ls_clip_text* h) { xfmr_close(h); }

int ls_clip_text_set_weight(ls_clip_text* h, const char* key, const float* data, size_t n) { return xfmr_set_weight(h, "ls_clip_text_set_weight", key, data, n); }

int ls_clip_text_commit_weights(ls_clip_text* h) {
    if (!h) return LS_EINVAL;
    HIPCHK(h, hipSetDevice(h->device));
    const size_t D = kD;
    Commit<ls_clip_text> c(h);
    if (const int rc = c.need("token_embedding.weight", (size_t)h->cfg.vocab_size * D, &h->tok_emb)) return rc;
    if (const int rc = c.need("positional_embedding", (size_t)h->cfg.context_length * D, &h->pos_emb)) return rc;
    if (const int rc = c.layers("transformer.resblocks.", h->cfg.layers, 4 * D, kClipRows)) return rc;
    if (const int rc = c.need("ln_final.weight", D, &h->lnf_w)) return rc;
    if (const int rc = c.need("ln_final.bias", D, &h->lnf_b)) return rc;
    if (const int rc = c.need("text_projection", D * D, nullptr)) return rc;      // the device reads its transposed copy, proj_t
    {   // features = x @ P: as the GEMM's W[n][k] that is P transposed, once
        const std::vector<float>& p = h->w.at("text_projection");
        std::vector<float> pt(D * D);
        for (size_t k = 0; k < D; ++k)
            for (size_t n = 0; n < D; ++n) pt[n * D + k] = p[k * D + n];
        HIPCHK(h, h->proj_t.ensure(pt.size() * sizeof(float)));
        HIPCHK(h, hipMemcpy(h->proj_t.p, pt.data(), pt.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return c.done();
}

// tokens_dev / out_dev: where the caller's tokens and output live
static int clip_encode_impl(ls_clip_text* h, int batch, bool tokens_dev, bool out_dev, const int64_t* tokens, int prune, float* out, bool wait) {
    if (!h || !tokens || !out) return fail(h, LS_EINVAL, "ls_clip_text_encode: null argument");
    if (!h->committed) return fail(h, LS_ESTATE, "ls_clip_text_encode before ls_clip_text_commit_weights");
    if (batch < 1) return fail(h, LS_EINVAL, "batch must be >= 1");
    const int B = batch, D = kD, FF = 4 * kD, ctx = h->cfg.context_length, H = h->cfg.heads, L = h->cfg.layers;
    // the LDS-DMA GEMM addresses an operand through 31-bit byte offsets: rows * 2048 floats must stay below 2^29
    if ((long long)pad_rows((long long)B * ctx) * FF >= (1ll << 29)) return fail(h, LS_EINVAL, "batch %d is too large for one encode", batch);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    const size_t ntok = (size_t)B * ctx * sizeof(int64_t);
    // an earlier asynchronous encode may still be reading the host copies of its plan and tokens, which this call rewrites
    if (h->pending_ms) HIPCHK(h, hipStreamSynchronize(st));
    h->hplan.resize((size_t)3 * B + 1);
    int* eot = h->hplan.data();
    int* row0 = eot + B;
    int* len = row0 + B;
    HIPCHK(h, h->tok.ensure(ntok));
    HIPCHK(h, h->plan.ensure(((size_t)3 * B + 1) * sizeof(int)));
    int* dplan = static_cast<int*>(h->plan.p);
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    const long long* dtok;
    if (tokens_dev) {
        // the one host wait of the call: the GEMM grids below need the packed row count
        dtok = reinterpret_cast<const long long*>(tokens);
        HIPCHK(h, launch_clip_plan(dtok, dplan, B, ctx, h->cfg.vocab_size, st));
        HIPCHK(h, hipMemcpyAsync(eot, dplan, ((size_t)B + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(h, hipStreamSynchronize(st));
        if (eot[B] != 0) return fail(h, LS_EINVAL, "%d token id(s) outside [0, %d)", eot[B], h->cfg.vocab_size);
    } else {
        if (!plan_rows(tokens, B, ctx, h->cfg.vocab_size, eot)) return fail(h, LS_EINVAL, "token id outside [0, %d)", h->cfg.vocab_size);
        h->htok.assign(tokens, tokens + (size_t)B * ctx);       // the caller's buffer may go before an asynchronous copy has read it
        HIPCHK(h, hipMemcpyAsync(h->tok.p, h->htok.data(), ntok, hipMemcpyHostToDevice, st));
        dtok = static_cast<const long long*>(h->tok.p);
    }
    long long R = 0;
    int max_len = 0;
    for (int b = 0; b < B; ++b) {
        len[b] = prune ? eot[b] + 1 : ctx;
        row0[b] = (int)R;
        R += len[b];
        if (len[b] > max_len) max_len = len[b];
    }
    HIPCHK(h, hipMemcpyAsync(dplan, eot, (size_t)3 * B * sizeof(int), hipMemcpyHostToDevice, st));
    const int* d_eot = dplan;
    const int* d_row0 = dplan + B;
    const int* d_len = dplan + 2 * B;
    const int M = (int)R, MP = pad_rows(R), BP = pad_rows(B);
    const size_t row = (size_t)D * sizeof(float);
    HIPCHK(h, h->x.ensure(MP * row)); HIPCHK(h, h->ln.ensure(MP * row)); HIPCHK(h, h->attn.ensure(MP * row));
    HIPCHK(h, h->qkv.ensure(3 * MP * row)); HIPCHK(h, h->hid.ensure((size_t)MP * FF * sizeof(float)));
    HIPCHK(h, h->e.ensure(BP * row)); HIPCHK(h, h->eln.ensure(BP * row)); HIPCHK(h, h->feat.ensure(BP * row));
    // the rows between the packed count and the tile edge: the GEMMs read and write them, nothing reads their results
    if (MP > M) {
        HIPCHK(h, hipMemsetAsync(h->x.f() + (size_t)M * D, 0, (MP - M) * row, st));
        HIPCHK(h, hipMemsetAsync(h->ln.f() + (size_t)M * D, 0, (MP - M) * row, st));
        HIPCHK(h, hipMemsetAsync(h->attn.f() + (size_t)M * D, 0, (MP - M) * row, st));
    }
    if (BP > B) HIPCHK(h, hipMemsetAsync(h->eln.f() + (size_t)B * D, 0, (BP - B) * row, st));
    HIPCHK(h, launch_clip_embed(dtok, d_row0, d_len, h->tok_emb, h->pos_emb, h->x.f(), B, ctx, st));
    float* x = h->x.f();
    for (int l = 0; l < L; ++l) {
        const Layer& w = h->layer[l];
        // x = x + out_proj(MHA(ln_1(x)))
        HIPCHK(h, launch_layernorm512(x, nullptr, 0, w.ln_att_w, w.ln_att_b, h->ln.f(), M, st));
        HIPCHK(h, launch_gemm_nt(h->ln.f(), D, w.in_w, D, w.in_b, nullptr, 0, h->qkv.f(), 3 * D, MP, 3 * D, D, 0, st));
        HIPCHK(h, launch_clip_attention(h->qkv.f(), h->attn.f(), d_row0, d_len, B, H, D, max_len, st));
        HIPCHK(h, launch_gemm_nt(h->attn.f(), D, w.out_w, D, w.out_b, x, D, x, D, MP, D, D, 0, st));
        // x = x + c_proj(QuickGELU(c_fc(ln_2(x))))
        HIPCHK(h, launch_layernorm512(x, nullptr, 0, w.ln_ffn_w, w.ln_ffn_b, h->ln.f(), M, st));
        HIPCHK(h, launch_gemm_nt(h->ln.f(), D, w.fc1_w, D, w.fc1_b, nullptr, 0, h->hid.f(), FF, MP, FF, D, 4, st));
        HIPCHK(h, launch_gemm_nt(h->hid.f(), FF, w.fc2_w, FF, w.fc2_b, x, D, x, D, MP, D, FF, 0, st));
    }
    // ln_final is row-wise, so it runs on the B rows that leave the tower only
    HIPCHK(h, launch_clip_gather_eot(x, d_row0, d_eot, h->e.f(), B, st));
    HIPCHK(h, launch_layernorm512(h->e.f(), nullptr, 0, h->lnf_w, h->lnf_b, h->eln.f(), B, st));
    HIPCHK(h, launch_gemm_nt(h->eln.f(), D, h->proj_t.f(), D, nullptr, nullptr, 0, h->feat.f(), D, BP, D, D, 0, st));
    return xfmr_finish(h, out, h->feat.p, (size_t)B * row, out_dev ? 1 : 0, wait);
}

int ls_clip_text_encode(ls_clip_text* h, int batch, int on_device, const int64_t* tokens, int prune, float* out) {
    if (on_device < 0 || on_device > 2) return fail(h, LS_EINVAL, "on_device must be 0, 1 or 2");
    return clip_encode_impl(h, batch, on_device == 1, on_device != 0, tokens, prune, out, true);
}

int ls_clip_text_encode_async(ls_clip_text* h, int batch, int tokens_on_device, const int64_t* tokens, int prune, float* out) {
    return clip_encode_impl(h, batch, tokens_on_device != 0, true, tokens, prune, out, false);
}

float ls_clip_text_last_encode_ms(const ls_clip_text* h) { return xfmr_last_ms(h); }

void* ls_clip_text_stream(const ls_clip_text* h) { return xfmr_stream(h); }

}  // extern "C"
