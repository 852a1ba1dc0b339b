// Host images of the sampling handle's weights (ls_weights.h): the key table and its resolver, then one function per group.  Every
// layout below is the per-lane operand order a kernel header documents; the index maps here are what those comments refer to.
#include "ls_weights.h"

#include <cstdio>
#include <cstring>

#include "ls_hip.h"

namespace ls {

namespace {

constexpr int D = kD;

// one row of the key table: the state-dict key, its element count, where the pointer goes
struct Row { std::string key; size_t n; const float** dst; };
// the same for a per-layer key: the suffix behind backbone.mlps.<l>.
struct LayerRow { const char* suffix; size_t n; const float* LayerWeights::*dst; };

int resolve(const WeightMap& m, const std::string& key, size_t want, const float** dst, std::string& msg) {
    char buf[512];
    auto it = m.find(key);
    if (it == m.end()) snprintf(buf, sizeof buf, "missing weight '%s'", key.c_str());
    else if (it->second.size() != want) snprintf(buf, sizeof buf, "weight '%s' has %zu elements, expected %zu", key.c_str(), it->second.size(), want);
    else { *dst = it->second.data(); return LS_OK; }
    msg = buf;
    return LS_ESTATE;
}

// bf16 round-to-nearest-even, as v_cvt_pk_bf16_f32 does on the device side of the split
unsigned short f32_to_bf16(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    u += 0x7FFFu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
float bf16_to_f32(unsigned short h) {
    const unsigned u = (unsigned)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// a row-major matrix, zero outside rows x cols: how every image pads
struct Mat {
    const float* p; int rows, cols, ld;
    float operator()(int r, int c) const { return r < rows && c < cols ? p[(size_t)r * ld + c] : 0.f; }
};
// WW = blockdiag(Wt, Wt) on the packed rows of a sample's two passes (R = 2 S rows)
struct BlockDiag {
    const float* wt; int S, R;
    float operator()(int r, int c) const { return r < R && c < R && r / S == c / S ? wt[(size_t)(r % S) * S + (c % S)] : 0.f; }
};

// img[i0][i1]...[i(N-1)] = at(i) for every index tuple below `ext`, the last index fastest
template <size_t N, class At>
Img pack(const int (&ext)[N], At at) {
    size_t n = 1;
    for (int e : ext) n *= (size_t)e;
    Img out(n);
    int i[N] = {};
    for (size_t o = 0; o < n; ++o) {
        out[o] = at(i);
        for (int k = N - 1; k >= 0 && ++i[k] == ext[k]; --k) i[k] = 0;
    }
    return out;
}
// the images of all layers, one behind the other
template <class One>
Img per_layer(const WeightDims& d, One one) {
    Img v;
    for (int l = 0; l < d.L; ++l) { const Img x = one(l); v.insert(v.end(), x.begin(), x.end()); }
    return v;
}

// the row / column a lane holds in a 16-wide fp32 MFMA operand tile
inline int s16(int lane) { return lane & 15; }
inline int g4(int lane) { return lane >> 4; }

// [w][p][q][c2][lane][j] = M[n = 64w + 16(2p+c2) + (lane&15)][k = 16q + 4(lane>>4) + j], nq k tiles: a wave's channel-mixing A operand
template <class M>
Img wave_rows(int nq, M m) {
    return pack({kWaves, 2, nq, 2, 64, 4}, [&](const int* i) { return m(64 * i[0] + 16 * (2 * i[1] + i[3]) + s16(i[4]), 16 * i[2] + 4 * g4(i[4]) + i[5]); });
}
// [nb][q][lane][j] = M[n = 16nb + (lane&15)][k = 16q + 4(lane>>4) + j] over all 32 k tiles of the 512 channels
template <class M>
Img row_tiles(int nb, M m) {
    return pack({nb, 32, 64, 4}, [&](const int* i) { return m(16 * i[0] + s16(i[2]), 16 * i[1] + 4 * g4(i[2]) + i[3]); });
}
// [t][ks][lane][e] = M[r = 16t + (lane&15)][r' = 32ks + 8(lane>>4) + e]: operand order of v_mfma_f32_16x16x32_bf16
template <class M>
Img bf16_tiles(int nt, int nks, M m) {
    return pack({nt, nks, 64, 8}, [&](const int* i) { return m(16 * i[0] + s16(i[2]), 32 * i[1] + 8 * g4(i[2]) + i[3]); });
}
// [q][mt][lane][e] = Wt[r = 16mt + (lane&15)][k = 16q + 4(lane>>4) + e], or k = 16q + 4e + (lane>>4) where the four lane groups of an
// MFMA k step read four CONSECUTIVE rows of the LDS operand (the mixer); nt x nt tiles, zero beyond S
Img tok_tiles(int nt, bool consecutive, Mat m) {
    return pack({nt, nt, 64, 4}, [&](const int* i) {
        return m(16 * i[1] + s16(i[2]), 16 * i[0] + (consecutive ? 4 * i[3] + g4(i[2]) : 4 * g4(i[2]) + i[3]));
    });
}

Mat tok(const Weights& w, const WeightDims& d, int l) { return Mat{w.layer[l].w_tok, d.S, d.S, d.S}; }
Mat folded(const Ln2Fold& f, int l) { return Mat{f.w.data() + (size_t)l * D * D, D, D, D}; }
Mat pose(const Weights& w, const WeightDims& d) { return Mat{w.w_out, d.JF, D, D}; }

}  // namespace

int resolve_weights(const WeightMap& m, const WeightDims& d, Weights& w, std::string& msg) {
    const size_t S = d.S, JF = d.JF;
    const LayerRow layer_rows[] = {
        {"block2.1.weight", (size_t)D * D, &LayerWeights::w_ch}, {"block2.1.bias", D, &LayerWeights::b_ch},
        {"block1.1.weight", S * S, &LayerWeights::w_tok},        {"block1.1.bias", S, &LayerWeights::b_tok},
        {"block1.0.alpha", D, &LayerWeights::ln1a},              {"block1.0.beta", D, &LayerWeights::ln1b},
        {"block2.0.alpha", D, &LayerWeights::ln2a},              {"block2.0.beta", D, &LayerWeights::ln2b},
    };
    w = Weights{};
    w.layer.assign(d.L, LayerWeights{});
    for (int l = 0; l < d.L; ++l)
        for (const LayerRow& r : layer_rows)
            if (const int rc = resolve(m, layer_key(l, r.suffix), r.n, &(w.layer[l].*r.dst), msg)) return rc;
    std::vector<Row> rows = {
        {"input_mapping.weight", (size_t)D * d.KIN, &w.w_in},
        {"output_process.poseFinal.weight", JF * D, &w.w_out},
        {"output_process.poseFinal.bias", JF, &w.b_out},
        {"input_mapping.bias", D, &w.b_in},
    };
    for (int i = 0; i < 4; ++i) {
        rows.push_back({conv_key(i, "weight"), (size_t)kConvCout[i] * kConvCin[i] * 15, &w.conv_w[i]});
        rows.push_back({conv_key(i, "bias"), (size_t)kConvCout[i], &w.conv_b[i]});
    }
    const Row tail[] = {
        {"speaker_embedding.weight", (size_t)d.n_speakers * 256, &w.spk_emb},
        {"speaker_mu.weight", (size_t)D * 256, &w.mu_w},         {"speaker_mu.bias", D, &w.mu_b},
        {"speaker_logvar.weight", (size_t)D * 256, &w.lv_w},     {"speaker_logvar.bias", D, &w.lv_b},
        {"backbone.embed_timestep.time_embed.0.weight", (size_t)D * D, &w.te_w0}, {"backbone.embed_timestep.time_embed.0.bias", D, &w.te_b0},
        {"backbone.embed_timestep.time_embed.2.weight", (size_t)D * D, &w.te_w2}, {"backbone.embed_timestep.time_embed.2.bias", D, &w.te_b2},
    };
    rows.insert(rows.end(), std::begin(tail), std::end(tail));
    if (d.n_emotions > 0) rows.push_back({"emotion_embedding.weight", (size_t)d.n_emotions * D, &w.emo_emb});
    for (const Row& r : rows)
        if (const int rc = resolve(m, r.key, r.n, r.dst, msg)) return rc;
    return LS_OK;
}

Ln2Fold fold_ln2(const Weights& w, const WeightDims& d) {
    Ln2Fold f{std::vector<float>((size_t)d.L * D * D), std::vector<float>((size_t)d.L * D), std::vector<float>((size_t)d.L * D)};
    for (int l = 0; l < d.L; ++l) {
        const LayerWeights& y = w.layer[l];
        for (int n = 0; n < D; ++n) {
            double sb = y.b_ch[n], sw = 0.0;
            for (int k = 0; k < D; ++k) {
                const float wv = y.w_ch[(size_t)n * D + k];
                const float wf = wv * y.ln2a[k];
                f.w[((size_t)l * D + n) * D + k] = wf;
                sb += (double)wv * (double)y.ln2b[k];
                sw += (double)wf;
            }
            f.b[(size_t)l * D + n] = (float)sb;
            f.wsum[(size_t)l * D + n] = (float)sw;
        }
    }
    return f;
}

// v = hi + mid + lo exactly, each bf16 round-to-nearest-even (both differences are exact in fp32): as many planes as `out` names
static void split_bf16(const Img& v, std::initializer_list<Img16*> out) {
    for (Img16* p : out) p->resize(v.size());
    for (size_t i = 0; i < v.size(); ++i) {
        float r = v[i];
        for (Img16* p : out) {
            (*p)[i] = f32_to_bf16(r);
            r = r - bf16_to_f32((*p)[i]);
        }
    }
}

// one member of every layer, `n` floats each: [L][n]
static Img stack(const Weights& w, const float* LayerWeights::*member, size_t n) {
    Img v(w.layer.size() * n);
    for (size_t l = 0; l < w.layer.size(); ++l) memcpy(&v[l * n], w.layer[l].*member, n * sizeof(float));
    return v;
}

// Long-sequence path (ls_long.hip): plain row-major weights for the batch-level kernels.  winx: the x_t columns of input_mapping, K padded
// to whole GEMM tiles.  wout: poseFinal padded with zero rows to whole 128-column GEMM tiles: N = 282 would send the product down the
// general staging path (41 TFLOP/s at 9728 rows); as 384 columns it is a full-tile LDS-DMA product, the extra columns are never read
LongImages long_images(const Weights& w, const WeightDims& d) {
    const Mat xcols{w.w_in, D, d.JF, d.KIN}, wout = pose(w, d);
    return {stack(w, &LayerWeights::w_tok, (size_t)d.S * d.S), stack(w, &LayerWeights::b_tok, d.S), stack(w, &LayerWeights::w_ch, (size_t)D * D),
            stack(w, &LayerWeights::b_ch, D), stack(w, &LayerWeights::ln1a, D), stack(w, &LayerWeights::ln1b, D), stack(w, &LayerWeights::ln2a, D),
            stack(w, &LayerWeights::ln2b, D), pack({D, d.JFP}, [&](const int* i) { return xcols(i[0], i[1]); }),
            pack({(d.JF + 127) / 128 * 128, D}, [&](const int* i) { return wout(i[0], i[1]); })};
}

// operand image of the fused token-mixing kernel (ls_long.hip), per-lane fragment order:
// img[l][q][mt][lane = s16 + 16 g][e] = Wt[l][16 mt + s16][16 q + 4 g + e], zero beyond S
Img lw_wtp(const Weights& w, const WeightDims& d, int tokpad) {
    return per_layer(d, [&](int l) { return tok_tiles(tokpad / 16, false, tok(w, d, l)); });
}

// operand images of the one-launch mixer (ls_mix_kernel.h).  wtok[l][q][mt][lane][e] = Wt[16 mt + s16][16 q + 4 e + g] (zero beyond S):
// the four lane groups of an MFMA k step read four CONSECUTIVE rows of the LDS operand; wch[l][gb][q][lane][j] = W'[16 gb + s16][16 q + 4 g + j]
MixerImages mixer_images(const Weights& w, const Ln2Fold& f, const WeightDims& d) {
    return {per_layer(d, [&](int l) { return tok_tiles(10, true, tok(w, d, l)); }), per_layer(d, [&](int l) { return row_tiles(32, folded(f, l)); })};
}
// poseFinal inside the mixer: wpose[nb][q][lane][j] = Wout[16 nb + s16][16 q + 4 g + j], zero rows beyond JF
Img mx_wpose(const Weights& w, const WeightDims& d, int tiles) { return row_tiles(tiles, pose(w, d)); }

// Device images whose element order is the per-lane MFMA operand order of the fused step kernels (ls_step_kernel.h)
FusedImages fused_images(const Weights& w, const Ln2Fold& f, const WeightDims& d) {
    const int KS = (d.R + 31) / 32, KS1 = (d.S + 31) / 32, MQ1 = ((d.S + 3) / 4 + 3) / 4;
    const Mat wout = pose(w, d);
    auto ww = [&](int l) { return BlockDiag{w.layer[l].w_tok, d.S, d.R}; };
    FusedImages o;
    // wch_img[l][w][p][q][c2][lane][j] = W'[n = 64w + 16(2p+c2) + (lane&15)][k = 16q + 4(lane>>4) + j]
    o.wch_img = per_layer(d, [&](int l) { return wave_rows(32, folded(f, l)); });
    // bf16 images, operand order of v_mfma_f32_16x16x32_bf16: [l][w][p][q16][c2][lane][8 k].  W' = hi + mid + lo exactly, each
    // round-to-nearest-even: hi = bf16(W'), mid = bf16(W' - hi), lo = bf16(W' - hi - mid) (both differences are exact in fp32).
    // bf16x3 uses hi and mid (its "lo" plane, wch_lo_img); split-fp32 (k_step PREC 2) all three.
    split_bf16(per_layer(d, [&](int l) {
                   return pack({kWaves, 2, 16, 2, 64, 8}, [&, m = folded(f, l)](const int* i) {
                       return m(64 * i[0] + 16 * (2 * i[1] + i[3]) + s16(i[4]), 32 * i[2] + 8 * g4(i[4]) + i[5]);
                   });
               }), {&o.wch_hi_img, &o.wch_lo_img, &o.wch_lo2_img});
    // ww_img[l][t][m][lane] = WW[r = 16t + (lane&15)][r' = 4m + (lane>>4)], WW = blockdiag(Wt, Wt) on packed rows
    o.ww_img = per_layer(d, [&](int l) { return pack({kNT, d.MK, 64}, [&, m = ww(l)](const int* i) { return m(16 * i[0] + s16(i[2]), 4 * i[1] + g4(i[2])); }); });
    // bf16x3 token-mix images: [l][t][ks][lane][e] = WW[r = 16t + (lane&15)][r' = 32ks + 8(lane>>4) + e]
    split_bf16(per_layer(d, [&](int l) { return bf16_tiles(kNT, KS, ww(l)); }), {&o.ww_hi_img, &o.ww_lo_img});
    // btok_rows[l][r] = b1[r % S] on the R packed rows (80 per layer, zero beyond R)
    o.btok_rows = per_layer(d, [&](int l) { return pack({80}, [&](const int* i) { return i[0] < d.R ? w.layer[l].b_tok[i[0] % d.S] : 0.f; }); });
    // wtail[l][k][i] = Wt[32 + i][k] (zero beyond the last row): the A operand of the ragged rows' 4x4x1 MFMAs (ls_pass_kernel.h)
    o.wtail = per_layer(d, [&](int l) { return pack({d.S, 4}, [&, m = tok(w, d, l)](const int* i) { return m(32 + i[1], i[0]); }); });
    // wtok1_hi / lo [l][t][ks][lane][e] = Wt[r = 16t + (lane&15)][r' = 32ks + 8(lane>>4) + e] of ONE pass as bf16 hi / lo planes (ls_pass_kernel.h)
    split_bf16(per_layer(d, [&](int l) { return bf16_tiles(3, KS1, tok(w, d, l)); }), {&o.wtok1_hi_img, &o.wtok1_lo_img});
    // wtok1_img[l][t][mq][lane][j] = Wt[r = 16t + (lane&15)][r' = 4(4mq + j) + (lane>>4)] of ONE pass, zero outside S x S (ls_coop_kernel.h)
    o.wtok1_img = per_layer(d, [&](int l) {
        return pack({3, MQ1, 64, 4}, [&, m = tok(w, d, l)](const int* i) { return m(16 * i[0] + s16(i[2]), 4 * (4 * i[1] + i[3]) + g4(i[2])); });
    });
    // winx_img: the x_t columns of input_mapping (RAG.py:62) in wch_img's order with KXQ k tiles, zero beyond JF
    o.winx_img = wave_rows(d.KXQ, Mat{w.w_in, D, d.JF, d.KIN});
    // wout_img[ob][q][lane][j] = Wout[c = 16ob + (lane&15)][k = 16q + 4(lane>>4) + j], zero rows beyond JF; bout likewise padded to NOB tiles
    o.wout_img = row_tiles(d.NOB, wout);
    o.bout = pack({d.NOB * 16}, [&](const int* i) { return i[0] < d.JF ? w.b_out[i[0]] : 0.f; });
    // wout_reg_img[w][ob][cb][lane][j] = Wout[c = 16ob + (lane&15)][k = 64w + 16cb + 4(lane>>4) + j]: the k order in which
    // wave w's residual registers X[cb][.][j] present the hidden state as an MFMA B operand
    o.wout_reg_img = pack({kWaves, d.NOB, kCB, 64, 4}, [&](const int* i) { return wout(16 * i[1] + s16(i[3]), 64 * i[0] + 16 * i[2] + 4 * g4(i[3]) + i[4]); });
    return o;
}

// Weights of the once-per-call stage that are not uploaded as they are: the same for the fused (34-frame) and the long-sequence path
CallImages call_images(const Weights& w, const WeightDims& d) {
    CallImages o;
    // the static columns JF.. of input_mapping, split by the features they multiply: [prefix poses | bit] (shared by both CFG
    // passes; zero-padded to a whole number of K tiles so the projection takes the GEMM's fast path) and the 256 audio columns
    // (cond pass only)
    const Mat pre{w.w_in + d.JF, D, d.JF + 1, d.KIN}, aud{w.w_in + 2 * d.JF + 1, D, kAudioFeat, d.KIN};
    o.win_pre = pack({D, d.KPP}, [&](const int* i) { return pre(i[0], i[1]); });
    o.win_aud = pack({D, kAudioFeat}, [&](const int* i) { return aud(i[0], i[1]); });
    // stride-6 conv layers (ls_conv.hip): image [co tile][chunk][k][lane][cig] = W[co = 16*ct + (lane&15)][ci = 16*chunk + 4*cig + (lane>>4)][k]
    for (int c = 1; c < 4; ++c)
        o.conv_img[c] = pack({kConvCout[c] / 16, kConvCin[c] / 16, 15, 64, 4}, [&, cw = w.conv_w[c], Cin = kConvCin[c]](const int* i) {
            return cw[((size_t)(16 * i[0] + s16(i[3])) * Cin + 16 * i[1] + 4 * i[4] + g4(i[3])) * 15 + i[2]];
        });
    // speaker_mu and speaker_logvar as ONE [1024][256] projection (rows 0..511 mu, 512..1023 logvar): one launch instead of three
    o.ml_w.assign(w.mu_w, w.mu_w + (size_t)D * 256);
    o.ml_w.insert(o.ml_w.end(), w.lv_w, w.lv_w + (size_t)D * 256);
    o.ml_b.assign(w.mu_b, w.mu_b + D);
    o.ml_b.insert(o.ml_b.end(), w.lv_b, w.lv_b + D);
    return o;
}

}  // namespace ls
