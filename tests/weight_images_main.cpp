// Host-only driver of csrc/ls_weights.cpp for tests/test_weight_images_host.py: fills a state dict for a named configuration from an
// integer hash, resolves it, builds every image that configuration uploads and writes each to <dir>/<DevBuf member>.bin (tokpad and
// mx_npt as text).  usage: weight_images <config> <dir> [drop <key> | resize <key>]; a resolver fault prints its message and exits 2.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "ls_hip.h"
#include "ls_weights.h"

using namespace ls;

namespace {

struct Config { const char* name; int njoints, nfeats, npre, nframes, layers, n_emotions; bool mixer; };
const Config kConfigs[] = {
    {"ted", 9, 3, 1, 34, 2, 0, false},
    {"beat", 47, 6, 2, 34, 2, 8, false},
    {"beat150", 47, 6, 2, 150, 2, 8, true},
    {"ted200", 9, 3, 1, 200, 1, 0, false},
};
constexpr int kSpeakers = 5;

// the handle's derived shape (ls_create)
WeightDims dims_of(const Config& c) {
    WeightDims d{};
    d.L = c.layers; d.JF = c.njoints * c.nfeats; d.S = c.nframes + c.npre; d.R = 2 * d.S; d.MK = (d.R + 3) / 4;
    d.NOB = (d.JF + 15) / 16; d.KXQ = (d.JF + 15) / 16; d.JFP = (d.JF + 31) / 32 * 32;
    d.KIN = 2 * d.JF + 1 + kAudioFeat; d.KPP = (d.JF + 1 + 31) / 32 * 32;
    d.n_speakers = kSpeakers; d.n_emotions = c.n_emotions;
    d.fused = c.nframes == kT; d.mixer = c.mixer;
    return d;
}

// element `i` of the key with ordinal `ord`: a fixed integer hash mapped to [-1, 1)
float value(uint32_t ord, uint32_t i) {
    uint32_t x = ord * 0x9E3779B9u + i * 0x85EBCA6Bu + 0x27D4EB2Fu;
    x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
    return (float)(int32_t)(x >> 8) * (1.0f / 8388608.0f) - 1.0f;
}

WeightMap make_weights(const WeightDims& d) {
    WeightMap m;
    uint32_t ord = 0;
    auto add = [&](const std::string& key, size_t n) {
        std::vector<float>& v = m[key];
        v.resize(n);
        for (size_t i = 0; i < n; ++i) v[i] = value(ord, (uint32_t)i);
        ++ord;
    };
    const size_t D = kD, S = d.S, JF = d.JF;
    for (int l = 0; l < d.L; ++l) {
        add(layer_key(l, "block2.1.weight"), D * D); add(layer_key(l, "block2.1.bias"), D);
        add(layer_key(l, "block1.1.weight"), S * S); add(layer_key(l, "block1.1.bias"), S);
        for (const char* s : {"block1.0.alpha", "block1.0.beta", "block2.0.alpha", "block2.0.beta"}) add(layer_key(l, s), D);
    }
    add("input_mapping.weight", D * d.KIN); add("output_process.poseFinal.weight", JF * D); add("output_process.poseFinal.bias", JF);
    add("input_mapping.bias", D);
    for (int i = 0; i < 4; ++i) { add(conv_key(i, "weight"), (size_t)kConvCout[i] * kConvCin[i] * 15); add(conv_key(i, "bias"), kConvCout[i]); }
    add("speaker_embedding.weight", (size_t)d.n_speakers * 256);
    for (const char* s : {"speaker_mu", "speaker_logvar"}) { add(std::string(s) + ".weight", D * 256); add(std::string(s) + ".bias", D); }
    for (const char* s : {"0", "2"}) {
        add(std::string("backbone.embed_timestep.time_embed.") + s + ".weight", D * D);
        add(std::string("backbone.embed_timestep.time_embed.") + s + ".bias", D);
    }
    if (d.n_emotions > 0) add("emotion_embedding.weight", (size_t)d.n_emotions * D);
    return m;
}

std::string g_dir;
void put(const std::string& name, const void* p, size_t bytes) {
    std::ofstream f(g_dir + "/" + name + ".bin", std::ios::binary);
    f.write(static_cast<const char*>(p), (std::streamsize)bytes);
}
template <class T>
void put(const std::string& name, const std::vector<T>& v) { put(name, v.data(), v.size() * sizeof(T)); }
void put_text(const std::string& name, int v) { std::ofstream(g_dir + "/" + name + ".txt") << v << "\n"; }

// ---- what ls_api.cpp's build_images uploads, buffer by buffer
int write_images(const WeightMap& m, const WeightDims& d) {
    Weights w;
    std::string msg;
    if (resolve_weights(m, d, w, msg) != LS_OK) { printf("%s\n", msg.c_str()); return 2; }
    const size_t D = kD;
    const LongImages lg = long_images(w, d);
    const Ln2Fold f = fold_ln2(w, d);
    put("lw_wt", lg.lw_wt); put("lw_bt", lg.lw_bt); put("lw_wc", lg.lw_wc); put("lw_bc", lg.lw_bc); put("lw_winx", lg.lw_winx); put("lw_wout", lg.lw_wout);
    put("ln1a", lg.ln1a); put("ln1b", lg.ln1b); put("ln2a", lg.ln2a); put("ln2b", lg.ln2b);
    if (d.S <= 160) {
        const int tokpad = d.S <= 48 ? 48 : 160;
        put("lw_wtp", lw_wtp(w, d, tokpad)); put_text("tokpad", tokpad);
        put("lw_wcf", f.w); put("lw_bcf", f.b); put("lw_wsum", f.wsum);
    }
    if (d.mixer) {
        const MixerImages mx = mixer_images(w, f, d);
        put("mx_wtok", mx.mx_wtok); put("mx_wch", mx.mx_wch);
    }
    const int npt = d.mixer && (d.JF + 15) / 16 <= 20 ? (d.JF + 15) / 16 : 0;
    if (npt > 0) put("mx_wpose", mx_wpose(w, d, npt));
    put_text("mx_npt", npt);
    if (d.fused) {
        const FusedImages fu = fused_images(w, f, d);
        put("wch_hi_img", fu.wch_hi_img); put("wch_lo_img", fu.wch_lo_img); put("wch_lo2_img", fu.wch_lo2_img); put("ww_hi_img", fu.ww_hi_img);
        put("ww_lo_img", fu.ww_lo_img); put("wtok1_hi_img", fu.wtok1_hi_img); put("wtok1_lo_img", fu.wtok1_lo_img);
        put("wch_img", fu.wch_img); put("bch", f.b); put("wtail", fu.wtail); put("ww_img", fu.ww_img); put("wtok1_img", fu.wtok1_img);
        put("btok_rows", fu.btok_rows); put("winx_img", fu.winx_img); put("wout_img", fu.wout_img); put("wout_reg_img", fu.wout_reg_img); put("bout", fu.bout);
    } else {
        put("bout", w.b_out, (size_t)d.JF * 4);
    }
    const CallImages ca = call_images(w, d);
    put("win_bias", w.b_in, D * 4); put("win_pre", ca.win_pre); put("win_aud", ca.win_aud);
    for (int i = 0; i < 4; ++i) {
        const std::string n = std::to_string(i);
        put("conv_w" + n, w.conv_w[i], (size_t)kConvCout[i] * kConvCin[i] * 15 * 4); put("conv_b" + n, w.conv_b[i], (size_t)kConvCout[i] * 4);
        if (i > 0) put("conv_img" + n, ca.conv_img[i]);
    }
    put("spk_emb", w.spk_emb, (size_t)d.n_speakers * 256 * 4); put("ml_w", ca.ml_w); put("ml_b", ca.ml_b);
    put("te_w0", w.te_w0, D * D * 4); put("te_b0", w.te_b0, D * 4); put("te_w2", w.te_w2, D * D * 4); put("te_b2", w.te_b2, D * 4);
    if (d.n_emotions > 0) put("emo_emb", w.emo_emb, (size_t)d.n_emotions * D * 4);
    return 0;
}
// ---- end of the images

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3 && argc != 5) { fprintf(stderr, "usage: %s <config> <dir> [drop <key> | resize <key>]\n", argv[0]); return 1; }
    const Config* c = nullptr;
    for (const Config& k : kConfigs) if (!strcmp(k.name, argv[1])) c = &k;
    if (!c) { fprintf(stderr, "unknown configuration '%s'\n", argv[1]); return 1; }
    g_dir = argv[2];
    const WeightDims d = dims_of(*c);
    WeightMap m = make_weights(d);
    if (argc == 5) {
        if (!m.count(argv[4])) { fprintf(stderr, "no key '%s'\n", argv[4]); return 1; }
        if (!strcmp(argv[3], "drop")) m.erase(argv[4]);
        else if (!strcmp(argv[3], "resize")) m[argv[4]].push_back(0.f);
        else { fprintf(stderr, "unknown fault '%s'\n", argv[3]); return 1; }
    }
    return write_images(m, d);
}
