// The sampling handle's weights on the host: the reference's state dict resolved once to pointers (resolve_weights), and one pure
// function per group of device images -- the per-lane MFMA operand orders of the step-kernel families, the long-sequence kernels, the
// mixer and the WavEncoder.  No HIP call and no handle in here: ls_api.cpp's build_images uploads what these return, tests/weight_images_main.cpp
// writes it to files.  Also the WavEncoder geometry and the key spellers the sampling handle and the trainer share.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "ls_internal.h"

namespace ls {

// WavEncoder (audio_enc.py:9-20): four Conv1d(k = 15); feat_extractor.<kConvKey[i]> in the state dict
constexpr int kConvCin[4] = {1, 32, 64, 128}, kConvCout[4] = {32, 64, 128, 256}, kConvStride[4] = {5, 6, 6, 6}, kConvPad[4] = {1600, 0, 0, 0},
              kConvKey[4] = {0, 3, 6, 9};
inline std::string layer_key(int l, const char* s) { return "backbone.mlps." + std::to_string(l) + "." + s; }
inline std::string conv_key(int i, const char* s) { return "audio_encoder.feat_extractor." + std::to_string(kConvKey[i]) + "." + s; }

// the handle's shape, as far as the images depend on it (ls_create fills the handle's fields of the same names)
struct WeightDims {
    int L, S, R, JF, KIN, KPP, JFP, MK, KXQ, NOB, n_speakers, n_emotions;
    bool fused, mixer;      // the model has the fused step kernels (34 frames) / the one-launch mixer (ls_mix_kernel.h)
};

// one MLPblock (mlp_module.py:51-60): Linear(512,512) [out][in], Conv1d(S,S,1) [out tok][in tok][1], the two LayerNorms
struct LayerWeights { const float *w_ch, *b_ch, *w_tok, *b_tok, *ln1a, *ln1b, *ln2a, *ln2b; };
struct Weights {
    std::vector<LayerWeights> layer;
    const float *w_in, *w_out, *b_out, *b_in;                           // input_mapping [512][KIN] (RAG.py:62), poseFinal [JF][512] (RAG.py:203)
    const float *conv_w[4], *conv_b[4];
    const float *spk_emb, *mu_w, *mu_b, *lv_w, *lv_b;                   // RAG.py:65-69
    const float *te_w0, *te_b0, *te_w2, *te_b2;                         // mlp_module.py:129-133
    const float* emo_emb;                                               // scripts_beat/model/RAG.py:72; null without emotions
};
using WeightMap = std::map<std::string, std::vector<float>>;

// Every key the sampling handle reads, looked up and size-checked once.  LS_OK, or LS_ESTATE with `msg` naming the first faulty key.
// `w` points into `m`: valid until the map changes.
int resolve_weights(const WeightMap& m, const WeightDims& d, Weights& w, std::string& msg);

// LayerNorm 2 folded around the channel-mixing product: W' = W diag(alpha2) [L][512][512], b' = b + W beta2, wsum[n] = sum_k W'[n][k]
struct Ln2Fold { std::vector<float> w, b, wsum; };
Ln2Fold fold_ln2(const Weights& w, const WeightDims& d);

// The images, in groups that exist together; every member is named after the handle buffer it is uploaded to.
using Img = std::vector<float>;
using Img16 = std::vector<unsigned short>;                  // a bf16 plane
struct LongImages { Img lw_wt, lw_bt, lw_wc, lw_bc, ln1a, ln1b, ln2a, ln2b, lw_winx, lw_wout; };       // batch-level kernels: every model
struct MixerImages { Img mx_wtok, mx_wch; };
struct FusedImages {                                                                                    // 34-frame step kernels
    Img16 wch_hi_img, wch_lo_img, wch_lo2_img, ww_hi_img, ww_lo_img, wtok1_hi_img, wtok1_lo_img;
    Img wch_img, wtail, ww_img, wtok1_img, btok_rows, winx_img, wout_img, wout_reg_img, bout;
};
struct CallImages { Img win_pre, win_aud, conv_img[4], ml_w, ml_b; };                                   // once-per-call stage ([0] stays empty)
LongImages long_images(const Weights& w, const WeightDims& d);
Img lw_wtp(const Weights& w, const WeightDims& d, int tokpad);          // token axis padded to `tokpad` (a multiple of 16, >= S)
MixerImages mixer_images(const Weights& w, const Ln2Fold& f, const WeightDims& d);
Img mx_wpose(const Weights& w, const WeightDims& d, int tiles);         // poseFinal inside the mixer, `tiles` 16-column tiles
FusedImages fused_images(const Weights& w, const Ln2Fold& f, const WeightDims& d);
CallImages call_images(const Weights& w, const WeightDims& d);

}  // namespace ls
