// mimi_model.h -- the Mimi handle, its loader helpers and the transformer program shared by the decode side (mimi.hip) and the
// optional encode side (mimi_encode.hip).
#pragma once
#include <string>
#include <vector>

#include "../../include/mia_mimi.h"
#include "codec.h"
#include "mimi.h"
#include "ops.h"
#include "tensor_loader.h"

constexpr int MIMI_MAX_RATIOS = 8;

struct MConv { float* w = nullptr; float* b = nullptr; int N = 0, Cin = 0, taps = 0; };                    // causal, dilation 1 (the stride is the caller's)
struct MConvT { float* w = nullptr; float* b = nullptr; int N = 0, Cin = 0, stride = 0; };                 // causal, kernel 2 * stride, phase weights
struct MLayer { float *ln1g, *ln1b, *ln2g, *ln2b, *win, *wout, *w1, *w2; };
struct SLayer { MConvT up; MConv c3, c1; };
struct ELayer { MConv c3, c1, down; int ratio = 0; };                                                    // SEANet encoder stage: residual block, then k = 2 r, stride r

// the encode side (Mimi.encode, Mimi.swift:174-182): present only when the checkpoint carries it
struct MimiEncoder {
  float *in_w = nullptr, *in_b = nullptr;             // input convolution [nfilters][ksize] (Cin = 1)
  ELayer el[MIMI_MAX_RATIOS];                         // in the order they run: ratios reversed
  MConv fin;
  std::vector<MLayer> layers;                         // encoder_transformer
  float* wdown = nullptr;                             // latent downsample [D][2 us][D], no bias
  float* wproj = nullptr;                             // [2 dq][D]: rvq_first.input_proj rows, then rvq_rest.input_proj rows
  float* c2 = nullptr;                                // [nq][bins]: ||e||^2 / 2 of the table `cb`
};

struct mia_mimi {
  mia_ctx* ctx = nullptr;
  mia_mimi_config cfg{};
  std::vector<void*> allocs;
  int D = 0, H = 0, L = 0, FF = 0, context = 0, us = 0, nq = 0, bins = 0, dq = 0, nr = 0;
  int64_t spf = 0;                                    // samples per frame
  float *cb = nullptr, *wfT = nullptr, *wrT = nullptr, *wup = nullptr;
  double* inv_freq = nullptr;
  std::vector<MLayer> layers;
  MConv init, fin;
  SLayer sl[MIMI_MAX_RATIOS];
  // a stream's carried convolution rows, one block of floats: offsets of each convolution's rows
  size_t st_z = 0, st_x = 0, st_up[MIMI_MAX_RATIOS] = {}, st_c3[MIMI_MAX_RATIOS] = {}, st_fin = 0, st_floats = 0;
  int live_streams = 0;
  bool has_encoder = false;
  MimiEncoder enc;
};

struct mia_mimi_stream {
  mia_mimi* m = nullptr;
  float* conv_state = nullptr;
  float* hist[2] = {nullptr, nullptr};
  size_t cap[2] = {0, 0};                             // rows per (layer, k | v) of each buffer
  int cur = 0;
  int64_t fill = 0, pos = 0;
  int n_q = -1;
  bool broken = false;                                // a launch failed after the state had been touched: reset first
};

struct MLoader : TensorLoader {
  bool conv(const std::string& p, int Cout, int K, int Cin, MConv& o) {
    std::vector<float> w, b;
    if (!f32(p + ".weight", w, {Cout, K, Cin}) || !f32(p + ".bias", b, {Cout})) return false;
    o.w = up(w); o.b = up(b); o.N = Cout; o.Cin = Cin; o.taps = K;
    return true;
  }
  // effective weight w[co][k][ci], k = 2 s: phase r holds [co][ x[t-1] tap: k = r + s | x[t] tap: k = r ][ci]
  bool convt(const std::string& p, int Cout, int s, int Cin, MConvT& o) {
    std::vector<float> w, b;
    if (!f32(p + ".weight", w, {Cout, 2 * s, Cin}) || !f32(p + ".bias", b, {Cout})) return false;
    std::vector<float> ph((size_t)s * Cout * 2 * Cin);
    for (int r = 0; r < s; ++r)
      for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci) {
          ph[(((size_t)r * Cout + co) * 2 + 0) * Cin + ci] = w[((size_t)co * 2 * s + r + s) * Cin + ci];
          ph[(((size_t)r * Cout + co) * 2 + 1) * Cin + ci] = w[((size_t)co * 2 * s + r) * Cin + ci];
        }
    o.w = up(ph); o.b = up(b); o.N = Cout; o.Cin = Cin; o.stride = s;
    return true;
  }
  // Linear weight [N][K], rows optionally scaled by a LayerScale vector (folded: scale * (W x) == (scale W) x up to one rounding)
  bool linear(const std::string& p, int N, int K, const std::string& scale, float*& o) {
    std::vector<float> w, sc;
    if (!f32(p + ".weight", w, {N, K})) return false;
    if (!scale.empty()) {
      if (!f32(scale, sc, {N})) return false;
      for (int n = 0; n < N; ++n) for (int k = 0; k < K; ++k) w[(size_t)n * K + k] *= sc[n];
    }
    o = up(w);
    return true;
  }
  bool vec(const std::string& p, int N, float*& o) { std::vector<float> v; if (!f32(p, v, {N})) return false; o = up(v); return true; }
  // output_proj [D][1][dq] -> transposed [dq][D]
  bool projT(const std::string& p, int D, int dq, float*& o) {
    std::vector<float> w;
    if (!f32(p, w, {D, 1, dq})) return false;
    std::vector<float> t((size_t)dq * D);
    for (int d = 0; d < D; ++d) for (int j = 0; j < dq; ++j) t[(size_t)j * D + d] = w[(size_t)d * dq + j];
    o = up(t);
    return true;
  }
  // the layers of one ProjectedTransformer ("decoder_transformer" / "encoder_transformer"), LayerScale folded into out_proj and linear2
  bool transformer(const std::string& name, const mia_mimi_config& g, std::vector<MLayer>& layers) {
    const int D = g.d_model, FF = g.dim_feedforward;
    layers.resize(g.n_layers);
    bool ok = true;
    for (int l = 0; l < g.n_layers && ok; ++l) {
      const std::string p = name + ".transformer.layers." + std::to_string(l) + ".";
      MLayer& y = layers[l];
      ok = vec(p + "norm1.weight", D, y.ln1g) && vec(p + "norm1.bias", D, y.ln1b) && vec(p + "norm2.weight", D, y.ln2g) && vec(p + "norm2.bias", D, y.ln2b) &&
           linear(p + "self_attn.in_proj", 3 * D, D, "", y.win) &&
           linear(p + "self_attn.out_proj", D, D, g.layer_scale ? p + "layer_scale_1.scale" : "", y.wout) &&
           linear(p + "gating.linear1", FF, D, "", y.w1) &&
           linear(p + "gating.linear2", D, FF, g.layer_scale ? p + "layer_scale_2.scale" : "", y.w2);
    }
    return ok;
  }
};

// the transformer's buffers of one call: nb / qkv / qb / ob / ff are P rows; kt / vt the keys and values of a whole-clip pass
struct MimiTfWork { float *nb, *qkv, *qb, *ob, *ff, *kt, *vt; };
// `layers` over the P rows of x, in place.  st == nullptr: full bidirectional attention at RoPE offset 0 (Mimi.decode, Mimi.encode);
// otherwise the pair-windowed attention against the stream's key history at its position.
int mimi_transformer_run(mia_mimi* m, const std::vector<MLayer>& layers, mia_mimi_stream* st, float* x, int64_t P, const MimiTfWork& w);

// mimi_encode.hip: loads the encode side when the tensors carry one (m->has_encoder); false = the load failed (L.err says why)
bool mimi_encoder_load(mia_mimi* m, MLoader& L);
