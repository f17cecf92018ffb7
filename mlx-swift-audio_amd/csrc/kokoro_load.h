// kokoro_load.h -- what both Kokoro handles (kokoro.hip, kokoro_text.hip) share on the host: the tap-GEMM form of a convolution, the
// loader of weight-normed convolutions (fold + ConvWeighted's orientation rule, see kokoro.hip) and the checked tap-GEMM launch.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "codec.h"
#include "mia_internal.h"
#include "tensor_loader.h"

inline int pad32(int c) { return (c + 31) / 32 * 32; }

struct KConv {
  float* w = nullptr; float* b = nullptr;
  int N = 0, Cin = 0, taps = 1, dil = 1, pad = 0, stride = 1;   // N, Cin: padded to 32 unless the loader was told to keep N
  int K = 0;                                                    // transposed conv: kernel size (taps = ceil(K / stride))
  uint16_t* w16 = nullptr;                                      // bf16 copy of w (mia_kokoro_use_w16), null in the text and ALBERT handles
  size_t w_elems() const { return (size_t)(K ? stride : 1) * N * taps * Cin; }     // a transposed conv holds `stride` phases
};

struct KConvLoader : TensorLoader {
  // weight-normed tensor `p`.weight_v / weight_g, folded, as stored
  bool folded(const std::string& p, std::vector<float>& w, int64_t d0, int64_t d1, int64_t d2) {
    std::vector<float> v, g;
    if (!f32(p + ".weight_v", v, {d0, d1, d2}) || !f32(p + ".weight_g", g, {d0, 1, 1})) return false;
    const int64_t inner = d1 * d2;
    w.resize(v.size());
    for (int64_t i = 0; i < d0; ++i) {
      float ss = 0.f;
      for (int64_t k = 0; k < inner; ++k) ss += v[i * inner + k] * v[i * inner + k];
      const float nrm = std::sqrt(ss) + 1e-7f;
      for (int64_t k = 0; k < inner; ++k) w[i * inner + k] = v[i * inner + k] / nrm * g[i];
    }
    return true;
  }
  // the folded weight as [Cout][K][Cin] by ConvWeighted's rule: as stored when the stored last axis is Cin, all axes reversed otherwise
  bool oriented(const std::string& p, std::vector<float>& w, int Cout, int K, int Cin) {
    const mia_tensor_view* t = find(p + ".weight_v");
    if (!t) return fail(MIA_ERR_INVALID_ARGUMENT, "missing tensor '" + p + ".weight_v'");
    if (t->ndim == 3 && t->shape[2] == Cin) return folded(p, w, Cout, K, Cin);
    std::vector<float> s;
    if (!folded(p, s, Cin, K, Cout)) return false;
    w.resize(s.size());
    for (int ci = 0; ci < Cin; ++ci) for (int k = 0; k < K; ++k) for (int co = 0; co < Cout; ++co)
      w[((size_t)co * K + k) * Cin + ci] = s[((size_t)ci * K + k) * Cout + co];
    return true;
  }
  bool bias_of(const std::string& p, bool has, int Cout, int Np, std::vector<float>& b) {
    b.assign(Np, 0.f);
    if (!has) return true;
    std::vector<float> t;
    if (!f32(p + ".bias", t, {Cout})) return false;
    std::copy(t.begin(), t.end(), b.begin());
    return true;
  }
  // [Cout][K][Cin] -> tap-GEMM weights [Np][K][Cp], zero rows / columns for the padding
  void place(const std::vector<float>& w, const std::vector<float>& b, int Cout, int K, int Cin, bool keepN, int dil, int pad, int stride, KConv& o) {
    const int Cp = pad32(Cin), Np = keepN ? Cout : pad32(Cout);
    std::vector<float> wp((size_t)Np * K * Cp, 0.f);
    for (int co = 0; co < Cout; ++co) for (int k = 0; k < K; ++k) for (int ci = 0; ci < Cin; ++ci)
      wp[((size_t)co * K + k) * Cp + ci] = w[((size_t)co * K + k) * Cin + ci];
    std::vector<float> bp(b); bp.resize(Np, 0.f);
    o.w = up(wp); o.b = up(bp); o.N = Np; o.Cin = Cp; o.taps = K; o.dil = dil; o.pad = pad; o.stride = stride;
  }
  bool conv_wn(const std::string& p, int Cout, int K, int Cin, int dil, int pad, bool has_bias, bool keepN, KConv& o) {
    std::vector<float> w, b;
    if (!oriented(p, w, Cout, K, Cin) || !bias_of(p, has_bias, Cout, Cout, b)) return false;
    place(w, b, Cout, K, Cin, keepN, dil, pad, 1, o);
    return true;
  }
};

struct COpt { const float* R = nullptr; int64_t ldr = 0; const float* R2 = nullptr; float scale = 0.f; float lrelu = 0.f; int64_t ldy = 0; };

// the checked tap-GEMM launch on the fp32 weights, or (w16: the decoder handle's switch) on their bf16 copies
inline int kconv_launch(mia_ctx* ctx, ConvGemmArgs& g, const KConv& c, int phases, bool w16) {
  if (!w16) { g.W = c.w; return codec_conv_gemm_run(ctx, g, phases, "kokoro"); }
  if (!c.w16) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro: a convolution has no bf16 copy of its weights");
  return conv_gemm_w16_run(ctx, g, c.w16, phases, "kokoro");
}

inline int kconv_run(mia_ctx* ctx, const KConv& c, const float* X, int64_t T_in, float* Y, int64_t T_out, const COpt& o = COpt(), bool w16 = false) {
  ConvGemmArgs g;
  g.X = X; g.ldx = c.Cin; g.T_in = (int)T_in; g.bias = c.b; g.lrelu_slope = o.lrelu;
  g.Y = Y; g.ldy = o.ldy ? o.ldy : c.N; g.T_out = (int)T_out; g.R = o.R; g.R2 = o.R2; g.ldr = o.ldr ? o.ldr : c.N; g.out_scale = o.scale;
  g.M = (int)T_out; g.N = c.N; g.Cin = c.Cin; g.taps = c.taps; g.dil = c.dil; g.pad = c.pad; g.x_row_mul = c.stride;
  return kconv_launch(ctx, g, c, 1, w16);
}
