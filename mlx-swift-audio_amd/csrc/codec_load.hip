// codec_load.hip -- SNAC / DAC checkpoints -> layer programs (codec_model.h): weight-norm folding, the kernels' weight layouts, upload.
#include <cmath>
#include <string>

#include "codec_model.h"
#include "tensor_loader.h"

namespace {

struct CodecLoader : TensorLoader {
  bool channels_mid = false;   // snake alphas are stored [1][C][1] (SNAC) or [1][1][C] (DAC)

  // g * v / (||v|| + 1e-12): v is [A][B][C]; the norm runs over every axis except `keep`; g has one entry per index of `keep`
  static void fold_wn(std::vector<float>& v, const std::vector<float>& g, int A, int B, int C, int keep) {
    const int n = keep == 0 ? A : (keep == 1 ? B : C);
    std::vector<double> ss(n, 0.0);
    for (int a = 0; a < A; ++a) for (int b = 0; b < B; ++b) for (int cc = 0; cc < C; ++cc) {
      const float x = v[((size_t)a * B + b) * C + cc];
      ss[keep == 0 ? a : (keep == 1 ? b : cc)] += (double)x * x;
    }
    for (int a = 0; a < A; ++a) for (int b = 0; b < B; ++b) for (int cc = 0; cc < C; ++cc) {
      const int k = keep == 0 ? a : (keep == 1 ? b : cc);
      float& x = v[((size_t)a * B + b) * C + cc];
      x = g[k] * x / ((float)std::sqrt((float)ss[k]) + 1e-12f);
    }
  }
  float* alpha(const std::string& n, int C) {
    std::vector<float> a;
    if (channels_mid) { if (!f32(n, a, {1, C, 1})) return nullptr; }
    else { if (!f32(n, a, {1, 1, C})) return nullptr; }
    return up(a);
  }
  // weight-normed Conv1d stored as v [Cout][K][Cin_g], g [Cout][1][1] -> dense tap-GEMM weights [Cout][K*Cin]
  bool dense_conv(const std::string& p, int Cout, int K, int Cin, bool bias, Op& op) {
    std::vector<float> v, g, b;
    if (!f32(p + ".weight_v", v, {Cout, K, Cin}) || !f32(p + ".weight_g", g, {Cout, 1, 1})) return false;
    fold_wn(v, g, Cout, K, Cin, 0);
    op.w = up(v); op.N = Cout; op.Cin = Cin; op.taps = K;
    if (bias) { if (!f32(p + ".bias", b, {Cout})) return false; op.b = up(b); }
    return true;
  }
  // depthwise Conv1d: v [C][K][1] -> [K][C]
  bool dw_conv(const std::string& p, int C, int K, Op& op) {
    std::vector<float> v, g, b;
    if (!f32(p + ".weight_v", v, {C, K, 1}) || !f32(p + ".weight_g", g, {C, 1, 1}) || !f32(p + ".bias", b, {C})) return false;
    fold_wn(v, g, C, K, 1, 0);
    std::vector<float> t((size_t)K * C);
    for (int cc = 0; cc < C; ++cc) for (int k = 0; k < K; ++k) t[(size_t)k * C + cc] = v[(size_t)cc * K + k];
    op.w = up(t); op.b = up(b); op.N = C; op.Cin = C; op.taps = K;
    return true;
  }
  // transposed conv, kernel 2*stride, given as effective MLX weight w[co][k][ci] -> per output phase r: [co][ x[t-1] tap: k=r+s | x[t] tap: k=r ][ci]
  void convt_phases(const std::vector<float>& wm, int Cout, int K, int Cin, int s, Op& op) {
    std::vector<float> ph((size_t)s * Cout * 2 * Cin);
    for (int r = 0; r < s; ++r) for (int co = 0; co < Cout; ++co) for (int ci = 0; ci < Cin; ++ci) {
      ph[(((size_t)r * Cout + co) * 2 + 0) * Cin + ci] = wm[((size_t)co * K + (r + s)) * Cin + ci];
      ph[(((size_t)r * Cout + co) * 2 + 1) * Cin + ci] = wm[((size_t)co * K + r) * Cin + ci];
    }
    op.w = up(ph); op.N = Cout; op.Cin = Cin; op.taps = 2; op.stride = s;
  }
  // upsample block head at prefix b: snake (b0) + weight-normed transposed conv (b1), kernel 2 s, normalised per INPUT channel.
  // cin_first: the weight is stored [Cin][K][Cout] with g [Cin][1][1] (SNAC; permuted to MLX [Cout][K][Cin] here), else already
  // [Cout][K][Cin] with g [1][1][Cin] (DAC: exceptDim 2, DACLayers.swift:161,173)
  void upsample(const std::string& b, int Cin, int Cout, int s, bool cin_first, std::vector<Op>& ops) {
    const int K = 2 * s;
    Op ct; ct.kind = OP_CONVT; ct.pad = (s + 1) / 2;
    ct.a_pre = alpha(b + "0.alpha", Cin);
    std::vector<float> v, g, bias;
    const bool ok = cin_first ? f32(b + "1.weight_v", v, {Cin, K, Cout}) && f32(b + "1.weight_g", g, {Cin, 1, 1})
                              : f32(b + "1.weight_v", v, {Cout, K, Cin}) && f32(b + "1.weight_g", g, {1, 1, Cin});
    if (ok && f32(b + "1.bias", bias, {Cout})) {
      if (cin_first) {
        fold_wn(v, g, Cin, K, Cout, 0);
        std::vector<float> wm((size_t)Cout * K * Cin);
        for (int ci = 0; ci < Cin; ++ci) for (int k = 0; k < K; ++k) for (int co = 0; co < Cout; ++co)
          wm[((size_t)co * K + k) * Cin + ci] = v[((size_t)ci * K + k) * Cout + co];
        v.swap(wm);
      } else fold_wn(v, g, Cout, K, Cin, 2);
      convt_phases(v, Cout, K, Cin, s, ct);
      ct.b = up(bias);
    }
    ops.push_back(ct);
  }
  // output stage: snake + conv7 (C -> 1) + tanh
  void out_conv(const std::string& alpha_name, const std::string& conv, int C, std::vector<Op>& ops) {
    Op o; o.kind = OP_OUT1; o.a_pre = alpha(alpha_name, C);
    dense_conv(conv, 1, 7, C, true, o);
    ops.push_back(o);
  }
  void residual_unit_snac(const std::string& p, int C, int dil, std::vector<Op>& ops) {
    Op dw; dw.kind = OP_DW; dw.residual = true; dw.dil = dil;
    dw.a_pre = alpha(p + ".block.layers.0.alpha", C);
    dw_conv(p + ".block.layers.1", C, 7, dw);
    dw.a_post = alpha(p + ".block.layers.2.alpha", C);
    ops.push_back(dw);
    Op pw; pw.kind = OP_CONV; pw.residual = true;
    dense_conv(p + ".block.layers.3", C, 1, C, true, pw);
    ops.push_back(pw);
  }
  // h = conv7_dilated(snake(x)) into the side buffer (x stays the stream); x += conv1x1(snake(h))
  void residual_unit_dac(const std::string& p, int C, int dil, std::vector<Op>& ops) {
    Op c1; c1.kind = OP_CONV; c1.side = true; c1.dil = dil; c1.pad = 3 * dil;
    c1.a_pre = alpha(p + ".block.layers.0.alpha", C);
    dense_conv(p + ".block.layers.1", C, 7, C, true, c1);
    Op c2; c2.kind = OP_CONV; c2.residual = true;
    c2.a_pre = alpha(p + ".block.layers.2.alpha", C);
    dense_conv(p + ".block.layers.3", C, 1, C, true, c2);
    ops.push_back(c1);
    ops.push_back(c2);
  }
  bool quantizers(mia_codec* c, int n, int latent, int cb_size, int cb_dim) {
    c->n_levels = n; c->latent = latent; c->cb_size = cb_size; c->cb_dim = cb_dim;
    for (int i = 0; i < n; ++i) {
      const std::string q = "quantizer.quantizers." + std::to_string(i);
      std::vector<float> cb, g, v, b;
      if (!f32(q + ".codebook.weight", cb, {cb_size, cb_dim}) || !f32(q + ".out_proj.weight_g", g, {latent, 1, 1}) ||
          !f32(q + ".out_proj.weight_v", v, {latent, 1, cb_dim}) || !f32(q + ".out_proj.bias", b, {latent})) return false;
      fold_wn(v, g, latent, 1, cb_dim, 0);     // per output channel over the codebook dim (SNACDecoder.swift:374-377)
      c->codebook[i] = up(cb); c->weff[i] = up(v); c->ebias[i] = up(b);
    }
    return true;
  }
};

CodecLoader make_loader(mia_codec* c, const mia_tensor_view* tensors, int n_tensors) {
  CodecLoader L; L.allocs = &c->allocs; L.channels_mid = c->kind == 0; L.index(tensors, n_tensors);
  return L;
}

mia_codec* codec_fail(mia_ctx* ctx, mia_codec* c, const std::string& m) {
  ctx->err = "codec_load: " + m;
  if (c) mia_codec_free(c);
  return nullptr;
}

const int DILS[3] = {1, 3, 9};

}  // namespace

extern "C" void mia_codec_free(mia_codec* c) {
  if (!c) return;
  (void)hipSetDevice(c->ctx->device);
  (void)hipStreamSynchronize(c->ctx->stream);
  for (void* p : c->allocs) (void)hipFree(p);
  for (void* p : {(void*)c->buf[0], (void*)c->buf[1], (void*)c->buf[2], (void*)c->d_codes, (void*)c->d_noise, (void*)c->d_pcm, c->d_tab,
                  (void*)c->d_audio, (void*)c->d_ze})
    if (p) (void)hipFree(p);
  if (c->h_tab) (void)hipHostFree(c->h_tab);
  if (c->tab_ev) (void)hipEventDestroy(c->tab_ev);
  delete c;
}

extern "C" mia_codec* mia_snac_load(mia_ctx* ctx, const mia_snac_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors || n_tensors <= 0) return codec_fail(ctx, nullptr, "null arguments");
  if (cfg->n_rates <= 0 || cfg->n_rates > MIA_CODEC_MAX_RATES || cfg->n_vq <= 0 || cfg->n_vq > MIA_MAX_LEVELS) return codec_fail(ctx, nullptr, "bad SNAC config");
  if (cfg->latent_dim % 32 || cfg->decoder_dim % 32 || (cfg->decoder_dim >> cfg->n_rates) % 4) return codec_fail(ctx, nullptr, "SNAC channel counts must be multiples of 32");
  if (!cfg->depthwise) return codec_fail(ctx, nullptr, "only the depthwise SNAC variant (snac_24khz) is supported");
  if (hipSetDevice(ctx->device) != hipSuccess) return codec_fail(ctx, nullptr, "hipSetDevice failed");
  mia_codec* c = new mia_codec(); c->ctx = ctx; c->kind = 0;
  CodecLoader L = make_loader(c, tensors, n_tensors);
  for (int i = 0; i < cfg->n_vq; ++i) c->vq_stride[i] = cfg->vq_strides[i];
  L.quantizers(c, cfg->n_vq, cfg->latent_dim, cfg->codebook_size, cfg->codebook_dim);
  const std::string P = "decoder.model.layers.";
  { Op dw; dw.kind = OP_DW; L.dw_conv(P + "0", cfg->latent_dim, 7, dw); c->ops.push_back(dw); }
  { Op pw; pw.kind = OP_CONV; L.dense_conv(P + "1", cfg->decoder_dim, 1, cfg->latent_dim, true, pw); c->ops.push_back(pw); }
  int Cin = cfg->decoder_dim;
  for (int i = 0; i < cfg->n_rates && L.err.empty(); ++i) {
    const int Cout = cfg->decoder_dim >> (i + 1), s = cfg->decoder_rates[i];
    if (s % 2) return codec_fail(ctx, c, "SNAC decoder rates must be even (the reference drops output_padding, ConvWeightedTranspose1d.swift:86-93)");
    const std::string b = P + std::to_string(2 + i) + ".block.layers.";
    L.upsample(b, Cin, Cout, s, true, c->ops);
    int ru = 2;
    if (cfg->noise) {
      // NoiseBlock.linear: [Cn][1][Cout] with Cn = 1 (this port's init) or Cout (upstream SNAC checkpoints)
      const mia_tensor_view* tv = L.find(b + "2.linear.weight_v");
      const int Cn = tv && tv->ndim == 3 ? (int)tv->shape[0] : 1;
      std::vector<float> v, g;
      if (L.f32(b + "2.linear.weight_v", v, {Cn, 1, Cout}) && L.f32(b + "2.linear.weight_g", g, {Cn, 1, 1})) {
        CodecLoader::fold_wn(v, g, Cn, 1, Cout, 0);
        Op nz; nz.kind = Cn == 1 ? OP_NOISE1 : OP_NOISEC; nz.N = Cn; nz.Cin = Cout; nz.w = L.up(v);
        if (Cn != 1 && Cn != Cout) return codec_fail(ctx, c, "noise block must have 1 or C output channels");
        c->ops.push_back(nz);
      }
      ru = 3;
    }
    for (int r = 0; r < 3; ++r) L.residual_unit_snac(b + std::to_string(ru + r), Cout, DILS[r], c->ops);
    Cin = Cout;
  }
  L.out_conv(P + std::to_string(2 + cfg->n_rates) + ".alpha", P + std::to_string(3 + cfg->n_rates), Cin, c->ops);
  if (!L.err.empty()) return codec_fail(ctx, c, L.err);
  if (hipDeviceSynchronize() != hipSuccess) return codec_fail(ctx, c, "device error during upload");
  return c;
}

extern "C" mia_codec* mia_dac_load(mia_ctx* ctx, const mia_dac_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors || n_tensors <= 0) return codec_fail(ctx, nullptr, "null arguments");
  if (cfg->n_rates <= 0 || cfg->n_rates > MIA_CODEC_MAX_RATES || cfg->n_codebooks <= 0 || cfg->n_codebooks > MIA_MAX_LEVELS) return codec_fail(ctx, nullptr, "bad DAC config (at most 4 codebooks)");
  if (cfg->latent_dim % 32 || cfg->decoder_dim % 32 || (cfg->decoder_dim >> cfg->n_rates) % 32) return codec_fail(ctx, nullptr, "DAC channel counts must be multiples of 32");
  if (hipSetDevice(ctx->device) != hipSuccess) return codec_fail(ctx, nullptr, "hipSetDevice failed");
  mia_codec* c = new mia_codec(); c->ctx = ctx; c->kind = 1;
  c->stack_budget = c->stack_budget_default = INT64_MAX;
  CodecLoader L = make_loader(c, tensors, n_tensors);
  L.quantizers(c, cfg->n_codebooks, cfg->latent_dim, cfg->codebook_size, cfg->codebook_dim);
  const std::string P = "decoder.model.layers.";
  { Op c0; c0.kind = OP_CONV; c0.pad = 3; L.dense_conv(P + "0", cfg->decoder_dim, 7, cfg->latent_dim, true, c0); c->ops.push_back(c0); }
  int Cin = cfg->decoder_dim;
  for (int i = 0; i < cfg->n_rates && L.err.empty(); ++i) {
    const int Cout = cfg->decoder_dim >> (i + 1);
    const std::string b = P + std::to_string(1 + i) + ".block.layers.";
    L.upsample(b, Cin, Cout, cfg->decoder_rates[i], false, c->ops);
    for (int r = 0; r < 3; ++r) L.residual_unit_dac(b + std::to_string(2 + r), Cout, DILS[r], c->ops);
    Cin = Cout;
  }
  L.out_conv(P + std::to_string(1 + cfg->n_rates) + ".alpha", P + std::to_string(2 + cfg->n_rates), Cin, c->ops);
  if (!L.err.empty()) return codec_fail(ctx, c, L.err);
  if (hipDeviceSynchronize() != hipSuccess) return codec_fail(ctx, c, "device error during upload");
  return c;
}

// ---- DAC encoder + residual vector quantisation (Codec/DAC/DACModel.swift:13-86,284-296; DACQuantize.swift:54-116,147-190) -------------------
extern "C" int mia_dac_load_encoder(mia_codec* c, const mia_dac_encoder_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 1, "dac_load_encoder: handle is not a DAC model");
  MIA_CHECK_ARG(ctx, cfg && tensors && n_tensors > 0 && cfg->n_rates > 0 && cfg->n_rates <= 8, "dac_load_encoder: bad arguments");
  // the RVQ kernel keeps a projected vector in <= 15 registers (codec_vq_assign_launch) and the staging buffer is sized from cb_dim;
  // a stride-1 "rate" would not halve-pad like the reference's k = 2 s, pad = ceil(s / 2) convolution (DACModel.swift:15-38)
  MIA_CHECK_ARG(ctx, c->cb_dim >= 1 && c->cb_dim <= 15, "dac_load_encoder: codebook_dim %d not supported by the RVQ kernel (1..15)", c->cb_dim);
  for (int i = 0; i < cfg->n_rates; ++i)
    MIA_CHECK_ARG(ctx, cfg->encoder_rates[i] >= 2, "dac_load_encoder: encoder rate %d must be >= 2 (got %d)", i, cfg->encoder_rates[i]);
  MIA_CHECK_ARG(ctx, cfg->encoder_dim % 32 == 0 && (cfg->encoder_dim << cfg->n_rates) == c->latent,
                "dac_load_encoder: encoder_dim * 2^n_rates (%d) must equal the latent width (%d) and be a multiple of 32", cfg->encoder_dim << cfg->n_rates, c->latent);
  MIA_CHECK_ARG(ctx, !c->has_encoder, "dac_load_encoder: encoder already loaded");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  CodecLoader L = make_loader(c, tensors, n_tensors);
  const std::string E = "encoder.block.layers.";
  int C = cfg->encoder_dim;
  {  // first conv: 1 -> C channels, k7
    std::vector<float> v, g, b;
    if (L.f32(E + "0.weight_v", v, {C, 7, 1}) && L.f32(E + "0.weight_g", g, {C, 1, 1}) && L.f32(E + "0.bias", b, {C})) {
      CodecLoader::fold_wn(v, g, C, 7, 1, 0);
      c->enc_in_w = L.up(v); c->enc_in_b = L.up(b);
    }
  }
  // a failed load leaves no half-built encoder program behind: the handle stays a decoder and may be given the encoder again
  std::vector<Op> enc_ops;
  int hop = 1;
  for (int i = 0; i < cfg->n_rates && L.err.empty(); ++i) {
    const int st = cfg->encoder_rates[i];
    const std::string b = E + std::to_string(1 + i) + ".block.layers.";
    for (int r = 0; r < 3; ++r) L.residual_unit_dac(b + std::to_string(r), C, DILS[r], enc_ops);
    Op dn; dn.kind = OP_CONV; dn.stride = st; dn.pad = (st + 1) / 2;
    dn.a_pre = L.alpha(b + "3.alpha", C);
    L.dense_conv(b + "4", 2 * C, 2 * st, C, true, dn);
    enc_ops.push_back(dn);
    C *= 2; hop *= st;
  }
  {
    Op fin; fin.kind = OP_CONV; fin.pad = 1;
    fin.a_pre = L.alpha(E + std::to_string(1 + cfg->n_rates) + ".alpha", C);
    L.dense_conv(E + std::to_string(2 + cfg->n_rates), c->latent, 3, C, true, fin);
    enc_ops.push_back(fin);
  }
  for (int i = 0; i < c->n_levels && L.err.empty(); ++i) {
    const std::string q = "quantizer.quantizers." + std::to_string(i);
    c->in_proj[i].kind = OP_CONV;
    L.dense_conv(q + ".in_proj", c->cb_dim, 1, c->latent, true, c->in_proj[i]);
    std::vector<float> cb;
    if (!L.f32(q + ".codebook.weight", cb, {c->cb_size, c->cb_dim})) break;
    std::vector<float> sq(c->cb_size);
    for (int j = 0; j < c->cb_size; ++j) {      // l2Normalize (DACQuantize.swift:14-20) in float32, then the row's squared norm
      float ss = 0.f;
      for (int d = 0; d < c->cb_dim; ++d) { const float a = std::fabs(cb[(size_t)j * c->cb_dim + d]); ss += a * a; }
      const float nrm = std::max(std::sqrt(ss), 1e-12f);
      float s2 = 0.f;
      for (int d = 0; d < c->cb_dim; ++d) { float& x = cb[(size_t)j * c->cb_dim + d]; x = x / nrm; s2 += x * x; }
      sq[j] = s2;
    }
    c->cbn[i] = L.up(cb); c->cbn_sq[i] = L.up(sq);
  }
  if (!L.err.empty()) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "dac_load_encoder: %s", L.err.c_str());
  MIA_HIP(ctx, hipDeviceSynchronize());
  c->enc_ops.swap(enc_ops);
  c->hop = hop;
  c->enc_dim = cfg->encoder_dim;
  c->has_encoder = true;
  return MIA_OK;
}
