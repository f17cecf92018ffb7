// codec.hip -- SNAC and DAC neural-codec decoders as layer programs over the fp32 kernels of codec_kernels.hip.
//
// Replaces SNACDecoder.decode(codes:) (TTS/Orpheus/SNAC/SNACDecoder.swift:250-289,328-407 with WNConv1d.swift:64-88,
// ConvWeightedTranspose1d.swift:70-100, ResidualUnit.swift:58-95, NoiseBlock.swift:27-41) and
// DACCodec.decodeFromCodes (Codec/DAC/DACModel.swift:303-306 -> DACQuantize.swift:192-220 -> DACModel.swift:120-164,
// DACLayers.swift).  Weight normalisation g*v/(||v||+1e-12) is folded ONCE at load (the reference recomputes it on every
// forward, WNConv1d.swift:73-74).  The Gaussian of SNAC's NoiseBlock is an explicit input (null = no noise).
#include <climits>
#include <cmath>
#include <cstdint>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "codec.h"
#include "mia_internal.h"

namespace {

enum OpKind { OP_CONV, OP_CONVT, OP_DW, OP_NOISE1, OP_NOISEC, OP_OUT1 };

struct Op {
  OpKind kind;
  float* w = nullptr;        // device weights in the kernel's layout
  float* b = nullptr;
  float* a_pre = nullptr;    // snake alpha applied to the input
  float* a_post = nullptr;   // snake alpha applied to the output (depthwise only)
  int N = 0, Cin = 0, taps = 1, dil = 1, pad = 0, stride = 1;
  bool residual = false;     // Y = X_res + conv(H)   (in place on the residual stream)
};

}  // namespace

struct mia_codec {
  mia_ctx* ctx = nullptr;
  int kind = 0;               // 0 = SNAC, 1 = DAC
  std::vector<void*> allocs;
  int n_levels = 0, cb_dim = 0, cb_size = 0, latent = 0;
  float* codebook[MIA_MAX_LEVELS] = {};
  float* weff[MIA_MAX_LEVELS] = {};
  float* ebias[MIA_MAX_LEVELS] = {};
  int vq_stride[MIA_MAX_LEVELS] = {1, 1, 1, 1};
  std::vector<Op> ops;
  // scratch (grow-only)
  float* buf[3] = {nullptr, nullptr, nullptr};
  size_t buf_floats = 0;
  int32_t* d_codes = nullptr; size_t codes_cap = 0;
  float* d_noise = nullptr; size_t noise_cap = 0;
  float* d_pcm = nullptr; size_t pcm_cap = 0;
  // per-call tables of the stacked decode (Stack below): pinned staging owned by the handle, so that the memory behind the upload
  // outlives it on every return path; tab_ev marks the last upload's end and is waited for before the staging is written again
  void* h_tab = nullptr; void* d_tab = nullptr; size_t tab_cap = 0;
  hipEvent_t tab_ev = nullptr;
  // bytes of activations up to which a stage of the batch entries runs stacked (mia_codec_set_stack_budget).  SNAC: the Infinity Cache;
  // DAC (mia_dac_load): no limit -- measured both ways, see decode_batch_enqueue
  int64_t stack_budget_default = 256ll << 20, stack_budget = 256ll << 20;
  // ---- encoder side (mia_dac_load_encoder): conv_in1 -> [3 residual units, snake + strided conv] x n -> snake + conv3, then the RVQ stages
  bool has_encoder = false;
  int enc_dim = 0, hop = 1;
  float* enc_in_w = nullptr; float* enc_in_b = nullptr;    // first conv [C][7], [C]
  std::vector<Op> enc_ops;
  Op in_proj[MIA_MAX_LEVELS];
  float* cbn[MIA_MAX_LEVELS] = {};                         // L2-normalised codebooks + their squared norms
  float* cbn_sq[MIA_MAX_LEVELS] = {};
  float* d_audio = nullptr; size_t audio_cap = 0;
  float* d_ze = nullptr; size_t ze_cap = 0;
};

namespace {

struct Loader {
  mia_codec* c;
  std::map<std::string, const mia_tensor_view*> by_name;
  std::string err;

  const mia_tensor_view* find(const std::string& n, bool required = true) {
    auto it = by_name.find(n);
    if (it == by_name.end()) { if (required && err.empty()) err = "missing tensor '" + n + "'"; return nullptr; }
    return it->second;
  }
  bool f32(const std::string& n, std::vector<float>& out, std::initializer_list<int64_t> shp, bool required = true) {
    const mia_tensor_view* t = find(n, required);
    if (!t) return false;
    if (t->dtype != MIA_F32) { if (err.empty()) err = "tensor '" + n + "' must be float32"; return false; }
    int64_t numel = 1; bool ok = t->ndim == (int)shp.size(); int i = 0;
    for (int64_t s : shp) { if (ok && s >= 0 && t->shape[i] != s) ok = false; ++i; }
    for (int k = 0; k < t->ndim; ++k) numel *= t->shape[k];
    if (!ok) { if (err.empty()) err = "tensor '" + n + "' has an unexpected shape"; return false; }
    out.assign((const float*)t->data, (const float*)t->data + numel);
    return true;
  }
  float* up(const std::vector<float>& v) {
    void* p = nullptr;
    if (hipMalloc(&p, v.size() * 4 + 16) != hipSuccess) { if (err.empty()) err = "hipMalloc failed"; return nullptr; }
    c->allocs.push_back(p);
    if (hipMemcpy(p, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess && err.empty()) err = "hipMemcpy failed";
    return (float*)p;
  }
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
  float* alpha(const std::string& n, int C, bool channels_mid) {
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
};

int ensure(mia_codec* c, size_t floats) {
  if (floats <= c->buf_floats) return MIA_OK;
  (void)hipStreamSynchronize(c->ctx->stream);
  for (int i = 0; i < 3; ++i) { if (c->buf[i]) (void)hipFree(c->buf[i]); c->buf[i] = nullptr; }
  for (int i = 0; i < 3; ++i)
    if (hipMalloc((void**)&c->buf[i], floats * 4 + 64) != hipSuccess) return mia_fail(c->ctx, MIA_ERR_OUT_OF_MEMORY, "codec: scratch hipMalloc failed");
  c->buf_floats = floats;
  return MIA_OK;
}

template <typename P>
int ensure_buf(mia_codec* c, P*& p, size_t& cap, size_t n) {
  if (n <= cap) return MIA_OK;
  (void)hipStreamSynchronize(c->ctx->stream);
  if (p) (void)hipFree(p);
  p = nullptr;
  if (hipMalloc((void**)&p, n * sizeof(P) + 64) != hipSuccess) return mia_fail(c->ctx, MIA_ERR_OUT_OF_MEMORY, "codec: hipMalloc failed");
  cap = n;
  return MIA_OK;
}

// sizes along the program for a latent of T0 rows: returns the largest T*C and the output length
void plan(const mia_codec* c, int64_t T0, size_t& max_floats, int64_t& T_final, std::vector<int64_t>* noise_offsets = nullptr, int64_t* noise_total = nullptr) {
  int64_t T = T0; int C = c->latent; max_floats = (size_t)T * C; int64_t noff = 0;
  for (const Op& op : c->ops) {
    if (op.kind == OP_CONV && !op.residual) C = op.N;
    else if (op.kind == OP_CONVT) { T = (T - 1) * op.stride - 2 * op.pad + 2 * op.stride; C = op.N; }
    else if (op.kind == OP_NOISE1 || op.kind == OP_NOISEC) { if (noise_offsets) noise_offsets->push_back(noff); noff += T; }
    if ((size_t)T * C > max_floats) max_floats = (size_t)T * C;
  }
  T_final = T;
  if (noise_total) *noise_total = noff;
}

// Stacked utterances (mia_snac_decode_batch / mia_dac_decode_batch): U sequences side by side in every buffer, sequence u at row
// u * (rows of the longest utterance at that stage) -- the layout of the HiFT batch.  Every table lives on the device:
//   len        [stages][U]  valid rows of each utterance; the stage advances at every transposed convolution
//   noise_off  [blocks][U]  where utterance u's values for that noise block start in the concatenated slabs
//   pcm_off    [U]          where utterance u's samples go
// Every sequence owns `slab` floats of each scratch buffer (a multiple of every channel count, so that it is a whole number of rows at
// every stage, and at least the largest stage of the longest utterance).
// U = 0 (the single-call entries): the launches are exactly the unstacked ones.
struct Stack {
  int U = 0;
  int64_t slab = 0;
  const int32_t* len = nullptr;
  const int32_t* noise_off = nullptr;
  const int64_t* pcm_off = nullptr;
};

// valid rows of a T0-row latent at every stage of the program
std::vector<int64_t> stage_rows(const mia_codec* c, int64_t T0) {
  std::vector<int64_t> r{T0};
  for (const Op& op : c->ops) if (op.kind == OP_CONVT) r.push_back((r.back() - 1) * op.stride - 2 * op.pad + 2 * op.stride);
  return r;
}

// where a run of the program stands: the stream x [T][C] with its two side buffers, the noise values consumed, the stage (transposed
// convolutions passed) and the noise blocks passed
struct Cursor {
  float* x; float* h; float* y;
  int64_t T; int C;
  int64_t noff = 0;
  int stage = 0, nblock = 0;
};

// run ops [begin, end) of the program from cursor k (op 0: k.x holds the latent [T0][latent]); the output conv writes T_final samples to
// d_pcm.  Stacked: k.T = the longest utterance's rows.
// (The DAC residual unit's first convolution is a "side" conv, stride == -1: h = conv(x) with x kept as the stream.)
int run(mia_codec* c, Cursor& k, size_t begin, size_t end, const float* d_noise, float* d_pcm, const Stack& st = Stack()) {
  hipStream_t s = c->ctx->stream;
  float*& x = k.x; float*& h = k.h; float*& y = k.y;
  int64_t& T = k.T; int& C = k.C; int64_t& noff = k.noff;
  int& stage = k.stage; int& nblock = k.nblock;
  auto seq = [&]() { SeqArgs q; if (st.U) { q.n = st.U; q.len = st.len + (size_t)stage * st.U; q.step = st.slab / C; } return q; };
  auto seq_gemm = [&](ConvGemmArgs& g) {
    if (!st.U) return;
    g.n_seq = st.U; g.x_seq_step = st.slab / g.ldx; g.y_seq_step = st.slab / g.ldy; g.seq_len = st.len + (size_t)stage * st.U;
  };
  for (size_t oi = begin; oi < end; ++oi) {
    const Op& op = c->ops[oi];
    switch (op.kind) {
      case OP_DW:
        if (codec_dwconv_launch(x, h, op.w, op.b, op.a_pre, op.a_post, (int)T, C, op.taps, op.dil, s, seq())) return mia_fail(c->ctx, MIA_ERR_DEVICE, "codec: dwconv launch failed");
        if (!op.residual) std::swap(x, h);     // plain depthwise layer: its output becomes the stream
        break;
      case OP_CONV: {
        const bool side = op.stride == -1;
        ConvGemmArgs g;
        g.X = op.residual ? h : x; g.ldx = op.Cin; g.T_in = (int)T; g.W = op.w; g.bias = op.b; g.alpha = op.a_pre;
        g.M = (int)T; g.N = op.N; g.Cin = op.Cin; g.taps = op.taps; g.dil = op.dil; g.pad = op.pad; g.T_out = (int)T;
        if (op.residual) { g.R = x; g.ldr = op.N; g.Y = x; g.ldy = op.N; }
        else { g.Y = side ? h : y; g.ldy = op.N; }
        seq_gemm(g);
        if (const char* e = codec_conv_gemm_check(g)) return mia_fail(c->ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
        if (codec_conv_gemm_launch(g, 1, s)) return mia_fail(c->ctx, MIA_ERR_DEVICE, "codec: conv launch failed");
        if (!op.residual && !side) { std::swap(x, y); C = op.N; }
        break;
      }
      case OP_CONVT: {
        const int64_t T_out = (T - 1) * op.stride - 2 * op.pad + 2 * op.stride;
        ConvGemmArgs g;
        g.X = x; g.ldx = op.Cin; g.T_in = (int)T; g.W = op.w; g.w_phase_stride = (int64_t)op.N * 2 * op.Cin; g.bias = op.b; g.alpha = op.a_pre;
        g.M = (int)T + 1; g.N = op.N; g.Cin = op.Cin; g.taps = 2; g.dil = 1; g.pad = 1;
        g.Y = y; g.ldy = op.N; g.T_out = (int)T_out; g.y_row_mul = op.stride; g.y_row_off = -op.pad; g.y_phase_step = 1;
        seq_gemm(g);
        if (const char* e = codec_conv_gemm_check(g)) return mia_fail(c->ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
        if (codec_conv_gemm_launch(g, op.stride, s)) return mia_fail(c->ctx, MIA_ERR_DEVICE, "codec: convT launch failed");
        std::swap(x, y); C = op.N; T = T_out; ++stage;
        break;
      }
      case OP_NOISE1:
        if (d_noise) {
          SeqArgs q = seq();
          if (st.U) q.noise_off = st.noise_off + (size_t)nblock * st.U;
          if (codec_noise1_launch(x, op.w, st.U ? d_noise : d_noise + noff, (int)T, C, s, q)) return mia_fail(c->ctx, MIA_ERR_DEVICE, "codec: noise launch failed");
        }
        noff += T; ++nblock;
        break;
      case OP_NOISEC:
        if (d_noise) {
          ConvGemmArgs g;
          g.X = x; g.ldx = C; g.T_in = (int)T; g.W = op.w; g.M = (int)T; g.N = C; g.Cin = C; g.T_out = (int)T;
          g.R = x; g.ldr = C; g.noise = st.U ? d_noise : d_noise + noff; g.Y = y; g.ldy = C;
          seq_gemm(g);
          if (st.U) g.noise_seq_off = st.noise_off + (size_t)nblock * st.U;
          if (const char* e = codec_conv_gemm_check(g)) return mia_fail(c->ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
          if (codec_conv_gemm_launch(g, 1, s)) return mia_fail(c->ctx, MIA_ERR_DEVICE, "codec: noise gemm launch failed");
          std::swap(x, y);
        }
        noff += T; ++nblock;
        break;
      case OP_OUT1: {
        SeqArgs q = seq();
        q.out_off = st.pcm_off;
        if (codec_conv_out1_launch(x, d_pcm, op.w, op.b, op.a_pre, (int)T, C, op.taps, s, q)) return mia_fail(c->ctx, MIA_ERR_DEVICE, "codec: output conv launch failed");
        break;
      }
    }
  }
  return MIA_OK;
}

void add_residual_unit_snac(Loader& L, const std::string& p, int C, int dil, std::vector<Op>& ops) {
  Op dw; dw.kind = OP_DW; dw.residual = true; dw.dil = dil;
  dw.a_pre = L.alpha(p + ".block.layers.0.alpha", C, true);
  L.dw_conv(p + ".block.layers.1", C, 7, dw);
  dw.a_post = L.alpha(p + ".block.layers.2.alpha", C, true);
  ops.push_back(dw);
  Op pw; pw.kind = OP_CONV; pw.residual = true;
  L.dense_conv(p + ".block.layers.3", C, 1, C, true, pw);
  ops.push_back(pw);
}

void add_residual_unit_dac(Loader& L, const std::string& p, int C, int dil, std::vector<Op>& ops) {
  // h = conv7_dilated(snake(x)) (not residual: goes to the side buffer); x += conv1x1(snake(h))
  Op c1; c1.kind = OP_CONV; c1.dil = dil; c1.pad = 3 * dil;
  c1.a_pre = L.alpha(p + ".block.layers.0.alpha", C, false);
  L.dense_conv(p + ".block.layers.1", C, 7, C, true, c1);
  Op c2; c2.kind = OP_CONV; c2.residual = true;
  c2.a_pre = L.alpha(p + ".block.layers.2.alpha", C, false);
  L.dense_conv(p + ".block.layers.3", C, 1, C, true, c2);
  // encode "side" conv as: OP_CONV writing into h.  The executor treats a non-residual OP_CONV as a stream change, so mark it
  // with N == Cin and a dedicated flag through `stride = -1` (run() keeps x as the stream for it).
  c1.stride = -1;
  ops.push_back(c1);
  ops.push_back(c2);
}

}  // namespace

static mia_codec* codec_fail(mia_ctx* ctx, mia_codec* c, const std::string& m) {
  ctx->err = "codec_load: " + m;
  if (c) mia_codec_free(c);
  return nullptr;
}

extern "C" void mia_codec_free(mia_codec* c) {
  if (!c) return;
  (void)hipSetDevice(c->ctx->device);
  (void)hipStreamSynchronize(c->ctx->stream);
  for (void* p : c->allocs) (void)hipFree(p);
  for (int i = 0; i < 3; ++i) if (c->buf[i]) (void)hipFree(c->buf[i]);
  if (c->d_codes) (void)hipFree(c->d_codes);
  if (c->d_noise) (void)hipFree(c->d_noise);
  if (c->d_pcm) (void)hipFree(c->d_pcm);
  if (c->d_tab) (void)hipFree(c->d_tab);
  if (c->h_tab) (void)hipHostFree(c->h_tab);
  if (c->tab_ev) (void)hipEventDestroy(c->tab_ev);
  if (c->d_audio) (void)hipFree(c->d_audio);
  if (c->d_ze) (void)hipFree(c->d_ze);
  delete c;
}

static bool load_quantizers(Loader& L, mia_codec* c, int n, int latent, int cb_size, int cb_dim) {
  c->n_levels = n; c->latent = latent; c->cb_size = cb_size; c->cb_dim = cb_dim;
  for (int i = 0; i < n; ++i) {
    const std::string q = "quantizer.quantizers." + std::to_string(i);
    std::vector<float> cb, g, v, b;
    if (!L.f32(q + ".codebook.weight", cb, {cb_size, cb_dim}) || !L.f32(q + ".out_proj.weight_g", g, {latent, 1, 1}) ||
        !L.f32(q + ".out_proj.weight_v", v, {latent, 1, cb_dim}) || !L.f32(q + ".out_proj.bias", b, {latent})) return false;
    Loader::fold_wn(v, g, latent, 1, cb_dim, 0);     // per output channel over the codebook dim (SNACDecoder.swift:374-377)
    c->codebook[i] = L.up(cb); c->weff[i] = L.up(v); c->ebias[i] = L.up(b);
  }
  return true;
}

extern "C" mia_codec* mia_snac_load(mia_ctx* ctx, const mia_snac_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors || n_tensors <= 0) return codec_fail(ctx, nullptr, "null arguments");
  if (cfg->n_rates <= 0 || cfg->n_rates > 8 || cfg->n_vq <= 0 || cfg->n_vq > MIA_MAX_LEVELS) return codec_fail(ctx, nullptr, "bad SNAC config");
  if (cfg->latent_dim % 32 || cfg->decoder_dim % 32 || (cfg->decoder_dim >> cfg->n_rates) % 4) return codec_fail(ctx, nullptr, "SNAC channel counts must be multiples of 32");
  if (!cfg->depthwise) return codec_fail(ctx, nullptr, "only the depthwise SNAC variant (snac_24khz) is supported");
  if (hipSetDevice(ctx->device) != hipSuccess) return codec_fail(ctx, nullptr, "hipSetDevice failed");
  mia_codec* c = new mia_codec(); c->ctx = ctx; c->kind = 0;
  Loader L; L.c = c;
  for (int i = 0; i < n_tensors; ++i) if (tensors[i].name && tensors[i].data) L.by_name[tensors[i].name] = &tensors[i];
  for (int i = 0; i < cfg->n_vq; ++i) c->vq_stride[i] = cfg->vq_strides[i];
  load_quantizers(L, c, cfg->n_vq, cfg->latent_dim, cfg->codebook_size, cfg->codebook_dim);
  const std::string P = "decoder.model.layers.";
  { Op dw; dw.kind = OP_DW; L.dw_conv(P + "0", cfg->latent_dim, 7, dw); c->ops.push_back(dw); }
  { Op pw; pw.kind = OP_CONV; L.dense_conv(P + "1", cfg->decoder_dim, 1, cfg->latent_dim, true, pw); c->ops.push_back(pw); }
  int Cin = cfg->decoder_dim;
  for (int i = 0; i < cfg->n_rates && L.err.empty(); ++i) {
    const int Cout = cfg->decoder_dim >> (i + 1), s = cfg->decoder_rates[i];
    if (s % 2) return codec_fail(ctx, c, "SNAC decoder rates must be even (the reference drops output_padding, ConvWeightedTranspose1d.swift:86-93)");
    const std::string b = P + std::to_string(2 + i) + ".block.layers.";
    Op ct; ct.kind = OP_CONVT; ct.pad = (s + 1) / 2;
    ct.a_pre = L.alpha(b + "0.alpha", Cin, true);
    {  // v [Cin][K][Cout], g [Cin][1][1]: normalise per input channel, then permute to MLX [Cout][K][Cin]
      std::vector<float> v, g, bias;
      const int K = 2 * s;
      if (L.f32(b + "1.weight_v", v, {Cin, K, Cout}) && L.f32(b + "1.weight_g", g, {Cin, 1, 1}) && L.f32(b + "1.bias", bias, {Cout})) {
        Loader::fold_wn(v, g, Cin, K, Cout, 0);
        std::vector<float> wm((size_t)Cout * K * Cin);
        for (int ci = 0; ci < Cin; ++ci) for (int k = 0; k < K; ++k) for (int co = 0; co < Cout; ++co)
          wm[((size_t)co * K + k) * Cin + ci] = v[((size_t)ci * K + k) * Cout + co];
        L.convt_phases(wm, Cout, K, Cin, s, ct);
        ct.b = L.up(bias);
      }
    }
    c->ops.push_back(ct);
    int ru = 2;
    if (cfg->noise) {
      // NoiseBlock.linear: [Cn][1][Cout] with Cn = 1 (this port's init) or Cout (upstream SNAC checkpoints)
      const mia_tensor_view* tv = L.find(b + "2.linear.weight_v");
      if (tv && tv->ndim == 3) {
        const int Cn = (int)tv->shape[0];
        std::vector<float> v, g;
        if (L.f32(b + "2.linear.weight_v", v, {Cn, 1, Cout}) && L.f32(b + "2.linear.weight_g", g, {Cn, 1, 1})) {
          Loader::fold_wn(v, g, Cn, 1, Cout, 0);
          Op nz; nz.kind = Cn == 1 ? OP_NOISE1 : OP_NOISEC; nz.N = Cn; nz.Cin = Cout; nz.w = L.up(v);
          if (Cn != 1 && Cn != Cout) return codec_fail(ctx, c, "noise block must have 1 or C output channels");
          c->ops.push_back(nz);
        }
      }
      ru = 3;
    }
    const int dils[3] = {1, 3, 9};
    for (int r = 0; r < 3; ++r) add_residual_unit_snac(L, b + std::to_string(ru + r), Cout, dils[r], c->ops);
    Cin = Cout;
  }
  { Op o; o.kind = OP_OUT1; o.a_pre = L.alpha(P + std::to_string(2 + cfg->n_rates) + ".alpha", Cin, true);
    Op tmp; L.dense_conv(P + std::to_string(3 + cfg->n_rates), 1, 7, Cin, true, tmp); o.w = tmp.w; o.b = tmp.b; o.taps = 7; o.Cin = Cin; o.N = 1;
    c->ops.push_back(o); }
  if (!L.err.empty()) return codec_fail(ctx, c, L.err);
  if (hipDeviceSynchronize() != hipSuccess) return codec_fail(ctx, c, "device error during upload");
  return c;
}

extern "C" mia_codec* mia_dac_load(mia_ctx* ctx, const mia_dac_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors || n_tensors <= 0) return codec_fail(ctx, nullptr, "null arguments");
  if (cfg->n_rates <= 0 || cfg->n_rates > 8 || cfg->n_codebooks <= 0 || cfg->n_codebooks > MIA_MAX_LEVELS) return codec_fail(ctx, nullptr, "bad DAC config (at most 4 codebooks)");
  if (cfg->latent_dim % 32 || cfg->decoder_dim % 32 || (cfg->decoder_dim >> cfg->n_rates) % 32) return codec_fail(ctx, nullptr, "DAC channel counts must be multiples of 32");
  if (hipSetDevice(ctx->device) != hipSuccess) return codec_fail(ctx, nullptr, "hipSetDevice failed");
  mia_codec* c = new mia_codec(); c->ctx = ctx; c->kind = 1;
  c->stack_budget = c->stack_budget_default = INT64_MAX;
  Loader L; L.c = c;
  for (int i = 0; i < n_tensors; ++i) if (tensors[i].name && tensors[i].data) L.by_name[tensors[i].name] = &tensors[i];
  load_quantizers(L, c, cfg->n_codebooks, cfg->latent_dim, cfg->codebook_size, cfg->codebook_dim);
  const std::string P = "decoder.model.layers.";
  { Op c0; c0.kind = OP_CONV; c0.pad = 3; L.dense_conv(P + "0", cfg->decoder_dim, 7, cfg->latent_dim, true, c0); c->ops.push_back(c0); }
  int Cin = cfg->decoder_dim;
  for (int i = 0; i < cfg->n_rates && L.err.empty(); ++i) {
    const int Cout = cfg->decoder_dim >> (i + 1), s = cfg->decoder_rates[i], K = 2 * s;
    const std::string b = P + std::to_string(1 + i) + ".block.layers.";
    Op ct; ct.kind = OP_CONVT; ct.pad = (s + 1) / 2;
    ct.a_pre = L.alpha(b + "0.alpha", Cin, false);
    {  // DAC stores the transposed-conv weight already as [Cout][K][Cin], normalised per INPUT channel (exceptDim 2, DACLayers.swift:161,173)
      std::vector<float> v, g, bias;
      if (L.f32(b + "1.weight_v", v, {Cout, K, Cin}) && L.f32(b + "1.weight_g", g, {1, 1, Cin}) && L.f32(b + "1.bias", bias, {Cout})) {
        Loader::fold_wn(v, g, Cout, K, Cin, 2);
        L.convt_phases(v, Cout, K, Cin, s, ct);
        ct.b = L.up(bias);
      }
    }
    c->ops.push_back(ct);
    const int dils[3] = {1, 3, 9};
    for (int r = 0; r < 3; ++r) add_residual_unit_dac(L, b + std::to_string(2 + r), Cout, dils[r], c->ops);
    Cin = Cout;
  }
  { Op o; o.kind = OP_OUT1; o.a_pre = L.alpha(P + std::to_string(1 + cfg->n_rates) + ".alpha", Cin, false);
    Op tmp; L.dense_conv(P + std::to_string(2 + cfg->n_rates), 1, 7, Cin, true, tmp); o.w = tmp.w; o.b = tmp.b; o.taps = 7; o.Cin = Cin; o.N = 1;
    c->ops.push_back(o); }
  if (!L.err.empty()) return codec_fail(ctx, c, L.err);
  if (hipDeviceSynchronize() != hipSuccess) return codec_fail(ctx, c, "device error during upload");
  return c;
}

// shared tail: codes already on the device, latent length T0
static int decode_common(mia_codec* c, const EmbedArgs& ea, int64_t T0, const float* noise, int64_t n_noise_given, float* pcm, int64_t* n_out, int mem) {
  mia_ctx* ctx = c->ctx;
  size_t max_floats; int64_t T_final, noise_total = 0; std::vector<int64_t> noffs;
  plan(c, T0, max_floats, T_final, &noffs, &noise_total);
  int rc = ensure(c, max_floats);
  if (rc != MIA_OK) return rc;
  if ((rc = ensure_buf(c, c->d_pcm, c->pcm_cap, (size_t)T_final)) != MIA_OK) return rc;
  const float* d_noise = nullptr;
  if (noise && noise_total > 0) {
    MIA_CHECK_ARG(ctx, n_noise_given == noise_total, "codec: noise must hold %lld values (got %lld)", (long long)noise_total, (long long)n_noise_given);
    if (mem == MIA_MEM_DEVICE) d_noise = noise;
    else {
      if ((rc = ensure_buf(c, c->d_noise, c->noise_cap, (size_t)noise_total)) != MIA_OK) return rc;
      MIA_HIP(ctx, hipMemcpyAsync(c->d_noise, noise, (size_t)noise_total * 4, hipMemcpyHostToDevice, ctx->stream));
      d_noise = c->d_noise;
    }
  }
  if (codec_embed_launch(ea, c->buf[0], (int)T0, c->latent, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "codec: embed launch failed");
  float* dst = mem == MIA_MEM_DEVICE ? pcm : c->d_pcm;
  Cursor k{c->buf[0], c->buf[1], c->buf[2], T0, c->latent};
  rc = run(c, k, 0, c->ops.size(), d_noise, dst);
  if (rc != MIA_OK) return rc;
  if (n_out) *n_out = T_final;
  if (mem == MIA_MEM_HOST) {
    MIA_HIP(ctx, hipMemcpyAsync(pcm, c->d_pcm, (size_t)T_final * 4, hipMemcpyDeviceToHost, ctx->stream));
    MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return MIA_OK;
}

extern "C" int mia_codec_set_stack_budget(mia_codec* c, int64_t bytes) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  c->stack_budget = bytes < 0 ? c->stack_budget_default : bytes;
  return MIA_OK;
}

extern "C" int64_t mia_codec_noise_len(mia_codec* c, int64_t latent_len) {
  if (!c || latent_len <= 0) return 0;
  size_t mf; int64_t tf, nt = 0; std::vector<int64_t> o;
  plan(c, latent_len, mf, tf, &o, &nt);
  return nt;
}

extern "C" int64_t mia_codec_output_len(mia_codec* c, int64_t latent_len) {
  if (!c || latent_len <= 0) return 0;
  size_t mf; int64_t tf;
  plan(c, latent_len, mf, tf);
  return tf;
}

extern "C" int mia_snac_decode(mia_codec* c, const int32_t* const* codes, const int32_t* n_codes, int n_levels, const float* noise,
                               int64_t n_noise, float* pcm, int64_t pcm_capacity, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 0, "snac_decode: handle is not a SNAC model");
  MIA_CHECK_ARG(ctx, codes && n_codes && pcm && n_levels > 0, "snac_decode: null arguments");
  MIA_CHECK_ARG(ctx, mem == MIA_MEM_HOST || mem == MIA_MEM_DEVICE, "snac_decode: bad mem");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  // expanded length = max_i n_i * stride_i; a level whose expansion differs is skipped, as embedCodes does (SNACDecoder.swift:337-402)
  int64_t T0 = 0; size_t total = 0;
  for (int i = 0; i < c->n_levels && i < n_levels; ++i) if (n_codes[i] > 0) { T0 = std::max<int64_t>(T0, (int64_t)n_codes[i] * c->vq_stride[i]); total += n_codes[i]; }
  MIA_CHECK_ARG(ctx, T0 > 0, "snac_decode: no codes");
  int rc = ensure_buf(c, c->d_codes, c->codes_cap, total);
  if (rc != MIA_OK) return rc;
  EmbedArgs ea{}; ea.n_levels = c->n_levels; ea.cb_dim = c->cb_dim;
  size_t off = 0;
  for (int i = 0; i < c->n_levels; ++i) {
    ea.codebook[i] = c->codebook[i]; ea.weff[i] = c->weff[i]; ea.bias[i] = c->ebias[i]; ea.stride[i] = c->vq_stride[i]; ea.codes[i] = nullptr;
    if (i >= n_levels || n_codes[i] <= 0 || (int64_t)n_codes[i] * c->vq_stride[i] != T0) continue;
    for (int k = 0; k < n_codes[i] && mem == MIA_MEM_HOST; ++k)
      if (codes[i][k] < 0 || codes[i][k] >= c->cb_size) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "snac_decode: code %d out of range at level %d", codes[i][k], i);
    MIA_HIP(ctx, hipMemcpyAsync(c->d_codes + off, codes[i], (size_t)n_codes[i] * 4, mem == MIA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    ea.codes[i] = c->d_codes + off; off += n_codes[i];
  }
  MIA_CHECK_ARG(ctx, pcm_capacity >= mia_codec_output_len(c, T0), "snac_decode: pcm buffer too small (%lld < %lld)", (long long)pcm_capacity, (long long)mia_codec_output_len(c, T0));
  return decode_common(c, ea, T0, noise, n_noise, pcm, n_samples, mem);
}

extern "C" int mia_dac_decode(mia_codec* c, const int32_t* codes, int n_codebooks, int64_t T, float* pcm, int64_t pcm_capacity, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 1, "dac_decode: handle is not a DAC model");
  MIA_CHECK_ARG(ctx, codes && pcm && T > 0 && n_codebooks > 0 && n_codebooks <= c->n_levels, "dac_decode: bad arguments");
  MIA_CHECK_ARG(ctx, mem == MIA_MEM_HOST || mem == MIA_MEM_DEVICE, "dac_decode: bad mem");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure_buf(c, c->d_codes, c->codes_cap, (size_t)n_codebooks * T);
  if (rc != MIA_OK) return rc;
  if (mem == MIA_MEM_HOST)
    for (int64_t k = 0; k < (int64_t)n_codebooks * T; ++k)
      if (codes[k] < 0 || codes[k] >= c->cb_size) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "dac_decode: code %d out of range", codes[k]);
  MIA_HIP(ctx, hipMemcpyAsync(c->d_codes, codes, (size_t)n_codebooks * T * 4, mem == MIA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
  EmbedArgs ea{}; ea.n_levels = n_codebooks; ea.cb_dim = c->cb_dim;
  for (int i = 0; i < n_codebooks; ++i) {
    ea.codebook[i] = c->codebook[i]; ea.weff[i] = c->weff[i]; ea.bias[i] = c->ebias[i]; ea.stride[i] = 1; ea.codes[i] = c->d_codes + (size_t)i * T;
  }
  MIA_CHECK_ARG(ctx, pcm_capacity >= mia_codec_output_len(c, T), "dac_decode: pcm buffer too small");
  return decode_common(c, ea, T, nullptr, 0, pcm, n_samples, mem);
}

// ---- stacked decode: n_utt utterances in one pass -----------------------------------------------------------------------------------------
namespace {

struct BatchUtt { int64_t T0 = 0, n_out = 0, noise_len = 0; int64_t code_off[MIA_MAX_LEVELS] = {-1, -1, -1, -1}; };

// enqueue one stacked decode: every argument has been checked, nothing has touched the GPU yet
int decode_batch_enqueue(mia_codec* c, std::vector<BatchUtt>& ut, const int strides[MIA_MAX_LEVELS], int n_levels, const int32_t* codes, size_t n_codes_total,
                        const float* noise, float* pcm, const int64_t* pcm_off, int64_t* n_samples, int mem) {
  mia_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  const int U = (int)ut.size();
  const bool dev = mem == MIA_MEM_DEVICE;
  int64_t Tmax = 0, pcm_total = 0, noise_total = 0;
  for (const BatchUtt& b : ut) { Tmax = std::max(Tmax, b.T0); pcm_total += b.n_out; noise_total += b.noise_len; }
  if (noise_total == 0) noise = nullptr;
  size_t max_floats; int64_t T_final;
  plan(c, Tmax, max_floats, T_final);
  const size_t n_stages = stage_rows(c, Tmax).size();
  size_t n_blocks = 0;
  for (const Op& op : c->ops) if (op.kind == OP_NOISE1 || op.kind == OP_NOISEC) ++n_blocks;
  // floats per utterance per buffer: the largest stage of the longest utterance, rounded up to a whole number of rows at every stage
  int64_t row_lcm = c->latent;
  for (const Op& op : c->ops) if (op.kind == OP_CONVT || (op.kind == OP_CONV && !op.residual)) row_lcm = std::lcm<int64_t>(row_lcm, op.N);
  const int64_t slab = ((int64_t)max_floats + row_lcm - 1) / row_lcm * row_lcm;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = ensure(c, (size_t)slab * (size_t)U);            // three buffers of n_utt x (largest stage of the longest utterance)
  if (rc != MIA_OK) return rc;
  if (!dev) {
    if ((rc = ensure_buf(c, c->d_pcm, c->pcm_cap, (size_t)pcm_total)) != MIA_OK) return rc;
    if ((rc = ensure_buf(c, c->d_codes, c->codes_cap, n_codes_total)) != MIA_OK) return rc;
    if (noise && (rc = ensure_buf(c, c->d_noise, c->noise_cap, (size_t)noise_total)) != MIA_OK) return rc;
  }
  // tables: [pcm_off U | code_off U x MIA_MAX_LEVELS] int64, then [len stages x U | noise_off blocks x U] int32 -- one upload per call
  const size_t n64 = (size_t)U * (1 + MIA_MAX_LEVELS), n32 = (size_t)U * (n_stages + n_blocks), bytes = n64 * 8 + n32 * 4;
  if (!c->tab_ev) MIA_HIP(ctx, hipEventCreateWithFlags(&c->tab_ev, hipEventDisableTiming));
  else MIA_HIP(ctx, hipEventSynchronize(c->tab_ev));       // the previous call's upload has left the staging
  if (bytes > c->tab_cap) {
    MIA_HIP(ctx, hipStreamSynchronize(s));
    if (c->d_tab) (void)hipFree(c->d_tab);
    if (c->h_tab) (void)hipHostFree(c->h_tab);
    c->d_tab = c->h_tab = nullptr; c->tab_cap = 0;
    MIA_HIP(ctx, hipHostMalloc(&c->h_tab, bytes, hipHostMallocDefault));
    MIA_HIP(ctx, hipMalloc(&c->d_tab, bytes));
    c->tab_cap = bytes;
  }
  int64_t* h64 = (int64_t*)c->h_tab; int32_t* h32 = (int32_t*)(h64 + n64);
  int64_t po = 0, zo = 0;
  for (int u = 0; u < U; ++u) {
    h64[u] = dev ? pcm_off[u] : po;                        // host: packed in d_pcm, copied out per utterance below
    for (int l = 0; l < MIA_MAX_LEVELS; ++l) h64[U + (size_t)u * MIA_MAX_LEVELS + l] = ut[u].code_off[l];
    const std::vector<int64_t> rows = stage_rows(c, ut[u].T0);
    for (size_t k = 0; k < n_stages; ++k) h32[k * U + u] = (int32_t)rows[k];
    std::vector<int64_t> noffs; size_t mf; int64_t tf;
    plan(c, ut[u].T0, mf, tf, &noffs);
    for (size_t k = 0; k < n_blocks; ++k) h32[(n_stages + k) * U + u] = (int32_t)(zo + noffs[k]);
    po += ut[u].n_out; zo += ut[u].noise_len;
  }
  MIA_HIP(ctx, hipMemcpyAsync(c->d_tab, c->h_tab, bytes, hipMemcpyHostToDevice, s));
  MIA_HIP(ctx, hipEventRecord(c->tab_ev, s));
  Stack st; st.U = U; st.slab = slab;
  st.pcm_off = (const int64_t*)c->d_tab;
  st.len = (const int32_t*)((const int64_t*)c->d_tab + n64);
  st.noise_off = st.len + n_stages * U;
  const int32_t* d_codes = codes; const float* d_noise = noise;
  if (!dev) {                                              // (decode_batch_common synchronises before the caller gets its arrays back)
    MIA_HIP(ctx, hipMemcpyAsync(c->d_codes, codes, n_codes_total * 4, hipMemcpyHostToDevice, s));
    d_codes = c->d_codes;
    if (noise) { MIA_HIP(ctx, hipMemcpyAsync(c->d_noise, noise, (size_t)noise_total * 4, hipMemcpyHostToDevice, s)); d_noise = c->d_noise; }
  }
  EmbedArgs ea{}; ea.n_levels = n_levels; ea.cb_dim = c->cb_dim;
  for (int i = 0; i < n_levels; ++i) { ea.codebook[i] = c->codebook[i]; ea.weff[i] = c->weff[i]; ea.bias[i] = c->ebias[i]; ea.stride[i] = strides[i]; }
  ea.codes_base = d_codes; ea.seq_code_off = (const int64_t*)c->d_tab + U;
  SeqArgs q0; q0.n = U; q0.len = st.len; q0.step = slab / c->latent;
  if (codec_embed_launch(ea, c->buf[0], (int)Tmax, c->latent, s, q0)) return mia_fail(ctx, MIA_ERR_DEVICE, "codec: embed launch failed");
  // Stages run stacked while all the utterances' activations there (three buffers) fit the budget.  SNAC: 256 MiB, the Infinity Cache.
  // Its early stages have too few rows per utterance to fill the CUs, and stacking fills them; from the first stage that does not fit,
  // every utterance runs the rest of the program on its own slab, one after the other, with the single call's launches.  A late
  // stage of ONE utterance fills the chip, and its depthwise + 1x1 layers are memory-bound and hand their activations over through
  // the cache, which a pass over all utterances per layer streams from HBM instead: every stage stacked measured 3-4 % SLOWER than
  // the loop of single calls at 8 and 32 chunks of 171 frames, this split 2 % faster.  DAC's dense 7-tap convolutions are
  // compute-bound and gain from the larger grids at every stage (8 x 750 steps: 10 % faster with every stage stacked, 1 % with the
  // split), so its default is no limit.  LABNOTES, "stacked codec decode".  Stage 0 is always stacked.
  size_t split = c->ops.size();
  { int64_t T = Tmax;
    for (size_t i = 0; i < c->ops.size(); ++i) {
      const Op& op = c->ops[i];
      if (op.kind != OP_CONVT) continue;
      T = (T - 1) * op.stride - 2 * op.pad + 2 * op.stride;
      if ((double)U * 3.0 * (double)T * op.N * 4.0 > (double)c->stack_budget) { split = i; break; }
    } }
  float* dst = dev ? pcm : c->d_pcm;
  Cursor k{c->buf[0], c->buf[1], c->buf[2], Tmax, c->latent};
  if ((rc = run(c, k, 0, split, d_noise, dst, st)) != MIA_OK) return rc;
  if (split < c->ops.size()) {
    int64_t zo_u = 0;
    for (int u = 0; u < U; ++u) {
      std::vector<int64_t> noffs; size_t mf; int64_t tf;
      plan(c, ut[u].T0, mf, tf, &noffs);
      Cursor ku{k.x + (int64_t)u * slab, k.h + (int64_t)u * slab, k.y + (int64_t)u * slab, stage_rows(c, ut[u].T0)[k.stage], k.C};
      ku.noff = zo_u + ((size_t)k.nblock < noffs.size() ? noffs[k.nblock] : 0); ku.stage = k.stage; ku.nblock = k.nblock;
      if ((rc = run(c, ku, split, c->ops.size(), d_noise, dst + h64[u])) != MIA_OK) return rc;
      zo_u += ut[u].noise_len;
    }
  }
  if (n_samples) for (int u = 0; u < U; ++u) n_samples[u] = ut[u].n_out;
  if (!dev) {
    po = 0;
    for (int u = 0; u < U; ++u) {
      MIA_HIP(ctx, hipMemcpyAsync(pcm + pcm_off[u], c->d_pcm + po, (size_t)ut[u].n_out * 4, hipMemcpyDeviceToHost, s));
      po += ut[u].n_out;
    }
  }
  return MIA_OK;
}

// shared tail of the two batch entries.  Host memory: the caller's codes / noise / pcm are behind asynchronous copies, so the stream is
// synchronised on EVERY return path, the failing ones included (the tables' staging belongs to the handle and needs no such care).
int decode_batch_common(mia_codec* c, std::vector<BatchUtt>& ut, const int strides[MIA_MAX_LEVELS], int n_levels, const int32_t* codes, size_t n_codes_total,
                        const float* noise, float* pcm, const int64_t* pcm_off, int64_t* n_samples, int mem) {
  int rc = decode_batch_enqueue(c, ut, strides, n_levels, codes, n_codes_total, noise, pcm, pcm_off, n_samples, mem);
  if (mem == MIA_MEM_HOST && hipStreamSynchronize(c->ctx->stream) != hipSuccess && rc == MIA_OK)
    rc = mia_fail(c->ctx, MIA_ERR_DEVICE, "codec: device error in the stacked decode");
  return rc;
}

// lengths every utterance needs, and the checks both entries share; `what` prefixes the messages
int batch_lengths(mia_codec* c, std::vector<BatchUtt>& ut, const float* noise, int64_t n_noise, const int64_t* pcm_off, const char* what) {
  mia_ctx* ctx = c->ctx;
  int64_t noise_total = 0;
  MIA_CHECK_ARG(ctx, pcm_off[0] >= 0, "%s: pcm_off[0] is negative", what);
  for (size_t u = 0; u < ut.size(); ++u) {
    ut[u].n_out = mia_codec_output_len(c, ut[u].T0);
    ut[u].noise_len = mia_codec_noise_len(c, ut[u].T0);
    noise_total += ut[u].noise_len;
    MIA_CHECK_ARG(ctx, pcm_off[u + 1] - pcm_off[u] >= ut[u].n_out, "%s: pcm room of utterance %d too small (%lld < %lld)", what, (int)u,
                  (long long)(pcm_off[u + 1] - pcm_off[u]), (long long)ut[u].n_out);
  }
  MIA_CHECK_ARG(ctx, noise_total < (1ll << 31), "%s: too many noise values for one call", what);
  if (noise && noise_total > 0)
    MIA_CHECK_ARG(ctx, n_noise == noise_total, "%s: noise must hold %lld values, the sum over the utterances (got %lld)", what, (long long)noise_total, (long long)n_noise);
  return MIA_OK;
}

}  // namespace

extern "C" int mia_snac_decode_batch(mia_codec* c, int n_utt, const int32_t* codes, const int32_t* n_codes, int n_levels, const float* noise,
                                     int64_t n_noise, float* pcm, const int64_t* pcm_off, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 0, "snac_decode_batch: handle is not a SNAC model");
  MIA_CHECK_ARG(ctx, n_utt >= 1 && n_utt <= 64, "snac_decode_batch: n_utt must be 1..64 (got %d)", n_utt);
  MIA_CHECK_ARG(ctx, codes && n_codes && pcm && pcm_off && n_levels > 0, "snac_decode_batch: null arguments");
  MIA_CHECK_ARG(ctx, mem == MIA_MEM_HOST || mem == MIA_MEM_DEVICE, "snac_decode_batch: bad mem");
  std::vector<BatchUtt> ut(n_utt);
  size_t off = 0;
  for (int u = 0; u < n_utt; ++u) {
    const int32_t* n = n_codes + (size_t)u * n_levels;
    // expanded length = max_i n_i * stride_i; a level whose expansion differs is skipped for this utterance, as embedCodes does
    for (int i = 0; i < c->n_levels && i < n_levels; ++i) if (n[i] > 0) ut[u].T0 = std::max<int64_t>(ut[u].T0, (int64_t)n[i] * c->vq_stride[i]);
    MIA_CHECK_ARG(ctx, ut[u].T0 > 0, "snac_decode_batch: utterance %d has no codes", u);
    for (int i = 0; i < n_levels; ++i) {
      if (n[i] <= 0) continue;
      if (i < c->n_levels && (int64_t)n[i] * c->vq_stride[i] == ut[u].T0) {
        for (int k = 0; k < n[i] && mem == MIA_MEM_HOST; ++k)
          MIA_CHECK_ARG(ctx, codes[off + k] >= 0 && codes[off + k] < c->cb_size, "snac_decode_batch: code %d out of range at level %d of utterance %d", codes[off + k], i, u);
        ut[u].code_off[i] = (int64_t)off;
      }
      off += n[i];
    }
  }
  if (int rc = batch_lengths(c, ut, noise, n_noise, pcm_off, "snac_decode_batch")) return rc;
  return decode_batch_common(c, ut, c->vq_stride, c->n_levels, codes, off, noise, pcm, pcm_off, n_samples, mem);
}

extern "C" int mia_dac_decode_batch(mia_codec* c, int n_utt, const int32_t* codes, int n_codebooks, const int64_t* T, float* pcm,
                                    const int64_t* pcm_off, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 1, "dac_decode_batch: handle is not a DAC model");
  MIA_CHECK_ARG(ctx, n_utt >= 1 && n_utt <= 64, "dac_decode_batch: n_utt must be 1..64 (got %d)", n_utt);
  MIA_CHECK_ARG(ctx, codes && T && pcm && pcm_off && n_codebooks > 0 && n_codebooks <= c->n_levels, "dac_decode_batch: bad arguments");
  MIA_CHECK_ARG(ctx, mem == MIA_MEM_HOST || mem == MIA_MEM_DEVICE, "dac_decode_batch: bad mem");
  std::vector<BatchUtt> ut(n_utt);
  size_t off = 0;
  for (int u = 0; u < n_utt; ++u) {
    MIA_CHECK_ARG(ctx, T[u] > 0 && T[u] < (1ll << 30), "dac_decode_batch: utterance %d has no codes (T = %lld)", u, (long long)T[u]);
    ut[u].T0 = T[u];
    for (int i = 0; i < n_codebooks; ++i) ut[u].code_off[i] = (int64_t)(off + (size_t)i * T[u]);
    const size_t n = (size_t)n_codebooks * T[u];
    for (size_t k = 0; k < n && mem == MIA_MEM_HOST; ++k)
      MIA_CHECK_ARG(ctx, codes[off + k] >= 0 && codes[off + k] < c->cb_size, "dac_decode_batch: code %d out of range in utterance %d", codes[off + k], u);
    off += n;
  }
  if (int rc = batch_lengths(c, ut, nullptr, 0, pcm_off, "dac_decode_batch")) return rc;
  const int ones[MIA_MAX_LEVELS] = {1, 1, 1, 1};
  return decode_batch_common(c, ut, ones, n_codebooks, codes, off, nullptr, pcm, pcm_off, n_samples, mem);
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
  Loader L; L.c = c;
  for (int i = 0; i < n_tensors; ++i) if (tensors[i].name && tensors[i].data) L.by_name[tensors[i].name] = &tensors[i];
  const std::string E = "encoder.block.layers.";
  int C = cfg->encoder_dim;
  {  // first conv: 1 -> C channels, k7
    std::vector<float> v, g, b;
    if (L.f32(E + "0.weight_v", v, {C, 7, 1}) && L.f32(E + "0.weight_g", g, {C, 1, 1}) && L.f32(E + "0.bias", b, {C})) {
      Loader::fold_wn(v, g, C, 7, 1, 0);
      c->enc_in_w = L.up(v); c->enc_in_b = L.up(b);
    }
  }
  c->hop = 1;
  const int dils[3] = {1, 3, 9};
  for (int i = 0; i < cfg->n_rates && L.err.empty(); ++i) {
    const int st = cfg->encoder_rates[i];
    MIA_CHECK_ARG(ctx, st >= 1, "dac_load_encoder: bad stride");
    const std::string b = E + std::to_string(1 + i) + ".block.layers.";
    for (int r = 0; r < 3; ++r) add_residual_unit_dac(L, b + std::to_string(r), C, dils[r], c->enc_ops);
    Op dn; dn.kind = OP_CONV; dn.stride = st; dn.pad = (st + 1) / 2;
    dn.a_pre = L.alpha(b + "3.alpha", C, false);
    L.dense_conv(b + "4", 2 * C, 2 * st, C, true, dn);
    c->enc_ops.push_back(dn);
    C *= 2; c->hop *= st;
  }
  {
    Op fin; fin.kind = OP_CONV; fin.pad = 1;
    fin.a_pre = L.alpha(E + std::to_string(1 + cfg->n_rates) + ".alpha", C, false);
    L.dense_conv(E + std::to_string(2 + cfg->n_rates), c->latent, 3, C, true, fin);
    c->enc_ops.push_back(fin);
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
  c->enc_dim = cfg->encoder_dim;
  c->has_encoder = true;
  return MIA_OK;
}

extern "C" int64_t mia_dac_code_len(mia_codec* c, int64_t n_samples) {
  if (!c || !c->has_encoder || n_samples <= 0) return 0;
  int64_t T = (n_samples + c->hop - 1) / c->hop * c->hop;
  for (const Op& op : c->enc_ops) if (op.kind == OP_CONV && op.stride > 1) T = (T + 2 * op.pad - op.taps) / op.stride + 1;
  return T;
}

extern "C" int mia_dac_encode(mia_codec* c, const float* pcm, int64_t n_samples, int n_quantizers, int32_t* codes, int64_t codes_capacity,
                              int64_t* n_steps, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 1 && c->has_encoder, "dac_encode: no encoder loaded (mia_dac_load_encoder)");
  MIA_CHECK_ARG(ctx, pcm && codes && n_samples > 0, "dac_encode: null pointer or empty audio");
  MIA_CHECK_ARG(ctx, mem == MIA_MEM_HOST || mem == MIA_MEM_DEVICE, "dac_encode: bad mem");
  const int nq = n_quantizers <= 0 ? c->n_levels : std::min(n_quantizers, c->n_levels);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t T0 = (n_samples + c->hop - 1) / c->hop * c->hop;          // preprocess: right-pad to the hop length (DACModel.swift:308-317)
  const int64_t Tc = mia_dac_code_len(c, n_samples);
  MIA_CHECK_ARG(ctx, Tc > 0 && codes_capacity >= Tc, "dac_encode: codes buffer too small (%lld < %lld steps)", (long long)codes_capacity, (long long)Tc);
  MIA_CHECK_ARG(ctx, T0 < (1ll << 30), "dac_encode: audio too long for one call");
  // widest activation: the first stage, T0 x encoder_dim (every later stage halves T*C or keeps it)
  size_t max_floats = (size_t)T0 * c->enc_dim;
  { int64_t T = T0; int C = c->enc_dim;
    for (const Op& op : c->enc_ops) if (op.kind == OP_CONV && !op.residual && op.stride != -1) { if (op.stride > 1) T = (T + 2 * op.pad - op.taps) / op.stride + 1; C = op.N; max_floats = std::max(max_floats, (size_t)T * C); } }
  int rc = ensure(c, max_floats);
  if (rc != MIA_OK) return rc;
  if ((rc = ensure_buf(c, c->d_audio, c->audio_cap, (size_t)T0)) != MIA_OK) return rc;
  if ((rc = ensure_buf(c, c->d_ze, c->ze_cap, (size_t)Tc * (size_t)std::max(c->cb_dim, 1))) != MIA_OK) return rc;
  if ((rc = ensure_buf(c, c->d_codes, c->codes_cap, (size_t)nq * Tc)) != MIA_OK) return rc;
  MIA_HIP(ctx, hipMemsetAsync(c->d_audio, 0, (size_t)T0 * 4, s));
  MIA_HIP(ctx, hipMemcpyAsync(c->d_audio, pcm, (size_t)n_samples * 4, mem == MIA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  float* x = c->buf[0]; float* h = c->buf[1]; float* y = c->buf[2];
  int64_t T = T0; int C = c->enc_dim;
  if (codec_conv_in1_launch(c->d_audio, x, c->enc_in_w, c->enc_in_b, T, C, 7, 3, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "dac_encode: input conv launch failed");
  for (const Op& op : c->enc_ops) {
    const bool side = op.stride == -1;
    const int st = op.stride > 1 ? op.stride : 1;
    const int64_t T_out = st > 1 ? (T + 2 * op.pad - op.taps) / st + 1 : T;
    ConvGemmArgs g;
    g.X = op.residual ? h : x; g.ldx = op.Cin; g.T_in = (int)T; g.W = op.w; g.bias = op.b; g.alpha = op.a_pre;
    g.M = (int)T_out; g.N = op.N; g.Cin = op.Cin; g.taps = op.taps; g.dil = op.dil; g.pad = op.pad; g.T_out = (int)T_out; g.x_row_mul = st;
    if (op.residual) { g.R = x; g.ldr = op.N; g.Y = x; g.ldy = op.N; }
    else { g.Y = side ? h : y; g.ldy = op.N; }
    if (const char* e = codec_conv_gemm_check(g)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
    if (codec_conv_gemm_launch(g, 1, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "dac_encode: conv launch failed");
    if (!op.residual && !side) { std::swap(x, y); C = op.N; T = T_out; }
  }
  // residual vector quantisation: x holds z [Tc][latent] and becomes the residual
  for (int i = 0; i < nq; ++i) {
    const Op& ip = c->in_proj[i];
    ConvGemmArgs g;
    g.X = x; g.ldx = c->latent; g.T_in = (int)T; g.W = ip.w; g.bias = ip.b; g.M = (int)T; g.N = c->cb_dim; g.Cin = c->latent; g.T_out = (int)T;
    g.Y = c->d_ze; g.ldy = c->cb_dim;
    if (const char* e = codec_conv_gemm_check(g)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
    if (codec_conv_gemm_launch(g, 1, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "dac_encode: in_proj launch failed");
    if (codec_vq_assign_launch(c->d_ze, c->cbn[i], c->cbn_sq[i], c->codebook[i], c->weff[i], c->ebias[i], x, c->d_codes + (size_t)i * T, (int)T, c->latent,
                               c->cb_size, c->cb_dim, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "dac_encode: vq launch failed");
  }
  if (n_steps) *n_steps = T;
  // codes [nq][T] -> caller's [nq][codes_capacity] rows
  MIA_HIP(ctx, hipMemcpy2DAsync(codes, (size_t)codes_capacity * 4, c->d_codes, (size_t)T * 4, (size_t)T * 4, nq, mem == MIA_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  if (mem == MIA_MEM_HOST) MIA_HIP(ctx, hipStreamSynchronize(s));
  return MIA_OK;
}
