// mimi.hip -- Mimi codec decode (TTS/Marvis/Mimi/): whole clips (Mimi.decode, Mimi.swift:184-192) and carried-state streaming
// (MimiStreamingDecoder.decodeFrames, Mimi.swift:227-238), fp32 like the reference.  Loader, layer program, stream state, C ABI.
// The handle's types and the loader helpers are in mimi_model.h, shared with the optional encode side (mimi_encode.hip).
//
// One layer program serves both entries.  Every convolution is causal, so a call's convolutions run ONCE over [carried context | new
// rows]: a stride-1 convolution carries its last (k - 1) dil input rows, a transposed one (k = 2 stride) its last input row, which
// is the input-side equivalent of the reference's k - stride carried output rows (prevYs, Conv.swift:313-336) -- the overlap the next
// call adds is that row's product with the upper half of the kernel, so carrying the row lets the same tap GEMM form each output's
// whole sum.  A whole-clip decode is the same program over a context of zeros (ELU(0) = 0: the zero padding the reference applies after the ELU).
// What differs between the two entries is the attention, as in the reference ("Mimi"): the whole clip runs full
// bidirectional attention at RoPE offset 0 (attn_f32), a stream the pair-windowed attention against its key history.
//
// Key / value history of a stream: per layer one linear run of rows in position order, [n_layers][2][cap][d_model].  A call appends
// its rows behind the `fill` rows already there; when they no longer fit, the last `context` rows are copied to the front of the
// stream's second buffer and the two swap (a copy between two buffers has no overlap to order).  Rows are therefore always contiguous:
// no call's keys wrap, and the attention and the QKV finish address them without a modulo.  With cap = context + max(rows of the call,
// context + 2) a frame-by-frame stream compacts once every (context + 2) / 2 calls.
#include <algorithm>
#include <cmath>

#include "mimi_model.h"

namespace {

const char* config_error(const mia_mimi_config& g) {
  if (g.d_model <= 0 || g.n_heads <= 0 || g.d_model != g.n_heads * 64) return "head_dim must be 64";
  if (g.kv_repeat != 1) return "kv_repeat must be 1";
  if (g.gating) return "gated feed-forward is not supported";
  if (!g.layer_norm) return "norm must be layer_norm";
  if (!g.seanet_causal) return "the SEANet must be causal";
  if (!g.seanet_pad_constant) return "the SEANet padding mode must be constant";
  if (!g.seanet_true_skip) return "the SEANet residual blocks must use the true skip";
  if (g.seanet_n_residual_layers != 1) return "one residual layer per SEANet stage is supported";
  if (g.upsample_stride != 2) return "the latent upsample stride must be 2";
  if (g.seanet_dimension != g.d_model) return "the transformer width must equal the SEANet dimension";
  if (g.n_layers < 1 || g.n_layers > 64 || g.context < 1 || g.context > 8190) return "n_layers must be in [1, 64] and context in [1, 8190]";
  if (g.nq < 1 || g.nq > 32 || g.bins < 1 || g.quantizer_dim < 1 || g.quantizer_dim > 4096) return "nq must be in [1, 32], bins >= 1, quantizer_dim in [1, 4096]";
  if (g.seanet_n_ratios < 1 || g.seanet_n_ratios > MIMI_MAX_RATIOS) return "1 to 8 SEANet ratios are supported";
  if (g.seanet_ksize < 1 || g.seanet_residual_ksize < 1 || g.seanet_last_ksize < 1 || g.seanet_compress < 1) return "bad SEANet kernel sizes";
  if (g.d_model % 32 || g.dim_feedforward <= 0 || g.dim_feedforward % 32) return "d_model and dim_feedforward must be multiples of 32 (tap GEMM)";
  if (g.seanet_nfilters <= 0 || g.seanet_nfilters % 32 || (g.seanet_nfilters / g.seanet_compress) % 32 || g.seanet_nfilters % g.seanet_compress)
    return "every SEANet channel count (nfilters and nfilters / compress) must be a multiple of 32 (tap GEMM)";
  if ((size_t)g.seanet_last_ksize * g.seanet_nfilters * 4 > 48 * 1024) return "the output convolution's weights must fit 48 KB";
  for (int i = 0; i < g.seanet_n_ratios; ++i) if (g.seanet_ratios[i] < 1) return "SEANet ratios must be >= 1";
  if (g.max_period <= 1) return "max_period must be > 1";
  return nullptr;
}

struct Run {
  mia_mimi* m; mia_mimi_stream* st; hipStream_t s;
  // carried rows in front of a convolution's input: from the stream's state, or zeros
  bool ctx_in(float* buf, size_t off, size_t floats) {
    if (!floats) return true;
    return (st ? hipMemcpyAsync(buf, st->conv_state + off, floats * 4, hipMemcpyDeviceToDevice, s) : hipMemsetAsync(buf, 0, floats * 4, s)) == hipSuccess;
  }
  // ... and the last ctx rows of [context | T new rows] back into the state
  bool ctx_out(const float* buf, size_t off, size_t floats, size_t new_floats) {
    if (!floats || !st) return true;
    return hipMemcpyAsync(st->conv_state + off, buf + new_floats, floats * 4, hipMemcpyDeviceToDevice, s) == hipSuccess;
  }
};

// the program over n frames; d_codes: device [n_q][n]; d_pcm: device, n * spf samples.  ws: the carved workspace.
struct Work { float *zp, *xb, *sb[3]; MimiTfWork tf; };

size_t seanet_buf_floats(const mia_mimi* m, int64_t P) {
  size_t mx = (size_t)(1 + P) * m->init.N;
  int64_t T = P;
  for (int i = 0; i < m->nr; ++i) {
    const SLayer& l = m->sl[i];
    T *= l.up.stride;
    mx = std::max(mx, (size_t)(T + std::max(m->cfg.seanet_residual_ksize, m->cfg.seanet_last_ksize)) * l.up.N);
  }
  return mx;
}

int mimi_run(mia_mimi* m, mia_mimi_stream* st, const int32_t* d_codes, int n_q, int64_t n, float* d_pcm, const Work& w) {
  mia_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  Run r{m, st, s};
  const int D = m->D, k0 = m->cfg.seanet_ksize;
  const int64_t P = n * m->us;
  auto dev_fail = [&](const char* what) { return mia_fail(ctx, MIA_ERR_DEVICE, "mimi: %s failed", what); };

  // ---- quantizer decode and upsample into the transformer's stream (which is also the first convolution's input: k0 - 1 rows of context)
  if (!r.ctx_in(w.zp, m->st_z, D)) return dev_fail("state copy");
  if (mimi_embed_launch(d_codes, n_q, n, m->cb, m->bins, m->dq, m->wfT, m->wrT, w.zp + D, D, s)) return dev_fail("embed launch");
  float* x = w.xb + (size_t)(k0 - 1) * D;
  if (mimi_upsample_launch(w.zp, m->wup, x, n, D, m->us, s)) return dev_fail("upsample launch");
  if (!r.ctx_out(w.zp, m->st_z, D, (size_t)n * D)) return dev_fail("state copy");

  // ---- transformer
  if (int rc = mimi_transformer_run(m, m->layers, st, x, P, w.tf)) return rc;

  // ---- SEANet decoder.  Buffers rotate: a = the stage's input, b = the transposed convolution's output (and the residual), c = hidden.
  auto conv = [&](const MConv& c, const float* X, int64_t T, float* Y, const float* R, int elu) {
    ConvGemmArgs g;          // X: [taps - 1 + T][Cin]
    g.X = X; g.ldx = c.Cin; g.T_in = (int)(T + c.taps - 1); g.W = c.w; g.bias = c.b; g.M = (int)T; g.N = c.N; g.Cin = c.Cin; g.taps = c.taps;
    g.Y = Y; g.ldy = c.N; g.T_out = (int)T; g.R = R; g.ldr = c.N; g.elu_pre = elu;
    return codec_conv_gemm_run(ctx, g, 1, "mimi");
  };
  float *a = w.sb[0], *b = w.sb[1], *c = w.sb[2];
  const int rk = m->cfg.seanet_residual_ksize, lk = m->cfg.seanet_last_ksize;
  if (!r.ctx_in(w.xb, m->st_x, (size_t)(k0 - 1) * D)) return dev_fail("state copy");
  if (int rc = conv(m->init, w.xb, P, a + m->init.N, nullptr, 0)) return rc;
  if (!r.ctx_out(w.xb, m->st_x, (size_t)(k0 - 1) * D, (size_t)P * D)) return dev_fail("state copy");
  int64_t T = P;
  for (int i = 0; i < m->nr; ++i) {
    const SLayer& l = m->sl[i];
    const int Ci = l.up.Cin, Co = l.up.N, s_ = l.up.stride;
    const int64_t To = T * s_;
    if (!r.ctx_in(a, m->st_up[i], Ci)) return dev_fail("state copy");
    if (!r.ctx_in(b, m->st_c3[i], (size_t)(rk - 1) * Co)) return dev_fail("state copy");
    {
      ConvGemmArgs g;          // X: [1 + T][Ci], row 0 = the carried input row; phase z writes rows t * stride + z
      g.X = a; g.ldx = Ci; g.T_in = (int)(T + 1); g.W = l.up.w; g.w_phase_stride = (int64_t)Co * 2 * Ci; g.bias = l.up.b; g.elu_pre = 1;
      g.M = (int)T; g.N = Co; g.Cin = Ci; g.taps = 2;
      g.Y = b + (size_t)(rk - 1) * Co; g.ldy = Co; g.T_out = (int)To; g.y_row_mul = s_; g.y_phase_step = 1;
      if (int rc = codec_conv_gemm_run(ctx, g, s_, "mimi")) return rc;
    }
    if (!r.ctx_out(a, m->st_up[i], Ci, (size_t)T * Ci)) return dev_fail("state copy");
    if (int rc = conv(l.c3, b, To, c, nullptr, 1)) return rc;
    if (!r.ctx_out(b, m->st_c3[i], (size_t)(rk - 1) * Co, (size_t)To * Co)) return dev_fail("state copy");
    const int next_ctx = i + 1 < m->nr ? 1 : lk - 1;
    if (int rc = conv(l.c1, c, To, a + (size_t)next_ctx * Co, b + (size_t)(rk - 1) * Co, 1)) return rc;
    T = To;
  }
  const int nf = m->fin.Cin;
  if (!r.ctx_in(a, m->st_fin, (size_t)(lk - 1) * nf)) return dev_fail("state copy");
  if (mimi_conv_out1_launch(a, m->fin.w, m->fin.b, d_pcm, T, nf, lk, s)) return dev_fail("output conv launch");
  if (!r.ctx_out(a, m->st_fin, (size_t)(lk - 1) * nf, (size_t)T * nf)) return dev_fail("state copy");
  return MIA_OK;
}

// arguments both decode entries share; nothing is launched before it returns MIA_OK.  *empty: a valid call with no frames.
int check_call(mia_mimi* m, const char* who, const int32_t* codes, int n_q, int64_t n, float* pcm, int64_t cap, int mem) {
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "%s: bad mem", who);
  MIA_CHECK_ARG(ctx, n_q >= 1 && n_q <= m->nq, "%s: n_q must be in [1, %d] (got %d)", who, m->nq, n_q);
  MIA_CHECK_ARG(ctx, n >= 0, "%s: negative frame count", who);
  if (n == 0) return MIA_OK;
  MIA_CHECK_ARG(ctx, codes && pcm, "%s: null argument", who);
  MIA_CHECK_ARG(ctx, (double)n * m->spf * m->cfg.seanet_nfilters * 2.0 < 1073741824.0, "%s: %lld frames in one call exceed the 31-bit row offsets of the tap GEMM", who, (long long)n);
  for (int64_t k = 0; k < (int64_t)n_q * n; ++k)
    if (codes[k] < 0 || codes[k] >= m->bins)
      return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s: id %d of codebook %lld, frame %lld is outside [0, %d)", who, codes[k], (long long)(k / n), (long long)(k % n), m->bins);
  MIA_CHECK_ARG(ctx, cap >= n * m->spf, "%s: pcm buffer too small (%lld < %lld)", who, (long long)cap, (long long)(n * m->spf));
  return MIA_OK;
}

int decode_call(mia_mimi* m, mia_mimi_stream* st, const int32_t* codes, int n_q, int64_t n, float* pcm, int64_t* n_samples, int mem) {
  mia_ctx* ctx = m->ctx;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const int D = m->D;
  const int64_t P = n * m->us, S = n * m->spf;
  HostIo io(ctx, mem);
  Carve cv;
  const size_t o_codes = cv.add((size_t)n_q * n * 4), o_pcm = cv.add(io.staged((size_t)S * 4));
  const size_t o_zp = cv.add((size_t)(1 + n) * D * 4), o_xb = cv.add((size_t)(m->cfg.seanet_ksize - 1 + P) * D * 4);
  const size_t o_nb = cv.add((size_t)P * D * 4), o_qkv = cv.add((size_t)P * 3 * D * 4), o_qb = cv.add((size_t)P * D * 4), o_ob = cv.add((size_t)P * D * 4);
  const size_t o_ff = cv.add((size_t)P * m->FF * 4);
  const size_t o_kt = cv.add(st ? 0 : (size_t)P * D * 4), o_vt = cv.add(st ? 0 : (size_t)P * D * 4);
  const size_t sbf = seanet_buf_floats(m, P);
  size_t o_sb[3];
  for (int i = 0; i < 3; ++i) o_sb[i] = cv.add(sbf * 4);
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  if (st) {              // room for this call's rows in the key / value history
    const size_t ctxr = (size_t)m->context;
    if ((size_t)st->fill + (size_t)P > st->cap[st->cur]) {
      const size_t keep = std::min((size_t)st->fill, ctxr);
      const int o = st->cur ^ 1;
      if (st->cap[o] < keep + (size_t)P) {
        const size_t rows = ctxr + std::max((size_t)P, ctxr + 2);
        size_t have = st->cap[o] * 2 * m->L * D;
        st->cap[o] = 0;
        if (int rc = mia_grow(ctx, st->hist[o], have, rows * 2 * m->L * D, "mimi: hipMalloc failed")) return rc;
        st->cap[o] = rows;
      }
      if (keep)
        MIA_HIP(ctx, hipMemcpy2DAsync(st->hist[o], st->cap[o] * D * 4, st->hist[st->cur] + ((size_t)st->fill - keep) * D, st->cap[st->cur] * D * 4,
                                      keep * D * 4, (size_t)2 * m->L, hipMemcpyDeviceToDevice, ctx->stream));
      st->cur = o;
      st->fill = (int64_t)keep;
    }
  }
  Work w;
  auto f = [&](size_t off) { return (float*)(ws + off); };
  w.zp = f(o_zp); w.xb = f(o_xb); w.tf = MimiTfWork{f(o_nb), f(o_qkv), f(o_qb), f(o_ob), f(o_ff), f(o_kt), f(o_vt)};
  for (int i = 0; i < 3; ++i) w.sb[i] = f(o_sb[i]);
  const int32_t* d_codes = io.table(codes, ws + o_codes, (size_t)n_q * n * 4);       // codes are host arrays whatever `mem` says of pcm
  float* d_pcm = io.out(pcm, ws + o_pcm, (size_t)S * 4);
  int rc = mimi_run(m, st, d_codes, n_q, n, d_pcm, w);
  if (st) {
    if (rc != MIA_OK) { st->broken = true; return rc; }
    st->fill += P; st->pos += P;
  }
  if (rc != MIA_OK) return rc;
  if (n_samples) *n_samples = S;
  return io.finish();
}

}  // namespace

int mimi_transformer_run(mia_mimi* m, const std::vector<MLayer>& layers, mia_mimi_stream* st, float* x, int64_t P, const MimiTfWork& w) {
  mia_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int D = m->D;
  auto dev_fail = [&](const char* what) { return mia_fail(ctx, MIA_ERR_DEVICE, "mimi: %s failed", what); };
  const int64_t pos0 = st ? st->pos : 0;
  auto gemm = [&](const float* X, int K, const float* W, int N, float* Y, const float* R, int act) {
    ConvGemmArgs g;
    g.X = X; g.ldx = K; g.T_in = (int)P; g.W = W; g.M = (int)P; g.N = N; g.Cin = K; g.taps = 1;
    g.Y = Y; g.ldy = N; g.T_out = (int)P; g.R = R; g.ldr = N; g.gelu = act;
    return codec_conv_gemm_run(ctx, g, 1, "mimi");
  };
  for (int l = 0; l < (int)layers.size(); ++l) {
    const MLayer& ly = layers[l];
    if (mia_norm_launch(x, D, ly.ln1g, ly.ln1b, w.nb, D, (int)P, D, 1e-5f, false, MIA_F32, s)) return dev_fail("norm launch");
    if (int rc = gemm(w.nb, D, ly.win, 3 * D, w.qkv, nullptr, 0)) return rc;
    float *kn = w.kt, *vn = w.vt, *Kl = nullptr, *Vl = nullptr;
    if (st) {
      const size_t cap = st->cap[st->cur];
      Kl = st->hist[st->cur] + ((size_t)l * 2 * cap) * D;
      Vl = Kl + cap * D;
      kn = Kl + (size_t)st->fill * D;
      vn = Vl + (size_t)st->fill * D;
    }
    if (mimi_qkv_finish_launch(w.qkv, w.qb, kn, vn, P, D, pos0, m->inv_freq, s)) return dev_fail("qkv finish launch");
    if (st) {
      if (mimi_window_attn_launch(w.qb, Kl, Vl, w.ob, P, D, m->H, pos0, pos0 - st->fill, m->context, 0.125f, s)) return dev_fail("window attention launch");
    } else {
      AttnF32Args a;
      a.q = w.qb; a.ldq = D; a.k = kn; a.ldk = D; a.v = vn; a.ldv = D; a.out = w.ob; a.ldo = D; a.B = 1; a.T = (int)P; a.H = m->H; a.scale = 0.125f;
      if (const char* e = mia_attn_f32_check(a)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "mimi: %s", e);
      if (mia_attn_f32_launch(a, s)) return dev_fail("attention launch");
    }
    if (int rc = gemm(w.ob, D, ly.wout, D, x, x, 0)) return rc;
    if (mia_norm_launch(x, D, ly.ln2g, ly.ln2b, w.nb, D, (int)P, D, 1e-5f, false, MIA_F32, s)) return dev_fail("norm launch");
    if (int rc = gemm(w.nb, D, ly.w1, m->FF, w.ff, nullptr, 7)) return rc;
    if (int rc = gemm(w.ff, m->FF, ly.w2, D, x, x, 0)) return rc;
  }
  return MIA_OK;
}

extern "C" {

mia_mimi* mia_mimi_load(mia_ctx* ctx, const mia_mimi_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "mimi_load: null argument"); return nullptr; }
  const mia_mimi_config& g = *cfg;
  if (const char* e = config_error(g)) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "mimi_load: %s", e); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { mia_fail(ctx, MIA_ERR_DEVICE, "mimi_load: hipSetDevice failed"); return nullptr; }
  mia_mimi* m = new mia_mimi();
  m->ctx = ctx; m->cfg = g;
  m->D = g.d_model; m->H = g.n_heads; m->L = g.n_layers; m->FF = g.dim_feedforward; m->context = g.context; m->us = g.upsample_stride;
  m->nq = g.nq; m->bins = g.bins; m->dq = g.quantizer_dim; m->nr = g.seanet_n_ratios;
  m->spf = m->us; for (int i = 0; i < m->nr; ++i) m->spf *= g.seanet_ratios[i];
  MLoader L; L.allocs = &m->allocs; L.index(tensors, n_tensors);
  const int D = m->D, dq = m->dq;
  bool ok = true;
  {   // codebooks: embedding_sum / max(cluster_usage, 1e-5) (Quantization.swift:38-42), all nq in one table
    std::vector<float> cb((size_t)m->nq * m->bins * dq), es, cu;
    for (int i = 0; i < m->nq && ok; ++i) {
      const std::string p = i == 0 ? "quantizer.rvq_first.vq.layers.0.codebook." : "quantizer.rvq_rest.vq.layers." + std::to_string(i - 1) + ".codebook.";
      ok = L.f32(p + "embedding_sum", es, {m->bins, dq}) && L.f32(p + "cluster_usage", cu, {m->bins});
      for (int b = 0; b < m->bins && ok; ++b) {
        const float u = std::max(cu[b], 1e-5f);
        for (int j = 0; j < dq; ++j) cb[((size_t)i * m->bins + b) * dq + j] = es[(size_t)b * dq + j] / u;
      }
    }
    if (ok) m->cb = L.up(cb);
  }
  ok = ok && L.projT("quantizer.rvq_first.output_proj.weight", D, dq, m->wfT);
  if (ok && m->nq > 1) ok = L.projT("quantizer.rvq_rest.output_proj.weight", D, dq, m->wrT);
  if (ok) { std::vector<float> wu; ok = L.f32("upsample.convtr.convtr.weight", wu, {1, 2 * m->us, D}); if (ok) m->wup = L.up(wu); }
  {
    std::vector<double> fr(32);
    for (int i = 0; i < 32; ++i) fr[i] = g.rope ? std::pow((double)g.max_period, -(double)(2 * i) / 64.0) : 0.0;
    m->inv_freq = (double*)L.put(fr.data(), fr.size() * 8);
  }
  ok = ok && L.transformer("decoder_transformer", g, m->layers);
  // SEANet decoder (Seanet.swift:334-387)
  int C = g.seanet_nfilters << m->nr;
  size_t off = 0;
  m->st_z = off; off += D;
  m->st_x = off; off += (size_t)(g.seanet_ksize - 1) * D;
  ok = ok && L.conv("decoder.init_conv1d.conv.conv", C, g.seanet_ksize, D, m->init);
  for (int i = 0; i < m->nr && ok; ++i) {
    const std::string p = "decoder.layers." + std::to_string(i) + ".";
    const int Co = C / 2, hid = Co / g.seanet_compress;
    SLayer& l = m->sl[i];
    ok = L.convt(p + "upsample.convtr.convtr", Co, g.seanet_ratios[i], C, l.up) &&
         L.conv(p + "residuals.0.block.0.conv.conv", hid, g.seanet_residual_ksize, Co, l.c3) &&
         L.conv(p + "residuals.0.block.1.conv.conv", Co, 1, hid, l.c1);
    m->st_up[i] = off; off += C;
    m->st_c3[i] = off; off += (size_t)(g.seanet_residual_ksize - 1) * Co;
    C = Co;
  }
  if (ok) {
    std::vector<float> w, b;
    ok = L.f32("decoder.final_conv1d.conv.conv.weight", w, {1, g.seanet_last_ksize, C}) && L.f32("decoder.final_conv1d.conv.conv.bias", b, {1});
    if (ok) { m->fin.w = L.up(w); m->fin.b = L.up(b); m->fin.N = 1; m->fin.Cin = C; m->fin.taps = g.seanet_last_ksize; }
  }
  m->st_fin = off; off += (size_t)(g.seanet_last_ksize - 1) * C;
  m->st_floats = off;
  ok = ok && mimi_encoder_load(m, L);
  if (!ok || !L.err.empty()) {
    mia_fail(ctx, L.err.empty() ? MIA_ERR_INVALID_ARGUMENT : L.code, "mimi_load: %s", L.err.empty() ? "failed" : L.err.c_str());
    mia_mimi_free(m);
    return nullptr;
  }
  return m;
}

void mia_mimi_free(mia_mimi* m) {
  if (!m) return;
  (void)hipStreamSynchronize(m->ctx->stream);
  for (void* p : m->allocs) (void)hipFree(p);
  delete m;
}

int64_t mia_mimi_output_len(mia_mimi* m, int64_t n_frames) { return !m || n_frames <= 0 ? 0 : n_frames * m->spf; }

int mia_mimi_decode(mia_mimi* m, const int32_t* codes, int n_q, int64_t T, float* pcm, int64_t pcm_capacity, int64_t* n_samples, int pcm_mem) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  if (int rc = check_call(m, "mimi_decode", codes, n_q, T, pcm, pcm_capacity, pcm_mem)) return rc;
  if (T == 0) { if (n_samples) *n_samples = 0; return MIA_OK; }
  return decode_call(m, nullptr, codes, n_q, T, pcm, n_samples, pcm_mem);
}

mia_mimi_stream* mia_mimi_stream_create(mia_mimi* m) {
  if (!m) return nullptr;
  mia_ctx* ctx = m->ctx;
  if (hipSetDevice(ctx->device) != hipSuccess) { mia_fail(ctx, MIA_ERR_DEVICE, "mimi_stream_create: hipSetDevice failed"); return nullptr; }
  mia_mimi_stream* s = new mia_mimi_stream();
  s->m = m;
  if (hipMalloc((void**)&s->conv_state, m->st_floats * 4 + 64) != hipSuccess) {
    mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "mimi_stream_create: hipMalloc failed");
    delete s;
    return nullptr;
  }
  if (mia_mimi_stream_reset(s) != MIA_OK) { (void)hipFree(s->conv_state); delete s; return nullptr; }
  ++m->live_streams;
  return s;
}

void mia_mimi_stream_free(mia_mimi_stream* s) {
  if (!s) return;
  (void)hipStreamSynchronize(s->m->ctx->stream);
  if (s->conv_state) (void)hipFree(s->conv_state);
  for (int i = 0; i < 2; ++i) if (s->hist[i]) (void)hipFree(s->hist[i]);
  --s->m->live_streams;
  delete s;
}

int mia_mimi_stream_reset(mia_mimi_stream* s) {
  if (!s) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = s->m->ctx;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipMemsetAsync(s->conv_state, 0, s->m->st_floats * 4, ctx->stream));
  s->fill = 0; s->pos = 0; s->n_q = -1; s->broken = false;
  return MIA_OK;
}

int mia_mimi_stream_decode(mia_mimi_stream* s, const int32_t* codes, int n_q, int64_t n, float* pcm, int64_t pcm_capacity, int64_t* n_samples, int pcm_mem) {
  if (!s) return MIA_ERR_MODEL_NOT_LOADED;
  mia_mimi* m = s->m;
  if (int rc = check_call(m, "mimi_stream_decode", codes, n_q, n, pcm, pcm_capacity, pcm_mem)) return rc;
  MIA_CHECK_ARG(m->ctx, !s->broken, "mimi_stream_decode: an earlier call failed on the device, reset the stream first");
  MIA_CHECK_ARG(m->ctx, s->n_q < 0 || s->n_q == n_q, "mimi_stream_decode: n_q changed from %d to %d within a stream (reset it first)", s->n_q, n_q);
  if (n == 0) { if (n_samples) *n_samples = 0; return MIA_OK; }
  s->n_q = n_q;
  return decode_call(m, s, codes, n_q, n, pcm, n_samples, pcm_mem);
}

}  // extern "C"
