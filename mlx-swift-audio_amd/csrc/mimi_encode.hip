// mimi_encode.hip -- Mimi encode (Mimi.encode, TTS/Marvis/Mimi/Mimi.swift:174-182; the audio half of MarvisTTS.tokenizeAudio,
// MarvisTTS.swift:318-348), fp32 like the reference: the optional encode side of a mia_mimi handle.  Loader, layer program, C ABI.
//
// Lengths.  StreamableConv1d.callAsFunction (Conv.swift:212-230) pads k_eff - stride in front and getExtraPaddingForConv1d behind, so a
// k = 2 r, stride r stage maps L rows to ceil(L / r) (r zero rows in front, ceil(L / r) r - L behind) and a stride-1 convolution keeps
// L.  n_samples therefore becomes P = the ceil chain over the ratios reversed, and T = ceil(P / downsample_stride) code frames.  The tap
// GEMM reads rows before 0 and past T_in as zero AFTER its ELU prologue, which is the reference's zero padding behind the ELU.
// The latent downsample pads with .edge instead; its rows are materialised (mimi_edge_rows).
//
// The encoder transformer gets a fresh cache and mask nil: full bidirectional attention over the P positions at RoPE offset 0, the
// program of the whole-clip decode (mimi_transformer_run) over the encoder_transformer weights.
//
// Clip limit: n_samples * nfilters <= 2^27, i.e. 2^21 samples (87 s at 24 kHz) for mimi_202407.  The widest activations are the
// three rotating SEANet buffers of n_samples x nfilters floats, 512 MiB each at the limit; the tap GEMM's 31-bit row offsets would
// allow four times as much.
#include <algorithm>
#include <cmath>

#include "host_io.h"
#include "mimi_model.h"

namespace {

constexpr double ENC_MAX_ROW_FLOATS = 134217728.0;      // 2^27

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// transformer positions of n_samples samples
int64_t enc_positions(const mia_mimi* m, int64_t n_samples) {
  int64_t L = n_samples;
  for (int i = 0; i < m->nr; ++i) L = ceil_div(L, m->enc.el[i].ratio);
  return L;
}

// fp32 sum of squares, pairwise below 8 terms' worth of blocks (the error of a 256-term serial sum is a few ulps of the result)
float sumsq(const float* v, int n) {
  if (n <= 8) { float s = 0.f; for (int i = 0; i < n; ++i) s += v[i] * v[i]; return s; }
  const int h = n / 2;
  return sumsq(v, h) + sumsq(v + h, n - h);
}

struct EncWork {
  float *sb[3], *x, *stg;
  MimiTfWork tf;
};
struct QWork {
  float *proj, *rb[2], *pd[3];
  int32_t* pi[3];
};

size_t enc_buf_floats(const mia_mimi* m, int64_t n_samples) {
  size_t mx = (size_t)n_samples * m->cfg.seanet_nfilters;
  int64_t L = n_samples;
  for (int i = 0; i < m->nr; ++i) {
    const ELayer& l = m->enc.el[i];
    L = ceil_div(L, l.ratio);
    mx = std::max(mx, (size_t)L * l.down.N);
  }
  return mx;
}

// pcm (device, n_samples) -> latent (device, [T][D])
int encode_latent_run(mia_mimi* m, const float* d_pcm, int64_t n_samples, float* d_lat, const EncWork& w) {
  mia_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const MimiEncoder& e = m->enc;
  const int D = m->D, us = m->us;
  auto dev_fail = [&](const char* what) { return mia_fail(ctx, MIA_ERR_DEVICE, "mimi_encode: %s failed", what); };
  auto conv = [&](const MConv& c, const float* X, int64_t Tin, int stride, int pad, int64_t Tout, float* Y, const float* R) {
    ConvGemmArgs g;          // rows before 0 and past Tin read as zero behind the ELU prologue
    g.X = X; g.ldx = c.Cin; g.T_in = (int)Tin; g.W = c.w; g.bias = c.b; g.M = (int)Tout; g.N = c.N; g.Cin = c.Cin; g.taps = c.taps; g.pad = pad;
    g.x_row_mul = stride; g.Y = Y; g.ldy = c.N; g.T_out = (int)Tout; g.R = R; g.ldr = c.N; g.elu_pre = 1;
    return codec_conv_gemm_run(ctx, g, 1, "mimi_encode");
  };
  // ---- SEANet encoder (Seanet.swift:167-276).  a = the stage's input (and the residual), c = hidden, b = the block's output
  float *a = w.sb[0], *b = w.sb[1], *c = w.sb[2];
  const int k0 = m->cfg.seanet_ksize, rk = m->cfg.seanet_residual_ksize, lk = m->cfg.seanet_last_ksize;
  if (codec_conv_in1_launch(d_pcm, a, e.in_w, e.in_b, n_samples, m->cfg.seanet_nfilters, k0, k0 - 1, s)) return dev_fail("input conv launch");
  int64_t L = n_samples;
  for (int i = 0; i < m->nr; ++i) {
    const ELayer& l = e.el[i];
    if (int rc = conv(l.c3, a, L, 1, rk - 1, L, c, nullptr)) return rc;
    if (int rc = conv(l.c1, c, L, 1, 0, L, b, a)) return rc;
    const int64_t Lo = ceil_div(L, l.ratio);
    if (int rc = conv(l.down, b, L, l.ratio, l.ratio, Lo, a, nullptr)) return rc;
    L = Lo;
  }
  const int64_t P = L, T = ceil_div(P, us);
  if (int rc = conv(e.fin, a, P, 1, lk - 1, P, w.x, nullptr)) return rc;
  // ---- encoder transformer, then the edge-padded k = 2 us, stride us downsample (Conv.swift:341-355)
  if (int rc = mimi_transformer_run(m, e.layers, nullptr, w.x, P, w.tf)) return rc;
  const int back = (int)(T * us - P);
  if (mimi_edge_rows_launch(w.x, w.stg, P, D, us, back, s)) return dev_fail("edge staging launch");
  ConvGemmArgs g;
  g.X = w.stg; g.ldx = D; g.T_in = (int)(us + P + back); g.W = e.wdown; g.M = (int)T; g.N = D; g.Cin = D; g.taps = 2 * us; g.x_row_mul = us;
  g.Y = d_lat; g.ldy = D; g.T_out = (int)T;
  return codec_conv_gemm_run(ctx, g, 1, "mimi_encode");
}

// latent (device, [T][D]) -> codes (device, [n_q][T]): SplitResidualVectorQuantizer.encode, the first n_q stages
int quantize_run(mia_mimi* m, const float* d_lat, int64_t T, int n_q, int32_t* d_codes, const QWork& w) {
  mia_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const int D = m->D, dq = m->dq, bins = m->bins;
  {   // both input projections in one GEMM: columns [0, dq) = rvq_first, [dq, 2 dq) = rvq_rest
    ConvGemmArgs g;
    g.X = d_lat; g.ldx = D; g.T_in = (int)T; g.W = m->enc.wproj; g.M = (int)T; g.N = m->nq > 1 ? 2 * dq : dq; g.Cin = D; g.taps = 1;
    g.Y = w.proj; g.ldy = 2 * dq; g.T_out = (int)T;
    if (int rc = codec_conv_gemm_run(ctx, g, 1, "mimi_quantize")) return rc;
  }
  auto fail = [&]() { return mia_fail(ctx, MIA_ERR_DEVICE, "mimi_quantize: chain stage launch failed"); };
  const size_t book = (size_t)bins * dq;
  MimiRvqChain first;
  first.r_in = w.proj; first.ld_in = 2 * dq; first.e = m->cb; first.c2 = m->enc.c2; first.pd = w.pd[2]; first.pi = w.pi[2];
  if (n_q == 1) {
    if (mimi_rvq_stage_launch(first, MimiRvqChain(), T, bins, dq, s)) return fail();
    if (mimi_rvq_finish_launch(w.pd[2], w.pi[2], d_codes, nullptr, nullptr, nullptr, T, bins, s)) return fail();
    return MIA_OK;
  }
  // rvq_rest: stage i works on r_i; r_1 = its projection, r_i = r_(i-1) - e_(i-1)[code_(i-1)] is formed by stage i's prologue
  for (int i = 1; i < n_q; ++i) {
    MimiRvqChain c;
    c.e = m->cb + (size_t)i * book; c.c2 = m->enc.c2 + (size_t)i * bins; c.pd = w.pd[i & 1]; c.pi = w.pi[i & 1];
    if (i <= 2) { c.r_in = w.proj + dq; c.ld_in = 2 * dq; } else { c.r_in = w.rb[(i - 1) & 1]; c.ld_in = dq; }
    if (i > 1) {
      c.prev_pd = w.pd[(i - 1) & 1]; c.prev_pi = w.pi[(i - 1) & 1]; c.e_prev = m->cb + (size_t)(i - 1) * book;
      c.prev_codes = d_codes + (size_t)(i - 1) * T; c.r_out = w.rb[i & 1];
    }
    if (mimi_rvq_stage_launch(c, i == 1 ? first : MimiRvqChain(), T, bins, dq, s)) return fail();
  }
  const int last = (n_q - 1) & 1;
  if (mimi_rvq_finish_launch(w.pd[last], w.pi[last], d_codes + (size_t)(n_q - 1) * T, w.pd[2], w.pi[2], d_codes, T, bins, s)) return fail();
  return MIA_OK;
}

// ---- workspace carving of the two halves
struct EncCarve { size_t sb[3], x, stg, nb, qkv, qb, ob, ff, kt, vt; };
EncCarve carve_enc(Carve& cv, const mia_mimi* m, int64_t n_samples, int64_t P, int64_t T) {
  EncCarve o;
  const size_t D = m->D, sbf = enc_buf_floats(m, n_samples);
  for (int i = 0; i < 3; ++i) o.sb[i] = cv.add(sbf * 4);
  o.x = cv.add((size_t)P * D * 4); o.stg = cv.add((size_t)(m->us + T * m->us) * D * 4);
  o.nb = cv.add((size_t)P * D * 4); o.qkv = cv.add((size_t)P * 3 * D * 4); o.qb = cv.add((size_t)P * D * 4); o.ob = cv.add((size_t)P * D * 4);
  o.ff = cv.add((size_t)P * m->FF * 4); o.kt = cv.add((size_t)P * D * 4); o.vt = cv.add((size_t)P * D * 4);
  return o;
}
EncWork enc_work(char* ws, const EncCarve& o) {
  auto f = [&](size_t off) { return (float*)(ws + off); };
  EncWork w;
  for (int i = 0; i < 3; ++i) w.sb[i] = f(o.sb[i]);
  w.x = f(o.x); w.stg = f(o.stg);
  w.tf = MimiTfWork{f(o.nb), f(o.qkv), f(o.qb), f(o.ob), f(o.ff), f(o.kt), f(o.vt)};
  return w;
}
struct QCarve { size_t proj, rb[2], pd[3], pi[3], codes; };
QCarve carve_q(Carve& cv, const mia_mimi* m, int64_t T, int n_q) {
  QCarve o;
  const size_t part = (size_t)mimi_rvq_slices(m->bins) * (size_t)ceil_div(T, MIMI_RVQ_TILE) * MIMI_RVQ_TILE;
  o.proj = cv.add((size_t)T * 2 * m->dq * 4);
  for (int i = 0; i < 2; ++i) o.rb[i] = cv.add((size_t)T * m->dq * 4);
  for (int i = 0; i < 3; ++i) { o.pd[i] = cv.add(part * 4); o.pi[i] = cv.add(part * 4); }
  o.codes = cv.add((size_t)n_q * T * 4);
  return o;
}
QWork q_work(char* ws, const QCarve& o) {
  QWork w;
  w.proj = (float*)(ws + o.proj);
  for (int i = 0; i < 2; ++i) w.rb[i] = (float*)(ws + o.rb[i]);
  for (int i = 0; i < 3; ++i) { w.pd[i] = (float*)(ws + o.pd[i]); w.pi[i] = (int32_t*)(ws + o.pi[i]); }
  return w;
}

// what every entry that takes samples refuses before anything is launched
int check_clip(mia_mimi* m, const char* who, const float* pcm, int64_t n_samples, int mem) {
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, m->has_encoder, "%s: no encoder loaded (the checkpoint carried no encoder-side tensors)", who);
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "%s: bad mem", who);
  MIA_CHECK_ARG(ctx, pcm, "%s: null argument", who);
  MIA_CHECK_ARG(ctx, n_samples >= 1, "%s: n_samples must be >= 1 (got %lld)", who, (long long)n_samples);
  MIA_CHECK_ARG(ctx, (double)n_samples * m->cfg.seanet_nfilters <= ENC_MAX_ROW_FLOATS, "%s: %lld samples in one call exceed the limit of %lld", who,
                (long long)n_samples, (long long)(ENC_MAX_ROW_FLOATS / m->cfg.seanet_nfilters));
  return MIA_OK;
}

}  // namespace

bool mimi_encoder_load(mia_mimi* m, MLoader& L) {
  bool any = false;
  for (const auto& kv : L.by_name) {
    const std::string& k = kv.first;
    if (k.rfind("encoder.", 0) == 0 || k.rfind("encoder_transformer.", 0) == 0 || k.rfind("downsample.", 0) == 0 || k.find(".input_proj.") != std::string::npos) { any = true; break; }
  }
  if (!any) return true;
  const mia_mimi_config& g = m->cfg;
  const int D = m->D, dq = m->dq, nf = g.seanet_nfilters;
  if (dq % 8 || dq > 504) return L.fail(MIA_ERR_INVALID_ARGUMENT, "the encode side needs quantizer_dim to be a multiple of 8, at most 504");
  if (nf % 4) return L.fail(MIA_ERR_INVALID_ARGUMENT, "the encode side needs nfilters to be a multiple of 4");
  MimiEncoder& e = m->enc;
  {
    std::vector<float> w, b;
    if (!L.f32("encoder.init_conv1d.conv.conv.weight", w, {nf, g.seanet_ksize, 1}) || !L.f32("encoder.init_conv1d.conv.conv.bias", b, {nf})) return false;
    e.in_w = L.up(w); e.in_b = L.up(b);
  }
  int C = nf;
  for (int i = 0; i < m->nr; ++i) {       // SeanetEncoder runs the ratios reversed (Seanet.swift:236)
    const std::string p = "encoder.layers." + std::to_string(i) + ".";
    ELayer& l = e.el[i];
    l.ratio = g.seanet_ratios[m->nr - 1 - i];
    const int hid = C / g.seanet_compress;
    if (!L.conv(p + "residuals.0.block.0.conv.conv", hid, g.seanet_residual_ksize, C, l.c3) || !L.conv(p + "residuals.0.block.1.conv.conv", C, 1, hid, l.c1) ||
        !L.conv(p + "downsample.conv.conv", 2 * C, 2 * l.ratio, C, l.down)) return false;
    C *= 2;
  }
  if (!L.conv("encoder.final_conv1d.conv.conv", g.seanet_dimension, g.seanet_last_ksize, C, e.fin)) return false;
  if (!L.transformer("encoder_transformer", g, e.layers)) return false;
  {
    std::vector<float> w;
    if (!L.f32("downsample.conv.conv.weight", w, {D, 2 * m->us, D})) return false;
    e.wdown = L.up(w);
  }
  {
    std::vector<float> wf, wr, both;
    if (!L.f32("quantizer.rvq_first.input_proj.weight", wf, {dq, 1, D})) return false;
    if (m->nq > 1 && !L.f32("quantizer.rvq_rest.input_proj.weight", wr, {dq, 1, D})) return false;
    both = wf;
    both.insert(both.end(), wr.begin(), wr.end());
    e.wproj = L.up(both);
  }
  {   // c2 = ||e||^2 / 2 (Quantization.swift:50-56) of the entries the decode side built: the same formula on the same tensors
    std::vector<float> c2((size_t)m->nq * m->bins), es, cu, row(dq);
    for (int i = 0; i < m->nq; ++i) {
      const std::string p = i == 0 ? "quantizer.rvq_first.vq.layers.0.codebook." : "quantizer.rvq_rest.vq.layers." + std::to_string(i - 1) + ".codebook.";
      if (!L.f32(p + "embedding_sum", es, {m->bins, dq}) || !L.f32(p + "cluster_usage", cu, {m->bins})) return false;
      for (int b = 0; b < m->bins; ++b) {
        const float u = std::max(cu[b], 1e-5f);
        for (int j = 0; j < dq; ++j) row[j] = es[(size_t)b * dq + j] / u;
        c2[(size_t)i * m->bins + b] = sumsq(row.data(), dq) / 2.0f;
      }
    }
    e.c2 = L.up(c2);
  }
  m->has_encoder = L.err.empty();
  return L.err.empty();
}

extern "C" {

int64_t mia_mimi_encode_frames(mia_mimi* m, int64_t n_samples) {
  if (!m || !m->has_encoder || n_samples <= 0) return 0;
  return ceil_div(enc_positions(m, n_samples), m->us);
}

int mia_mimi_encode_latent(mia_mimi* m, const float* pcm, int64_t n_samples, float* latent, int64_t capacity, int64_t* n_frames, int data_mem) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  if (int rc = check_clip(m, "mimi_encode_latent", pcm, n_samples, data_mem)) return rc;
  MIA_CHECK_ARG(ctx, latent, "mimi_encode_latent: null argument");
  const int64_t P = enc_positions(m, n_samples), T = ceil_div(P, m->us);
  MIA_CHECK_ARG(ctx, capacity >= T, "mimi_encode_latent: latent buffer too small (%lld < %lld frames)", (long long)capacity, (long long)T);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io(ctx, data_mem);
  Carve cv;
  const size_t o_pcm = cv.add(io.staged((size_t)n_samples * 4)), o_lat = cv.add(io.staged((size_t)T * m->D * 4));
  const EncCarve ec = carve_enc(cv, m, n_samples, P, T);
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  const float* d_pcm = io.in(pcm, ws + o_pcm, (size_t)n_samples * 4);
  float* d_lat = io.out(latent, ws + o_lat, (size_t)T * m->D * 4);
  if (int rc = encode_latent_run(m, d_pcm, n_samples, d_lat, enc_work(ws, ec))) return rc;
  if (n_frames) *n_frames = T;
  return io.finish();
}

int mia_mimi_quantize(mia_mimi* m, const float* latent, int64_t T, int n_q, int32_t* codes, int latent_mem) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, m->has_encoder, "mimi_quantize: no encoder loaded (the checkpoint carried no encoder-side tensors)");
  MIA_CHECK_ARG(ctx, HostIo::valid(latent_mem), "mimi_quantize: bad mem");
  MIA_CHECK_ARG(ctx, latent && codes, "mimi_quantize: null argument");
  MIA_CHECK_ARG(ctx, n_q >= 1 && n_q <= m->nq, "mimi_quantize: n_q must be in [1, %d] (got %d)", m->nq, n_q);
  MIA_CHECK_ARG(ctx, T >= 1 && T <= (1 << 21), "mimi_quantize: T must be in [1, %d] (got %lld)", 1 << 21, (long long)T);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io(ctx, latent_mem);
  Carve cv;
  const size_t o_lat = cv.add(io.staged((size_t)T * m->D * 4));
  const QCarve qc = carve_q(cv, m, T, n_q);
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  const float* d_lat = io.in(latent, ws + o_lat, (size_t)T * m->D * 4);
  int32_t* d_codes = (int32_t*)(ws + qc.codes);
  if (int rc = quantize_run(m, d_lat, T, n_q, d_codes, q_work(ws, qc))) return rc;
  io.fetch(codes, d_codes, (size_t)n_q * T * 4);          // codes are a host array whatever `latent_mem` says of the latent
  return io.finish();
}

int mia_mimi_encode(mia_mimi* m, const float* pcm, int64_t n_samples, int n_q, int32_t* codes, int64_t codes_capacity, int64_t* n_frames, int pcm_mem) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  if (int rc = check_clip(m, "mimi_encode", pcm, n_samples, pcm_mem)) return rc;
  MIA_CHECK_ARG(ctx, codes, "mimi_encode: null argument");
  MIA_CHECK_ARG(ctx, n_q >= 1 && n_q <= m->nq, "mimi_encode: n_q must be in [1, %d] (got %d)", m->nq, n_q);
  const int64_t P = enc_positions(m, n_samples), T = ceil_div(P, m->us);
  MIA_CHECK_ARG(ctx, codes_capacity >= T, "mimi_encode: codes buffer too small (%lld < %lld frames)", (long long)codes_capacity, (long long)T);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io(ctx, pcm_mem);
  Carve cv;
  const size_t o_pcm = cv.add(io.staged((size_t)n_samples * 4)), o_lat = cv.add((size_t)T * m->D * 4);
  const EncCarve ec = carve_enc(cv, m, n_samples, P, T);
  const QCarve qc = carve_q(cv, m, T, n_q);
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  const float* d_pcm = io.in(pcm, ws + o_pcm, (size_t)n_samples * 4);
  float* d_lat = (float*)(ws + o_lat);
  if (int rc = encode_latent_run(m, d_pcm, n_samples, d_lat, enc_work(ws, ec))) return rc;
  int32_t* d_codes = (int32_t*)(ws + qc.codes);
  if (int rc = quantize_run(m, d_lat, T, n_q, d_codes, q_work(ws, qc))) return rc;
  if (n_frames) *n_frames = T;
  io.fetch(codes, d_codes, (size_t)n_q * T * 4);          // dense [n_q][T] rows: codes_capacity only has to cover T
  return io.finish();
}

}  // extern "C"
