// kokoro.hip -- Kokoro's waveform half, fp32, gfx950: the F0 / N predictor blocks (TTSEngine/KokoroModel.swift:66-89, after `shared`),
// KokoroDecoder (Decoder/KokoroDecoder.swift:83-112) and its iSTFTNet Generator (Decoder/Generator.swift:133-192) with the harmonic
// source (KokoroSineGen.swift, KokoroSourceModuleHnNSF.swift) and the STFT pair (MLXSTFT.swift).
//
// Layout: every activation is time-major fp32 [T][Cp], Cp = the channel count rounded up to 32.  The padding columns are zero and stay
// zero: weights carry zero rows / columns for them, and an AdaIN maps them to zero (kokoro.h).  A concatenation is one such buffer that
// its producers write column ranges of (encode / decode blocks -> [0, hidden), asr_res -> [hidden, hidden + asr_res), F0_conv / N_conv
// -> the two columns behind): no concat copy exists.  Every convolution runs on the fp32 tap GEMM of codec_kernels.hip, with exactly
// the launches other models use (leaky-ReLU prologue, residual / scale / second-residual epilogues, transposed convolutions as phases).
//
// AdaIN is MATERIALISED: statistics (two launches), then one element-wise pass that writes act(AdaIN(x)), which the convolution reads
// with no prologue -- so the zero padding of the convolution applies to the ACTIVATED tensor, as in the reference.  The variant that
// folds the affine step into the tap GEMM's prologue is not built ("Kokoro").
//
// Weight norm is folded at load (ConvWeighted.swift:36-63): w = g v / (||v|| + 1e-7), the norm over every axis but 0 of the tensor as
// stored, and the result is oriented by ConvWeighted's own rule (:118-122): used as stored when its last axis is the input's channel
// count (or the convolution is grouped), with all axes reversed otherwise -- which is how `ups` ([Cin][K][Cout] after sanitising)
// becomes the [Cout][K][Cin] a transposed convolution takes, and why `pool` ([C][3][1], grouped) is used as stored.
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mia_kokoro.h"
#include "codec.h"
#include "kokoro.h"
#include "mia_internal.h"
#include "tensor_loader.h"

namespace {

inline int pad32(int c) { return (c + 31) / 32 * 32; }

struct KConv {
  float* w = nullptr; float* b = nullptr;
  int N = 0, Cin = 0, taps = 1, dil = 1, pad = 0, stride = 1;   // N, Cin: padded to 32 unless the loader was told to keep N
  int K = 0;                                                    // transposed conv: kernel size (taps = ceil(K / stride))
};
struct KAda { int off = 0, C = 0; };                            // gamma at style[off .. off + C), beta behind it
struct KBlk {                                                   // AdainResBlk1d
  KConv c1, c2, sc;
  KAda n1, n2;
  bool learned = false, up = false;
  float* pool_w = nullptr; float* pool_b = nullptr;
};
struct KRes {                                                   // AdaINResBlock1
  KConv c1[3], c2[3];
  KAda a1[3], a2[3];
  float *al1[3] = {}, *ral1[3] = {}, *al2[3] = {}, *ral2[3] = {};
};
struct StyleSet { std::vector<float> hw, hb; float* W = nullptr; float* b = nullptr; int rows = 0; };

constexpr int KOKORO_NBUF = 10;

}  // namespace

struct mia_kokoro {
  mia_ctx* ctx = nullptr;
  mia_kokoro_config cfg{};
  std::vector<void*> allocs;
  int up = 0, H = 0, sd = 0;
  int Cp0 = 0, Cpc = 0, C0 = 0;          // padded widths of the two concatenations; generator input channels
  int maxC = 0;
  KBlk encode, decode[4];
  KConv asr_res;
  float* f0conv = nullptr; float* nconv = nullptr;        // folded [3] + bias [1]
  KConv ups[4], nzc[4], post;
  KRes nres[4], rb[4][4];
  int chp[4] = {};
  float* lw = nullptr; float lb = 0.f;
  StyleSet sdec, spred;
  bool has_pred = false;
  KBlk pF0[3], pN[3];
  KConv projF0, projN;
  float* arena = nullptr; size_t arena_floats = 0;
};

namespace {

struct KLoader : TensorLoader {
  int sd = 0;
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
  // Conv1dInference: plain weight [Cout][K][Cin] + bias
  bool conv_plain(const std::string& p, int Cout, int K, int Cin, int pad, int stride, bool keepN, KConv& o) {
    std::vector<float> w, b;
    if (!f32(p + ".weight", w, {Cout, K, Cin}) || !bias_of(p, true, Cout, Cout, b)) return false;
    place(w, b, Cout, K, Cin, keepN, 1, pad, stride, o);
    return true;
  }
  // ConvTransposed1d, y[t s + k - p] += x[t] w[.][k][.], as s phase GEMMs (hift.hip: convt)
  bool convt_wn(const std::string& p, int Cout, int K, int Cin, int s, int pad, KConv& o) {
    std::vector<float> w, b;
    if (!oriented(p, w, Cout, K, Cin) || !bias_of(p, true, Cout, pad32(Cout), b)) return false;
    const int nt = (K + s - 1) / s, Cp = pad32(Cin), Np = pad32(Cout);
    std::vector<float> ph((size_t)s * Np * nt * Cp, 0.f);
    for (int r = 0; r < s; ++r) for (int co = 0; co < Cout; ++co) for (int q = 0; q < nt; ++q) {
      const int k = r + (nt - 1 - q) * s;
      if (k >= K) continue;
      for (int ci = 0; ci < Cin; ++ci) ph[(((size_t)r * Np + co) * nt + q) * Cp + ci] = w[((size_t)co * K + k) * Cin + ci];
    }
    o.w = up(ph); o.b = up(b); o.N = Np; o.Cin = Cp; o.taps = nt; o.stride = s; o.pad = pad; o.K = K;
    return true;
  }
  bool adain(const std::string& p, int C, StyleSet& S, KAda& a) {
    std::vector<float> w, b;
    if (!f32(p + ".fc.weight", w, {2 * C, sd}) || !f32(p + ".fc.bias", b, {2 * C})) return false;
    a.off = S.rows; a.C = C; S.rows += 2 * C;
    S.hw.insert(S.hw.end(), w.begin(), w.end()); S.hb.insert(S.hb.end(), b.begin(), b.end());
    return true;
  }
  bool block(const std::string& p, int Cin, int Cout, bool upsample, StyleSet& S, KBlk& k) {
    k.up = upsample; k.learned = Cin != Cout;
    if (upsample && !k.learned) return fail(MIA_ERR_INVALID_ARGUMENT, "kokoro_load: an up-sampling block needs a learned shortcut");
    if (!conv_wn(p + ".conv1", Cout, 3, Cin, 1, 1, true, false, k.c1) || !conv_wn(p + ".conv2", Cout, 3, Cout, 1, 1, true, false, k.c2)) return false;
    if (!adain(p + ".norm1", Cin, S, k.n1) || !adain(p + ".norm2", Cout, S, k.n2)) return false;
    if (k.learned && !conv_wn(p + ".conv1x1", Cout, 1, Cin, 1, 0, false, false, k.sc)) return false;
    if (upsample) {                       // grouped: used as stored, [C][3][1]
      std::vector<float> w, b;
      if (!folded(p + ".pool", w, Cin, 3, 1) || !bias_of(p + ".pool", true, Cin, pad32(Cin), b)) return false;
      w.resize((size_t)pad32(Cin) * 3, 0.f);
      k.pool_w = up(w); k.pool_b = up(b);
    }
    return true;
  }
  // alpha [1][C][1] -> (alpha, 1 / alpha) padded with ones
  bool snake(const std::string& n, int C, float*& al, float*& ral) {
    std::vector<float> a;
    if (!f32(n, a, {1, C, 1})) return false;
    std::vector<float> ap(pad32(C), 1.f), rp(pad32(C), 1.f);
    for (int i = 0; i < C; ++i) { ap[i] = a[i]; rp[i] = 1.0f / a[i]; }
    al = up(ap); ral = up(rp);
    return true;
  }
  bool resblock(const std::string& p, int C, int k, const int* dil, StyleSet& S, KRes& r) {
    for (int i = 0; i < 3; ++i) {
      const std::string si = std::to_string(i);
      const int d = dil[i];
      if (!conv_wn(p + ".convs1." + si, C, k, C, d, (k * d - d) / 2, true, false, r.c1[i])) return false;
      if (!conv_wn(p + ".convs2." + si, C, k, C, 1, (k - 1) / 2, true, false, r.c2[i])) return false;
      if (!adain(p + ".adain1." + si, C, S, r.a1[i]) || !adain(p + ".adain2." + si, C, S, r.a2[i])) return false;
      if (!snake(p + ".alpha1." + si, C, r.al1[i], r.ral1[i]) || !snake(p + ".alpha2." + si, C, r.al2[i], r.ral2[i])) return false;
    }
    return true;
  }
  // 1 -> 1 weight-normed convolution, k 3: folded taps and the bias
  bool curve(const std::string& p, float*& o) {
    std::vector<float> w, b;
    if (!folded(p, w, 1, 3, 1) || !f32(p + ".bias", b, {1})) return false;
    w.push_back(b[0]);
    o = up(w);
    return true;
  }
  void finish(StyleSet& S) { if (S.rows) { S.W = up(S.hw); S.b = up(S.hb); } S.hw.clear(); S.hb.clear(); }
};

// ---- per-call scratch ------------------------------------------------------------------------------------------------------------------
struct Scratch {
  float *style, *mean, *a, *beta, *part, *sv, *f0, *n, *raw, *noise, *src, *P, *har, *har22, *post, *fr, *pcm, *big[KOKORO_NBUF];
  size_t big_floats;
};

int64_t gen_rows(const mia_kokoro* h, int64_t L, int stage) {
  int64_t r = L;
  for (int i = 0; i <= stage; ++i) { r *= h->cfg.up_rates[i]; if (i == h->cfg.n_ups - 1) r += 1; }
  return r;
}

// T: rows of the decoder / predictor blocks (0: none), L: rows the generator sees (0: none)
int carve(mia_kokoro* h, int64_t T, int64_t L, Scratch& sc) {
  const mia_kokoro_config& g = h->cfg;
  auto al = [](size_t n) { return (n + 63) / 64 * 64; };
  size_t big = (size_t)2 * T * h->maxC;
  big = std::max(big, (size_t)L * h->C0);
  for (int i = 0; i < g.n_ups && L; ++i) big = std::max(big, (size_t)gen_rows(h, L, i) * h->chp[i]);
  big = al(big + 64);
  const int64_t n = L * h->up, F = n / KOKORO_HOP + 1;
  const size_t raw = std::max({(size_t)T * g.dim_in, (size_t)T * g.pred_dim, (size_t)L * g.up_initial});
  size_t sizes[] = {al((size_t)std::max(h->sdec.rows, h->spred.rows)), al(h->maxC), al(h->maxC), al(h->maxC), al(3 * ((size_t)131072 + h->maxC)),
                    al(h->sd), al(2 * T + L), al(2 * T), al(raw), al((size_t)n * h->H), al(n), al((size_t)L * h->H), al((size_t)F * 32),
                    al((size_t)F * 22), al((size_t)F * 22), al((size_t)F * KOKORO_NFFT), al(n)};
  size_t tot = (size_t)KOKORO_NBUF * big;
  for (size_t s : sizes) tot += s;
  if (int rc = mia_grow(h->ctx, h->arena, h->arena_floats, tot, "kokoro: scratch hipMalloc failed")) return rc;
  float* q = h->arena;
  float** dst[] = {&sc.style, &sc.mean, &sc.a, &sc.beta, &sc.part, &sc.sv, &sc.f0, &sc.n, &sc.raw, &sc.noise, &sc.src, &sc.P, &sc.har,
                   &sc.har22, &sc.post, &sc.fr, &sc.pcm};
  for (int i = 0; i < 17; ++i) { *dst[i] = q; q += sizes[i]; }
  for (int i = 0; i < KOKORO_NBUF; ++i) { sc.big[i] = q; q += big; }
  sc.big_floats = big;
  return MIA_OK;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------------
struct COpt { const float* R = nullptr; int64_t ldr = 0; const float* R2 = nullptr; float scale = 0.f; float lrelu = 0.f; int64_t ldy = 0; };

int run_conv(mia_kokoro* h, const KConv& c, const float* X, int64_t T_in, float* Y, int64_t T_out, const COpt& o = COpt()) {
  ConvGemmArgs g;
  g.X = X; g.ldx = c.Cin; g.T_in = (int)T_in; g.W = c.w; g.bias = c.b; g.lrelu_slope = o.lrelu;
  g.Y = Y; g.ldy = o.ldy ? o.ldy : c.N; g.T_out = (int)T_out; g.R = o.R; g.R2 = o.R2; g.ldr = o.ldr ? o.ldr : c.N; g.out_scale = o.scale;
  g.M = (int)T_out; g.N = c.N; g.Cin = c.Cin; g.taps = c.taps; g.dil = c.dil; g.pad = c.pad; g.x_row_mul = c.stride;
  return codec_conv_gemm_run(h->ctx, g, 1, "kokoro");
}

// k = 1 convolution on T rows, every row written twice (rows 2 t and 2 t + 1): the nearest x 2 up-sampling of the shortcut commutes with it
int run_conv_dup(mia_kokoro* h, const KConv& c, const float* X, int64_t T, float* Y) {
  ConvGemmArgs g;
  g.X = X; g.ldx = c.Cin; g.T_in = (int)T; g.W = c.w; g.bias = c.b;
  g.Y = Y; g.ldy = c.N; g.T_out = (int)(2 * T); g.y_row_mul = 2; g.y_phase_step = 1;
  g.M = (int)T; g.N = c.N; g.Cin = c.Cin; g.taps = 1; g.dil = 1; g.pad = 0;
  return codec_conv_gemm_run(h->ctx, g, 2, "kokoro");
}

// transposed conv: Y rows [row_shift, row_shift + T_out)
int run_convt(mia_kokoro* h, const KConv& c, const float* X, int64_t T_in, float* Y, int64_t T_out, int row_shift, float lrelu) {
  ConvGemmArgs g;
  g.X = X; g.ldx = c.Cin; g.T_in = (int)T_in; g.W = c.w; g.w_phase_stride = (int64_t)c.N * c.taps * c.Cin; g.bias = c.b; g.lrelu_slope = lrelu;
  g.M = (int)T_in + c.taps - 1; g.N = c.N; g.Cin = c.Cin; g.taps = c.taps; g.dil = 1; g.pad = c.taps - 1;
  g.Y = Y + (int64_t)row_shift * c.N; g.ldy = c.N; g.T_out = (int)T_out; g.y_row_mul = c.stride; g.y_row_off = -c.pad; g.y_phase_step = 1;
  return codec_conv_gemm_run(h->ctx, g, c.stride, "kokoro");
}

#define KOK_LAUNCH(h, expr) do { if (expr) return mia_fail((h)->ctx, MIA_ERR_DEVICE, "kokoro: kernel launch failed (%s)", #expr); } while (0)

// y = act(AdaIN(x)) over rows x C (C: padded width, the last a.C.. columns give zero)
int run_adain(mia_kokoro* h, const Scratch& sc, const KAda& a, const float* x, int64_t ldx, int64_t rows, int C, float* y, const float* alpha,
              const float* ralpha) {
  hipStream_t s = h->ctx->stream;
  KOK_LAUNCH(h, kokoro_inorm_launch(x, ldx, rows, C, sc.part, sc.style + a.off, sc.style + a.off + a.C, a.C, sc.mean, sc.a, sc.beta, s));
  KOK_LAUNCH(h, kokoro_adain_act_launch(x, ldx, y, C, rows, C, sc.mean, sc.a, sc.beta, alpha, ralpha, 0.2f, s));
  return MIA_OK;
}

int run_style(mia_kokoro* h, const Scratch& sc, const StyleSet& S, const float* sv) {
  KOK_LAUNCH(h, kokoro_style_launch(S.W, S.b, sv, sc.style, S.rows, h->sd, h->ctx->stream));
  return MIA_OK;
}

// AdainResBlk1d (AdainResBlk1d.swift:78-125): X [T][ldx = c1.Cin] -> Y [T or 2 T] with row stride ldy (0: c2.N); t: four scratch buffers
int run_block(mia_kokoro* h, const Scratch& sc, const KBlk& b, const float* X, int64_t T, float* Y, int64_t ldy, float* const* t) {
  const int Cp = b.c1.Cin, Np = b.c1.N;
  if (int rc = run_adain(h, sc, b.n1, X, Cp, T, Cp, t[0], nullptr, nullptr)) return rc;
  const float* in1 = t[0];
  int64_t T2 = T;
  if (b.up) {
    KOK_LAUNCH(h, kokoro_pool_launch(t[0], t[1], b.pool_w, b.pool_b, T, Cp, h->ctx->stream));
    in1 = t[1]; T2 = 2 * T;
  }
  if (int rc = run_conv(h, b.c1, in1, T2, t[2], T2)) return rc;
  if (int rc = run_adain(h, sc, b.n2, t[2], Np, T2, Np, t[0], nullptr, nullptr)) return rc;
  COpt o; o.scale = 0.70710678118654752f; o.ldy = ldy;
  if (b.learned) {
    if (int rc = b.up ? run_conv_dup(h, b.sc, X, T, t[3]) : run_conv(h, b.sc, X, T, t[3], T)) return rc;
    o.R = t[3]; o.ldr = Np;
  } else { o.R = X; o.ldr = Cp; }
  return run_conv(h, b.c2, t[0], T2, Y, T2, o);
}

// AdaINResBlock1 (AdaINResBlock1.swift:77-105).  x: input (left untouched); res, t1, t2: scratch; the last pair writes
// out = scale (conv2(..) + res) + R2, so sums and means fold into the final epilogue (hift.hip: run_resblock)
int run_resblock(mia_kokoro* h, const Scratch& sc, const KRes& r, const float* x, float* res, float* t1, float* t2, float* out, int64_t T, float scale,
                 const float* R2) {
  const int C = r.c1[0].Cin;
  for (int i = 0; i < 3; ++i) {
    const float* in = i == 0 ? x : res;
    if (int rc = run_adain(h, sc, r.a1[i], in, C, T, C, t1, r.al1[i], r.ral1[i])) return rc;
    if (int rc = run_conv(h, r.c1[i], t1, T, t2, T)) return rc;
    if (int rc = run_adain(h, sc, r.a2[i], t2, C, T, C, t1, r.al2[i], r.ral2[i])) return rc;
    COpt o; o.R = in;
    float* dst = res;
    if (i == 2) { dst = out; o.scale = scale; o.R2 = R2; }
    if (int rc = run_conv(h, r.c2[i], t1, T, dst, T, o)) return rc;
  }
  return MIA_OK;
}

// f0 [L] -> src [L up] -> har [F][32]
int dev_source(mia_kokoro* h, const Scratch& sc, const float* f0, int64_t L, const float* noise) {
  hipStream_t s = h->ctx->stream;
  KOK_LAUNCH(h, kokoro_source_launch(f0, sc.P, noise, h->lw, h->lb, sc.src, L, h->up, h->H, (float)h->cfg.sample_rate, (float)h->cfg.voiced_threshold, s));
  KOK_LAUNCH(h, kokoro_stft_launch(sc.src, sc.har, L * h->up, s));
  return MIA_OK;
}

// Generator.callAsFunction from har: x = big[6] [L][C0] -> pcm.  Uses big[0], big[1], big[2], big[3], big[6], big[7].
int dev_generate(mia_kokoro* h, const Scratch& sc, int64_t L) {
  hipStream_t s = h->ctx->stream;
  const mia_kokoro_config& g = h->cfg;
  const int64_t F = L * h->up / KOKORO_HOP + 1;
  float* A = sc.big[6]; float* D = sc.big[7]; float* Cb = sc.big[0]; float* res = sc.big[1]; float* t1 = sc.big[2]; float* t2 = sc.big[3];
  int64_t rows = L;
  for (int i = 0; i < g.n_ups; ++i) {
    const bool last = i == g.n_ups - 1;
    const int64_t r_out = gen_rows(h, L, i); const int Ci = h->chp[i];
    // leaky-ReLU 0.1 -> ConvTransposed1d (-> the reflected sample in front: new[0] = old[1] = new[2])
    if (int rc = run_convt(h, h->ups[i], A, rows, D, last ? r_out - 1 : r_out, last ? 1 : 0, 0.1f)) return rc;
    if (last) MIA_HIP(h->ctx, hipMemcpyAsync(D, D + 2 * (int64_t)Ci, (size_t)Ci * 4, hipMemcpyDeviceToDevice, s));
    const KConv& nc = h->nzc[i];
    const int64_t nc_rows = (F + 2 * nc.pad - nc.taps) / nc.stride + 1;
    if (nc_rows != r_out) return mia_fail(h->ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro: noise_convs.%d yields %lld rows, the stream has %lld", i, (long long)nc_rows, (long long)r_out);
    if (int rc = run_conv(h, nc, sc.har, F, Cb, r_out)) return rc;
    if (int rc = run_resblock(h, sc, h->nres[i], Cb, res, t1, t2, D, r_out, 1.0f, D)) return rc;     // x = ups(..) + noise_res(noise_conv(har))
    const float inv = 1.0f / (float)g.n_res_kernels;
    for (int k = 0; k < g.n_res_kernels; ++k)
      if (int rc = run_resblock(h, sc, h->rb[i][k], D, res, t1, t2, A, r_out, inv, k == 0 ? nullptr : A)) return rc;
    rows = r_out;
  }
  COpt o; o.lrelu = 0.01f;
  if (int rc = run_conv(h, h->post, A, rows, sc.post, rows, o)) return rc;
  KOK_LAUNCH(h, kokoro_istft_launch(sc.post, 2 * KOKORO_BINS, sc.fr, sc.pcm, rows, s));
  return MIA_OK;
}

int check_rows(mia_kokoro* h, int64_t T, const char* who) {
  if (!h) return MIA_ERR_INVALID_ARGUMENT;
  if (T < 1 || T > 10000) return mia_fail(h->ctx, MIA_ERR_INVALID_ARGUMENT, "%s: the row count must be in [1, 10000] (got %lld)", who, (long long)T);
  return MIA_OK;
}

}  // namespace

extern "C" {

mia_kokoro* mia_kokoro_load(mia_ctx* ctx, const mia_kokoro_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_load: null argument"); return nullptr; }
  const mia_kokoro_config& g = *cfg;
  bool cfg_ok = g.n_ups >= 1 && g.n_ups <= 4 && g.n_res_kernels >= 1 && g.n_res_kernels <= 4 && g.n_dilations == 3 && g.n_fft == KOKORO_NFFT &&
                g.hop == KOKORO_HOP && g.n_harmonics >= 0 && g.n_harmonics < KOKORO_MAX_HARM && g.dim_in >= 32 && g.dim_in % 32 == 0 &&
                g.hidden >= 32 && g.hidden % 32 == 0 && g.asr_res_dim >= 32 && g.asr_res_dim % 32 == 0 && g.style_dim >= 1 && g.pred_dim >= 0 &&
                g.pred_dim % 64 == 0 && g.up_initial >= (1 << g.n_ups) && g.up_initial % (1 << g.n_ups) == 0 && g.sample_rate > 0;
  for (int i = 0; cfg_ok && i < g.n_ups; ++i) {
    const int k = g.up_kernels[i], u = g.up_rates[i];
    cfg_ok = u >= 1 && k >= u && (k - u) % 2 == 0;
  }
  if (!cfg_ok) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_load: unsupported configuration"); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { mia_fail(ctx, MIA_ERR_DEVICE, "kokoro_load: hipSetDevice failed"); return nullptr; }
  mia_kokoro* h = new mia_kokoro();
  h->ctx = ctx; h->cfg = g; h->H = g.n_harmonics + 1; h->sd = g.style_dim; h->C0 = pad32(g.up_initial);
  h->up = g.hop; for (int i = 0; i < g.n_ups; ++i) h->up *= g.up_rates[i];
  const int cat = g.hidden + g.asr_res_dim + 2;
  h->Cp0 = pad32(g.dim_in + 2); h->Cpc = pad32(cat);
  h->maxC = std::max({h->Cp0, h->Cpc, g.hidden, h->C0, g.pred_dim});
  KLoader L; L.sd = g.style_dim; L.allocs = &h->allocs; L.index(tensors, n_tensors);
  const std::string D = "decoder.", G = "decoder.generator.";
  bool ok = L.block(D + "encode", g.dim_in + 2, g.hidden, false, h->sdec, h->encode);
  for (int i = 0; i < 4 && ok; ++i) ok = L.block(D + "decode." + std::to_string(i), cat, i == 3 ? g.up_initial : g.hidden, i == 3, h->sdec, h->decode[i]);
  ok = ok && L.curve(D + "F0_conv", h->f0conv) && L.curve(D + "N_conv", h->nconv);
  if (ok) {   // asr_res reads the first concatenation ([dim_in | F0 | N], Cp0 wide): its weights are zero on the two curve columns
    std::vector<float> w, b;
    ok = L.oriented(D + "asr_res.0", w, g.asr_res_dim, 1, g.dim_in) && L.bias_of(D + "asr_res.0", true, g.asr_res_dim, g.asr_res_dim, b);
    if (ok) {
      std::vector<float> wp((size_t)g.asr_res_dim * h->Cp0, 0.f);
      for (int co = 0; co < g.asr_res_dim; ++co) for (int ci = 0; ci < g.dim_in; ++ci) wp[(size_t)co * h->Cp0 + ci] = w[(size_t)co * g.dim_in + ci];
      h->asr_res.w = L.up(wp); h->asr_res.b = L.up(b); h->asr_res.N = g.asr_res_dim; h->asr_res.Cin = h->Cp0;
    }
  }
  if (ok) {
    std::vector<float> w, b;
    ok = L.f32(G + "m_source.l_linear.weight", w, {1, h->H}) && L.f32(G + "m_source.l_linear.bias", b, {1});
    if (ok) { h->lw = L.up(w); h->lb = b[0]; }
  }
  static const int nres_dil[3] = {1, 3, 5};
  for (int i = 0; i < g.n_ups && ok; ++i) {
    const std::string si = std::to_string(i);
    const int Cin = g.up_initial >> i, Cout = g.up_initial >> (i + 1);
    h->chp[i] = pad32(Cout);
    ok = L.convt_wn(G + "ups." + si, Cout, g.up_kernels[i], Cin, g.up_rates[i], (g.up_kernels[i] - g.up_rates[i]) / 2, h->ups[i]);
    int dr = 1; for (int j = i + 1; j < g.n_ups; ++j) dr *= g.up_rates[j];
    const bool last = i + 1 == g.n_ups;
    if (ok) ok = last ? L.conv_plain(G + "noise_convs." + si, Cout, 1, g.n_fft + 2, 0, 1, false, h->nzc[i])
                      : L.conv_plain(G + "noise_convs." + si, Cout, 2 * dr, g.n_fft + 2, (dr + 1) / 2, dr, false, h->nzc[i]);
    if (ok) ok = L.resblock(G + "noise_res." + si, Cout, last ? 11 : 7, nres_dil, h->sdec, h->nres[i]);
    for (int k = 0; k < g.n_res_kernels && ok; ++k)
      ok = L.resblock(G + "resblocks." + std::to_string(i * g.n_res_kernels + k), Cout, g.res_kernels[k], g.dilations, h->sdec, h->rb[i][k]);
  }
  ok = ok && L.conv_wn(G + "conv_post", g.n_fft + 2, 7, g.up_initial >> g.n_ups, 1, 3, true, true, h->post);
  if (ok && g.pred_dim > 0 && L.has("predictor.F0.0.conv1.weight_v")) {
    const int P = g.pred_dim;
    for (int i = 0; i < 3 && ok; ++i) {
      const int Cin = i < 2 ? P : P / 2, Cout = i == 0 ? P : P / 2;
      ok = L.block("predictor.F0." + std::to_string(i), Cin, Cout, i == 1, h->spred, h->pF0[i]) &&
           L.block("predictor.N." + std::to_string(i), Cin, Cout, i == 1, h->spred, h->pN[i]);
    }
    ok = ok && L.conv_plain("predictor.F0_proj", 1, 1, P / 2, 0, 1, true, h->projF0) && L.conv_plain("predictor.N_proj", 1, 1, P / 2, 0, 1, true, h->projN);
    h->has_pred = ok;
  }
  if (ok) { L.finish(h->sdec); L.finish(h->spred); }
  if (!ok || !L.err.empty()) {
    mia_fail(ctx, L.err.empty() ? MIA_ERR_INVALID_ARGUMENT : L.code, "kokoro_load: %s", L.err.empty() ? "failed" : L.err.c_str());
    mia_kokoro_free(h);
    return nullptr;
  }
  return h;
}

void mia_kokoro_free(mia_kokoro* h) {
  if (!h) return;
  (void)hipStreamSynchronize(h->ctx->stream);
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->arena) (void)hipFree(h->arena);
  delete h;
}

int64_t mia_kokoro_output_len(const mia_kokoro* h, int64_t T) { return h && T > 0 ? 2 * T * h->up : 0; }

int mia_kokoro_f0n(mia_kokoro* h, const float* x, int T, const float* s_pred, float* f0, float* n, int mem) {
  if (int rc = check_rows(h, T, "kokoro_f0n")) return rc;
  MIA_CHECK_ARG(h->ctx, h->has_pred, "kokoro_f0n: the handle was loaded without the predictor tensors");
  MIA_CHECK_ARG(h->ctx, x && s_pred && f0 && n && HostIo::valid(mem), "kokoro_f0n: bad argument");
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  Scratch sc;
  if (int rc = carve(h, T, 0, sc)) return rc;
  hipStream_t s = h->ctx->stream;
  const int P = h->cfg.pred_dim;
  HostIo io(h->ctx, mem);
  const float* xr = io.in(x, sc.raw, (size_t)P * T * 4);
  const float* sv = io.in(s_pred, sc.sv, (size_t)h->sd * 4);
  float* d_f0 = io.out(f0, sc.f0, (size_t)2 * T * 4);
  float* d_n = io.out(n, sc.n, (size_t)2 * T * 4);
  KOK_LAUNCH(h, kokoro_pack_launch(xr, sc.big[0], P, 0, P, T, s));
  if (int rc = run_style(h, sc, h->spred, sv)) return rc;
  float* const* t = &sc.big[2];
  for (int br = 0; br < 2; ++br) {
    const KBlk* b = br == 0 ? h->pF0 : h->pN;
    if (int rc = run_block(h, sc, b[0], sc.big[0], T, sc.big[1], 0, t)) return rc;
    if (int rc = run_block(h, sc, b[1], sc.big[1], T, sc.big[6], 0, t)) return rc;
    if (int rc = run_block(h, sc, b[2], sc.big[6], 2 * T, sc.big[7], 0, t)) return rc;
    COpt o; o.ldy = 1;
    if (int rc = run_conv(h, br == 0 ? h->projF0 : h->projN, sc.big[7], 2 * T, br == 0 ? d_f0 : d_n, 2 * T, o)) return rc;
  }
  return io.finish();
}

int mia_kokoro_source(mia_kokoro* h, const float* f0, int L, const float* noise, float* source, float* har, int mem) {
  if (int rc = check_rows(h, (L + 1) / 2, "kokoro_source")) return rc;
  MIA_CHECK_ARG(h->ctx, L >= 1 && f0 && HostIo::valid(mem), "kokoro_source: bad argument");
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  Scratch sc;
  if (int rc = carve(h, 0, L, sc)) return rc;
  const int64_t n = (int64_t)L * h->up, F = n / KOKORO_HOP + 1;
  HostIo io(h->ctx, mem);
  const float* d_f0 = io.in(f0, sc.f0, (size_t)L * 4);
  const float* d_noise = io.in(noise, sc.noise, (size_t)n * h->H * 4);
  if (source) sc.src = io.out(source, sc.src, (size_t)n * 4);
  if (int rc = dev_source(h, sc, d_f0, L, d_noise)) return rc;
  if (har) io.check(hipMemcpy2DAsync(har, 22 * 4, sc.har, 32 * 4, 22 * 4, (size_t)F, io.to_caller(), h->ctx->stream));
  return io.finish();
}

int mia_kokoro_generate(mia_kokoro* h, const float* x, int L, const float* s, const float* har, float* pcm, int mem) {
  if (int rc = check_rows(h, (L + 1) / 2, "kokoro_generate")) return rc;
  MIA_CHECK_ARG(h->ctx, L >= 1 && x && s && har && pcm && HostIo::valid(mem), "kokoro_generate: bad argument");
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  Scratch sc;
  if (int rc = carve(h, 0, L, sc)) return rc;
  hipStream_t st = h->ctx->stream;
  const int64_t n = (int64_t)L * h->up, F = n / KOKORO_HOP + 1;
  HostIo io(h->ctx, mem);
  const float* xr = io.in(x, sc.raw, (size_t)h->cfg.up_initial * L * 4);
  const float* sv = io.in(s, sc.sv, (size_t)h->sd * 4);
  sc.pcm = io.out(pcm, sc.pcm, (size_t)n * 4);
  MIA_HIP(h->ctx, hipMemsetAsync(sc.har, 0, (size_t)F * 32 * 4, st));
  io.check(hipMemcpy2DAsync(sc.har, 32 * 4, har, 22 * 4, 22 * 4, (size_t)F, io.from_caller(), st));
  if (h->C0 != h->cfg.up_initial) MIA_HIP(h->ctx, hipMemsetAsync(sc.big[6], 0, (size_t)L * h->C0 * 4, st));
  KOK_LAUNCH(h, kokoro_pack_launch(xr, sc.big[6], h->C0, 0, h->cfg.up_initial, L, st));
  if (int rc = run_style(h, sc, h->sdec, sv)) return rc;
  if (int rc = dev_generate(h, sc, L)) return rc;
  return io.finish();
}

int mia_kokoro_decode(mia_kokoro* h, const float* asr, int T, const float* f0, const float* n, const float* s, const float* noise, float* pcm,
                      int mem) {
  if (int rc = check_rows(h, T, "kokoro_decode")) return rc;
  MIA_CHECK_ARG(h->ctx, asr && f0 && n && s && pcm && HostIo::valid(mem), "kokoro_decode: bad argument");
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  const mia_kokoro_config& g = h->cfg;
  const int64_t L = 2 * (int64_t)T, ns = L * h->up;
  Scratch sc;
  if (int rc = carve(h, T, L, sc)) return rc;
  hipStream_t st = h->ctx->stream;
  HostIo io(h->ctx, mem);
  const float* ar = io.in(asr, sc.raw, (size_t)g.dim_in * T * 4);
  const float* d_f0 = io.in(f0, sc.f0, (size_t)L * 4);
  const float* d_n = io.in(n, sc.n, (size_t)L * 4);
  const float* sv = io.in(s, sc.sv, (size_t)h->sd * 4);
  const float* d_noise = io.in(noise, sc.noise, (size_t)ns * h->H * 4);
  sc.pcm = io.out(pcm, sc.pcm, (size_t)ns * 4);
  float* X0 = sc.big[0]; float* cat = sc.big[1];
  MIA_HIP(h->ctx, hipMemsetAsync(X0, 0, (size_t)T * h->Cp0 * 4, st));
  MIA_HIP(h->ctx, hipMemsetAsync(cat, 0, (size_t)T * h->Cpc * 4, st));
  KOK_LAUNCH(h, kokoro_pack_launch(ar, X0, h->Cp0, 0, g.dim_in, T, st));
  KOK_LAUNCH(h, kokoro_curve_cols_launch(d_f0, d_n, h->f0conv, h->nconv, X0, h->Cp0, g.dim_in, cat, h->Cpc, g.hidden + g.asr_res_dim, T, st));
  if (int rc = run_style(h, sc, h->sdec, sv)) return rc;
  if (int rc = dev_source(h, sc, d_f0, L, d_noise)) return rc;
  float* const* t = &sc.big[2];
  if (int rc = run_block(h, sc, h->encode, X0, T, cat, h->Cpc, t)) return rc;
  COpt o; o.ldy = h->Cpc;
  if (int rc = run_conv(h, h->asr_res, X0, T, cat + g.hidden, T, o)) return rc;
  for (int i = 0; i < 3; ++i)
    if (int rc = run_block(h, sc, h->decode[i], cat, T, cat, h->Cpc, t)) return rc;
  if (int rc = run_block(h, sc, h->decode[3], cat, T, sc.big[6], 0, t)) return rc;
  if (int rc = dev_generate(h, sc, L)) return rc;
  return io.finish();
}

int mia_op_instance_norm(mia_ctx* ctx, const float* x, int64_t ld, int64_t T, int C, float* mean, float* rstd) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, x && mean && rstd && T >= 1 && C >= 1 && ld >= C && T <= (1ll << 24), "op_instance_norm: bad argument");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  float* part = (float*)mia_workspace(ctx, kokoro_inorm_scratch(T, C) * 4);
  if (!part) return MIA_ERR_OUT_OF_MEMORY;
  if (kokoro_inorm_launch(x, ld, T, C, part, nullptr, nullptr, 0, mean, rstd, nullptr, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_instance_norm: launch failed");
  return MIA_OK;
}

}  // extern "C"
