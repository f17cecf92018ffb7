// kokoro_text.hip -- Kokoro's text half behind ALBERT, fp32, gfx950, B = 1 (masks are no-ops there and are not implemented):
// DurationEncoder (TTSEngine/DurationEncoder.swift) -> predictor.lstm -> the duration head (KokoroTTS.swift:303-315), TextEncoder
// (TTSEngine/TextEncoder.swift), the alignment (KokoroTTS.swift:318-407: both matmuls with pred_aln_trg are row gathers) and
// predictor.shared (KokoroModel.swift:68).  The six BiLSTMs run on kokoro_lstm.hip, the convolutions on the fp32 tap GEMM; this file
// holds the small kernels around them, the loader and the C ABI (mia_kokoro_text_*).
//
// A concatenation with the style vector is one [N][d_model + style] buffer: its style columns are written once per call, and each
// AdaLayerNorm writes columns [0, d_model) of it.  No concat copy exists.
#include <string>
#include <vector>

#include "../../include/mia_kokoro.h"
#include "kokoro.h"
#include "kokoro_load.h"
#include "kokoro_text.h"

namespace {

constexpr float LN_EPS = 1e-5f;
constexpr int KTEXT_MAX_DEPTH = 8;

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A[n] = d_en[n] | s
__global__ __launch_bounds__(256) void ktext_cat_style(const float* __restrict__ d_en, const float* __restrict__ s, float* __restrict__ A, int N, int D, int S) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * (D + S)) return;
  const int n = i / (D + S), c = i - n * (D + S);
  A[i] = c < D ? d_en[n * D + c] : s[c - D];
}

// One wave per row: mean and biased variance over the C channels with x - mean explicit, then
// act((one + gamma) (x - mean) / sqrt(var + eps) + beta), act = leaky-ReLU(slope) (slope 1: none).
// AdaLayerNorm: one = 1, gamma | beta from fc(style); LayerNormInference + LeakyReLU 0.2: one = 0, the layer's own gamma / beta.
__global__ __launch_bounds__(256) void ktext_layernorm(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int N, int C,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float one, float slope) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= N) return;
  const float* xr = x + (int64_t)r * ldx;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) { const float d = xr[c] - mean; q += d * d; }
  const float den = sqrtf(wave_sum(q) / (float)C + LN_EPS);
  for (int c = lane; c < C; c += 64) {
    const float v = (one + gamma[c]) * ((xr[c] - mean) / den) + beta[c];
    y[(int64_t)r * ldy + c] = v > 0.f ? v : slope * v;
  }
}

// One wave per token: duration_proj, sigmoid, the sum over the bins, / speed, rint (half to even, as MLX round), clamp to >= 1.
// The head is a few thousand operations per token and its result is rounded to an integer, so it is carried in double from the fp32
// inputs on (dot products, exp, the sum over the bins): the value before rounding is then the correctly rounded function of the
// LSTM's output, and the only error left in it is the one that output carries.
__global__ __launch_bounds__(256) void ktext_duration(const float* __restrict__ x, int64_t ld, const float* __restrict__ W, const float* __restrict__ b,
                                                      int bins, int D, float speed, int32_t* __restrict__ dur, float* __restrict__ raw, int N) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  const float* xr = x + (int64_t)n * ld;
  double tot = 0.0;
  for (int k = 0; k < bins; ++k) {
    double a = 0.0;
    for (int c = lane; c < D; c += 64) a = fma((double)W[(int64_t)k * D + c], (double)xr[c], a);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    tot += 1.0 / (1.0 + exp(-(a + (double)b[k])));
  }
  const float v = (float)(tot / (double)speed);
  if (lane == 0) { raw[n] = v; dur[n] = max(1, (int)rintf(fminf(v, 1.0e6f))); }
}

// Workgroup n copies source row n to rows [before, before + dur[n]) of en (time-major, ldd wide) and of asr (channel-major
// [D][total]); before = the exclusive scan of the durations, total = their sum, both exact integer sums formed per workgroup.
// Nothing is written when the total is outside [1, cap].
__global__ __launch_bounds__(256) void ktext_align(const float* __restrict__ d, int ldd, const float* __restrict__ ten, int D,
                                                   const int32_t* __restrict__ dur, int N, float* __restrict__ en, float* __restrict__ asr, int cap,
                                                   int32_t* __restrict__ total_out) {
  __shared__ int sh[2][4];
  const int n = blockIdx.x, tid = threadIdx.x;
  int before = 0, tot = 0;
  for (int i = tid; i < N; i += 256) {
    const int v = min(max(dur[i], 0), 1 << 20);
    tot += v;
    if (i < n) before += v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { tot += __shfl_xor(tot, o); before += __shfl_xor(before, o); }
  if ((tid & 63) == 0) { sh[0][tid >> 6] = tot; sh[1][tid >> 6] = before; }
  __syncthreads();
  tot = sh[0][0] + sh[0][1] + sh[0][2] + sh[0][3];
  before = sh[1][0] + sh[1][1] + sh[1][2] + sh[1][3];
  if (n == 0 && tid == 0) *total_out = tot;
  if (tot < 1 || tot > cap) return;
  const int my = min(max(dur[n], 0), 1 << 20);
  for (int i = tid; i < my * ldd; i += 256) {
    const int r = i / ldd, c = i - r * ldd;
    en[(int64_t)(before + r) * ldd + c] = d[(int64_t)n * ldd + c];
  }
  for (int i = tid; i < my * D; i += 256) {
    const int c = i / my, r = i - c * my;
    asr[(int64_t)c * tot + before + r] = ten[(int64_t)n * D + c];
  }
}

__global__ __launch_bounds__(256) void ktext_embed(const int32_t* __restrict__ ids, const float* __restrict__ emb, int n_sym, float* __restrict__ X, int N, int D) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * D) return;
  const int n = i / D, c = i - n * D, id = ids[n];
  X[i] = (id >= 0 && id < n_sym) ? emb[(int64_t)id * D + c] : 0.f;
}

unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

struct mia_kokoro_text {
  mia_ctx* ctx = nullptr;
  mia_kokoro_text_config cfg{};
  std::vector<void*> allocs;
  int D = 0, S = 0, H = 0, bins = 0;
  KokoroLstm enc[3], plstm, shared, tlstm;
  float* normW = nullptr; float* normB = nullptr;       // fc of the three AdaLayerNorms, concatenated: [3][2 D][S], [3][2 D]
  float* durW = nullptr; float* durB = nullptr;         // duration_proj [bins][D], [bins]
  float* emb = nullptr;
  KConv conv[KTEXT_MAX_DEPTH];
  float* lnG[KTEXT_MAX_DEPTH] = {}; float* lnB[KTEXT_MAX_DEPTH] = {};
  float* arena = nullptr; size_t arena_floats = 0;
};

namespace {

// the eight tensors of `p` -> one packed block (kokoro_text.h); the raw copies live on the device only until the repack has run
bool load_lstm(KConvLoader& L, hipStream_t st, const std::string& p, int In, int H, KokoroLstm& w) {
  static const char* dirs[2] = {"", "_reverse"};
  std::vector<float> host, t;
  size_t off[8];
  for (int d = 0; d < 2; ++d) {
    const std::string names[4] = {p + ".weight_ih_l0" + dirs[d], p + ".weight_hh_l0" + dirs[d], p + ".bias_ih_l0" + dirs[d], p + ".bias_hh_l0" + dirs[d]};
    for (int k = 0; k < 4; ++k) {
      const bool ok = k == 0 ? L.f32(names[k], t, {4 * H, In}) : k == 1 ? L.f32(names[k], t, {4 * H, H}) : L.f32(names[k], t, {4 * H});
      if (!ok) return false;
      off[d * 4 + k] = host.size();
      host.insert(host.end(), t.begin(), t.end());
    }
  }
  float* block = (float*)L.alloc(kokoro_lstm_floats(In, H) * 4);
  if (!block) return false;
  float* tmp = nullptr;
  if (hipMalloc((void**)&tmp, host.size() * 4) != hipSuccess) return L.fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed");
  bool ok = hipMemcpy(tmp, host.data(), host.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
  const KokoroLstmRaw raw = {{tmp + off[0], tmp + off[4]}, {tmp + off[1], tmp + off[5]}, {tmp + off[2], tmp + off[6]}, {tmp + off[3], tmp + off[7]}};
  ok = ok && kokoro_lstm_pack_launch(raw, In, H, block, w, st) == 0;
  ok = hipStreamSynchronize(st) == hipSuccess && ok;
  (void)hipFree(tmp);
  return ok || L.fail(MIA_ERR_DEVICE, "repack of '" + p + "' failed");
}

// `n` blocks of the handle's arena, each a multiple of 64 floats
int carve(mia_kokoro_text* h, const size_t* sizes, float** out, int n) {
  size_t tot = 0;
  for (int i = 0; i < n; ++i) tot += (sizes[i] + 63) / 64 * 64;
  if (int rc = mia_grow(h->ctx, h->arena, h->arena_floats, tot, "kokoro_text: scratch hipMalloc failed")) return rc;
  float* q = h->arena;
  for (int i = 0; i < n; ++i) { out[i] = q; q += (sizes[i] + 63) / 64 * 64; }
  return MIA_OK;
}

int check_tokens(mia_kokoro_text* h, int N, const char* who) {
  if (!h) return MIA_ERR_INVALID_ARGUMENT;
  if (N < 1 || N > KOKORO_MAX_TOKENS) return mia_fail(h->ctx, MIA_ERR_INVALID_ARGUMENT, "%s: the token count must be in [1, %d] (got %d)", who, KOKORO_MAX_TOKENS, N);
  return MIA_OK;
}

#define KTEXT_LAUNCHED(h, what) do { if (hipGetLastError() != hipSuccess) return mia_fail((h)->ctx, MIA_ERR_DEVICE, "kokoro_text: kernel launch failed (%s)", what); } while (0)

}  // namespace

extern "C" {

mia_kokoro_text* mia_kokoro_text_load(mia_ctx* ctx, const mia_kokoro_text_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_text_load: null argument"); return nullptr; }
  const mia_kokoro_text_config& g = *cfg;
  if (g.d_model < 32 || g.d_model % 32 || !kokoro_lstm_shape_ok(g.d_model + g.style_dim, g.d_model / 2) || g.style_dim < 32 || g.style_dim % 32 ||
      g.n_symbols < 1 || g.kernel < 1 || g.kernel > 11 || g.kernel % 2 == 0 || g.depth < 1 || g.depth > KTEXT_MAX_DEPTH) {
    mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_text_load: unsupported configuration (d_model and style_dim multiples of 32, d_model <= 512, d_model + style_dim <= 1024, odd kernel <= 11, depth <= 8)");
    return nullptr;
  }
  if (hipSetDevice(ctx->device) != hipSuccess) { mia_fail(ctx, MIA_ERR_DEVICE, "kokoro_text_load: hipSetDevice failed"); return nullptr; }
  mia_kokoro_text* h = new mia_kokoro_text();
  h->ctx = ctx; h->cfg = g; h->D = g.d_model; h->S = g.style_dim; h->H = g.d_model / 2;
  const int D = h->D, S = h->S, H = h->H;
  KConvLoader L; L.allocs = &h->allocs; L.index(tensors, n_tensors);
  hipStream_t st = ctx->stream;
  const std::string P = "predictor.", E = "text_encoder.";
  bool ok = true;
  std::vector<float> nw, nb, t;
  for (int i = 0; i < 3 && ok; ++i) {
    const std::string si = std::to_string(i);
    ok = load_lstm(L, st, P + "text_encoder.lstm" + si, D + S, H, h->enc[i]);
    ok = ok && L.f32(P + "text_encoder.norm" + si + ".fc.weight", t, {2 * D, S});
    if (ok) nw.insert(nw.end(), t.begin(), t.end());
    ok = ok && L.f32(P + "text_encoder.norm" + si + ".fc.bias", t, {2 * D});
    if (ok) nb.insert(nb.end(), t.begin(), t.end());
  }
  if (ok) { h->normW = L.up(nw); h->normB = L.up(nb); }
  ok = ok && load_lstm(L, st, P + "lstm", D + S, H, h->plstm) && load_lstm(L, st, P + "shared", D + S, H, h->shared);
  if (ok) {                                            // the bin count is the tensor's, not the constructor's 1
    const mia_tensor_view* dp = L.find(P + "duration_proj.weight");
    h->bins = dp && dp->ndim == 2 ? (int)dp->shape[0] : 1;
    ok = h->bins >= 1 && h->bins <= 1024 && L.f32(P + "duration_proj.weight", t, {h->bins, D});
    if (ok) h->durW = L.up(t);
    ok = ok && L.f32(P + "duration_proj.bias", t, {h->bins});
    if (ok) h->durB = L.up(t);
  }
  ok = ok && L.f32(E + "embedding.weight", t, {g.n_symbols, D});
  if (ok) h->emb = L.up(t);
  for (int i = 0; i < g.depth && ok; ++i) {
    const std::string c = E + "cnn." + std::to_string(i);
    ok = L.conv_wn(c + ".conv", D, g.kernel, D, 1, (g.kernel - 1) / 2, true, false, h->conv[i]);
    ok = ok && L.f32(c + ".norm.gamma", t, {D});
    if (ok) h->lnG[i] = L.up(t);
    ok = ok && L.f32(c + ".norm.beta", t, {D});
    if (ok) h->lnB[i] = L.up(t);
  }
  ok = ok && load_lstm(L, st, E + "lstm", D, H, h->tlstm);
  if (!ok || !L.err.empty()) {
    mia_fail(ctx, L.err.empty() ? MIA_ERR_INVALID_ARGUMENT : L.code, "kokoro_text_load: %s", L.err.empty() ? "failed" : L.err.c_str());
    mia_kokoro_text_free(h);
    return nullptr;
  }
  return h;
}

void mia_kokoro_text_free(mia_kokoro_text* h) {
  if (!h) return;
  (void)hipStreamSynchronize(h->ctx->stream);
  for (void* p : h->allocs) (void)hipFree(p);
  if (h->arena) (void)hipFree(h->arena);
  delete h;
}

int mia_kokoro_text_durations(mia_kokoro_text* h, const float* d_en, int N, const float* s_pred, float speed, float* d_out, int32_t* dur_out,
                              float* dur_raw, int mem) {
  if (int rc = check_tokens(h, N, "kokoro_text_durations")) return rc;
  MIA_CHECK_ARG(h->ctx, d_en && s_pred && d_out && dur_out && dur_raw && speed > 0.f && HostIo::valid(mem), "kokoro_text_durations: bad argument");
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  const int D = h->D, S = h->S, H = h->H;
  const size_t sizes[] = {(size_t)N * (D + S), (size_t)N * D, kokoro_lstm_scratch(N, H), (size_t)6 * D, (size_t)S, (size_t)N * D, (size_t)N, (size_t)N};
  float* b[8];
  if (int rc = carve(h, sizes, b, 8)) return rc;
  float* Lb = b[1]; float* scr = b[2]; float* style = b[3];
  hipStream_t st = h->ctx->stream;
  HostIo io(h->ctx, mem);
  const float* den = io.in(d_en, b[5], (size_t)N * D * 4);
  const float* sv = io.in(s_pred, b[4], (size_t)S * 4);
  float* A = io.out(d_out, b[0], (size_t)N * (D + S) * 4);
  int32_t* dur = io.out(dur_out, b[6], (size_t)N * 4);
  float* raw = io.out(dur_raw, b[7], (size_t)N * 4);
  if (kokoro_style_launch(h->normW, h->normB, sv, style, 6 * D, S, st)) return mia_fail(h->ctx, MIA_ERR_DEVICE, "kokoro_text: kernel launch failed (style)");
  hipLaunchKernelGGL(ktext_cat_style, dim3(blocks((int64_t)N * (D + S))), dim3(256), 0, st, den, sv, A, N, D, S);
  KTEXT_LAUNCHED(h, "cat_style");
  for (int i = 0; i < 3; ++i) {
    if (int rc = kokoro_lstm_run(h->ctx, h->enc[i], A, D + S, N, scr, Lb, D)) return rc;
    hipLaunchKernelGGL(ktext_layernorm, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, Lb, (int64_t)D, A, (int64_t)(D + S), N, D,
                       style + (size_t)i * 2 * D, style + (size_t)i * 2 * D + D, 1.0f, 1.0f);
    KTEXT_LAUNCHED(h, "ada_layer_norm");
  }
  if (int rc = kokoro_lstm_run(h->ctx, h->plstm, A, D + S, N, scr, Lb, D)) return rc;
  hipLaunchKernelGGL(ktext_duration, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, Lb, (int64_t)D, h->durW, h->durB, h->bins, D, speed, dur, raw, N);
  KTEXT_LAUNCHED(h, "duration");
  return io.finish();
}

int mia_kokoro_text_encode(mia_kokoro_text* h, const int32_t* ids, int N, float* t_en_out, int mem) {
  if (int rc = check_tokens(h, N, "kokoro_text_encode")) return rc;
  MIA_CHECK_ARG(h->ctx, ids && t_en_out && HostIo::valid(mem), "kokoro_text_encode: bad argument");
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  const int D = h->D, H = h->H;
  HostIo io(h->ctx, mem);
  if (io.host())
    for (int i = 0; i < N; ++i)
      MIA_CHECK_ARG(h->ctx, ids[i] >= 0 && ids[i] < h->cfg.n_symbols, "kokoro_text_encode: id %d at position %d is outside the symbol table (%d)", ids[i], i, h->cfg.n_symbols);
  const size_t sizes[] = {(size_t)N, (size_t)N * D, (size_t)N * D, kokoro_lstm_scratch(N, H), (size_t)N * D};
  float* b[5];
  if (int rc = carve(h, sizes, b, 5)) return rc;
  float* X = b[1]; float* Y = b[2];
  hipStream_t st = h->ctx->stream;
  const int32_t* di = io.in(ids, b[0], (size_t)N * 4);
  float* out = io.out(t_en_out, b[4], (size_t)N * D * 4);
  hipLaunchKernelGGL(ktext_embed, dim3(blocks((int64_t)N * D)), dim3(256), 0, st, di, h->emb, h->cfg.n_symbols, X, N, D);
  KTEXT_LAUNCHED(h, "embed");
  for (int i = 0; i < h->cfg.depth; ++i) {
    if (int rc = kconv_run(h->ctx, h->conv[i], X, N, Y, N)) return rc;
    hipLaunchKernelGGL(ktext_layernorm, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, Y, (int64_t)D, X, (int64_t)D, N, D, h->lnG[i], h->lnB[i], 0.0f, 0.2f);
    KTEXT_LAUNCHED(h, "layer_norm");
  }
  if (int rc = kokoro_lstm_run(h->ctx, h->tlstm, X, D, N, b[3], out, D)) return rc;
  return io.finish();
}

int mia_kokoro_text_align(mia_kokoro_text* h, const float* d, const float* t_en, const int32_t* dur, int N, float* en_out, float* asr_out, int* T,
                          int mem) {
  if (int rc = check_tokens(h, N, "kokoro_text_align")) return rc;
  MIA_CHECK_ARG(h->ctx, d && t_en && dur && en_out && asr_out && T && HostIo::valid(mem), "kokoro_text_align: bad argument");
  MIA_CHECK_ARG(h->ctx, *T >= 1, "kokoro_text_align: *T must hold the row capacity of en_out and asr_out on entry (got %d)", *T);
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  const int D = h->D, W = h->D + h->S, cap = *T < KOKORO_MAX_ROWS ? *T : KOKORO_MAX_ROWS;
  HostIo io(h->ctx, mem);
  const bool host = io.host();
  if (host) for (int i = 0; i < N; ++i) MIA_CHECK_ARG(h->ctx, dur[i] >= 0, "kokoro_text_align: duration %d at position %d is negative", dur[i], i);
  const size_t rows = host ? (size_t)cap : 0;
  const size_t sizes[] = {(size_t)N * W, (size_t)N * D, (size_t)N, rows * W, rows * D, 64};
  float* b[6];
  if (int rc = carve(h, sizes, b, 6)) return rc;
  hipStream_t st = h->ctx->stream;
  const float* dd = io.in(d, b[0], (size_t)N * W * 4);
  const float* dt = io.in(t_en, b[1], (size_t)N * D * 4);
  const int32_t* du = io.in(dur, b[2], (size_t)N * 4);
  float* en = host ? b[3] : en_out; float* asr = host ? b[4] : asr_out;
  hipLaunchKernelGGL(ktext_align, dim3((unsigned)N), dim3(256), 0, st, dd, W, dt, D, du, N, en, asr, cap, (int32_t*)b[5]);
  KTEXT_LAUNCHED(h, "align");
  int32_t total = 0;
  io.fetch(&total, b[5], 4);                        // the one value of the chain the host reads back: it sizes everything behind
  if (int rc = io.finish()) return rc;
  if (total < 1 || total > KOKORO_MAX_ROWS)
    return mia_fail(h->ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_text_align: the durations sum to %d rows, outside [1, %d]", total, KOKORO_MAX_ROWS);
  if (total > cap) return mia_fail(h->ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_text_align: the durations sum to %d rows, the outputs hold %d", total, cap);
  if (host) {
    io.check(hipMemcpyAsync(en_out, en, (size_t)total * W * 4, io.to_caller(), st));
    io.check(hipMemcpyAsync(asr_out, asr, (size_t)total * D * 4, io.to_caller(), st));
  }
  *T = total;
  return io.finish();
}

int mia_kokoro_text_shared(mia_kokoro_text* h, const float* en, int T, float* x_out, int mem) {
  if (!h) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(h->ctx, T >= 1 && T <= KOKORO_MAX_ROWS, "kokoro_text_shared: the row count must be in [1, %d] (got %d)", KOKORO_MAX_ROWS, T);
  MIA_CHECK_ARG(h->ctx, en && x_out && HostIo::valid(mem), "kokoro_text_shared: bad argument");
  MIA_HIP(h->ctx, hipSetDevice(h->ctx->device));
  const int D = h->D, W = h->D + h->S;
  const size_t sizes[] = {(size_t)T * W, (size_t)T * D, kokoro_lstm_scratch(T, h->H), (size_t)T * D};
  float* b[4];
  if (int rc = carve(h, sizes, b, 4)) return rc;
  HostIo io(h->ctx, mem);
  const float* de = io.in(en, b[0], (size_t)T * W * 4);
  float* xo = io.out(x_out, b[3], (size_t)T * D * 4);
  if (int rc = kokoro_lstm_run(h->ctx, h->shared, de, W, T, b[2], b[1], D)) return rc;
  // time-major [T][D] -> the channel-major [D][T] mia_kokoro_f0n takes: kokoro_pack with the roles of rows and channels swapped
  if (kokoro_pack_launch(b[1], xo, T, 0, T, D, h->ctx->stream)) return mia_fail(h->ctx, MIA_ERR_DEVICE, "kokoro_text: kernel launch failed (transpose)");
  return io.finish();
}

}  // extern "C"
