// kokoro_bert.hip -- Kokoro's ALBERT (TTS/Kokoro/Albert/*.swift) and bert_encoder, fp32, gfx950, B = 1: padded phoneme ids ->
// sequence output [N][hidden] -> d_en [N][out_dim], the input of mia_kokoro_text_durations (KokoroTTS.swift:262-287).  The attention
// mask of the one padded sequence is all ones, so (1 - mask) * -10000 adds zero and no mask is implemented; the pooler has no caller
// and is not built.  One group with one inner layer: the same weights serve every layer application.
//
// Two kernels live here, both one wave per row with the row in registers and both built on one statistics rule (row_stats):
//   albert_embed_ln   word[id] + position[n] + token_type[0] (in that order), then LayerNorm over the E embedding columns
//   albert_ln_rows    LayerNorm over `hidden` columns; the residual it follows rides in the producing GEMM's R epilogue
// The Linears run on the fp32 tap GEMM (taps = 1), the attention on attn_f32 reading q | k | v as column ranges of one [N][3 hidden]
// buffer.  Per layer: QKV GEMM, attention, dense (+ x), LayerNorm, ffn (exact-erf GELU), ffn_output (+ attention output), LayerNorm.
#include <string>
#include <vector>

#include "../../include/mia_kokoro.h"
#include "codec.h"
#include "kokoro_text.h"
#include "ops.h"
#include "tensor_loader.h"

namespace {

constexpr float ALBERT_EPS = 1e-12f;
constexpr int ALBERT_MAX_HIDDEN = 1024, ALBERT_MAX_EMBED = 256;

// Mean and 1 / sqrt(biased variance + eps) of the row a wave holds as NV float4 per lane (`live`: the lane's float4 j lies inside the
// row; the others hold zeros and are kept out of the squares).  Two steps with x - mean explicit: with eps = 1e-12 a constant row has
// rstd = 1e6, and only an exact zero survives that factor.  The in-lane sums pair up ((x + y) + (z + w)) and the lanes meet in a fixed
// xor butterfly, so every partial sum of a constant row is a doubling wherever the column count is a power of two (exact), every lane
// ends with the same bits, and two runs give the same bits.  No LDS, no atomics.
template <int NV>
__device__ __forceinline__ void row_stats(const float4 (&v)[NV], const bool (&live)[NV], int C, float& mean, float& den) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  mean = s / (float)C;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d = v[j].w - mean;
    q += live[j] ? (a * a + b * b) + (c * c + d * d) : 0.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  den = sqrtf(q / (float)C + ALBERT_EPS);
}

__device__ __forceinline__ float4 ln_apply(const float4 x, float mean, float den, const float4 g, const float4 b) {
  return make_float4(g.x * ((x.x - mean) / den) + b.x, g.y * ((x.y - mean) / den) + b.y, g.z * ((x.z - mean) / den) + b.z,
                     g.w * ((x.w - mean) / den) + b.w);
}

// One wave per token, four tokens per workgroup.  E / 4 <= 64 lanes each gather one float4 of the three table rows; the ids were
// range-checked on the host.
__global__ __launch_bounds__(256) void albert_embed_ln(const int32_t* __restrict__ ids, const float* __restrict__ word, const float* __restrict__ pos,
                                                       const float* __restrict__ type, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ y, int N, int E) {
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (n >= N) return;
  const bool live[1] = {lane * 4 < E};
  float4 v[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
  if (live[0]) {
    const float4 w = *reinterpret_cast<const float4*>(word + (int64_t)ids[n] * E + lane * 4);
    const float4 p = *reinterpret_cast<const float4*>(pos + (int64_t)n * E + lane * 4);
    const float4 t = *reinterpret_cast<const float4*>(type + lane * 4);
    v[0] = make_float4((w.x + p.x) + t.x, (w.y + p.y) + t.y, (w.z + p.z) + t.z, (w.w + p.w) + t.w);
  }
  float mean, den;
  row_stats<1>(v, live, E, mean, den);
  if (live[0])
    *reinterpret_cast<float4*>(y + (int64_t)n * E + lane * 4) =
        ln_apply(v[0], mean, den, *reinterpret_cast<const float4*>(gamma + lane * 4), *reinterpret_cast<const float4*>(beta + lane * 4));
}

// One wave per row of C floats (C % 64 == 0, C <= 256 NV), four rows per workgroup: the row is read once, as float4 j * 64 + lane of it
// (a wave's load covers 1 KB of consecutive bytes), and stays in registers through both statistics passes and the write.  x and y may
// be the same buffer.
template <int NV>
__global__ __launch_bounds__(256) void albert_ln_rows(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int N, int C) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= N) return;
  const float* xr = x + (int64_t)r * C;
  float4 v[NV];
  bool live[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    live[j] = (j * 64 + lane) * 4 < C;
    v[j] = live[j] ? *reinterpret_cast<const float4*>(xr + (j * 64 + lane) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  float mean, den;
  row_stats<NV>(v, live, C, mean, den);
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int c = (j * 64 + lane) * 4;
    if (live[j])
      *reinterpret_cast<float4*>(y + (int64_t)r * C + c) =
          ln_apply(v[j], mean, den, *reinterpret_cast<const float4*>(gamma + c), *reinterpret_cast<const float4*>(beta + c));
  }
}

struct Linear { float* w = nullptr; float* b = nullptr; int out = 0, in = 0; };
struct Norm { float* g = nullptr; float* b = nullptr; };

}  // namespace

struct mia_kokoro_bert {
  mia_ctx* ctx = nullptr;
  mia_kokoro_bert_config cfg{};
  std::vector<void*> allocs;
  float *word = nullptr, *pos = nullptr, *type = nullptr;
  Norm emb_ln, attn_ln, full_ln;
  Linear map_in, qkv, dense, ffn, ffn_out, enc;         // qkv: query | key | value stacked to [3 hidden][hidden]
};

namespace {

const char* config_error(const mia_kokoro_bert_config& g) {
  if (g.hidden < 64 || g.hidden % 64 || g.hidden > ALBERT_MAX_HIDDEN) return "hidden must be a multiple of 64 up to 1024";
  if (g.heads < 1 || (int64_t)g.heads * 64 != g.hidden) return "heads x 64 must equal hidden (the attention kernel's head width)";
  if (g.embed < 32 || g.embed % 32 || g.embed > ALBERT_MAX_EMBED) return "embed must be a multiple of 32 up to 256";
  if (g.intermediate < 32 || g.intermediate % 32) return "intermediate must be a multiple of 32";
  if (g.out_dim < 32 || g.out_dim % 32) return "out_dim must be a multiple of 32";
  if (g.vocab < 1 || g.n_layers < 1 || g.max_positions < 1 || g.type_vocab < 1) return "vocab, n_layers, max_positions and type_vocab must be positive";
  return nullptr;
}

struct BertLoader : TensorLoader {
  bool vec(const std::string& n, int64_t d, float*& out) {
    std::vector<float> t;
    if (!f32(n, t, {d})) return false;
    out = up(t);
    return out != nullptr;
  }
  bool table(const std::string& n, int64_t rows, int64_t cols, float*& out) {
    std::vector<float> t;
    if (!f32(n, t, {rows, cols})) return false;
    out = up(t);
    return out != nullptr;
  }
  bool norm(const std::string& p, int d, Norm& o) { return vec(p + ".weight", d, o.g) && vec(p + ".bias", d, o.b); }
  // the Linears of `names`, stacked along the output axis, as stored ([out][in], what the tap GEMM takes as W)
  bool linear(std::initializer_list<std::string> names, int out, int in, Linear& o) {
    std::vector<float> w, b, t;
    for (const std::string& p : names) {
      if (!f32(p + ".weight", t, {out, in})) return false;
      w.insert(w.end(), t.begin(), t.end());
      if (!f32(p + ".bias", t, {out})) return false;
      b.insert(b.end(), t.begin(), t.end());
    }
    o.w = up(w); o.b = up(b); o.out = out * (int)names.size(); o.in = in;
    return o.w && o.b;
  }
};

// Y [N][l.out] = act(X [N][l.in] W^T + b) + R
int linear_run(mia_ctx* ctx, const Linear& l, const float* X, int N, float* Y, const float* R, int act) {
  ConvGemmArgs g;
  g.X = X; g.ldx = l.in; g.T_in = N; g.W = l.w; g.bias = l.b; g.M = N; g.N = l.out; g.Cin = l.in; g.taps = 1;
  g.Y = Y; g.ldy = l.out; g.T_out = N; g.R = R; g.ldr = l.out; g.gelu = act;
  return codec_conv_gemm_run(ctx, g, 1, "kokoro_bert");
}

int ln_rows_run(mia_ctx* ctx, const float* x, float* y, const Norm& n, int N, int C) {
  const dim3 grid((unsigned)((N + 3) / 4)), block(256);
  switch ((C + 255) / 256) {
    case 1: hipLaunchKernelGGL(albert_ln_rows<1>, grid, block, 0, ctx->stream, x, y, n.g, n.b, N, C); break;
    case 2: hipLaunchKernelGGL(albert_ln_rows<2>, grid, block, 0, ctx->stream, x, y, n.g, n.b, N, C); break;
    case 3: hipLaunchKernelGGL(albert_ln_rows<3>, grid, block, 0, ctx->stream, x, y, n.g, n.b, N, C); break;
    default: hipLaunchKernelGGL(albert_ln_rows<4>, grid, block, 0, ctx->stream, x, y, n.g, n.b, N, C); break;
  }
  return hipGetLastError() == hipSuccess ? MIA_OK : mia_fail(ctx, MIA_ERR_DEVICE, "kokoro_bert: kernel launch failed (layer norm)");
}

}  // namespace

extern "C" {

mia_kokoro_bert* mia_kokoro_bert_load(mia_ctx* ctx, const mia_kokoro_bert_config* cfg, const mia_tensor_view* tensors, int n_tensors) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_bert_load: null argument"); return nullptr; }
  const mia_kokoro_bert_config& g = *cfg;
  if (const char* e = config_error(g)) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_bert_load: %s", e); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { mia_fail(ctx, MIA_ERR_DEVICE, "kokoro_bert_load: hipSetDevice failed"); return nullptr; }
  mia_kokoro_bert* h = new mia_kokoro_bert();
  h->ctx = ctx; h->cfg = g;
  BertLoader L; L.allocs = &h->allocs; L.index(tensors, n_tensors);          // bert.pooler.* and *position_ids are never asked for
  const std::string B = "bert.embeddings.", E = "bert.encoder.", Y = "bert.encoder.albert_layer_groups.0.albert_layers.0.";
  const int Hd = g.hidden;
  const bool ok = L.table(B + "word_embeddings.weight", g.vocab, g.embed, h->word) &&
                  L.table(B + "position_embeddings.weight", g.max_positions, g.embed, h->pos) &&
                  L.table(B + "token_type_embeddings.weight", g.type_vocab, g.embed, h->type) && L.norm(B + "LayerNorm", g.embed, h->emb_ln) &&
                  L.linear({E + "embedding_hidden_mapping_in"}, Hd, g.embed, h->map_in) &&
                  L.linear({Y + "attention.query", Y + "attention.key", Y + "attention.value"}, Hd, Hd, h->qkv) &&
                  L.linear({Y + "attention.dense"}, Hd, Hd, h->dense) && L.norm(Y + "attention.LayerNorm", Hd, h->attn_ln) &&
                  L.linear({Y + "ffn"}, g.intermediate, Hd, h->ffn) && L.linear({Y + "ffn_output"}, Hd, g.intermediate, h->ffn_out) &&
                  L.norm(Y + "full_layer_layer_norm", Hd, h->full_ln) && L.linear({"bert_encoder"}, g.out_dim, Hd, h->enc);
  if (!ok || !L.err.empty()) {
    mia_fail(ctx, L.err.empty() ? MIA_ERR_INVALID_ARGUMENT : L.code, "kokoro_bert_load: %s", L.err.empty() ? "failed" : L.err.c_str());
    mia_kokoro_bert_free(h);
    return nullptr;
  }
  return h;
}

void mia_kokoro_bert_free(mia_kokoro_bert* h) {
  if (!h) return;
  (void)hipStreamSynchronize(h->ctx->stream);
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
}

int mia_kokoro_bert_encode(mia_kokoro_bert* h, const int32_t* ids, int N, int n_layers, float* hidden_out, float* d_en_out, int mem) {
  if (!h) return MIA_ERR_INVALID_ARGUMENT;
  mia_ctx* ctx = h->ctx;
  const mia_kokoro_bert_config& g = h->cfg;
  const int n_max = g.max_positions < KOKORO_MAX_TOKENS ? g.max_positions : KOKORO_MAX_TOKENS;
  MIA_CHECK_ARG(ctx, N >= 1 && N <= n_max, "kokoro_bert_encode: the token count must be in [1, %d] (got %d)", n_max, N);
  MIA_CHECK_ARG(ctx, ids && (hidden_out || d_en_out) && HostIo::valid(mem), "kokoro_bert_encode: bad argument (ids and at least one output are required)");
  MIA_CHECK_ARG(ctx, n_layers <= g.n_layers, "kokoro_bert_encode: n_layers must be at most %d (got %d)", g.n_layers, n_layers);
  for (int i = 0; i < N; ++i)
    MIA_CHECK_ARG(ctx, ids[i] >= 0 && ids[i] < g.vocab, "kokoro_bert_encode: id %d at position %d is outside the vocabulary (%d)", ids[i], i, g.vocab);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const int layers = n_layers > 0 ? n_layers : g.n_layers, Hd = g.hidden;
  const size_t row = (size_t)N * 4;
  HostIo io(ctx, mem);
  Carve cv;
  const size_t o_ids = cv.add(row), o_emb = cv.add(row * g.embed), o_x = cv.add(row * Hd), o_qkv = cv.add(row * 3 * Hd), o_ctx = cv.add(row * Hd);
  const size_t o_t = cv.add(row * Hd), o_a = cv.add(row * Hd), o_ff = cv.add(row * g.intermediate), o_den = cv.add(io.staged(row * g.out_dim));
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  auto f = [&](size_t off) { return (float*)(ws + off); };
  float *emb = f(o_emb), *x = f(o_x), *qkv = f(o_qkv), *att = f(o_ctx), *t = f(o_t), *a = f(o_a), *ff = f(o_ff);
  const int32_t* d_ids = io.table(ids, ws + o_ids, row);                      // ids are a host array whatever `mem` says of the outputs
  float* last = io.out(hidden_out, x, row * Hd);                              // what the last layer writes: the caller's buffer (device), else x
  if (!last) last = x;
  float* den = io.out(d_en_out, ws + o_den, row * g.out_dim);
  hipLaunchKernelGGL(albert_embed_ln, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, ctx->stream, d_ids, h->word, h->pos, h->type, h->emb_ln.g, h->emb_ln.b,
                     emb, N, g.embed);
  if (hipGetLastError() != hipSuccess) return mia_fail(ctx, MIA_ERR_DEVICE, "kokoro_bert: kernel launch failed (embeddings)");
  if (int rc = linear_run(ctx, h->map_in, emb, N, x, nullptr, 0)) return rc;
  for (int l = 0; l < layers; ++l) {
    if (int rc = linear_run(ctx, h->qkv, x, N, qkv, nullptr, 0)) return rc;
    AttnF32Args q;
    q.q = qkv; q.k = qkv + Hd; q.v = qkv + 2 * Hd; q.ldq = q.ldk = q.ldv = 3 * Hd; q.out = att; q.ldo = Hd; q.B = 1; q.T = N; q.H = g.heads; q.scale = 0.125f;
    if (const char* e = mia_attn_f32_check(q)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "kokoro_bert: %s", e);
    if (mia_attn_f32_launch(q, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "kokoro_bert: attention launch failed");
    if (int rc = linear_run(ctx, h->dense, att, N, t, x, 0)) return rc;
    if (int rc = ln_rows_run(ctx, t, a, h->attn_ln, N, Hd)) return rc;
    if (int rc = linear_run(ctx, h->ffn, a, N, ff, nullptr, 1)) return rc;
    if (int rc = linear_run(ctx, h->ffn_out, ff, N, t, a, 0)) return rc;
    if (int rc = ln_rows_run(ctx, t, l + 1 == layers ? last : x, h->full_ln, N, Hd)) return rc;
  }
  if (den)
    if (int rc = linear_run(ctx, h->enc, last, N, den, nullptr, 0)) return rc;
  return io.finish();
}

}  // extern "C"
