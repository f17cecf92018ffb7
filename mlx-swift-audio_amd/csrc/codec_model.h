// codec_model.h -- the SNAC / DAC handle: its layer program (Op), the program's geometry, and what the codec*.hip files share.
//   codec_load.hip    builds the programs from a checkpoint           codec.hip         runs them (single decode, length queries)
//   codec_batch.hip   stacked decode of several utterances            codec_encode.hip  DAC encoder + residual vector quantisation
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "codec.h"
#include "mia_internal.h"

// the library's own types and functions below are hidden: they add nothing to its dynamic symbols
#pragma GCC visibility push(hidden)
enum OpKind { OP_CONV, OP_CONVT, OP_DW, OP_NOISE1, OP_NOISEC, OP_OUT1 };

struct Op {
  OpKind kind;
  float* w = nullptr;        // device weights in the kernel's layout
  float* b = nullptr;
  float* a_pre = nullptr;    // snake alpha applied to the input
  float* a_post = nullptr;   // snake alpha applied to the output (depthwise only)
  int N = 0, Cin = 0, taps = 1, dil = 1, pad = 0;
  int stride = 1;            // OP_CONVT: upsampling factor; OP_CONV: > 1 = strided (the DAC encoder's down-convolution)
  bool residual = false;     // Y = X_res + conv(H)   (in place on the residual stream)
  bool side = false;         // OP_CONV: h = conv(x) into the side buffer, x stays the stream (first conv of the DAC residual unit)
};

#pragma GCC visibility pop

constexpr int MIA_CODEC_MAX_RATES = 8;   // upsampling stages of a decoder (checked at load); at most one noise block follows each

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
  // scratch (grow-only, mia_grow): the stream and its two side buffers always asked for at one size (codec_scratch)
  float* buf[3] = {nullptr, nullptr, nullptr};
  size_t buf_cap[3] = {0, 0, 0};
  int32_t* d_codes = nullptr; size_t codes_cap = 0;
  float* d_noise = nullptr; size_t noise_cap = 0;
  float* d_pcm = nullptr; size_t pcm_cap = 0;
  // per-call tables of the stacked decode (Stack below): pinned staging owned by the handle, so that the memory behind the upload
  // outlives it on every return path; tab_ev marks the last upload's end and is waited for before the staging is written again
  void* h_tab = nullptr; void* d_tab = nullptr; size_t tab_cap = 0;
  hipEvent_t tab_ev = nullptr;
  // bytes of activations up to which a stage of the batch entries runs stacked (mia_codec_set_stack_budget).  SNAC: the Infinity Cache;
  // DAC (mia_dac_load): no limit -- measured both ways, see decode_batch_common
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

#pragma GCC visibility push(hidden)
// ---- geometry ---------------------------------------------------------------------------------------------------------------------------
// rows after a transposed convolution with kernel 2 * stride
static inline int64_t convt_rows(const Op& op, int64_t T) { return (T - 1) * op.stride - 2 * op.pad + 2 * op.stride; }
// rows after a strided convolution
static inline int64_t strided_rows(const Op& op, int64_t T) { return (T + 2 * op.pad - op.taps) / op.stride + 1; }

// everything a decode of a T0-row latent needs to know about sizes, from one walk of the program (no heap: the single call runs it per chunk)
struct Geometry {
  int n_stages = 1, n_blocks = 0;                  // a stage ends at every transposed convolution; blocks = noise blocks
  int64_t rows[MIA_CODEC_MAX_RATES + 1] = {};      // valid rows at every stage
  int64_t noise_off[MIA_CODEC_MAX_RATES] = {};     // where each noise block's values start
  int64_t noise_total = 0;
  size_t max_floats = 0;                           // the largest T * C along the program
  int64_t T_final = 0;
};

static inline Geometry codec_geometry(const mia_codec* c, int64_t T0) {
  Geometry g;
  int64_t T = T0; int C = c->latent;
  g.rows[0] = T0; g.max_floats = (size_t)T * C;
  for (const Op& op : c->ops) {
    if (op.kind == OP_CONV && !op.residual) C = op.N;
    else if (op.kind == OP_CONVT) { T = convt_rows(op, T); C = op.N; g.rows[g.n_stages++] = T; }
    else if (op.kind == OP_NOISE1 || op.kind == OP_NOISEC) { g.noise_off[g.n_blocks++] = g.noise_total; g.noise_total += T; }
    g.max_floats = std::max(g.max_floats, (size_t)T * C);
  }
  g.T_final = T;
  return g;
}

// ---- pieces the entries share -------------------------------------------------------------------------------------------------------------
// the three scratch buffers at `floats` each.  A failed allocation leaves that buffer empty on record (mia_grow), so the next call grows it again.
static inline int codec_scratch(mia_codec* c, size_t floats) {
  for (int i = 0; i < 3; ++i)
    if (int rc = mia_grow(c->ctx, c->buf[i], c->buf_cap[i], floats, "codec: scratch hipMalloc failed")) return rc;
  return MIA_OK;
}

// the quantiser side of the embedding kernel's arguments for the first n_levels levels; the caller adds where the codes are
static inline EmbedArgs codec_embed_args(const mia_codec* c, int n_levels, const int* strides) {
  EmbedArgs ea{}; ea.n_levels = n_levels; ea.cb_dim = c->cb_dim;
  for (int i = 0; i < n_levels; ++i) { ea.codebook[i] = c->codebook[i]; ea.weff[i] = c->weff[i]; ea.bias[i] = c->ebias[i]; ea.stride[i] = strides[i]; }
  return ea;
}

// tap-GEMM arguments of an OP_CONV over T rows: x = the stream, h = its side buffer, y = the spare.  A residual conv reads h and adds into
// x; a side conv writes h; any other writes y, which the caller then swaps in as the stream (g.T_out rows, fewer than T when strided).
static inline ConvGemmArgs codec_conv_args(const Op& op, float* x, float* h, float* y, int64_t T) {
  const int st = op.stride > 1 ? op.stride : 1;
  const int64_t T_out = st > 1 ? strided_rows(op, T) : T;
  ConvGemmArgs g;
  g.X = op.residual ? h : x; g.ldx = op.Cin; g.T_in = (int)T; g.W = op.w; g.bias = op.b; g.alpha = op.a_pre;
  g.M = (int)T_out; g.N = op.N; g.Cin = op.Cin; g.taps = op.taps; g.dil = op.dil; g.pad = op.pad; g.T_out = (int)T_out; g.x_row_mul = st;
  if (op.residual) { g.R = x; g.ldr = op.N; }
  g.Y = op.residual ? x : (op.side ? h : y); g.ldy = op.N;
  return g;
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

// where a run of the program stands: the stream x [T][C] with its two side buffers, the noise values consumed, the stage (transposed
// convolutions passed) and the noise blocks passed
struct Cursor {
  float* x; float* h; float* y;
  int64_t T; int C;
  int64_t noff = 0;
  int stage = 0, nblock = 0;
};

// the executor (codec.hip)
int codec_run(mia_codec* c, Cursor& k, size_t begin, size_t end, const float* d_noise, float* d_pcm, const Stack& st = Stack());
#pragma GCC visibility pop
