// lm.h -- host-side interface between the LM decode sources: lm.hip (step kernels, prompt pass, step graph, entry points),
// the samplers (lm_sample_top_p.hip: Orpheus top-p; lm_sample_ras.hip: CosyVoice2 RAS; lm_sample_topk.hip: Fun-ASR greedy and top-k / top-p;
// their shared device code is lm_sample_device.h), lm_load.hip (checkpoint loader, state buffers, packed-weight attach) and lm_kvq.hip
// (the quantised KV cache: its prompt-pass quantiser and its attention); lm_prefill_attn.hip (the prompt pass's tiled causal attention) reads it too.
#pragma once
#include <vector>

#include "mia_internal.h"

struct LmState { int pos; int n_hist; int finished; int n_gen; int n_embeds; int n_out; int u_cursor; int n_prompt; int min_len; int max_len; int frozen; };   // min/max_len: RAS and greedy loops, per sequence
// frozen (the Marvis frame sets it when a sequence has drawn its all-zero frame; 0 everywhere else): the step's kernels on the 16-bit cache
// are no-ops for the sequence -- no embedding, no K/V row, no position advance -- so steps launched before the host reads the flag touch nothing of it

struct RasParams { float top_p; int top_k; int win; float tau; int eos; int min_len; int max_len; int n_uniforms; };

// MLX-affine 4- / 6- / 8-bit copy of one fused matrix in MFMA fragment order (skinny_quant.hip: skinny_gemm_qi); null = use the 16-bit weights
struct Q4W { uint32_t* wfrag = nullptr; float* stfrag = nullptr; };

struct LmLayer {
  Q4W q_qkv, q_o, q_gu, q_down;
  float* in_norm = nullptr; float* post_norm = nullptr;
  // the same gains times mia_carry_prescale (skinny.h) for the fused chain's SK_RESID producers, and 1 / that scale for the consumers
  float* in_norm_c = nullptr; float* post_norm_c = nullptr; float in_rs = 1.f, post_rs = 1.f;
  void* wqkv = nullptr; float* bqkv = nullptr;   // [(Hq+2Hkv)*dh][hidden]
  void* wo = nullptr;                            // [hidden][Hq*dh]
  void* wgu = nullptr;                           // [2*inter][hidden], rows interleaved gate/up
  void* wdown = nullptr;                         // [hidden][inter]
  // the same four in MFMA-fragment order (skinny.h) for the decode step's skinny GEMMs: one contiguous 1 KB per wave load instead of
  // 16 rows x 64 B (tools/micro/skinny_probe.hip, Orpheus-3B shapes, one sequence: 48.3 -> 43.7 us per layer); the batched prompt
  // pass (gemm.hip) keeps reading the row-major copies.  All eight are allocations of their own: mia_lm_release_dense frees them
  void* wqkv_f = nullptr; void* wo_f = nullptr; void* wgu_f = nullptr; void* wdown_f = nullptr;
};

struct mia_lm {
  mia_ctx* ctx = nullptr;
  mia_lm_config cfg{};
  int dtype = MIA_BF16;
  std::vector<void*> allocs;
  void* embed = nullptr;        // 16-bit [V][hidden]
  void* lm_head = nullptr;      // 16-bit [V][hidden] (== embed when tied)
  void* lm_head_f = nullptr;    // lm_head in MFMA-fragment order (decode step)
  Q4W q_head;                   // 4-bit copy of lm_head (mia_lm_attach_q4)
  int q_bits = 0;               // 4 | 6 | 8 once packed weights are attached (mia_lm_attach_quantized), 0 = none
  bool q4 = false;              // the step GEMVs stream the packed weights
  float* head_bias = nullptr;   // optional (CosyVoice2 llm_decoder)
  int head_vocab = 0;           // rows of lm_head (CosyVoice2: speech vocabulary + 3)
  void* gen_embed = nullptr;    // 16-bit [rows][hidden]: embedding of GENERATED ids when it differs from embed (speech_embedding)
  int gen_rows = 0;
  float* embeds = nullptr;      // fp32 [max_ctx][hidden]: caller-provided prompt embeddings (Qwen2LM.inference builds its prompt from three tables)
  int32_t* out_tokens = nullptr;  // [max_ctx] emitted tokens of the RAS loop
  float* final_norm = nullptr; float* final_norm_c = nullptr; float final_rs = 1.f;
  float* inv_freq = nullptr;    // [dh/2]
  // Qwen3: per-head RMSNorm gains of q and k, fp32 [n_layers][2][dh] (q_norm | k_norm), applied between the split-K sum (+ bias) and RoPE;
  // null = the checkpoint has none (Llama-3 / Qwen2) and the handle launches the kernel instances without the norm
  float* qk_norm = nullptr;
  std::vector<LmLayer> layers;
  // state
  void* k_cache = nullptr; void* v_cache = nullptr;   // [L][B][Hkv][max_ctx][dh]; null while the cache is quantised
  // quantised cache (mia_lm_set_kv_quant, lm_kvq.hip): codes [L][B][Hkv][max_ctx][dh * kv_bits / 32], pairs [L][B][Hkv][max_ctx][dh / 64]
  int kv_bits = 0;              // 0 = 16-bit cache, 4 | 8
  uint32_t* kq_codes = nullptr; uint32_t* vq_codes = nullptr; uint32_t* kq_pairs = nullptr; uint32_t* vq_pairs = nullptr;
  float* x = nullptr; void* h = nullptr; float* qkv_part = nullptr; void* q = nullptr; void* att = nullptr; void* act = nullptr;
  float* partial = nullptr; float* logits = nullptr;
  float* ss = nullptr;          // [2][hidden / 16][B]: per-tile partial sums of squares of the residual stream (SK_RESID producers)
  int32_t* tokens = nullptr;    // [max_ctx] full sequence
  int32_t* hist = nullptr;      // [64] repetition window (ring, oldest first)
  float* uniforms = nullptr;    // [max_ctx]
  void* smx = nullptr;            // top-p sampler scratch, lm_sample_ws_bytes() per sequence (slice records + radix slabs)
  LmState* state = nullptr;
  hipGraphExec_t graph = nullptr;       // one decode step (forward / top-p / RAS / greedy sampler), re-captured when its sampler arguments change
  int graph_mode = -1;                  // LM_STEP_* below
  int debug_flags = 0;                  // test hook (mia_lm_set_debug): bit 0 = no hipGraph, bit 1 = no batched prompt pass
  int prompt_attn = 0;                  // mia_lm_set_prompt_attention: 0 = the row kernel (lm_attention), 1 = lm_prefill_attn.hip on the 16-bit cache
  int prompt_packed = 0;                // mia_lm_set_prompt_weights: 0 = the prompt pass multiplies the 16-bit copy (gemm.hip), 1 = the packed weights (gemm_quant.hip)
  bool dense_released = false;          // mia_lm_release_dense: the layers' 16-bit Linears and their fragment copies are gone; q4 and prompt_packed stay 1
  mia_lm_sampler graph_sampler{};
  RasParams graph_ras{};
  int graph_top_k = 0;                  // LM_STEP_TOPK: the effective k (temperature and top_p travel in graph_sampler)
  int S_qkv = 1, S_o = 1, S_down = 1;
  // batched prompt pass (lm_prefill_rows): row buffers for one chunk of PF_ROWS positions, allocated on first use
  char* pf_buf = nullptr;
  // sequences decoded side by side (mia_lm_set_batch): every state buffer above holds B_cap rows / caches; the single-sequence entry
  // points use row 0
  int B_cap = 1;
  int graph_nb = 0;
  std::vector<void*> state_allocs;
};

// what ends a decode step: nothing (the host reads the logits), the top-p sampler, the RAS sampler, the greedy argmax, the top-k / top-p sampler
enum { LM_STEP_FORWARD = 0, LM_STEP_TOP_P = 1, LM_STEP_RAS = 2, LM_STEP_GREEDY = 3, LM_STEP_TOPK = 4 };

// launch a kernel template's F16 or BF16 instance; expects `const bool f16` and `hipStream_t s` in scope
#define LAUNCH_T(kern, grid, block, lds, ...) do { if (f16) hipLaunchKernelGGL((kern<F16>), grid, block, lds, s, __VA_ARGS__); else hipLaunchKernelGGL((kern<BF16>), grid, block, lds, s, __VA_ARGS__); } while (0)

// ---- lm_sample_*.hip: row b of every array belongs to sequence b (logits [B][V]; tokens / uniforms / out_tokens [B][max_ctx]; hist [B][64]) ----
// top-p sampler, six launches.  ws: lm_sample_ws_bytes() per sequence.  n_prompt < 0: every sequence's state holds its own prompt length
void lm_sample_launch(hipStream_t s, float* logits, int V, int32_t* tokens, int32_t* hist, const float* uniforms, LmState* st, void* ws, const mia_lm_sampler& sp,
                      int n_prompt, int max_ctx, int B);
size_t lm_sample_ws_bytes();
// RAS sampler, one launch; V <= LM_RAS_MAX_VOCAB (the kernel keeps the whole row in registers)
constexpr int LM_RAS_MAX_VOCAB = 8192;
void lm_sample_ras_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, const float* uniforms, LmState* st, const RasParams& rp,
                          int max_ctx, int B);
// greedy sampler, two launches: argmax per vocabulary slice, then one wave per sequence picks the winner (lowest index on exact ties),
// tests it against sp.stop_ids and appends it to tokens / out_tokens.  The prompt is embedding rows (LmState::n_embeds), the budget is
// LmState::max_len.  ws: the top-p workspace (lm_sample_ws_bytes() per sequence)
void lm_sample_greedy_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, LmState* st, void* ws, const mia_lm_sampler& sp,
                             int max_ctx, int B);
// top-k / top-p sampler (Fun-ASR's temperature > 0 branch; the rule is stated at mia_lm_generate_topk in mia.h), six launches: a 4-level
// radix select of the k-th largest logit over the vocabulary slices, a gather of the kept entries, one finishing workgroup per sequence
// (sort, nucleus, draw, the greedy loop's bookkeeping).  sp: temperature, top_p and the stop ids; k: the effective k, 1 <= k <=
// LM_TOPK_MAX_K (the caller clamps it to V).  Sequence b draws uniforms[b][LmState::u_cursor].  kept_ids / n_kept: null in the step; the
// standalone op reads the kept set through them (one sequence).  ws: the top-p workspace
constexpr int LM_TOPK_MAX_K = 1024;
void lm_sample_topk_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, const float* uniforms, LmState* st, void* ws,
                           const mia_lm_sampler& sp, int k, int max_ctx, int B, int32_t* kept_ids = nullptr, int32_t* n_kept = nullptr);

// ---- lm.hip: the two launch sites that branch on the cache mode (layer l of the handle's caches; the op ABI calls them on a bare handle) ----
// q|k|v rows of the prompt pass -> RoPE -> q rows + the layer's K/V rows at rowmap's (sequence, position)
void lm_launch_rope_cache(mia_lm* m, int layer, const float* qkv, const float* bias, void* q, const int2* rowmap, int M);
// fused: rows = sequences (row b uses state b and the b-th cache of the layer); otherwise rows = (sequence, position) pairs of rowmap
int lm_launch_attention(mia_lm* m, bool fused, int rows, const void* q, int layer, void* att, const int2* rowmap, const float* part, int S, const float* bias);

// ---- lm.hip: the pieces of one decode step, shared by the LM step (lm_enqueue_step) and the Marvis frame (marvis.hip) ----
// rows 0 .. nb-1 = sequences 0 .. nb-1 at their own LmState::pos: embedding (token id or the embedding row at that position) + first norm,
// then every layer (q|k|v GEMM -> RoPE + cache row + attention -> o-proj -> gate|up -> down).  Leaves the residual stream in m->x and the
// last layer's carried activation in m->h; positions are NOT advanced.  -1 when a launch is refused
int lm_enqueue_layers(mia_lm* m, int nb);
// out [nb][ldo] fp32 = final_norm(last hidden state) . W^T (+ bias), W [N][hidden] (Wf: its fragment-order copy or null; qw: packed copy or null)
int lm_enqueue_linear_of_last(mia_lm* m, int nb, const void* W, const void* Wf, const float* bias, const Q4W* qw, float* out, int64_t ldo, int N);
// pos += 1 for sequences 0 .. nb-1
void lm_enqueue_advance(mia_lm* m, int nb);
// whether the handle's step carries the RMSNorm across its GEMMs (capacity <= 4) or runs the split-K + reduce / norm chain
bool lm_fused_norm(const mia_lm* m);
// batched prompt pass.  rows: (sequence, position) pairs, every sequence's positions ascending; after the pass set_pos[b] (if >= 0) becomes
// state b's position.  Only K/V rows are produced: the caller runs each prompt's last position through the step
constexpr int LM_PREFILL_MIN_ROWS = 8;     // below this the step is as fast
bool lm_prefill_supported(const mia_lm* m);
int lm_prefill_rows(mia_lm* m, const std::vector<int2>& rows, const std::vector<int>& set_pos);

// ---- lm_kvq.hip ----
// one layer's packed cache (all sequences) and what its kernels need of the model
struct LmKvq {
  int dtype, dh, bits, Hq, Hkv, max_ctx;
  uint32_t* kq; uint32_t* vq; uint32_t* kp; uint32_t* vp;
  const LmState* st; const float* inv_freq;
};
// null when (bits, group_size, head_dim) is supported, else the message and, in *code, MIA_ERR_INVALID_ARGUMENT / MIA_ERR_UNSUPPORTED
const char* lm_kvq_check(int bits, int group_size, int head_dim, int* code);
void lm_kvq_launch_rope_cache(hipStream_t s, const LmKvq& a, const float* part, const float* bias, uint16_t* qout, const int2* rowmap, int M);
void lm_kvq_launch_attention(hipStream_t s, const LmKvq& a, bool fused, int rows, const uint16_t* q, uint16_t* out, const int2* rowmap, const float* part, int S,
                             const float* bias);
// host: n_rows packed rows -> fp32 [n_rows][dh] (scale * code + bias)
void lm_kvq_read_rows(const uint32_t* codes, const uint32_t* pairs, int64_t n_rows, int dh, int bits, int dtype, float* out);

// ---- lm_prefill_attn.hip: tiled causal GQA attention of a prompt-pass chunk over one layer's 16-bit cache ----
struct LmPromptAttn {
  const uint16_t* q = nullptr;            // [M][Hq * dh], rotated
  const uint16_t* kc = nullptr; const uint16_t* vc = nullptr;   // the layer's caches [B_cap][Hkv][max_ctx][dh], the chunk's rows already written
  uint16_t* out = nullptr;                // [M][Hq * dh]
  const int4* tiles = nullptr; int n_tiles = 0;   // device: (sequence, first position, first row, positions <= query tile) per query tile
  int Hq = 0, Hkv = 0, dh = 0, max_ctx = 0;
  int64_t seq_stride = 0;                 // Hkv * max_ctx * dh
  int dtype = MIA_BF16;
};
// positions per query tile for this head grouping (128, 64 or 32)
int lm_prefill_attn_qtile(int Hq, int Hkv);
// the chunk's rows (every sequence's positions ascending and contiguous) cut into runs and the runs into query tiles
void lm_prefill_attn_tiles(const int2* rows, int M, int qtile, std::vector<int4>& tiles);
const char* lm_prefill_attn_check(const LmPromptAttn& a);
int lm_prefill_attn_launch(const LmPromptAttn& a, hipStream_t s);

// ---- lm_load.hip ----
// The packed-weight attach in two halves, so that a caller with several handles (marvis.hip: two stacks) packs all of them or none.
// lm_attach_prepare checks the arguments and the tensors, repacks and uploads every step Linear into `out` and changes nothing of the
// handle; on failure its buffers are freed again, the context holds the message ("<who>: ...") and the MIA_ERR_* code is returned.
// lm_attach_commit hands the buffers to the handle, re-picks the splits and switches the step to the packed weights (cannot fail).
struct LmPacked { std::vector<void*> fresh; std::vector<Q4W> layers; Q4W head; int bits = 0; };      // layers: q_qkv, q_o, q_gu, q_down per layer
int lm_attach_prepare(mia_lm* m, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits, const char* who, LmPacked& out);
void lm_attach_commit(mia_lm* m, LmPacked& p);
void lm_attach_discard(LmPacked& p);
// every per-sequence buffer, for B sequences side by side (rows of the skinny GEMMs; caches [L][B][Hkv][max_ctx][dh]); drops the step graph
int lm_alloc_state(mia_lm* m, int B);
