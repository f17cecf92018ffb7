// marvis.hip -- Marvis TTS (CSM) frame generation on gfx950: MarvisModel.generateFrame (TTS/Marvis/Models/MarvisModel.swift:466-545) and
// the loop around it (MarvisTTS.decodePrompt, TTS/Marvis/MarvisTTS.swift:452-523).
//
// Both Llama stacks (MarvisLlamaBackbone.swift:169-292) are mia_lm handles built by the LM loader from re-keyed tensor views, and a frame
// is the LM step's own pieces (lm.h: lm_enqueue_layers / lm_enqueue_linear_of_last) chained twice: one backbone step, codebook0_head,
// a draw, then `codebooks` single-row decoder steps on a cache that starts empty, each behind the projection of its input row and --
// from position 1 on -- in front of its own head and draw.  The two-row first decoder pass of the reference is run as two single-row
// steps (row 0 contributes only its K/V).  Interleaved RoPE is turned into the step kernels' split-half form by permuting the rows of
// every q_proj / k_proj head at load ("Marvis").  The kernels the frame adds are marvis_kernels.hip.  Input rows reach the
// stacks as fp32 embedding rows (mia_lm::embeds), which lm_embed_norm turns into the first layer's normalised activation.
// mia_marvis_attach_quantized puts the checkpoint's packed Linears (MLX-affine 4 / 6 / 8 bit) beside the 16-bit ones: both stacks through
// the LM attach (lm.h: lm_attach_prepare / lm_attach_commit), the projection into a Q4W of this handle; the frame's GEMMs then stream them.
// mia_marvis_set_batch sizes the handle and both stacks for B sentences side by side (row b of every step = sequence b); one graph launch
// per frame for all of them.
#include <algorithm>
#include <cmath>
#include <deque>
#include <string>
#include <vector>

#include "../../include/mia_marvis.h"
#include "gemm.h"
#include "marvis.h"
#include "quant_repack.h"
#include "skinny.h"

struct mia_marvis {
  mia_ctx* ctx = nullptr;
  mia_marvis_config cfg{};
  int dtype = MIA_BF16;
  mia_lm* bb = nullptr; mia_lm* dec = nullptr;
  std::vector<void*> allocs;
  void* text_emb = nullptr;      // 16-bit [text_vocab][D]
  void* audio_emb = nullptr;     // 16-bit [K * V][D]
  void* proj = nullptr; void* proj_f = nullptr;          // 16-bit [d_dec][D], row-major and in fragment order
  Q4W q_proj;                    // packed copy of the projection (mia_marvis_attach_quantized); the stacks' own packed copies are in bb / dec
  int q_bits = 0;                // 4 | 6 | 8 once packed weights are attached; bb->q4 / dec->q4 say whether the frame streams them
  std::vector<void*> head, head_f;                       // K - 1 heads, transposed to [V][d_dec]; the fragment copies pad the rows to 16 with zeros
  // device state, B_cap sequences side by side (mia_marvis_set_batch): row / record b belongs to sequence b
  int B_cap = 1;
  std::vector<void*> state_allocs;
  MvState* st = nullptr;         // [B]
  int32_t* frame = nullptr;      // [B][K] the frame being drawn
  int32_t* forced = nullptr;     // [B][K]
  int32_t* frames_out = nullptr; // [B][max_ctx][K] frames emitted by the running call
  float* uniforms = nullptr;     // [B][max_ctx * K]
  float* logits = nullptr;       // [B][K][V] every head's logits of the last frame
  uint16_t* a16 = nullptr;       // [B][D] embedding row of the id just drawn
  int32_t* rows = nullptr;       // [2][B * max_ctx][K + 1] ids | mask of the rows being appended
  int2* rowmap = nullptr;        // [B * max_ctx] (sequence, position) of those rows
  // host mirror of sequence 0 (the single-sequence entry points; mia_marvis_generate_batch starts and ends on a reset handle)
  int pos = 0;                   // rows in the backbone cache
  bool started = false;          // a frame has been drawn since the last reset: the fed-back row is in place
  bool finished = false;         // the all-zero frame has been drawn
  int last_cb = 0;
  int debug_flags = 0;           // bit 0: launch every frame directly (no hipGraph); bit 1: no batched prompt pass
  hipGraphExec_t graph = nullptr;
  int g_cb = 0, g_nb = 0; float g_temp = 0.f, g_top_p = 0.f; bool g_forced = false;
};

namespace {

// Llama3ScaledRoPE.ropeInit + applyScaling (MarvisLlamaBackbone.swift:75-127) in its own fp32 operation order
std::vector<float> mv_inv_freq(int dims, float base, const mia_marvis_config& c) {
  std::vector<float> th(dims / 2);
  const float two_pi = 2.0f * (float)M_PI;
  for (int i = 0; i < dims / 2; ++i) {
    const float exponent = (float)(2 * i) / (float)dims;
    const float freq = powf(base, -exponent);
    float out = freq;
    if (c.rope_llama3) {
      const float wavelen = two_pi / freq;
      const float hi_thr = c.rope_old_ctx / c.rope_high, lo_thr = c.rope_old_ctx / c.rope_low;
      const float freq_div = freq / c.rope_factor;
      const float smooth_raw = (c.rope_old_ctx / wavelen - c.rope_low) / (c.rope_high - c.rope_low);
      const float smooth = fminf(fmaxf(smooth_raw, 0.0f), 1.0f);
      const float blend = (1.0f - smooth) * freq_div + smooth * freq;
      const float mid = wavelen > lo_thr ? freq_div : blend;
      out = wavelen < hi_thr ? freq : mid;
    }
    th[i] = out;
  }
  return th;
}

// one stack's tensors under the LM loader's names; q_proj / k_proj rows permuted per head: new[i] = old[2i], new[i + dh/2] = old[2i + 1]
struct StackViews {
  std::deque<std::string> names;
  std::deque<std::vector<char>> bufs;
  std::vector<mia_tensor_view> views;
  void alias(const mia_tensor_view& src, const std::string& name) {
    names.push_back(name);
    mia_tensor_view v = src; v.name = names.back().c_str();
    views.push_back(v);
  }
  void permuted(const mia_tensor_view& src, const std::string& name, int heads, int dh) {
    const size_t es = src.dtype == MIA_U32 ? 4 : mia_dtype_size(src.dtype);      // (packed codes: mia_dtype_size knows the float types only)
    if (src.ndim != 2 || src.shape[0] != (int64_t)heads * dh || (src.dtype != MIA_F32 && src.dtype != MIA_F16 && src.dtype != MIA_BF16 && src.dtype != MIA_U32)) { alias(src, name); return; }   // the loader names what is wrong
    const size_t row = (size_t)src.shape[1] * es;
    bufs.emplace_back((size_t)heads * dh * row);
    char* dst = bufs.back().data();
    const char* s = (const char*)src.data;
    for (int h = 0; h < heads; ++h)
      for (int i = 0; i < dh / 2; ++i) {
        memcpy(dst + ((size_t)h * dh + i) * row, s + ((size_t)h * dh + 2 * i) * row, row);
        memcpy(dst + ((size_t)h * dh + i + dh / 2) * row, s + ((size_t)h * dh + 2 * i + 1) * row, row);
      }
    names.push_back(name);
    mia_tensor_view v = src; v.name = names.back().c_str(); v.data = dst;
    views.push_back(v);
  }
};

struct Stack { const char* prefix; int hidden, inter, layers, heads, kv_heads, head_dim, max_ctx; float eps, theta; };

// head: the handle's tied embedding / head [V][hidden] fp32.  The backbone's is codebook0_head, which the frame uses through the handle.  The
// decoder's (audio_head[0] transposed) is only there because the loader asks for one: the frame reads its K - 1 heads from mia_marvis::head
mia_lm* mv_load_stack(mia_ctx* ctx, const mia_marvis_config& c, const Stack& sk, const TensorLoader& L, const std::vector<float>& head, int dtype) {
  StackViews sv;
  const std::string p = sk.prefix;
  const char* parts[] = {".self_attn.v_proj.weight", ".self_attn.o_proj.weight", ".mlp.gate_proj.weight", ".mlp.up_proj.weight", ".mlp.down_proj.weight",
                         ".input_layernorm.weight", ".post_attention_layernorm.weight"};
  for (int l = 0; l < sk.layers; ++l) {
    const std::string src = p + ".layers." + std::to_string(l), dst = "model.layers." + std::to_string(l);
    if (const mia_tensor_view* v = L.find(src + ".self_attn.q_proj.weight")) sv.permuted(*v, dst + ".self_attn.q_proj.weight", sk.heads, sk.head_dim);
    if (const mia_tensor_view* v = L.find(src + ".self_attn.k_proj.weight")) sv.permuted(*v, dst + ".self_attn.k_proj.weight", sk.kv_heads, sk.head_dim);
    for (const char* part : parts) if (const mia_tensor_view* v = L.find(src + part)) sv.alias(*v, dst + part);
  }
  if (const mia_tensor_view* v = L.find(p + ".norm.weight")) sv.alias(*v, "model.norm.weight");
  mia_tensor_view hv{};
  hv.dtype = MIA_F32; hv.ndim = 2; hv.shape[0] = c.audio_vocab; hv.shape[1] = sk.hidden; hv.data = head.data();
  sv.alias(hv, "model.embed_tokens.weight");
  mia_lm_config lc{};
  lc.vocab = c.audio_vocab; lc.hidden = sk.hidden; lc.inter = sk.inter; lc.n_layers = sk.layers; lc.n_heads = sk.heads; lc.n_kv_heads = sk.kv_heads;
  lc.head_dim = sk.head_dim; lc.max_ctx = sk.max_ctx; lc.rms_eps = sk.eps; lc.rope_theta = sk.theta; lc.rope_llama3 = 0; lc.rope_factor = 1.f; lc.rope_low = 1.f;
  lc.rope_high = 4.f; lc.rope_old_ctx = 8192; lc.qkv_bias = 0; lc.tie_embeddings = 1;
  mia_lm* m = mia_lm_load(ctx, &lc, sv.views.data(), (int)sv.views.size(), dtype);
  if (!m) {        // the loader's message names the tensor under its own key: put the stack's prefix back
    size_t at;
    while ((at = ctx->err.find("'model.")) != std::string::npos) ctx->err.replace(at, 7, "'" + p + ".");
    return nullptr;
  }
  const std::vector<float> th = mv_inv_freq(sk.head_dim, sk.theta, c);
  if (hipMemcpy(m->inv_freq, th.data(), th.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { ctx->err = "marvis_load: inv_freq upload failed"; mia_lm_free(m); return nullptr; }
  return m;
}

void mv_drop_graph(mia_marvis* mv) { if (mv->graph) { (void)hipGraphExecDestroy(mv->graph); mv->graph = nullptr; } }

// the per-sequence buffers for B sequences
int mv_alloc_state(mia_marvis* mv, int B) {
  const mia_marvis_config& c = mv->cfg;
  for (void* p : mv->state_allocs) (void)hipFree(p);
  mv->state_allocs.clear();
  mv_drop_graph(mv);
  bool ok = true;
  auto dev = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, bytes + 64) != hipSuccess || hipMemset(p, 0, bytes) != hipSuccess) { ok = false; return nullptr; }
    mv->state_allocs.push_back(p);
    return p;
  };
  const size_t K = c.n_codebooks, W = K + 1, rows = (size_t)B * c.max_ctx;
  mv->st = (MvState*)dev(sizeof(MvState) * B);
  mv->frame = (int32_t*)dev(B * K * 4); mv->forced = (int32_t*)dev(B * K * 4);
  mv->frames_out = (int32_t*)dev(rows * K * 4); mv->uniforms = (float*)dev(rows * K * 4);
  mv->logits = (float*)dev(B * K * c.audio_vocab * 4); mv->a16 = (uint16_t*)dev((size_t)B * c.bb_hidden * 2);
  mv->rows = (int32_t*)dev(2 * rows * W * 4); mv->rowmap = (int2*)dev(rows * sizeof(int2));
  mv->B_cap = B;
  return ok ? 0 : -1;
}

// one generateFrame for sequences 0 .. nb-1, each behind the row at its backbone position (its embedding is in bb->embeds)
int mv_enqueue_frame(mia_marvis* mv, int nb, int cb, float temperature, float top_p, bool forced) {
  mia_lm* bb = mv->bb; mia_lm* dec = mv->dec;
  hipStream_t s = mv->ctx->stream;
  const mia_marvis_config& c = mv->cfg;
  const int V = c.audio_vocab, D = c.bb_hidden, Dd = c.dec_hidden, K = c.n_codebooks;
  const int64_t ld_lg = (int64_t)K * V, ld_de = (int64_t)dec->cfg.max_ctx * Dd;      // rows of the logit record / of the decoder's embedding rows, per sequence
  auto sample = [&](int i) {
    MvSampleArgs a{};
    a.ld_logits = ld_lg; a.ld_uniforms = (int64_t)c.max_ctx * K; a.ld_ids = K;
    a.logits = mv->logits + (size_t)i * V; a.V = V; a.temperature = temperature; a.top_p = top_p;
    a.uniforms = mv->uniforms; a.n_uniforms = c.max_ctx * K; a.st = mv->st; a.out = mv->frame + i; a.forced = forced ? mv->forced + i : nullptr;
    if (i + 1 < cb) { a.emb = (const uint16_t*)mv->audio_emb + (size_t)i * V * D; a.emb_out = mv->a16; a.D = D; }
    mv_launch_sample(s, a, nb);
  };
  if (lm_enqueue_layers(bb, nb)) return -1;
  if (lm_enqueue_linear_of_last(bb, nb, bb->lm_head, bb->lm_head_f, nullptr, &bb->q_head, mv->logits, ld_lg, V)) return -1;      // codebook0_head(lastH)
  sample(0);
  if (cb > 1) {
    // decoder row 0 = projection(lastH), from the backbone's last carried activation exactly as the head reads it
    if (lm_enqueue_linear_of_last(bb, nb, mv->proj, mv->proj_f, nullptr, &mv->q_proj, dec->embeds, ld_de, Dd)) return -1;
    if (lm_enqueue_layers(dec, nb)) return -1;
    lm_enqueue_advance(dec, nb);
    for (int i = 1; i < cb; ++i) {       // row i = projection(audio_emb(i - 1, c_{i-1})) -> audio_head[i - 1] -> c_i
      SkinnyArgs a{mv->a16, D, (const uint16_t*)mv->proj_f, nullptr, dec->embeds + (size_t)i * Dd, ld_de, nullptr, nullptr, nullptr, nb, Dd, D, 1, MIA_ACT_NONE, 0, 0, 0};
      a.w_frag = 1;
      if (bb->q4 && mv->q_proj.wfrag) { if (skinny_gemm_q_launch(a, mv->q_proj.wfrag, mv->q_proj.stfrag, mv->q_bits, SK_OUTF32, mv->dtype, s, mv->B_cap)) return -1; }
      else if (skinny_gemm_launch(a, SK_OUTF32, mv->dtype, s)) return -1;
      if (lm_enqueue_layers(dec, nb)) return -1;
      if (lm_enqueue_linear_of_last(dec, nb, mv->head[i - 1], mv->head_f[i - 1], nullptr, nullptr, mv->logits + (size_t)i * V, ld_lg, V)) return -1;
      lm_enqueue_advance(dec, nb);
      sample(i);
    }
  }
  lm_enqueue_advance(bb, nb);
  MvFrameEndArgs e{mv->st, bb->state, dec->state, mv->frame, K, cb, mv->frames_out, c.max_ctx, mv->audio_emb, V, D, bb->embeds, c.max_ctx};
  mv_launch_frame_end(s, mv->dtype, e, nb);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// launch one frame: the captured graph (re-captured when its key changes) or, with debug bit 0, the kernels directly
int mv_launch_frame(mia_marvis* mv, int nb, int cb, float temperature, float top_p, bool forced) {
  mia_ctx* ctx = mv->ctx;
  if (mv->debug_flags & 1) {
    if (mv_enqueue_frame(mv, nb, cb, temperature, top_p, forced)) return mia_fail(ctx, MIA_ERR_DEVICE, "marvis: frame launch failed");
    return MIA_OK;
  }
  if (!(mv->graph && mv->g_cb == cb && mv->g_nb == nb && mv->g_temp == temperature && mv->g_top_p == top_p && mv->g_forced == forced)) {
    mv_drop_graph(mv);
    hipGraph_t g = nullptr;
    MIA_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    const int erc = mv_enqueue_frame(mv, nb, cb, temperature, top_p, forced);
    const hipError_t ce = hipStreamEndCapture(ctx->stream, &g);
    if (erc != 0 || ce != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); return mia_fail(ctx, MIA_ERR_DEVICE, "marvis: frame graph capture failed"); }
    const hipError_t ie = hipGraphInstantiate(&mv->graph, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ie != hipSuccess) { mv->graph = nullptr; return mia_fail(ctx, MIA_ERR_DEVICE, "marvis: hipGraphInstantiate failed"); }
    mv->g_cb = cb; mv->g_nb = nb; mv->g_temp = temperature; mv->g_top_p = top_p; mv->g_forced = forced;
  }
  MIA_HIP(ctx, hipGraphLaunch(mv->graph, ctx->stream));
  return MIA_OK;
}

// what every entry point checks of its rows before anything is launched
int mv_check_rows(mia_marvis* mv, const char* who, const int32_t* tokens, const int32_t* mask, int64_t T) {
  const mia_marvis_config& c = mv->cfg;
  const int W = c.n_codebooks + 1;
  for (int64_t r = 0; r < T; ++r)
    for (int k = 0; k < W; ++k) {
      const int id = tokens[r * W + k], mk = mask[r * W + k];
      MIA_CHECK_ARG(mv->ctx, mk == 0 || mk == 1, "%s: mask[%lld][%d] = %d is not 0 or 1", who, (long long)r, k, mk);
      MIA_CHECK_ARG(mv->ctx, id >= 0 && id < (k < c.n_codebooks ? c.audio_vocab : c.text_vocab), "%s: id %d at row %lld, column %d is outside its table", who, id, (long long)r, k);
    }
  return MIA_OK;
}

int mv_check_sampler(mia_marvis* mv, const char* who, int max_codebooks, float temperature, float top_p) {
  MIA_CHECK_ARG(mv->ctx, max_codebooks >= 1, "%s: max_codebooks must be at least 1 (got %d)", who, max_codebooks);
  MIA_CHECK_ARG(mv->ctx, std::isfinite(temperature) && temperature > 0.f, "%s: temperature must be finite and positive", who);
  MIA_CHECK_ARG(mv->ctx, std::isfinite(top_p) && top_p > 0.f && top_p <= 1.f, "%s: top_p must be in (0, 1]", who);
  return MIA_OK;
}

// append checked rows -- all rows back to back, offsets [n_seq + 1], sequence b's first row at position pos0[b]: embed all of them, run all
// but each sequence's last through the backbone (K/V only); the last is the next frame's row.  A failure past the first launch leaves
// device positions the host cannot know: the caller resets the handle
int mv_feed_rows(mia_marvis* mv, HostIo& io, const int32_t* tokens, const int32_t* mask, const int32_t* offsets, const int* pos0, int n_seq) {
  mia_ctx* ctx = mv->ctx;
  mia_lm* bb = mv->bb;
  const mia_marvis_config& c = mv->cfg;
  const int W = c.n_codebooks + 1, T = offsets[n_seq];
  const size_t bytes = (size_t)T * W * 4;
  std::vector<int2> map(T), rows;
  std::vector<int> set_pos(n_seq, -1);
  for (int b = 0; b < n_seq; ++b) {
    const int n = offsets[b + 1] - offsets[b];
    for (int i = 0; i < n; ++i) { map[offsets[b] + i] = make_int2(b, pos0[b] + i); if (i + 1 < n) rows.push_back(make_int2(b, pos0[b] + i)); }
    if (n > 1) set_pos[b] = pos0[b] + n - 1;
  }
  const int32_t* d_ids = io.in(tokens, mv->rows, bytes);
  const int32_t* d_mask = io.in(mask, mv->rows + (size_t)mv->B_cap * c.max_ctx * W, bytes);
  const int2* d_map = io.table(map.data(), mv->rowmap, (size_t)T * sizeof(int2));
  mv_launch_embed_rows(ctx->stream, mv->dtype, d_ids, d_mask, d_map, T, c.n_codebooks, c.audio_vocab, c.text_vocab, mv->audio_emb, mv->text_emb, bb->embeds, c.max_ctx, c.bb_hidden, bb->state);
  MIA_HIP(ctx, hipGetLastError());
  if (rows.empty()) return MIA_OK;
  if (lm_prefill_supported(bb)) return lm_prefill_rows(bb, rows, set_pos);
  if (n_seq != 1) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "marvis: sequences side by side need the batched prompt pass (hidden, heads * head_dim and inter multiples of 64; debug bit 1 off)");
  for (size_t i = 0; i < rows.size(); ++i) {          // row by row through the step (debug bit 1, or shapes the prompt pass does not take)
    if (lm_enqueue_layers(bb, 1)) return mia_fail(ctx, MIA_ERR_DEVICE, "marvis: backbone step launch failed");
    lm_enqueue_advance(bb, 1);
  }
  return MIA_OK;
}

// the call's starting records: frames and uniform cursors at 0, `finished` as given (sequence 0; the others not finished), stacks thawed to match
void mv_put_state(mia_marvis* mv, HostIo& io, int nb, bool finished0) {
  std::vector<MvState> st(nb, MvState{0, 0, 0, 0});
  st[0].finished = finished0 ? 1 : 0;
  const int frozen0 = finished0 ? 1 : 0, zero = 0;
  hipStream_t s = mv->ctx->stream;
  io.check(hipMemcpyAsync(mv->st, st.data(), sizeof(MvState) * nb, hipMemcpyHostToDevice, s));
  for (int b = 0; b < nb; ++b)
    for (mia_lm* m : {mv->bb, mv->dec}) io.check(hipMemcpyAsync(&m->state[b].frozen, b == 0 ? &frozen0 : &zero, 4, hipMemcpyHostToDevice, s));
  io.check(hipStreamSynchronize(s));      // the sources are this call's stack
}

int mv_reset(mia_marvis* mv) {
  mia_ctx* ctx = mv->ctx;
  const int B = mv->B_cap;
  std::vector<LmState> zero(B), dst(B);
  for (LmState& d : dst) d.n_embeds = mv->dec->cfg.max_ctx;      // every decoder position is an embedding row
  MIA_HIP(ctx, hipMemcpyAsync(mv->bb->state, zero.data(), sizeof(LmState) * B, hipMemcpyHostToDevice, ctx->stream));
  MIA_HIP(ctx, hipMemcpyAsync(mv->dec->state, dst.data(), sizeof(LmState) * B, hipMemcpyHostToDevice, ctx->stream));
  MIA_HIP(ctx, hipMemsetAsync(mv->st, 0, sizeof(MvState) * B, ctx->stream));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mv->pos = 0; mv->started = false; mv->finished = false; mv->last_cb = 0;
  return MIA_OK;
}

// a launch failed after others were queued: device positions and the host mirror may disagree, so the handle goes back to its reset state
int mv_fail_reset(mia_marvis* mv, int rc) {
  const std::string msg = mv->ctx->err;
  (void)hipStreamSynchronize(mv->ctx->stream);
  (void)mv_reset(mv);
  mv->ctx->err = msg + " (the handle has been reset)";
  return rc;
}

}  // namespace

extern "C" void mia_marvis_free(mia_marvis* mv) {
  if (!mv) return;
  (void)hipSetDevice(mv->ctx->device);
  (void)hipStreamSynchronize(mv->ctx->stream);
  mv_drop_graph(mv);
  if (mv->bb) mia_lm_free(mv->bb);
  if (mv->dec) mia_lm_free(mv->dec);
  for (void* p : mv->allocs) (void)hipFree(p);
  for (void* p : mv->state_allocs) (void)hipFree(p);
  delete mv;
}

extern "C" int mia_marvis_reset(mia_marvis* mv) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_HIP(mv->ctx, hipSetDevice(mv->ctx->device));
  return mv_reset(mv);
}

// capacity for max_batch sentences side by side: every per-sequence buffer of the handle and of its two stacks (K/V caches included) is
// re-allocated, the frame graph dropped and every sequence reset
extern "C" int mia_marvis_set_batch(mia_marvis* mv, int max_batch) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = mv->ctx;
  MIA_CHECK_ARG(ctx, max_batch >= 1 && max_batch <= 32, "marvis_set_batch: max_batch must be in 1..32 (got %d)", max_batch);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (lm_alloc_state(mv->bb, max_batch) || lm_alloc_state(mv->dec, max_batch) || mv_alloc_state(mv, max_batch)) {
    (void)lm_alloc_state(mv->bb, 1); (void)lm_alloc_state(mv->dec, 1); (void)mv_alloc_state(mv, 1); (void)mv_reset(mv);
    return mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "marvis_set_batch: hipMalloc failed (state for %d sequences); the capacity is 1", max_batch);
  }
  return mv_reset(mv);
}

extern "C" mia_marvis* mia_marvis_load(mia_ctx* ctx, const mia_marvis_config* cfg, const mia_tensor_view* tensors, int n_tensors, int dtype, int32_t* status) {
  if (status) *status = MIA_ERR_INVALID_ARGUMENT;
  if (!ctx) return nullptr;
  mia_marvis* mv = nullptr;
  auto fail = [&](int code, const std::string& msg) -> mia_marvis* {
    if (status) *status = code;
    if (mv) mia_marvis_free(mv);
    ctx->err = "marvis_load: " + msg;
    return nullptr;
  };
  if (!cfg || !tensors || n_tensors <= 0) return fail(MIA_ERR_INVALID_ARGUMENT, "null arguments");
  if (dtype != MIA_BF16 && dtype != MIA_F16) return fail(MIA_ERR_INVALID_ARGUMENT, "dtype must be MIA_BF16 or MIA_F16");
  const mia_marvis_config& c = *cfg;
  if (c.attention_bias || c.mlp_bias) return fail(MIA_ERR_UNSUPPORTED, "attention_bias / mlp_bias checkpoints are not supported");
  if (c.audio_vocab > MV_MAX_VOCAB) return fail(MIA_ERR_UNSUPPORTED, "audio_vocab " + std::to_string(c.audio_vocab) + " exceeds the frame sampler's " + std::to_string(MV_MAX_VOCAB));
  if (c.audio_vocab < 2 || c.text_vocab < 1 || c.n_codebooks < 2 || c.n_codebooks > MV_MAX_CODEBOOKS || c.max_ctx < 2 || c.max_ctx > 8192)
    return fail(MIA_ERR_INVALID_ARGUMENT, "audio_vocab >= 2, text_vocab >= 1, n_codebooks in 2..32 and max_ctx in 2..8192 required");
  if (c.bb_hidden <= 0 || c.dec_hidden <= 0 || c.bb_hidden % 32 || c.dec_hidden % 32) return fail(MIA_ERR_INVALID_ARGUMENT, "hidden sizes must be positive multiples of 32");
  if (c.rope_llama3 && !(c.rope_factor > 0.f && c.rope_high != c.rope_low && c.rope_low > 0.f && c.rope_high > 0.f && c.rope_old_ctx > 0.f))
    return fail(MIA_ERR_INVALID_ARGUMENT, "rope scaling constants must be positive, with high_freq_factor != low_freq_factor");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(MIA_ERR_DEVICE, "hipSetDevice failed");
  if (mv_sampler_init()) return fail(MIA_ERR_DEVICE, "the frame sampler's LDS limit could not be set");
  mv = new mia_marvis(); mv->ctx = ctx; mv->cfg = c; mv->dtype = dtype;
  TensorLoader L; L.allocs = &mv->allocs;
  L.index(tensors, n_tensors);
  const int K = c.n_codebooks, V = c.audio_vocab, D = c.bb_hidden, Dd = c.dec_hidden;
  std::vector<float> t, head0, c0;
  if (L.read("text_embeddings.weight", t, {c.text_vocab, D})) mv->text_emb = L.up16(t, dtype);
  if (L.read("audio_embeddings.weight", t, {(int64_t)K * V, D})) mv->audio_emb = L.up16(t, dtype);
  if (L.read("projection.weight", t, {Dd, D})) mv->proj = L.up16(t, dtype);
  L.read("codebook0_head.weight", c0, {V, D});
  std::vector<std::vector<float>> heads(K - 1);
  if (L.read("audio_head", t, {K - 1, Dd, V}))        // applied as x @ W: stored transposed relative to a Linear
    for (int h = 0; h < K - 1; ++h) {
      heads[h].resize((size_t)V * Dd);
      for (int d = 0; d < Dd; ++d) for (int v = 0; v < V; ++v) heads[h][(size_t)v * Dd + d] = t[((size_t)h * Dd + d) * V + v];
      mv->head.push_back(L.up16(heads[h], dtype));
    }
  if (!L.err.empty()) return fail(L.code, L.err);
  const Stack sb{"backbone", D, c.bb_inter, c.bb_layers, c.bb_heads, c.bb_kv_heads, c.bb_head_dim, c.max_ctx, c.bb_rms_eps, c.bb_rope_theta};
  const Stack sd{"decoder", Dd, c.dec_inter, c.dec_layers, c.dec_heads, c.dec_kv_heads, c.dec_head_dim, std::max(K, 8), c.dec_rms_eps, c.dec_rope_theta};
  if (!(mv->bb = mv_load_stack(ctx, c, sb, L, c0, dtype))) { const std::string e = ctx->err; return fail(MIA_ERR_INVALID_ARGUMENT, e); }
  if (!(mv->dec = mv_load_stack(ctx, c, sd, L, heads[0], dtype))) { const std::string e = ctx->err; return fail(MIA_ERR_INVALID_ARGUMENT, e); }
  if (mia_lm_set_prompt_attention(mv->bb, 1) != MIA_OK) return fail(MIA_ERR_DEVICE, "prompt attention mode refused");      // the voice prompt is several hundred rows: the tiled prompt attention (lm_prefill_attn.hip)
  bool ok = dec_wfrag_copy(mv->proj, Dd, D, mv->allocs, ctx->stream, &mv->proj_f);
  mv->head_f.assign(K - 1, nullptr);
  for (int h = 0; h < K - 1 && ok; ++h) ok = dec_wfrag_copy(mv->head[h], V, Dd, mv->allocs, ctx->stream, &mv->head_f[h]);
  if (!ok) return fail(MIA_ERR_OUT_OF_MEMORY, "fragment-order repack of the projection / heads failed");
  if (mv_alloc_state(mv, 1)) return fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed (state buffers)");
  if (mv_reset(mv) != MIA_OK || hipDeviceSynchronize() != hipSuccess) return fail(MIA_ERR_DEVICE, "device error during upload");
  if (status) *status = MIA_OK;
  return mv;
}

namespace {

// one stack's packed tensors under the LM attach's names; q_proj / k_proj: the loader's row permutation on codes, scales and biases alike
void mv_packed_views(const Stack& sk, const TensorLoader& L, StackViews& sv) {
  const std::string p = sk.prefix;
  const char* lin[] = {".self_attn.v_proj", ".self_attn.o_proj", ".mlp.gate_proj", ".mlp.up_proj", ".mlp.down_proj"};
  const char* part[] = {".weight", ".scales", ".biases"};
  for (int l = 0; l < sk.layers; ++l) {
    const std::string src = p + ".layers." + std::to_string(l), dst = "model.layers." + std::to_string(l);
    for (const char* t : part) {
      if (const mia_tensor_view* v = L.find(src + ".self_attn.q_proj" + t)) sv.permuted(*v, dst + ".self_attn.q_proj" + t, sk.heads, sk.head_dim);
      if (const mia_tensor_view* v = L.find(src + ".self_attn.k_proj" + t)) sv.permuted(*v, dst + ".self_attn.k_proj" + t, sk.kv_heads, sk.head_dim);
      for (const char* n : lin) if (const mia_tensor_view* v = L.find(src + n + t)) sv.alias(*v, dst + n + t);
    }
  }
}

// the LM attach names a tensor under its own key: put the stack's prefix back (as mv_load_stack does)
void mv_rename_error(mia_ctx* ctx, const char* prefix) {
  size_t at;
  while ((at = ctx->err.find("'model.embed_tokens")) != std::string::npos) ctx->err.replace(at, 19, "'codebook0_head");
  while ((at = ctx->err.find("'model.")) != std::string::npos) ctx->err.replace(at, 7, std::string("'") + prefix + ".");
}

}  // namespace

extern "C" int mia_marvis_attach_quantized(mia_marvis* mv, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = mv->ctx;
  const mia_marvis_config& c = mv->cfg;
  MIA_CHECK_ARG(ctx, tensors && n_tensors > 0 && group_size == 64 && (bits == 4 || bits == 6 || bits == 8), "marvis_attach_quantized: tensors required, group size 64, 4, 6 or 8 bits");
  MIA_CHECK_ARG(ctx, mv->q_bits == 0, "marvis_attach_quantized: packed weights are already attached to this handle (load a fresh handle to replace them)");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  TensorLoader L;
  L.index(tensors, n_tensors);
  const Stack sb{"backbone", c.bb_hidden, c.bb_inter, c.bb_layers, c.bb_heads, c.bb_kv_heads, c.bb_head_dim, 0, 0.f, 0.f};
  const Stack sd{"decoder", c.dec_hidden, c.dec_inter, c.dec_layers, c.dec_heads, c.dec_kv_heads, c.dec_head_dim, 0, 0.f, 0.f};
  StackViews vb, vd;
  mv_packed_views(sb, L, vb);
  mv_packed_views(sd, L, vd);
  // codebook0_head is the backbone handle's tied head: the LM attach packs it when its `.scales` is there
  for (const char* t : {".weight", ".scales", ".biases"})
    if (const mia_tensor_view* v = L.find(std::string("codebook0_head") + t)) vb.alias(*v, std::string("model.embed_tokens") + t);
  LmPacked pb, pd;
  if (vb.views.empty() || vd.views.empty()) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "marvis_attach_quantized: no packed tensor of the %s stack in the list", vb.views.empty() ? "backbone" : "decoder");
  if (const int rc = lm_attach_prepare(mv->bb, vb.views.data(), (int)vb.views.size(), group_size, bits, "marvis_attach_quantized", pb)) { mv_rename_error(ctx, "backbone"); return rc; }
  if (const int rc = lm_attach_prepare(mv->dec, vd.views.data(), (int)vd.views.size(), group_size, bits, "marvis_attach_quantized", pd)) {
    lm_attach_discard(pb);
    mv_rename_error(ctx, "decoder");
    return rc;
  }
  // the projection [d_dec][D]: K = the backbone's hidden size, which the backbone's attach has checked against the 128-input block
  std::vector<void*> fresh;
  TensorLoader P; P.allocs = &fresh;
  P.index(tensors, n_tensors);
  Q4Src src{};
  int sdt = -1;
  Q4W qp;
  std::vector<std::pair<int, int>> rows;
  for (int n = 0; n < c.dec_hidden; ++n) rows.push_back({0, n});
  const bool ok = q_find_linear(P, "projection", c.dec_hidden, c.bb_hidden, bits, false, &sdt, src) &&
                  q_upload(P, {src}, rows, c.bb_hidden, bits, sdt, mv->dtype == MIA_F16 ? 1024.0f : 128.0f, &qp.wfrag, &qp.stfrag) &&
                  (hipDeviceSynchronize() == hipSuccess || P.fail(MIA_ERR_DEVICE, "device error during upload"));
  if (!ok) {      // neither stack has been touched yet
    for (void* p : fresh) (void)hipFree(p);
    lm_attach_discard(pb); lm_attach_discard(pd);
    return mia_fail(ctx, P.code, "marvis_attach_quantized: %s", P.err.c_str());
  }
  // everything is in place: nothing below can fail
  lm_attach_commit(mv->bb, pb);
  lm_attach_commit(mv->dec, pd);
  mv->allocs.insert(mv->allocs.end(), fresh.begin(), fresh.end());
  mv->q_proj = qp;
  mv->q_bits = bits;
  mv_drop_graph(mv);            // the captured frame holds the 16-bit launches
  return MIA_OK;
}

// the frame on the packed (1) or the 16-bit (0) weights of a handle that has both
extern "C" int mia_marvis_use_packed(mia_marvis* mv, int on) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(mv->ctx, !on || mv->q_bits != 0, "marvis_use_packed: no packed weights attached (mia_marvis_attach_quantized)");
  if (!on && mv->bb->dense_released) return mia_fail(mv->ctx, MIA_ERR_UNSUPPORTED, "marvis_use_packed: the 16-bit Linears of this handle were released (mia_marvis_release_dense)");
  MIA_HIP(mv->ctx, hipSetDevice(mv->ctx->device));
  MIA_HIP(mv->ctx, hipStreamSynchronize(mv->ctx->stream));
  mv->bb->q4 = mv->dec->q4 = on != 0;
  mv->bb->graph_mode = mv->dec->graph_mode = -1;
  mv_drop_graph(mv);
  return MIA_OK;
}

// the backbone's prompt pass on the packed (1) or the 16-bit (0) weights; the decoder has no prompt pass and the frame graph does not hold
// the prompt pass, so nothing is dropped
extern "C" int mia_marvis_use_packed_prompt(mia_marvis* mv, int on) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(mv->ctx, !on || mv->q_bits != 0, "marvis_use_packed_prompt: no packed weights attached (mia_marvis_attach_quantized)");
  return mia_lm_set_prompt_weights(mv->bb, on ? 1 : 0);
}

// both stacks give up their 16-bit layer Linears (mia_lm_release_dense); the frame and the prompt pass run packed from here on
extern "C" int mia_marvis_release_dense(mia_marvis* mv) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(mv->ctx, mv->q_bits != 0, "marvis_release_dense: no packed weights attached (mia_marvis_attach_quantized)");
  MIA_HIP(mv->ctx, hipSetDevice(mv->ctx->device));
  MIA_HIP(mv->ctx, hipStreamSynchronize(mv->ctx->stream));
  if (const int rc = mia_lm_release_dense(mv->bb)) return rc;
  if (const int rc = mia_lm_release_dense(mv->dec)) return rc;
  mv_drop_graph(mv);            // a frame captured on the 16-bit weights must not be replayed
  return MIA_OK;
}

// test hook: bit 0 launches every frame's kernels directly (no hipGraph), bit 1 walks prompts through the step (no batched prompt pass)
extern "C" int mia_marvis_set_debug(mia_marvis* mv, int flags) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(mv->ctx, flags >= 0 && flags <= 3, "marvis_set_debug: flags must be 0..3 (got %d)", flags);
  mv->debug_flags = flags;
  mv->bb->debug_flags = flags & 2;
  return MIA_OK;
}

extern "C" int mia_marvis_frame(mia_marvis* mv, const int32_t* tokens, const int32_t* mask, int T, int max_codebooks, float temperature, float top_p,
                                const float* uniforms, const int32_t* forced, int32_t* ids_out, float* logits_out) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = mv->ctx;
  const mia_marvis_config& c = mv->cfg;
  MIA_CHECK_ARG(ctx, tokens && mask && uniforms && ids_out, "marvis_frame: tokens, mask, uniforms and ids_out are required");
  MIA_CHECK_ARG(ctx, T >= 1 && (int64_t)mv->pos + T <= c.max_ctx, "marvis_frame: T must be at least 1 and the rows must fit max_ctx %d (%d in the cache, T %d)", c.max_ctx, mv->pos, T);
  if (const int rc = mv_check_sampler(mv, "marvis_frame", max_codebooks, temperature, top_p)) return rc;
  if (const int rc = mv_check_rows(mv, "marvis_frame", tokens, mask, T)) return rc;
  const int cb = std::min(c.n_codebooks, max_codebooks);
  if (forced) for (int i = 0; i < cb; ++i) MIA_CHECK_ARG(ctx, forced[i] >= 0 && forced[i] < c.audio_vocab, "marvis_frame: forced[%d] = %d is outside the audio vocabulary", i, forced[i]);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io = HostIo::host(ctx);
  mv_put_state(mv, io, 1, false);
  io.in(uniforms, mv->uniforms, (size_t)cb * 4);
  if (forced) io.in(forced, mv->forced, (size_t)cb * 4);
  const int32_t offsets[2] = {0, T};
  if (const int rc = mv_feed_rows(mv, io, tokens, mask, offsets, &mv->pos, 1)) return mv_fail_reset(mv, rc);
  if (const int rc = mv_launch_frame(mv, 1, cb, temperature, top_p, forced != nullptr)) return mv_fail_reset(mv, rc);
  MvState st{}; LmState ls{};
  io.fetch(&st, mv->st, sizeof(st));
  io.fetch(&ls, mv->bb->state, sizeof(ls));
  io.fetch(ids_out, mv->frame, (size_t)cb * 4);
  if (logits_out) io.fetch(logits_out, mv->logits, (size_t)cb * c.audio_vocab * 4);
  if (const int rc = io.finish()) return mv_fail_reset(mv, rc);
  mv->pos = ls.pos; mv->started = true; mv->last_cb = cb; mv->finished = st.finished != 0;
  return MIA_OK;
}

extern "C" int mia_marvis_generate(mia_marvis* mv, const int32_t* tokens, const int32_t* mask, int T, int max_codebooks, float temperature, float top_p,
                                   int max_frames, const float* uniforms, int32_t* frames_out, int32_t* n_frames) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = mv->ctx;
  const mia_marvis_config& c = mv->cfg;
  MIA_CHECK_ARG(ctx, uniforms && frames_out && n_frames && T >= 0 && (T == 0 || (tokens && mask)), "marvis_generate: null pointer or negative T");
  MIA_CHECK_ARG(ctx, max_frames >= 1, "marvis_generate: max_frames must be at least 1 (got %d)", max_frames);
  MIA_CHECK_ARG(ctx, (int64_t)mv->pos + T + max_frames <= c.max_ctx, "marvis_generate: %d rows in the cache + T %d + max_frames %d exceed max_ctx %d", mv->pos, T, max_frames, c.max_ctx);
  if (const int rc = mv_check_sampler(mv, "marvis_generate", max_codebooks, temperature, top_p)) return rc;
  const int cb = std::min(c.n_codebooks, max_codebooks), K = c.n_codebooks;
  if (T == 0) {
    MIA_CHECK_ARG(ctx, mv->started, "marvis_generate: T = 0 continues a sentence, and this handle has not drawn a frame since its reset");
    MIA_CHECK_ARG(ctx, cb == mv->last_cb, "marvis_generate: a continuation must keep the codebook count (%d, got %d)", mv->last_cb, cb);
  } else if (const int rc = mv_check_rows(mv, "marvis_generate", tokens, mask, T)) return rc;
  *n_frames = 0;
  if (T == 0 && mv->finished) return MIA_OK;          // finished until mia_marvis_reset
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io = HostIo::host(ctx);
  mv_put_state(mv, io, 1, false);
  io.in(uniforms, mv->uniforms, (size_t)max_frames * cb * 4);
  const int32_t offsets[2] = {0, T};
  if (T > 0) { if (const int rc = mv_feed_rows(mv, io, tokens, mask, offsets, &mv->pos, 1)) return mv_fail_reset(mv, rc); }
  MvState st{}; LmState ls{};
  for (int f = 0; f < max_frames; ++f) {
    if (const int rc = mv_launch_frame(mv, 1, cb, temperature, top_p, false)) return mv_fail_reset(mv, rc);
    if ((f + 1) % 16 == 0 && f + 1 < max_frames) {      // the finished flag, every 16th frame
      io.fetch(&st, mv->st, sizeof(st));
      if (const int rc = io.finish()) return mv_fail_reset(mv, rc);
      if (st.finished) break;
    }
  }
  io.fetch(&st, mv->st, sizeof(st));
  io.fetch(&ls, mv->bb->state, sizeof(ls));
  if (const int rc = io.finish()) return mv_fail_reset(mv, rc);
  mv->pos = ls.pos; mv->started = true; mv->last_cb = cb; mv->finished = st.finished != 0;      // (a frozen sequence's position stopped at its last real row)
  const int n = std::min(st.n_frames, max_frames);
  std::vector<int32_t> rec((size_t)n * K);
  io.fetch(rec.data(), mv->frames_out, rec.size() * 4);
  if (const int rc = io.finish()) return rc;
  for (int f = 0; f < n; ++f) memcpy(frames_out + (size_t)f * cb, rec.data() + (size_t)f * K, (size_t)cb * 4);
  *n_frames = n;
  return MIA_OK;
}

extern "C" int mia_marvis_generate_batch(mia_marvis* mv, const int32_t* tokens, const int32_t* mask, const int32_t* prompt_offsets, int n_seq, int max_codebooks,
                                         float temperature, float top_p, int max_frames, const float* uniforms, int32_t* frames_out, int32_t* n_frames) {
  if (!mv) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = mv->ctx;
  const mia_marvis_config& c = mv->cfg;
  MIA_CHECK_ARG(ctx, tokens && mask && prompt_offsets && uniforms && frames_out && n_frames, "marvis_generate_batch: null pointer");
  MIA_CHECK_ARG(ctx, n_seq >= 1 && n_seq <= mv->B_cap, "marvis_generate_batch: n_seq %d is outside the handle's capacity %d (mia_marvis_set_batch)", n_seq, mv->B_cap);
  MIA_CHECK_ARG(ctx, max_frames >= 1, "marvis_generate_batch: max_frames must be at least 1 (got %d)", max_frames);
  MIA_CHECK_ARG(ctx, prompt_offsets[0] == 0, "marvis_generate_batch: prompt_offsets[0] must be 0");
  for (int b = 0; b < n_seq; ++b) {
    const int64_t T = (int64_t)prompt_offsets[b + 1] - prompt_offsets[b];
    MIA_CHECK_ARG(ctx, T >= 1 && T + max_frames <= c.max_ctx, "marvis_generate_batch: prompt %d has %lld rows; 1 <= rows and rows + max_frames %d <= max_ctx %d required", b, (long long)T, max_frames, c.max_ctx);
  }
  if (const int rc = mv_check_sampler(mv, "marvis_generate_batch", max_codebooks, temperature, top_p)) return rc;
  if (const int rc = mv_check_rows(mv, "marvis_generate_batch", tokens, mask, prompt_offsets[n_seq])) return rc;
  MIA_CHECK_ARG(ctx, !(mv->debug_flags & 2) || n_seq == 1, "marvis_generate_batch: debug bit 1 (no batched prompt pass) takes one sequence only");
  const int cb = std::min(c.n_codebooks, max_codebooks), K = c.n_codebooks;
  for (int b = 0; b < n_seq; ++b) n_frames[b] = 0;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  if (const int rc = mv_reset(mv)) return rc;          // every sentence starts on empty caches
  HostIo io = HostIo::host(ctx);
  const size_t urow = (size_t)max_frames * cb * 4;
  io.check(hipMemcpy2DAsync(mv->uniforms, (size_t)c.max_ctx * K * 4, uniforms, urow, urow, n_seq, io.from_caller(), ctx->stream));
  const std::vector<int> pos0(n_seq, 0);
  if (const int rc = mv_feed_rows(mv, io, tokens, mask, prompt_offsets, pos0.data(), n_seq)) return mv_fail_reset(mv, rc);
  std::vector<MvState> st(n_seq);
  auto all_finished = [&] { for (const MvState& x : st) if (!x.finished) return false; return true; };
  for (int f = 0; f < max_frames; ++f) {
    if (const int rc = mv_launch_frame(mv, n_seq, cb, temperature, top_p, false)) return mv_fail_reset(mv, rc);
    if ((f + 1) % 16 == 0 && f + 1 < max_frames) {      // the finished flags, every 16th frame
      io.fetch(st.data(), mv->st, sizeof(MvState) * n_seq);
      if (const int rc = io.finish()) return mv_fail_reset(mv, rc);
      if (all_finished()) break;
    }
  }
  io.fetch(st.data(), mv->st, sizeof(MvState) * n_seq);
  if (const int rc = io.finish()) return mv_fail_reset(mv, rc);
  std::vector<int32_t> rec((size_t)max_frames * K);
  for (int b = 0; b < n_seq; ++b) {
    const int n = std::min(st[b].n_frames, max_frames);
    io.fetch(rec.data(), mv->frames_out + (size_t)b * c.max_ctx * K, (size_t)n * K * 4);
    if (const int rc = io.finish()) return mv_fail_reset(mv, rc);
    for (int f = 0; f < n; ++f) memcpy(frames_out + ((size_t)b * max_frames + f) * cb, rec.data() + (size_t)f * K, (size_t)cb * 4);
    n_frames[b] = n;
  }
  return mv_reset(mv);          // the single-sequence entry points find a fresh handle
}

// one draw of the frame sampler on caller-provided logits (host pointers)
extern "C" int mia_sample_top_p_ascending(mia_ctx* ctx, const float* logits, int V, float temperature, float top_p, float uniform, int32_t* out,
                                          int32_t* kept_ids, int32_t* n_kept) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, logits && out && V > 0, "sample_top_p_ascending: logits, out and V > 0 required");
  MIA_CHECK_ARG(ctx, std::isfinite(temperature) && temperature > 0.f, "sample_top_p_ascending: temperature must be finite and positive");
  MIA_CHECK_ARG(ctx, std::isfinite(top_p) && top_p > 0.f && top_p <= 1.f, "sample_top_p_ascending: top_p must be in (0, 1]");
  if (V > MV_MAX_VOCAB) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "sample_top_p_ascending: V %d exceeds %d", V, MV_MAX_VOCAB);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  if (mv_sampler_init()) return mia_fail(ctx, MIA_ERR_DEVICE, "sample_top_p_ascending: the kernel's LDS limit could not be set");
  Carve cv;
  const size_t o_logits = cv.add((size_t)V * 4), o_u = cv.add(4), o_out = cv.add(8), o_kept = cv.add((size_t)V * 4);
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  HostIo io = HostIo::host(ctx);
  MvSampleArgs a{};
  a.logits = io.in(logits, ws + o_logits, (size_t)V * 4); a.V = V; a.temperature = temperature; a.top_p = top_p;
  a.uniforms = io.table(&uniform, ws + o_u, 4); a.n_uniforms = 1;
  a.out = (int32_t*)(ws + o_out); a.n_kept = a.out + 1; a.kept_ids = (int32_t*)(ws + o_kept);
  mv_launch_sample(ctx->stream, a, 1);
  MIA_HIP(ctx, hipGetLastError());
  int32_t res[2] = {0, 0};
  io.fetch(res, a.out, 8);
  if (const int rc = io.finish()) return rc;
  *out = res[0];
  if (n_kept) *n_kept = res[1];
  if (kept_ids && res[1] > 0) { io.fetch(kept_ids, a.kept_ids, (size_t)std::min(res[1], V) * 4); return io.finish(); }
  return MIA_OK;
}
