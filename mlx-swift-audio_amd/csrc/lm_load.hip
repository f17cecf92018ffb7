// lm_load.hip -- the LM handle's life cycle: mia_lm_load (16-bit upload of a Llama-3 / Qwen2 / Qwen3 checkpoint, fused q|k|v and gate|up
// matrices, fragment-order copies for the decode step), the per-sequence state buffers, mia_lm_free, and the MLX-affine 4- / 8-bit
// packed weights of the step (mia_lm_attach_quantized: host repack into the layout skinny_quant.hip reads).
#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "lm.h"
#include "quant_repack.h"
#include "skinny.h"

namespace {

// the LM's tensors on top of the shared loader: what is fused (q|k|v stacked, gate / up interleaved) and the carried RMSNorm gains
struct LmLoader : TensorLoader {
  int dtype = MIA_BF16;
  // a norm gain [D]: the plain copy, the pre-scaled one for the fused chain's producers and 1 / that scale (skinny.h, mia_carry_gain)
  void norm(const std::string& n, int D, float*& plain, float*& scaled, float& rs) {
    std::vector<float> g;
    if (read(n, g, {D})) { plain = up(g); scaled = mia_carry_gain(*this, g, dtype, plain, &rs); }
  }
  // tensors `<p><part><suffix>` of the given row counts stacked along the rows; cols == 0: vectors (the biases)
  bool stacked(const std::string& p, std::initializer_list<std::pair<const char*, int>> parts, const char* suffix, int cols, std::vector<float>& out) {
    std::vector<float> t;
    out.clear();
    for (const auto& part : parts) {
      const std::string n = p + part.first + suffix;
      if (!(cols ? read(n, t, {part.second, cols}) : read(n, t, {part.second}))) return false;
      out.insert(out.end(), t.begin(), t.end());
    }
    return true;
  }
};

int pick_split(int K, int want) { for (int s = want; s > 1; --s) if (K % (32 * s) == 0) return s; return 1; }

}  // namespace

int lm_alloc_state(mia_lm* m, int B) {
  const mia_lm_config& c = m->cfg;
  const int D = c.hidden, dh = c.head_dim, Nq = c.n_heads * dh, Nk = c.n_kv_heads * dh;
  for (void* p : m->state_allocs) (void)hipFree(p);
  m->state_allocs.clear();
  if (m->graph) { (void)hipGraphExecDestroy(m->graph); m->graph = nullptr; }
  bool ok = true;
  auto dev = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, bytes + 64) != hipSuccess) { ok = false; return nullptr; }
    m->state_allocs.push_back(p);
    return p;
  };
  // K/V: the 16-bit caches, or (mia_lm_set_kv_quant) code dwords + one (scale, bias) dword per 64 values -- never both
  const size_t kv_rows = (size_t)c.n_layers * B * c.n_kv_heads * c.max_ctx;
  const size_t kv = m->kv_bits ? 0 : kv_rows * dh * 2, kvq = kv_rows * dh * m->kv_bits / 8, kvp = m->kv_bits ? kv_rows * (dh / 64) * 4 : 0;
  m->k_cache = m->v_cache = nullptr; m->kq_codes = m->vq_codes = m->kq_pairs = m->vq_pairs = nullptr;
  if (m->kv_bits) { m->kq_codes = (uint32_t*)dev(kvq); m->vq_codes = (uint32_t*)dev(kvq); m->kq_pairs = (uint32_t*)dev(kvp); m->vq_pairs = (uint32_t*)dev(kvp); }
  else { m->k_cache = dev(kv); m->v_cache = dev(kv); }
  m->x = (float*)dev((size_t)B * D * 4); m->h = dev((size_t)B * D * 2);
  m->qkv_part = (float*)dev((size_t)4 * B * (Nq + 2 * Nk) * 4); m->q = dev((size_t)B * Nq * 2); m->att = dev((size_t)B * Nq * 2); m->act = dev((size_t)B * c.inter * 2);
  m->ss = (float*)dev((size_t)2 * ((D + 15) / 16) * B * 4);
  m->partial = (float*)dev((size_t)8 * B * D * 4); m->logits = (float*)dev((size_t)B * std::max(c.vocab, m->head_vocab) * 4);
  m->tokens = (int32_t*)dev((size_t)B * c.max_ctx * 4); m->hist = (int32_t*)dev((size_t)B * 64 * 4); m->uniforms = (float*)dev((size_t)B * c.max_ctx * 4);
  m->state = (LmState*)dev(sizeof(LmState) * B); m->smx = dev(lm_sample_ws_bytes() * B);
  m->embeds = (float*)dev((size_t)B * c.max_ctx * D * 4); m->out_tokens = (int32_t*)dev((size_t)B * c.max_ctx * 4);
  if (!ok) return -1;
  if (m->kv_bits) { (void)hipMemset(m->kq_codes, 0, kvq); (void)hipMemset(m->vq_codes, 0, kvq); (void)hipMemset(m->kq_pairs, 0, kvp); (void)hipMemset(m->vq_pairs, 0, kvp); }
  else { (void)hipMemset(m->k_cache, 0, kv); (void)hipMemset(m->v_cache, 0, kv); }
  (void)hipMemset(m->state, 0, sizeof(LmState) * B);
  m->B_cap = B;
  return 0;
}

extern "C" void mia_lm_free(mia_lm* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  if (m->graph) (void)hipGraphExecDestroy(m->graph);
  for (void* p : m->allocs) (void)hipFree(p);
  for (void* p : m->state_allocs) (void)hipFree(p);
  delete m;
}

extern "C" mia_lm* mia_lm_load(mia_ctx* ctx, const mia_lm_config* cfg, const mia_tensor_view* tensors, int n_tensors, int dtype) {
  if (!ctx) return nullptr;
  auto fail = [&](mia_lm* m, const std::string& msg) -> mia_lm* { ctx->err = "lm_load: " + msg; if (m) mia_lm_free(m); return nullptr; };
  if (!cfg || !tensors || n_tensors <= 0) return fail(nullptr, "null arguments");
  if (dtype != MIA_BF16 && dtype != MIA_F16) return fail(nullptr, "dtype must be MIA_BF16 or MIA_F16");
  const mia_lm_config& c = *cfg;
  if (c.head_dim != 64 && c.head_dim != 128) return fail(nullptr, "head_dim must be 64 or 128");
  if (c.hidden % 32 || c.hidden > 4096 || c.inter % 32 || c.n_heads % c.n_kv_heads || c.vocab <= 0 || c.n_layers <= 0 || c.max_ctx <= 0 || c.max_ctx > 8192)
    return fail(nullptr, "unsupported dimensions (hidden <= 4096 and % 32, inter % 32, max_ctx <= 8192)");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(nullptr, "hipSetDevice failed");
  mia_lm* m = new mia_lm(); m->ctx = ctx; m->cfg = c; m->dtype = dtype;
  LmLoader L; L.allocs = &m->allocs; L.dtype = dtype;
  L.index(tensors, n_tensors);
  const int D = c.hidden, dh = c.head_dim, Nq = c.n_heads * dh, Nk = c.n_kv_heads * dh;
  std::vector<float> t, t2;
  if (L.read("model.embed_tokens.weight", t, {c.vocab, D})) m->embed = L.up16(t, dtype);
  if (c.tie_embeddings) m->lm_head = m->embed;
  else if (L.has("lm_head.weight") && L.read("lm_head.weight", t, {c.vocab, D})) m->lm_head = L.up16(t, dtype);
  L.norm("model.norm.weight", D, m->final_norm, m->final_norm_c, m->final_rs);
  if (const mia_tensor_view* hv = L.find("llm_decoder.weight")) {      // Qwen2LM: separate output head + speech embedding
    if (hv->ndim == 2 && hv->shape[1] == D) {
      m->head_vocab = (int)hv->shape[0];
      if (L.read("llm_decoder.weight", t, {m->head_vocab, D})) m->lm_head = L.up16(t, dtype);
      if (L.has("llm_decoder.bias") && L.read("llm_decoder.bias", t, {m->head_vocab})) m->head_bias = L.up(t);
    } else L.fail(MIA_ERR_INVALID_ARGUMENT, "llm_decoder.weight has an unexpected shape");
  }
  if (const mia_tensor_view* gv = L.find("speech_embedding.weight")) {
    if (gv->ndim == 2 && gv->shape[1] == D) { m->gen_rows = (int)gv->shape[0]; if (L.read("speech_embedding.weight", t, {m->gen_rows, D})) m->gen_embed = L.up16(t, dtype); }
    else L.fail(MIA_ERR_INVALID_ARGUMENT, "speech_embedding.weight has an unexpected shape");
  }
  {  // rotary inverse frequencies: plain RoPE(base) or Llama3RoPE (Llama3RoPE.swift:41-65: period-like `freqs`, MLX divides positions by them)
    std::vector<float> inv(dh / 2);
    for (int i = 0; i < dh / 2; ++i) {
      float freq = powf(c.rope_theta, (float)(2 * i) / (float)dh);
      if (c.rope_llama3) {
        const float low_wl = (float)c.rope_old_ctx / c.rope_low, high_wl = (float)c.rope_old_ctx / c.rope_high;
        const float wl = 2.0f * (float)M_PI * freq;
        float f = wl > low_wl ? freq * c.rope_factor : freq;
        if (wl > high_wl && wl < low_wl) {
          const float smooth = ((float)c.rope_old_ctx / wl - c.rope_low) / (c.rope_high - c.rope_low);
          f = f / ((1.0f - smooth) / c.rope_factor + smooth);
        }
        freq = f;
      }
      inv[i] = 1.0f / freq;
    }
    m->inv_freq = L.up(inv);
  }
  m->layers.resize(c.n_layers);
  // Qwen3's per-head q / k RMSNorm (STT/FunASR/Layers/Qwen3Model.swift:32-35,57-59) is switched by tensor presence, like the CosyVoice2
  // head above: both gains [head_dim] in every layer, or none in any
  std::vector<float> qkn;
  for (int l = 0; l < c.n_layers && L.err.empty(); ++l) {
    const std::string p = "model.layers." + std::to_string(l);
    LmLayer& ly = m->layers[l];
    {
      const std::string qn = p + ".self_attn.q_norm.weight", kn = p + ".self_attn.k_norm.weight";
      const bool has_q = L.has(qn), has_k = L.has(kn);
      if (has_q != has_k) L.fail(MIA_ERR_INVALID_ARGUMENT, "missing tensor '" + (has_q ? kn : qn) + "' (q_norm and k_norm come as a pair)");
      else if (l > 0 && has_q != !qkn.empty())
        L.fail(MIA_ERR_INVALID_ARGUMENT, "tensor '" + qn + "' is " + (has_q ? "present" : "missing") + ": q_norm / k_norm must be in every layer or in none");
      else if (has_q && L.read(qn, t, {dh}) && L.read(kn, t2, {dh})) { qkn.insert(qkn.end(), t.begin(), t.end()); qkn.insert(qkn.end(), t2.begin(), t2.end()); }
    }
    L.norm(p + ".input_layernorm.weight", D, ly.in_norm, ly.in_norm_c, ly.in_rs);
    L.norm(p + ".post_attention_layernorm.weight", D, ly.post_norm, ly.post_norm_c, ly.post_rs);
    const std::initializer_list<std::pair<const char*, int>> qkv = {{"q_proj", Nq}, {"k_proj", Nk}, {"v_proj", Nk}};
    if (L.stacked(p + ".self_attn.", qkv, ".weight", D, t)) ly.wqkv = L.up16(t, dtype);
    if (c.qkv_bias && L.stacked(p + ".self_attn.", qkv, ".bias", 0, t)) ly.bqkv = L.up(t);
    if (L.read(p + ".self_attn.o_proj.weight", t, {D, Nq})) ly.wo = L.up16(t, dtype);
    if (L.read(p + ".mlp.gate_proj.weight", t, {c.inter, D}) && L.read(p + ".mlp.up_proj.weight", t2, {c.inter, D})) {
      std::vector<float> gu((size_t)2 * c.inter * D);
      for (int r = 0; r < c.inter; ++r) { memcpy(&gu[(size_t)(2 * r) * D], &t[(size_t)r * D], (size_t)D * 4); memcpy(&gu[(size_t)(2 * r + 1) * D], &t2[(size_t)r * D], (size_t)D * 4); }
      ly.wgu = L.up16(gu, dtype);
    }
    if (L.read(p + ".mlp.down_proj.weight", t, {D, c.inter})) ly.wdown = L.up16(t, dtype);
  }
  if (L.err.empty() && !qkn.empty()) m->qk_norm = L.up(qkn);
  if (!L.err.empty()) return fail(m, L.err);
  {  // fragment-order copies for the decode step (one device repack per matrix)
    bool ok = true;
    auto frag = [&](const void* src, int N, int K, void** dst) { ok = ok && dec_wfrag_copy(src, N, K, m->allocs, ctx->stream, dst); };
    for (LmLayer& ly : m->layers) {
      frag(ly.wqkv, Nq + 2 * Nk, D, &ly.wqkv_f); frag(ly.wo, D, Nq, &ly.wo_f);
      frag(ly.wgu, 2 * c.inter, D, &ly.wgu_f); frag(ly.wdown, D, c.inter, &ly.wdown_f);
    }
    frag(m->lm_head, m->head_vocab > 0 ? m->head_vocab : c.vocab, D, &m->lm_head_f);
    if (!ok) return fail(m, "fragment-order repack of the step weights failed");
  }
  m->S_qkv = pick_split(D, 4); m->S_o = pick_split(Nq, 4); m->S_down = pick_split(c.inter, 8);
  if (lm_alloc_state(m, 1)) return fail(m, "hipMalloc failed (state buffers)");
  if (hipDeviceSynchronize() != hipSuccess) return fail(m, "device error during upload");
  return m;
}

// ---- MLX-affine 4- / 6- / 8-bit weights for the decode step (OrpheusWeightLoader.swift:28-60: the reference's default checkpoints are q4, group 64) ----
// tensors: for every Linear of the step, `<name>.weight` (MIA_U32 packed codes [N][K * bits / 32]), `<name>.scales`, `<name>.biases`
// ([N][K/64], both MIA_F16 or both MIA_BF16), names as in the checkpoint (model.layers.L.self_attn.{q,k,v,o}_proj, mlp.{gate,up,down}_proj,
// model.embed_tokens / lm_head).  The handle must already hold the de-quantised 16-bit weights (mia_lm_load on the expanded
// checkpoint): the batched prompt pass keeps using them until mia_lm_set_prompt_weights(1), the per-token step switches to the packed form.  Nothing of the handle changes
// unless every matrix was repacked and uploaded.  A bad argument or tensor list is MIA_ERR_INVALID_ARGUMENT; a refused hipMalloc
// MIA_ERR_OUT_OF_MEMORY, a failed upload MIA_ERR_DEVICE.
// (the two halves are declared in lm.h: marvis.hip packs its two stacks through them)
void lm_attach_discard(LmPacked& p) {
  for (void* q : p.fresh) (void)hipFree(q);
  p = LmPacked{};
}

int lm_attach_prepare(mia_lm* m, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits, const char* who, LmPacked& out) {
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, tensors && n_tensors > 0 && group_size == 64 && (bits == 4 || bits == 6 || bits == 8), "%s: tensors required, group size 64, 4, 6 or 8 bits", who);
  MIA_CHECK_ARG(ctx, m->q_bits == 0, "%s: packed weights are already attached to this handle (load a fresh handle to replace them)", who);
  const mia_lm_config& c = m->cfg;
  const int D = c.hidden, dh = c.head_dim, Nq = c.n_heads * dh, Nk = c.n_kv_heads * dh;
  MIA_CHECK_ARG(ctx, D % 128 == 0 && Nq % 128 == 0 && c.inter % 128 == 0, "%s: hidden, n_heads*head_dim and inter must be multiples of 128", who);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  out = LmPacked{};
  out.layers.assign((size_t)4 * c.n_layers, Q4W{});
  std::vector<void*>& fresh = out.fresh;         // joins m->allocs only when everything is in place (lm_attach_commit)
  TensorLoader L; L.allocs = &fresh;
  L.index(tensors, n_tensors);
  int sdt = -1;
  const float mag = m->dtype == MIA_F16 ? 1024.0f : 128.0f;
  // parts (name, rows) fused as the dense loader fuses them: stacked along N, or their rows interleaved (gate / up, like wgu)
  auto pack = [&](const std::string& p, std::initializer_list<std::pair<const char*, int>> parts, int K, bool interleave, Q4W& out) -> bool {
    std::vector<Q4Src> src(parts.size());
    std::vector<std::pair<int, int>> rows;
    int i = 0;
    for (const auto& part : parts) {
      if (!q_find_linear(L, p + part.first, part.second, K, bits, false, &sdt, src[i])) return false;
      if (!interleave) for (int n = 0; n < part.second; ++n) rows.push_back({i, n});
      ++i;
    }
    if (interleave) for (int n = 0; n < parts.begin()->second; ++n) for (int j = 0; j < i; ++j) rows.push_back({j, n});
    return q_upload(L, src, rows, K, bits, sdt, mag, &out.wfrag, &out.stfrag);
  };
  bool ok = true;
  for (int l = 0; l < c.n_layers && ok; ++l) {
    const std::string p = "model.layers." + std::to_string(l);
    Q4W* ly = &out.layers[(size_t)4 * l];
    ok = pack(p + ".self_attn.", {{"q_proj", Nq}, {"k_proj", Nk}, {"v_proj", Nk}}, D, false, ly[0]) && pack(p + ".self_attn.", {{"o_proj", D}}, Nq, false, ly[1]) &&
         pack(p + ".mlp.", {{"gate_proj", c.inter}, {"up_proj", c.inter}}, D, true, ly[2]) && pack(p + ".mlp.", {{"down_proj", D}}, c.inter, false, ly[3]);
  }
  // the tied / plain LM head, when the checkpoint packs it (the CosyVoice2 speech head stays 16-bit: it is not quantised there)
  const char* hp = c.tie_embeddings ? "model.embed_tokens" : "lm_head";
  if (ok && m->head_vocab == 0 && L.has(std::string(hp) + ".scales")) ok = pack("", {{hp, c.vocab}}, D, false, out.head);
  if (ok && hipDeviceSynchronize() != hipSuccess) ok = L.fail(MIA_ERR_DEVICE, "device error during upload");
  if (!ok) {      // nothing of the handle was touched: drop the attach's buffers
    lm_attach_discard(out);
    return mia_fail(ctx, L.code, "%s: %s", who, L.err.c_str());
  }
  out.bits = bits;
  return MIA_OK;
}

void lm_attach_commit(mia_lm* m, LmPacked& p) {
  const mia_lm_config& c = m->cfg;
  const int D = c.hidden, Nq = c.n_heads * c.head_dim;
  for (int l = 0; l < c.n_layers; ++l) {
    LmLayer& ly = m->layers[l];
    ly.q_qkv = p.layers[(size_t)4 * l]; ly.q_o = p.layers[(size_t)4 * l + 1]; ly.q_gu = p.layers[(size_t)4 * l + 2]; ly.q_down = p.layers[(size_t)4 * l + 3];
  }
  m->q_head = p.head;
  m->allocs.insert(m->allocs.end(), p.fresh.begin(), p.fresh.end());
  // the packed kernel splits K in 128-input blocks: re-pick the cross-workgroup splits on that granule (the 16-bit step uses the same
  // splits from here on)
  auto split128 = [](int K, int want) { for (int sp = want; sp > 1; --sp) if (K % (128 * sp) == 0) return sp; return 1; };
  m->S_qkv = split128(D, 4); m->S_o = split128(Nq, 4); m->S_down = split128(c.inter, 8);
  m->q_bits = p.bits;
  m->q4 = true;
  m->graph_mode = -1;          // the captured step holds the 16-bit launches: re-capture
  p = LmPacked{};
}

extern "C" int mia_lm_attach_quantized(mia_lm* m, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  LmPacked p;
  if (const int rc = lm_attach_prepare(m, tensors, n_tensors, group_size, bits, "lm_attach_quantized", p)) return rc;
  lm_attach_commit(m, p);
  return MIA_OK;
}

extern "C" int mia_lm_attach_q4(mia_lm* m, const mia_tensor_view* tensors, int n_tensors, int group_size) {
  return mia_lm_attach_quantized(m, tensors, n_tensors, group_size, 4);
}

// switch the step between the packed (1) and the 16-bit (0) weights of a handle that has both (A/B timing, parity tests)
extern "C" int mia_lm_use_q4(mia_lm* m, int on) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(m->ctx, !on || m->q_bits != 0, "lm_use_q4: no packed weights attached");
  if (!on && m->dense_released) return mia_fail(m->ctx, MIA_ERR_UNSUPPORTED, "lm_use_q4: the 16-bit Linears of this handle were released (mia_lm_release_dense)");
  m->q4 = on != 0;
  m->graph_mode = -1;
  return MIA_OK;
}

// which weights the batched prompt pass multiplies: 0 = the 16-bit copy (gemm.hip; the default), 1 = the packed ones (gemm_quant.hip)
extern "C" int mia_lm_set_prompt_weights(mia_lm* m, int mode) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(m->ctx, mode == 0 || mode == 1, "lm_set_prompt_weights: mode must be 0 or 1 (got %d)", mode);
  MIA_CHECK_ARG(m->ctx, !mode || m->q_bits != 0, "lm_set_prompt_weights: no packed weights attached (mia_lm_attach_quantized)");
  if (!mode && m->dense_released) return mia_fail(m->ctx, MIA_ERR_UNSUPPORTED, "lm_set_prompt_weights: the 16-bit Linears of this handle were released (mia_lm_release_dense)");
  m->prompt_packed = mode;      // the prompt pass is launched directly, never captured: nothing to drop
  return MIA_OK;
}

namespace {

// the four Linears of a layer as (N, K): q|k|v, o, gate|up, down
void lm_linear_dims(const mia_lm_config& c, int64_t (&nk)[4][2]) {
  const int64_t D = c.hidden, Nq = (int64_t)c.n_heads * c.head_dim, Nk = (int64_t)c.n_kv_heads * c.head_dim;
  nk[0][0] = Nq + 2 * Nk; nk[0][1] = D; nk[1][0] = D; nk[1][1] = Nq; nk[2][0] = 2 * (int64_t)c.inter; nk[2][1] = D; nk[3][0] = D; nk[3][1] = c.inter;
}
int64_t pad16(int64_t n) { return (n + 15) / 16 * 16; }
// codes + (scale, offset) pairs of one packed matrix (quant_repack.hip: [tiles][K / 128] blocks)
int64_t packed_bytes(int64_t N, int64_t K, int bits) { return pad16(N) / 16 * (K / 128) * ((bits == 6 ? 1536 : 256 * bits) + 256); }

}  // namespace

// Frees the layers' 16-bit Linears (row-major and fragment order) of a handle whose step and prompt pass can both run packed; both are
// switched to the packed weights first, and the two switches back are MIA_ERR_UNSUPPORTED from here on.  The embedding table, the norms,
// the biases and the head (16-bit and packed) stay.
extern "C" int mia_lm_release_dense(mia_lm* m) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, m->q_bits != 0, "lm_release_dense: no packed weights attached (mia_lm_attach_quantized)");
  if (m->dense_released) return MIA_OK;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));      // nothing in flight reads what is about to go
  m->q4 = true; m->prompt_packed = 1; m->graph_mode = -1;
  auto drop = [&](void*& p) {
    if (!p) return;
    auto it = std::find(m->allocs.begin(), m->allocs.end(), p);
    if (it != m->allocs.end()) { (void)hipFree(p); m->allocs.erase(it); }
    p = nullptr;
  };
  for (LmLayer& ly : m->layers) {
    drop(ly.wqkv); drop(ly.wo); drop(ly.wgu); drop(ly.wdown);
    drop(ly.wqkv_f); drop(ly.wo_f); drop(ly.wgu_f); drop(ly.wdown_f);
  }
  m->dense_released = true;
  return MIA_OK;
}

// device bytes of weight matrices the handle holds now: *dense = the 16-bit ones (embedding tables, the head and its fragment copy, the
// layers' Linears in both orders), *packed = the attached codes and (scale, offset) pairs.  Norm gains, biases and state are not counted.
extern "C" int mia_lm_weight_bytes(mia_lm* m, int64_t* dense, int64_t* packed) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(m->ctx, dense && packed, "lm_weight_bytes: null pointer");
  const mia_lm_config& c = m->cfg;
  const int64_t D = c.hidden, HV = m->head_vocab > 0 ? m->head_vocab : c.vocab;
  int64_t nk[4][2];
  lm_linear_dims(c, nk);
  int64_t d = 0, q = 0;
  if (m->embed) d += (int64_t)c.vocab * D * 2;
  if (m->lm_head && m->lm_head != m->embed) d += HV * D * 2;
  if (m->lm_head_f) d += pad16(HV) * D * 2;
  if (m->gen_embed) d += (int64_t)m->gen_rows * D * 2;
  for (const LmLayer& ly : m->layers) {
    const void* rm[4] = {ly.wqkv, ly.wo, ly.wgu, ly.wdown};
    const void* fr[4] = {ly.wqkv_f, ly.wo_f, ly.wgu_f, ly.wdown_f};
    const Q4W* qw[4] = {&ly.q_qkv, &ly.q_o, &ly.q_gu, &ly.q_down};
    for (int i = 0; i < 4; ++i) {
      if (rm[i]) d += nk[i][0] * nk[i][1] * 2;
      if (fr[i]) d += pad16(nk[i][0]) * nk[i][1] * 2;
      if (qw[i]->wfrag) q += packed_bytes(nk[i][0], nk[i][1], m->q_bits);
    }
  }
  if (m->q_head.wfrag) q += packed_bytes(HV, D, m->q_bits);
  *dense = d; *packed = q;
  return MIA_OK;
}
