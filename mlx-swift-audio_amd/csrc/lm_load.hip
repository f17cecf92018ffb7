// lm_load.hip -- the LM handle's life cycle: mia_lm_load (16-bit upload of a Llama-3 / Qwen2 / Qwen3 checkpoint, fused q|k|v and gate|up
// matrices, fragment-order copies for the decode step), the per-sequence state buffers, mia_lm_free, and the MLX-affine 4- / 8-bit
// packed weights of the step (mia_lm_attach_quantized: host repack into the layout skinny_quant.hip reads).
#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "lm.h"
#include "quant_repack.h"
#include "skinny.h"

namespace {

struct LmLoader {
  mia_lm* m;
  std::map<std::string, const mia_tensor_view*> by_name;
  std::string err;
  const mia_tensor_view* find(const std::string& n, bool req = true) {
    auto it = by_name.find(n);
    if (it == by_name.end()) { if (req && err.empty()) err = "missing tensor '" + n + "'"; return nullptr; }
    return it->second;
  }
  static float h2f(uint16_t h) { _Float16 x; memcpy(&x, &h, 2); return (float)x; }
  bool to_f32(const std::string& n, std::vector<float>& out, int64_t rows, int64_t cols, bool req = true) {
    const mia_tensor_view* t = find(n, req);
    if (!t) return false;
    const bool ok = cols > 0 ? (t->ndim == 2 && t->shape[0] == rows && t->shape[1] == cols) : (t->ndim == 1 && t->shape[0] == rows);
    if (!ok) { if (err.empty()) err = "tensor '" + n + "' has an unexpected shape"; return false; }
    const int64_t numel = rows * (cols > 0 ? cols : 1);
    out.resize(numel);
    if (t->dtype == MIA_F32) memcpy(out.data(), t->data, numel * 4);
    else if (t->dtype == MIA_F16) { const uint16_t* p = (const uint16_t*)t->data; for (int64_t i = 0; i < numel; ++i) out[i] = h2f(p[i]); }
    else { const uint16_t* p = (const uint16_t*)t->data; for (int64_t i = 0; i < numel; ++i) { uint32_t u = (uint32_t)p[i] << 16; memcpy(&out[i], &u, 4); } }
    return true;
  }
  void* dev(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes + 64) != hipSuccess) { if (err.empty()) err = "hipMalloc failed"; return nullptr; }
    m->allocs.push_back(p);
    return p;
  }
  float* up32(const std::vector<float>& v) { float* d = (float*)dev(v.size() * 4); if (d) (void)hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice); return d; }
  // the gain of a carried RMSNorm times its pre-scale (skinny.h, mia_carry_prescale); *rs = 1 / scale.  `plain` when the scale is 1.
  float* carried(const std::vector<float>& g, float* rs, float* plain) {
    const float p = mia_carry_prescale(g.data(), (int)g.size(), m->dtype);
    *rs = 1.f / p;
    if (p == 1.f) return plain;
    std::vector<float> v(g);
    for (float& x : v) x *= p;
    return up32(v);
  }
  void* up16(const std::vector<float>& v) {
    std::vector<uint16_t> q(v.size());
    if (m->dtype == MIA_F16) for (size_t i = 0; i < v.size(); ++i) { _Float16 hh = (_Float16)v[i]; memcpy(&q[i], &hh, 2); }
    else for (size_t i = 0; i < v.size(); ++i) { uint32_t u; memcpy(&u, &v[i], 4); u += 0x7fffu + ((u >> 16) & 1); q[i] = (uint16_t)(u >> 16); }
    void* d = dev(q.size() * 2);
    if (d) (void)hipMemcpy(d, q.data(), q.size() * 2, hipMemcpyHostToDevice);
    return d;
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
  LmLoader L; L.m = m;
  for (int i = 0; i < n_tensors; ++i) if (tensors[i].name && tensors[i].data) L.by_name[tensors[i].name] = &tensors[i];
  const int D = c.hidden, dh = c.head_dim, Nq = c.n_heads * dh, Nk = c.n_kv_heads * dh;
  std::vector<float> t, t2, t3;
  if (L.to_f32("model.embed_tokens.weight", t, c.vocab, D)) m->embed = L.up16(t);
  if (c.tie_embeddings) m->lm_head = m->embed;
  else if (L.find("lm_head.weight", false) && L.to_f32("lm_head.weight", t, c.vocab, D)) m->lm_head = L.up16(t);
  if (L.to_f32("model.norm.weight", t, D, 0)) { m->final_norm = L.up32(t); m->final_norm_c = L.carried(t, &m->final_rs, m->final_norm); }
  if (const mia_tensor_view* hv = L.find("llm_decoder.weight", false)) {      // Qwen2LM: separate output head + speech embedding
    if (hv->ndim == 2 && hv->shape[1] == D) {
      m->head_vocab = (int)hv->shape[0];
      if (L.to_f32("llm_decoder.weight", t, m->head_vocab, D)) m->lm_head = L.up16(t);
      if (L.find("llm_decoder.bias", false) && L.to_f32("llm_decoder.bias", t, m->head_vocab, 0)) m->head_bias = L.up32(t);
    } else L.err = "llm_decoder.weight has an unexpected shape";
  }
  if (const mia_tensor_view* gv = L.find("speech_embedding.weight", false)) {
    if (gv->ndim == 2 && gv->shape[1] == D) { m->gen_rows = (int)gv->shape[0]; if (L.to_f32("speech_embedding.weight", t, m->gen_rows, D)) m->gen_embed = L.up16(t); }
    else L.err = "speech_embedding.weight has an unexpected shape";
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
    m->inv_freq = L.up32(inv);
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
      const bool has_q = L.find(qn, false) != nullptr, has_k = L.find(kn, false) != nullptr;
      if (has_q != has_k) L.err = "missing tensor '" + (has_q ? kn : qn) + "' (q_norm and k_norm come as a pair)";
      else if (l > 0 && has_q != !qkn.empty()) L.err = "tensor '" + qn + "' is " + (has_q ? "present" : "missing") + ": q_norm / k_norm must be in every layer or in none";
      else if (has_q && L.to_f32(qn, t, dh, 0) && L.to_f32(kn, t2, dh, 0)) { qkn.insert(qkn.end(), t.begin(), t.end()); qkn.insert(qkn.end(), t2.begin(), t2.end()); }
    }
    if (L.to_f32(p + ".input_layernorm.weight", t, D, 0)) { ly.in_norm = L.up32(t); ly.in_norm_c = L.carried(t, &ly.in_rs, ly.in_norm); }
    if (L.to_f32(p + ".post_attention_layernorm.weight", t, D, 0)) { ly.post_norm = L.up32(t); ly.post_norm_c = L.carried(t, &ly.post_rs, ly.post_norm); }
    std::vector<float> qkv((size_t)(Nq + 2 * Nk) * D);
    if (L.to_f32(p + ".self_attn.q_proj.weight", t, Nq, D) && L.to_f32(p + ".self_attn.k_proj.weight", t2, Nk, D) && L.to_f32(p + ".self_attn.v_proj.weight", t3, Nk, D)) {
      memcpy(qkv.data(), t.data(), t.size() * 4); memcpy(qkv.data() + t.size(), t2.data(), t2.size() * 4); memcpy(qkv.data() + t.size() + t2.size(), t3.data(), t3.size() * 4);
      ly.wqkv = L.up16(qkv);
    }
    if (c.qkv_bias) {
      std::vector<float> b((size_t)Nq + 2 * Nk);
      if (L.to_f32(p + ".self_attn.q_proj.bias", t, Nq, 0) && L.to_f32(p + ".self_attn.k_proj.bias", t2, Nk, 0) && L.to_f32(p + ".self_attn.v_proj.bias", t3, Nk, 0)) {
        memcpy(b.data(), t.data(), t.size() * 4); memcpy(b.data() + Nq, t2.data(), t2.size() * 4); memcpy(b.data() + Nq + Nk, t3.data(), t3.size() * 4);
        ly.bqkv = L.up32(b);
      }
    }
    if (L.to_f32(p + ".self_attn.o_proj.weight", t, D, Nq)) ly.wo = L.up16(t);
    if (L.to_f32(p + ".mlp.gate_proj.weight", t, c.inter, D) && L.to_f32(p + ".mlp.up_proj.weight", t2, c.inter, D)) {
      std::vector<float> gu((size_t)2 * c.inter * D);
      for (int r = 0; r < c.inter; ++r) { memcpy(&gu[(size_t)(2 * r) * D], &t[(size_t)r * D], (size_t)D * 4); memcpy(&gu[(size_t)(2 * r + 1) * D], &t2[(size_t)r * D], (size_t)D * 4); }
      ly.wgu = L.up16(gu);
    }
    if (L.to_f32(p + ".mlp.down_proj.weight", t, D, c.inter)) ly.wdown = L.up16(t);
  }
  if (L.err.empty() && !qkn.empty()) m->qk_norm = L.up32(qkn);
  if (!L.err.empty()) return fail(m, L.err);
  {  // fragment-order copies for the decode step (one device repack per matrix)
    bool ok = true;
    auto frag = [&](const void* src, int N, int K) -> void* {
      if (!ok || !src || K % 32 != 0) return nullptr;
      void* dst = nullptr;
      if (hipMalloc(&dst, (size_t)((N + 15) / 16) * 16 * K * 2) != hipSuccess) { ok = false; return nullptr; }
      m->allocs.push_back(dst);
      if (dec_launch_repack_wfrag(src, dst, N, K, ctx->stream) != 0) ok = false;
      return dst;
    };
    for (LmLayer& ly : m->layers) {
      ly.wqkv_f = frag(ly.wqkv, Nq + 2 * Nk, D); ly.wo_f = frag(ly.wo, D, Nq);
      ly.wgu_f = frag(ly.wgu, 2 * c.inter, D); ly.wdown_f = frag(ly.wdown, D, c.inter);
    }
    m->lm_head_f = frag(m->lm_head, m->head_vocab > 0 ? m->head_vocab : c.vocab, D);
    if (!ok) return fail(m, "fragment-order repack of the step weights failed");
  }
  m->S_qkv = pick_split(D, 4); m->S_o = pick_split(Nq, 4); m->S_down = pick_split(c.inter, 8);
  if (lm_alloc_state(m, 1)) return fail(m, "hipMalloc failed (state buffers)");
  if (hipDeviceSynchronize() != hipSuccess) return fail(m, "device error during upload");
  return m;
}

// ---- MLX-affine 4-bit weights for the decode step (OrpheusWeightLoader.swift:28-60: the reference's default checkpoints are q4, group 64) ----
namespace {

// rows[i] = (tensor index, row): the fused matrix's row i.  Builds the fragment-ordered arrays (quant_repack.h; layout and arithmetic:
// skinny_gemm_qi) and uploads them.  bits 4 | 8; mag = the 16-bit float the codes are OR-ed into (128 for bf16, 1024 for f16 compute).
bool q_repack(LmLoader& L, const std::vector<Q4Src>& src, const std::vector<std::pair<int, int>>& rows, int K, int bits, int sdt, float mag, Q4W& out) {
  std::vector<uint32_t> wf;
  std::vector<float> st;
  q_repack_host(src, rows, K, bits, sdt, mag, wf, st);
  out.wfrag = (uint32_t*)L.dev(wf.size() * 4);
  out.stfrag = (float*)L.dev(st.size() * 4);
  if (!out.wfrag || !out.stfrag) { if (L.err.empty()) L.err = "hipMalloc failed for the packed weights"; return false; }
  if (hipMemcpy(out.wfrag, wf.data(), wf.size() * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(out.stfrag, st.data(), st.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
    if (L.err.empty()) L.err = "upload of the packed weights failed";
    return false;
  }
  return true;
}

}  // namespace

// tensors: for every Linear of the step, `<name>.weight` (MIA_U32 packed codes [N][K * bits / 32]), `<name>.scales`, `<name>.biases`
// ([N][K/64], both MIA_F16 or both MIA_BF16), names as in the checkpoint (model.layers.L.self_attn.{q,k,v,o}_proj, mlp.{gate,up,down}_proj,
// model.embed_tokens / lm_head).  The handle must already hold the de-quantised 16-bit weights (mia_lm_load on the expanded
// checkpoint): the batched prompt pass keeps using them, the per-token step switches to the packed form.
extern "C" int mia_lm_attach_quantized(mia_lm* m, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, tensors && n_tensors > 0 && group_size == 64 && (bits == 4 || bits == 8), "lm_attach_quantized: tensors required, group size 64, 4 or 8 bits");
  MIA_CHECK_ARG(ctx, m->q_bits == 0, "lm_attach_quantized: packed weights are already attached to this handle (load a fresh handle to replace them)");
  const mia_lm_config& c = m->cfg;
  const int D = c.hidden, dh = c.head_dim, Nq = c.n_heads * dh, Nk = c.n_kv_heads * dh;
  MIA_CHECK_ARG(ctx, D % 128 == 0 && Nq % 128 == 0 && c.inter % 128 == 0, "lm_attach_quantized: hidden, n_heads*head_dim and inter must be multiples of 128");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  LmLoader L; L.m = m;
  for (int i = 0; i < n_tensors; ++i) if (tensors[i].name && tensors[i].data) L.by_name[tensors[i].name] = &tensors[i];
  int sdt = 0;
  const float mag = m->dtype == MIA_F16 ? 1024.0f : 128.0f;
  auto get = [&](const std::string& p, int N, int K, Q4Src& q) -> bool {
    const mia_tensor_view* w = L.find(p + ".weight"); const mia_tensor_view* s = L.find(p + ".scales"); const mia_tensor_view* b = L.find(p + ".biases");
    if (!w || !s || !b) return false;
    const bool ok = w->dtype == MIA_U32 && w->ndim == 2 && w->shape[0] == N && w->shape[1] == (int64_t)K * bits / 32 && s->ndim == 2 && s->shape[0] == N && s->shape[1] == K / 64 &&
                    b->ndim == 2 && b->shape[0] == N && b->shape[1] == K / 64 && s->dtype == b->dtype && (s->dtype == MIA_F16 || s->dtype == MIA_BF16);
    if (!ok) { if (L.err.empty()) L.err = "'" + p + "' is not a " + std::to_string(bits) + "-bit group-64 Linear of the expected shape (scales / biases must be f16 or bf16)"; return false; }
    if (sdt == 0) sdt = s->dtype;
    if (sdt != s->dtype) { if (L.err.empty()) L.err = "mixed scale dtypes"; return false; }
    q = Q4Src{(const uint32_t*)w->data, s->data, b->data};
    return true;
  };
  auto seq = [](int tensor, int n, std::vector<std::pair<int, int>>& rows) { for (int i = 0; i < n; ++i) rows.push_back({tensor, i}); };
  for (int l = 0; l < c.n_layers && L.err.empty(); ++l) {
    const std::string p = "model.layers." + std::to_string(l);
    LmLayer& ly = m->layers[l];
    std::vector<Q4Src> src(3);
    std::vector<std::pair<int, int>> rows;
    if (get(p + ".self_attn.q_proj", Nq, D, src[0]) && get(p + ".self_attn.k_proj", Nk, D, src[1]) && get(p + ".self_attn.v_proj", Nk, D, src[2])) {
      seq(0, Nq, rows); seq(1, Nk, rows); seq(2, Nk, rows);
      if (!q_repack(L, src, rows, D, bits, sdt, mag, ly.q_qkv)) break;
    }
    src.assign(1, Q4Src{}); rows.clear();
    if (get(p + ".self_attn.o_proj", D, Nq, src[0])) { seq(0, D, rows); if (!q_repack(L, src, rows, Nq, bits, sdt, mag, ly.q_o)) break; }
    src.assign(2, Q4Src{}); rows.clear();
    if (get(p + ".mlp.gate_proj", c.inter, D, src[0]) && get(p + ".mlp.up_proj", c.inter, D, src[1])) {
      for (int i = 0; i < c.inter; ++i) { rows.push_back({0, i}); rows.push_back({1, i}); }      // gate / up rows interleaved like wgu
      if (!q_repack(L, src, rows, D, bits, sdt, mag, ly.q_gu)) break;
    }
    src.assign(1, Q4Src{}); rows.clear();
    if (get(p + ".mlp.down_proj", D, c.inter, src[0])) { seq(0, D, rows); if (!q_repack(L, src, rows, c.inter, bits, sdt, mag, ly.q_down)) break; }
  }
  if (L.err.empty() && m->head_vocab == 0) {     // the tied / plain LM head (the CosyVoice2 speech head stays 16-bit: it is not quantised there)
    std::vector<Q4Src> src(1);
    std::vector<std::pair<int, int>> rows;
    const std::string hp = c.tie_embeddings ? "model.embed_tokens" : "lm_head";
    if (L.find(hp + ".scales", false)) { if (get(hp, c.vocab, D, src[0])) { seq(0, c.vocab, rows); q_repack(L, src, rows, D, bits, sdt, mag, m->q_head); } }
  }
  if (!L.err.empty()) {
    // a partly packed handle must not run: drop every packed pointer (the buffers stay with the handle's allocation list until mia_lm_free)
    for (LmLayer& ly : m->layers) { ly.q_qkv = Q4W{}; ly.q_o = Q4W{}; ly.q_gu = Q4W{}; ly.q_down = Q4W{}; }
    m->q_head = Q4W{};
    const bool oom = L.err.find("hipMalloc") != std::string::npos;
    return mia_fail(ctx, oom ? MIA_ERR_OUT_OF_MEMORY : MIA_ERR_INVALID_ARGUMENT, "lm_attach_quantized: %s", L.err.c_str());
  }
  MIA_HIP(ctx, hipDeviceSynchronize());
  // the packed kernel splits K in 128-input blocks: re-pick the cross-workgroup splits on that granule (the 16-bit step uses the same
  // splits from here on)
  auto split128 = [](int K, int want) { for (int sp = want; sp > 1; --sp) if (K % (128 * sp) == 0) return sp; return 1; };
  m->S_qkv = split128(D, 4); m->S_o = split128(Nq, 4); m->S_down = split128(c.inter, 8);
  m->q_bits = bits;
  m->q4 = true;
  m->graph_mode = -1;          // the captured step holds the 16-bit launches: re-capture
  return MIA_OK;
}

extern "C" int mia_lm_attach_q4(mia_lm* m, const mia_tensor_view* tensors, int n_tensors, int group_size) {
  return mia_lm_attach_quantized(m, tensors, n_tensors, group_size, 4);
}

// switch the step between the packed (1) and the 16-bit (0) weights of a handle that has both (A/B timing, parity tests)
extern "C" int mia_lm_use_q4(mia_lm* m, int on) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(m->ctx, !on || m->q_bits != 0, "lm_use_q4: no packed weights attached");
  m->q4 = on != 0;
  m->graph_mode = -1;
  return MIA_OK;
}
