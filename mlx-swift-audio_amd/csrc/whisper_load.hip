// whisper_load.hip -- upload a Whisper checkpoint (named host tensors) into the HBM layout of whisper.h.
// Replaces the tensor side of WhisperModel.load (STT/Whisper/WhisperModel.swift:184-206); key names are the
// reference's Module property paths (Layers/*.swift @ModuleInfo keys).
#include <cmath>

#include "decode.h"
#include "quant_repack.h"

namespace {

// Whisper's tensors on top of the shared loader: LayerNorms, Linears stacked along N, the two convolutions
struct Loader : TensorLoader {
  int dtype = MIA_BF16;
  // `gain` keeps the host copy of the gamma (the carried LayerNorms scale it again: mia_carry_gain)
  LNW ln(const std::string& p, int D, std::vector<float>* gain = nullptr) {
    LNW o;
    std::vector<float> g, b;
    if (!read(p + ".weight", g, {D}) || !read(p + ".bias", b, {D})) return o;
    o.g = up(g); o.gc = o.g; o.b = up(b);
    if (gain) gain->swap(g);
    return o;
  }
  // one or several [N_i][K] matrices stacked along N; has_bias[i] says whether part i has a bias
  LinearW linear(const std::vector<std::string>& parts, const std::vector<bool>& has_bias, int N_each, int K) {
    LinearW o; o.N = N_each * (int)parts.size(); o.K = K;
    std::vector<float> wv, bv((size_t)o.N, 0.f), tmp;
    bool any_bias = false;
    for (size_t i = 0; i < parts.size(); ++i) {
      if (!read(parts[i] + ".weight", tmp, {N_each, K})) return o;
      wv.insert(wv.end(), tmp.begin(), tmp.end());
      if (has_bias[i]) {
        if (!read(parts[i] + ".bias", tmp, {N_each})) return o;
        memcpy(&bv[i * (size_t)N_each], tmp.data(), tmp.size() * 4); any_bias = true;
      }
    }
    o.w = up16(wv, dtype);
    if (any_bias) o.b = up(bv);
    return o;
  }
  // Conv1d weight [Cout][3][Cin] -> [Cout][Kpad] (tap-major rows == the overlapping-window GEMM's K order)
  LinearW conv(const std::string& p, int Cout, int Cin, int Kpad) {
    LinearW o; o.N = Cout; o.K = Kpad;
    std::vector<float> src, wv((size_t)Cout * Kpad, 0.f), bv;
    if (!read(p + ".weight", src, {Cout, 3, Cin}) || !read(p + ".bias", bv, {Cout})) return o;
    for (int c = 0; c < Cout; ++c) memcpy(&wv[(size_t)c * Kpad], &src[(size_t)c * 3 * Cin], (size_t)3 * Cin * 4);
    o.w = up16(wv, dtype);
    o.b = up(bv);
    return o;
  }
};

}  // namespace

extern "C" mia_whisper* mia_whisper_load(mia_ctx* ctx, const mia_whisper_dims* dims, const mia_tensor_view* tensors,
                                         int n_tensors, int compute_dtype) {
  if (!ctx) return nullptr;
  auto fail = [&](const std::string& m) -> mia_whisper* { ctx->err = "whisper_load: " + m; return nullptr; };
  if (!dims || !tensors || n_tensors <= 0) return fail("null arguments");
  if (compute_dtype != MIA_BF16 && compute_dtype != MIA_F16) return fail("compute_dtype must be MIA_BF16 or MIA_F16");
  const mia_whisper_dims& d = *dims;
  if (d.n_audio_state <= 0 || d.n_audio_state % 64 || d.n_audio_head * 64 != d.n_audio_state)
    return fail("n_audio_state must equal 64 * n_audio_head (Whisper head dim is 64)");
  if (d.n_text_state % 64 || d.n_text_head * 64 != d.n_text_state) return fail("n_text_state must equal 64 * n_text_head");
  if (d.n_text_state != d.n_audio_state) return fail("n_text_state must equal n_audio_state");
  if (d.n_text_state > 2048) return fail("n_text_state must be <= 2048 (decode row kernels keep a row in registers)");
  if (d.n_mels <= 0 || d.n_mels > 128 || d.n_mels % 8) return fail("n_mels must be a multiple of 8 in 8..128");
  if (d.n_audio_ctx <= 0 || d.n_audio_ctx % 4) return fail("n_audio_ctx must be a positive multiple of 4");
  if (d.n_vocab <= 0 || d.n_text_ctx <= 0 || d.n_audio_layer <= 0 || d.n_text_layer <= 0) return fail("bad dims");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail("hipSetDevice failed");

  mia_whisper* w = new mia_whisper();
  w->ctx = ctx; w->dims = d; w->dtype = compute_dtype;
  w->kpad_conv1 = (int)align_up((size_t)3 * d.n_mels, 64);
  Loader L; L.allocs = &w->allocs; L.dtype = compute_dtype;
  for (int i = 0; i < n_tensors; ++i)
    if (!tensors[i].name || !tensors[i].data) { mia_whisper_free(w); return fail("tensor view with null name/data"); }
  L.index(tensors, n_tensors);
  const int D = d.n_audio_state;
  w->conv1 = L.conv("encoder.conv1", D, d.n_mels, w->kpad_conv1);
  w->conv2 = L.conv("encoder.conv2", D, D, 3 * D);
  {
    std::vector<float> pos;
    if (L.has("encoder.positional_embedding")) L.read("encoder.positional_embedding", pos, {d.n_audio_ctx, D});
    else {  // sinusoids(length:channels:) AudioEncoder.swift:78-96, fp32 math
      pos.resize((size_t)d.n_audio_ctx * D);
      const float inc = logf(10000.0f) / (float)(D / 2 - 1);
      for (int p = 0; p < d.n_audio_ctx; ++p)
        for (int i = 0; i < D / 2; ++i) {
          const float st = (float)p * expf(-inc * (float)i);
          pos[(size_t)p * D + i] = sinf(st);
          pos[(size_t)p * D + D / 2 + i] = cosf(st);
        }
    }
    if (!pos.empty()) w->enc_pos = L.up(pos);
  }
  w->enc.resize(d.n_audio_layer);
  std::vector<std::vector<float>> enc_mlp_g(d.n_audio_layer), cross_g(d.n_text_layer), mlp_g(d.n_text_layer);   // gammas of the carried LayerNorms
  for (int l = 0; l < d.n_audio_layer && L.err.empty(); ++l) {
    const std::string p = "encoder.blocks." + std::to_string(l);
    EncBlockW& b = w->enc[l];
    b.attn_ln = L.ln(p + ".attn_ln", D);
    b.qkv = L.linear({p + ".attn.query", p + ".attn.key", p + ".attn.value"}, {true, false, true}, D, D);
    b.out = L.linear({p + ".attn.out"}, {true}, D, D);
    b.mlp_ln = L.ln(p + ".mlp_ln", D, &enc_mlp_g[l]);
    b.mlp1 = L.linear({p + ".mlp1"}, {true}, 4 * D, D);
    b.mlp2 = L.linear({p + ".mlp2"}, {true}, D, 4 * D);
  }
  w->ln_post = L.ln("encoder.ln_post", D);
  {
    std::vector<float> v;
    if (L.read("decoder.token_embedding.weight", v, {d.n_vocab, D})) w->tok_emb = L.up16(v, compute_dtype);
    if (L.read("decoder.positional_embedding", v, {d.n_text_ctx, D})) w->dec_pos = L.up(v);
  }
  w->dec.resize(d.n_text_layer);
  for (int l = 0; l < d.n_text_layer && L.err.empty(); ++l) {
    const std::string p = "decoder.blocks." + std::to_string(l);
    DecBlockW& b = w->dec[l];
    b.attn_ln = L.ln(p + ".attn_ln", D);
    b.qkv = L.linear({p + ".attn.query", p + ".attn.key", p + ".attn.value"}, {true, false, true}, D, D);
    b.out = L.linear({p + ".attn.out"}, {true}, D, D);
    b.cross_ln = L.ln(p + ".cross_attn_ln", D, &cross_g[l]);
    b.cq = L.linear({p + ".cross_attn.query"}, {true}, D, D);
    b.ck = L.linear({p + ".cross_attn.key"}, {false}, D, D);
    b.cv = L.linear({p + ".cross_attn.value"}, {true}, D, D);
    b.cout = L.linear({p + ".cross_attn.out"}, {true}, D, D);
    b.mlp_ln = L.ln(p + ".mlp_ln", D, &mlp_g[l]);
    b.mlp1 = L.linear({p + ".mlp1"}, {true}, 4 * D, D);
    b.mlp2 = L.linear({p + ".mlp2"}, {true}, D, 4 * D);
  }
  w->dec_ln = L.ln("decoder.ln", D);
  if (!L.err.empty()) { mia_whisper_free(w); return fail(L.err); }
  {  // the decode step reads its weights in MFMA-fragment order (skinny.h): one repack per matrix, on the device
    bool ok = true;
    for (DecBlockW& b : w->dec)
      for (LinearW* lw : {&b.qkv, &b.out, &b.cq, &b.cout, &b.mlp1, &b.mlp2}) ok = ok && dec_wfrag_copy(lw->w, lw->N, lw->K, w->allocs, ctx->stream, &lw->wf);
    ok = ok && dec_wfrag_copy(w->tok_emb, d.n_vocab, D, w->allocs, ctx->stream, &w->tok_emb_f);
    if (!ok) { mia_whisper_free(w); return fail("fragment-order repack of the decoder weights failed"); }
    // LayerNorm fold constants of every decoder Linear that consumes a LayerNorm (whisper.h LinearW::c1 / c2; skinny.h)
    // carried LayerNorms (decoder: cross_attn_ln, mlp_ln; encoder: mlp_ln) get the pre-scaled gain of skinny.h (mia_carry_prescale)
    auto carried = [&](LNW& ln, const std::vector<float>& g, LinearW& consumer) { ln.gc = mia_carry_gain(L, g, w->dtype, ln.g, &consumer.ln_rs); };
    auto fold = [&](const void* w16, int N, const LNW& ln, float** c1, float** c2, const float* bias = nullptr) {
      if (!ok || !w16) return;
      void* p1 = nullptr; void* p2 = nullptr;
      if (hipMalloc(&p1, (size_t)N * 4) != hipSuccess) { ok = false; return; }
      w->allocs.push_back(p1);
      if (hipMalloc(&p2, (size_t)N * 4) != hipSuccess) { ok = false; return; }
      w->allocs.push_back(p2);
      *c1 = (float*)p1; *c2 = (float*)p2;
      if (dec_launch_lnfold(w16, N, D, ln.gc, ln.b, *c1, *c2, w->dtype, ctx->stream, bias) != 0) ok = false;
    };
    for (int l = 0; l < d.n_text_layer; ++l) {
      DecBlockW& b = w->dec[l];
      carried(b.cross_ln, cross_g[l], b.cq);
      carried(b.mlp_ln, mlp_g[l], b.mlp1);
      fold(b.qkv.w, b.qkv.N, b.attn_ln, &b.qkv.c1, &b.qkv.c2);
      fold(b.cq.w, b.cq.N, b.cross_ln, &b.cq.c1, &b.cq.c2);
      fold(b.mlp1.w, b.mlp1.N, b.mlp_ln, &b.mlp1.c1, &b.mlp1.c2);
    }
    fold(w->tok_emb, d.n_vocab, w->dec_ln, &w->emb_c1, &w->emb_c2);
    // encoder: the Linear behind mlp_ln takes its LayerNorm through the GEMM (gemm.h "LayerNorm carried across two GEMMs"); c2 includes the bias
    if (d.n_audio_state == D)
      for (int l = 0; l < d.n_audio_layer; ++l) { EncBlockW& b = w->enc[l]; carried(b.mlp_ln, enc_mlp_g[l], b.mlp1); fold(b.mlp1.w, b.mlp1.N, b.mlp_ln, &b.mlp1.c1, &b.mlp1.c2, b.mlp1.b); }
    if (!ok || !L.err.empty()) { mia_whisper_free(w); return fail("LayerNorm fold of the decoder weights failed"); }
  }
  if (hipDeviceSynchronize() != hipSuccess) { mia_whisper_free(w); return fail("device error during upload"); }
  return w;
}

extern "C" void mia_whisper_free(mia_whisper* w) {
  if (!w) return;
  if (w->n_clones > 0) { mia_fail(w->ctx, MIA_ERR_INVALID_ARGUMENT, "whisper_free: %d clone(s) still share these weights; free them first", w->n_clones); return; }
  (void)hipSetDevice(w->ctx->device);
  (void)hipStreamSynchronize(w->ctx->stream);
  if (w->step_graph) (void)hipGraphExecDestroy(w->step_graph);
  if (w->step_graph_n) (void)hipGraphExecDestroy(w->step_graph_n);
  for (void* p : w->batch_allocs) (void)hipFree(p);
  for (void* p : w->allocs) (void)hipFree(p);
  if (w->ev_enc_begin) (void)hipEventDestroy(w->ev_enc_begin);
  if (w->ev_enc_end) (void)hipEventDestroy(w->ev_enc_end);
  if (w->win_dev) (void)hipFree(w->win_dev);
  if (w->win_host) (void)hipHostFree(w->win_host);
  if (w->ev_win) (void)hipEventDestroy(w->ev_win);
  if (w->trace) (void)hipFree(w->trace);
  if (w->trace_clips) (void)hipFree(w->trace_clips);
  if (w->parent) w->parent->n_clones -= 1;
  delete w;
}

// A second handle on the SAME weights with its own activations, KV caches, decode state and step graph, bound to another context
// (HIP stream) of the same device: batches decoded on different streams then stream one weight copy (the second reader mostly hits
// L2 / the Infinity Cache) instead of one copy each.
extern "C" mia_whisper* mia_whisper_clone(mia_whisper* src, mia_ctx* ctx) {
  if (!src || !ctx) return nullptr;
  mia_whisper* root = src->parent ? src->parent : src;
  if (ctx->device != root->ctx->device) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "whisper_clone: the context must be on the device that holds the weights"); return nullptr; }
  mia_whisper* w = new mia_whisper();
  w->ctx = ctx; w->dims = root->dims; w->dtype = root->dtype; w->kpad_conv1 = root->kpad_conv1;
  w->conv1 = root->conv1; w->conv2 = root->conv2; w->enc_pos = root->enc_pos; w->enc = root->enc; w->ln_post = root->ln_post;
  w->tok_emb = root->tok_emb; w->tok_emb_f = root->tok_emb_f; w->emb_c1 = root->emb_c1; w->emb_c2 = root->emb_c2; w->dec_pos = root->dec_pos; w->dec = root->dec; w->dec_ln = root->dec_ln;
  w->emb_qw = root->emb_qw; w->emb_qst = root->emb_qst; w->q_bits = root->q_bits; w->use_packed = src->use_packed;      // (LinearW::qw / qst came with w->dec)
  w->parent = root;
  root->n_clones += 1;
  return w;
}

// ---- MLX-affine 4- / 8-bit weights for the decode step (WhisperModel.swift:189-196: the reference's default engine loads Whisper in 4 bit,
// group 64, and multiplies packed).  tensors: `<p>.weight` (MIA_U32 codes [N][K * bits / 32]), `<p>.scales`, `<p>.biases` ([N][K / 64]; f16,
// bf16 or f32, one type for all) of every decoder matrix the step reads -- decoder.blocks.L.{attn.{query,key,value,out},
// cross_attn.{query,out}, mlp1, mlp2} and decoder.token_embedding.  Encoder tensors and cross_attn.{key,value} are ignored: they run at
// 1500 rows per clip in the encode call (MFMA-bound) on the 16-bit copy.  Nothing of the handle changes unless every matrix was repacked
// and uploaded.  A bad argument or tensor list is MIA_ERR_INVALID_ARGUMENT; a refused hipMalloc MIA_ERR_OUT_OF_MEMORY, a failed upload
// MIA_ERR_DEVICE.
extern "C" int mia_whisper_attach_quantized(mia_whisper* w, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits) {
  if (!w) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = w->ctx;
  MIA_CHECK_ARG(ctx, tensors && n_tensors > 0 && group_size == 64 && (bits == 4 || bits == 8), "whisper_attach_quantized: tensors required, group size 64, 4 or 8 bits");
  MIA_CHECK_ARG(ctx, !w->parent, "whisper_attach_quantized: this handle is a clone (attach to the handle that owns the weights, before cloning)");
  MIA_CHECK_ARG(ctx, w->n_clones == 0, "whisper_attach_quantized: %d clone(s) share these weights; attach before cloning", w->n_clones);
  MIA_CHECK_ARG(ctx, w->q_bits == 0, "whisper_attach_quantized: packed weights are already attached to this handle (load a fresh handle to replace them)");
  const int D = w->dims.n_text_state, V = w->dims.n_vocab;
  MIA_CHECK_ARG(ctx, D % 128 == 0, "whisper_attach_quantized: n_text_state must be a multiple of 128 (the packed kernels take 128-input blocks)");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  std::vector<void*> fresh;                      // joins w->allocs only when everything is in place
  TensorLoader T; T.allocs = &fresh;
  T.index(tensors, n_tensors);
  int sdt = -1;
  const float mag = w->dtype == MIA_F16 ? 1024.0f : 128.0f;
  struct QPair { uint32_t* qw = nullptr; float* qst = nullptr; };
  // parts stacked along N as the dense loader stacks them (Loader::linear)
  auto pack = [&](const std::vector<std::string>& parts, int N_each, int K, QPair& out) -> bool {
    std::vector<Q4Src> src(parts.size());
    std::vector<std::pair<int, int>> rows;
    for (size_t i = 0; i < parts.size(); ++i) {
      if (!q_find_linear(T, parts[i], N_each, K, bits, true, &sdt, src[i])) return false;
      for (int n = 0; n < N_each; ++n) rows.push_back({(int)i, n});
    }
    return q_upload(T, src, rows, K, bits, sdt, mag, &out.qw, &out.qst);
  };
  const int L = (int)w->dec.size();
  std::vector<QPair> qp((size_t)L * 6);
  QPair emb;
  bool ok = true;
  for (int l = 0; l < L && ok; ++l) {
    const std::string p = "decoder.blocks." + std::to_string(l);
    QPair* q = &qp[(size_t)l * 6];
    ok = pack({p + ".attn.query", p + ".attn.key", p + ".attn.value"}, D, D, q[0]) && pack({p + ".attn.out"}, D, D, q[1]) &&
         pack({p + ".cross_attn.query"}, D, D, q[2]) && pack({p + ".cross_attn.out"}, D, D, q[3]) &&
         pack({p + ".mlp1"}, 4 * D, D, q[4]) && pack({p + ".mlp2"}, D, 4 * D, q[5]);
  }
  ok = ok && pack({"decoder.token_embedding"}, V, D, emb);
  if (ok && hipDeviceSynchronize() != hipSuccess) ok = T.fail(MIA_ERR_DEVICE, "device error during upload");
  if (!ok) {
    for (void* p : fresh) (void)hipFree(p);
    return mia_fail(ctx, T.code, "whisper_attach_quantized: %s", T.err.c_str());
  }
  for (int l = 0; l < L; ++l) {
    DecBlockW& b = w->dec[l];
    LinearW* lw[6] = {&b.qkv, &b.out, &b.cq, &b.cout, &b.mlp1, &b.mlp2};
    for (int i = 0; i < 6; ++i) { lw[i]->qw = qp[(size_t)l * 6 + i].qw; lw[i]->qst = qp[(size_t)l * 6 + i].qst; }
  }
  w->emb_qw = emb.qw; w->emb_qst = emb.qst;
  w->allocs.insert(w->allocs.end(), fresh.begin(), fresh.end());
  w->q_bits = bits;
  return MIA_OK;
}

// The step's GEMMs read the packed weights (1) or the 16-bit copy (0, the default).  Packed loads take their cache policy from the same rule
// as the 16-bit ones (whisper_decode.hip: dec_cache_policy; q4 and q8 of large-v3-turbo fit the budget whole and are kept).  Takes effect at the next decode (the step graph is re-captured: DecodeParams::packed).
extern "C" int mia_whisper_use_packed(mia_whisper* w, int on) {
  if (!w) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(w->ctx, !on || w->q_bits != 0, "whisper_use_packed: no packed weights attached (mia_whisper_attach_quantized)");
  w->use_packed = on ? 1 : 0;
  return MIA_OK;
}
