// sensevoice.hip -- Fun-ASR's audio half as a model handle: the SenseVoice SANM encoder and the audio adaptor (FunASRModel.encodeAudio,
// STT/FunASR/FunASRModel.swift:41-58), on the Whisper encoder's arithmetic: Linear weights in the handle's 16-bit type, an fp32 residual
// stream, fp32 LayerNorm (eps 1e-5) emitting the 16-bit GEMM operand, GEMMs through mia_gemm_launch.
//
//   encoder (SenseVoiceEncoder.swift:98-135)   x = feats * sqrt(encoder_dim); encoders0 (1, 560 -> 512, no attention residual: inSize != size,
//                                              EncoderLayerSANM.swift:83-85), encoders, after_norm, tp_encoders, tp_norm
//   SANM layer (EncoderLayerSANM.swift:75-94)  norm1 -> q|k|v -> (attn128 -> linear_out) + fsmn_add -> + residual -> norm2 -> w_1 / ReLU -> w_2 + residual
//   adaptor (AudioAdaptor.swift:67-118)        zero rows up to a multiple of k per utterance, [T][D] seen as [ceil(T / k)][D k], linear1 / ReLU,
//                                              linear2, then pre-norm blocks of plain MHA (head dim 128) + ReLU ffn of llm_dim / 4
//
// Stacked utterances live in a padded [B][Tmax] row layout: every GEMM, norm and element-wise kernel runs over all B * Tmax rows at once,
// attention and FSMN read seq_len.  Every kernel on the path computes a row from that row's sequence alone and in an order that does not
// depend on B or Tmax -- which is why the GEMMs are pinned to ONE kernel (variant 1, the 128^2 LDS-DMA tile: the auto rule would switch
// tiles, and summation orders, with the row count) -- so utterance b's rows are those of its own B = 1 call bit for bit.  Padding rows hold
// arbitrary finite-or-not values that no valid row reads.  Layer 0's K = 560 is not a multiple of the GEMM's 64: the weight is zero-padded
// to 576 columns at load and norm1 writes into operand rows of 576 whose tail is zeroed.
#include "funasr_host.h"
#include "gemm.h"
#include "mia_device.h"
#include "ops.h"
#include "sensevoice.h"
#include "tensor_loader.h"

#include <cmath>

struct SvLinear { void* w = nullptr; float* b = nullptr; int N = 0, K = 0; };      // w 16-bit [N][K] (K padded to 64)
struct SvNorm { float* g = nullptr; float* b = nullptr; };
struct SvLayer {             // one EncoderLayerSANM, or one FunASREncoderLayer (fsmn == nullptr, qkv = linear_q | linear_k | linear_v)
  SvNorm norm1, norm2;
  SvLinear qkv, out, w1, w2;
  float* fsmn = nullptr;     // [K][D]
  int in_dim = 0;
};

struct mia_sensevoice {
  mia_ctx* ctx = nullptr;
  mia_sensevoice_config cfg{};
  int dtype = MIA_BF16;
  std::vector<void*> allocs;
  std::vector<SvLayer> enc;           // encoders0 + encoders + tp_encoders, in order
  SvNorm after_norm, tp_norm;
  SvLinear lin1, lin2;
  std::vector<SvLayer> blocks;
  // grow-only scratch (mia_grow): element counts
  float* fin = nullptr; size_t fin_cap = 0;        // fp32 [M][input_dim] scaled features, padded layout
  float* x = nullptr; size_t x_cap = 0;            // fp32 residual stream
  float* xb = nullptr; size_t xb_cap = 0;          // fp32: after_norm / tp_norm output
  uint16_t* h = nullptr; size_t h_cap = 0;         // 16-bit GEMM operand (norm output, adaptor input)
  uint16_t* qkv = nullptr; size_t qkv_cap = 0;
  uint16_t* att = nullptr; size_t att_cap = 0;
  uint16_t* g = nullptr; size_t g_cap = 0;         // ffn hidden
  int32_t* lens = nullptr; size_t lens_cap = 0;    // device [2][B]: t_lfr | n_out
  float* feats = nullptr; size_t feats_cap = 0;    // encode_audio: the front end's output
  char* fscratch = nullptr; size_t fscratch_cap = 0;
  float* stage = nullptr; size_t stage_cap = 0;    // host-memory calls: device copies of feats / pcm and of the outputs
};

namespace {

struct SvLoader : TensorLoader {
  int dtype = MIA_BF16;
  // Linear [N][K] + bias [N]; the weight's K is zero-padded to a multiple of 64
  bool linear(const std::string& n, SvLinear& l, int N, int K) {
    std::vector<float> w, b;
    if (!f32(n + ".weight", w, {N, K}) || !f32(n + ".bias", b, {N})) return false;
    const int Kp = (K + 63) / 64 * 64;
    if (Kp != K) {
      std::vector<float> wp((size_t)N * Kp, 0.f);
      for (int r = 0; r < N; ++r) memcpy(&wp[(size_t)r * Kp], &w[(size_t)r * K], (size_t)K * 4);
      w.swap(wp);
    }
    l.w = up16(w, dtype); l.b = up(b); l.N = N; l.K = Kp;
    return l.w && l.b;
  }
  // three Linears [D][D] stacked into one [3 D][D] (the adaptor's linear_q / linear_k / linear_v)
  bool linear3(const std::string& p, SvLinear& l, int D) {
    std::vector<float> w, b, wi, bi;
    for (const char* n : {"linear_q", "linear_k", "linear_v"}) {
      if (!f32(p + "." + n + ".weight", wi, {D, D}) || !f32(p + "." + n + ".bias", bi, {D})) return false;
      w.insert(w.end(), wi.begin(), wi.end()); b.insert(b.end(), bi.begin(), bi.end());
    }
    l.w = up16(w, dtype); l.b = up(b); l.N = 3 * D; l.K = D;
    return l.w && l.b;
  }
  bool norm(const std::string& n, SvNorm& ln, int D) {
    std::vector<float> g, b;
    if (!f32(n + ".weight", g, {D}) || !f32(n + ".bias", b, {D})) return false;
    ln.g = up(g); ln.b = up(b);
    return ln.g && ln.b;
  }
  // fsmn_block.weight: [D][1][K] (the checkpoint's torch Conv1d) or [D][K][1] (after FunASRModel.sanitize) -> [K][D]
  bool fsmn(const std::string& n, float*& out, int D, int K) {
    const mia_tensor_view* t = find(n);
    if (!t) return fail(MIA_ERR_INVALID_ARGUMENT, "missing tensor '" + n + "'");
    const bool shape_ok = t->dtype == MIA_F32 && t->ndim == 3 && t->shape[0] == D &&
                          ((t->shape[1] == 1 && t->shape[2] == K) || (t->shape[1] == K && t->shape[2] == 1));
    if (!shape_ok) return fail(MIA_ERR_INVALID_ARGUMENT, "tensor '" + n + "' must be float32 [D][1][K] or [D][K][1]");
    const float* src = (const float*)t->data;        // both layouts are [D][K] in memory
    std::vector<float> w((size_t)K * D);
    for (int d = 0; d < D; ++d)
      for (int k = 0; k < K; ++k) w[(size_t)k * D + d] = src[(size_t)d * K + k];
    out = up(w);
    return out != nullptr;
  }
};

bool load_sanm(SvLoader& L, const std::string& p, SvLayer& l, int in_dim, const mia_sensevoice_config& c) {
  const int D = c.encoder_dim;
  l.in_dim = in_dim;
  return L.norm(p + ".norm1", l.norm1, in_dim) && L.linear(p + ".self_attn.linear_q_k_v", l.qkv, 3 * D, in_dim) &&
         L.linear(p + ".self_attn.linear_out", l.out, D, D) && L.fsmn(p + ".self_attn.fsmn_block.weight", l.fsmn, D, c.kernel_size) &&
         L.norm(p + ".norm2", l.norm2, D) && L.linear(p + ".feed_forward.w_1", l.w1, c.ffn_dim, D) && L.linear(p + ".feed_forward.w_2", l.w2, D, c.ffn_dim);
}

int sv_gemm(mia_sensevoice* sv, GemmArgs g) {
  g.variant = 1;      // one kernel at every size (file header)
  if (const char* e = mia_gemm_check(g)) return mia_fail(sv->ctx, MIA_ERR_INVALID_ARGUMENT, "sensevoice: %s", e);
  const int rec = mia_prof_begin(sv->ctx, MIA_PROF_ENC_GEMM, 2.0 * g.M * (double)g.N * g.K);
  const int rc = mia_gemm_launch(g, sv->dtype, sv->ctx->stream);
  mia_prof_end(sv->ctx, rec);
  return rc ? mia_fail(sv->ctx, MIA_ERR_DEVICE, "sensevoice: gemm launch failed") : MIA_OK;
}

int sv_linear(mia_sensevoice* sv, const void* a, const SvLinear& l, int M, int act, const float* r, void* c, bool out_f32) {
  GemmArgs g;
  g.A = a; g.lda = l.K; g.W = l.w; g.bias = l.b; g.M = M; g.N = l.N; g.K = l.K; g.act = act;
  g.R = r; g.ldr = l.N; g.C = c; g.ldc = l.N; g.out_f32 = out_f32 ? 1 : 0;
  return sv_gemm(sv, g);
}

int sv_norm(mia_sensevoice* sv, const float* x, int D, const SvNorm& ln, void* y, int64_t ldy, int M, int out_dtype) {
  if (const char* e = mia_norm_check(M, D, D, ldy)) return mia_fail(sv->ctx, MIA_ERR_INVALID_ARGUMENT, "sensevoice: %s", e);
  const int rec = mia_prof_begin(sv->ctx, MIA_PROF_ENC_NORM, (double)M * D * (4.0 + mia_dtype_size(out_dtype)));
  const int rc = mia_norm_launch(x, D, ln.g, ln.b, y, ldy, M, D, 1e-5f, false, out_dtype, sv->ctx->stream);
  mia_prof_end(sv->ctx, rec);
  return rc ? mia_fail(sv->ctx, MIA_ERR_DEVICE, "sensevoice: norm launch failed") : MIA_OK;
}

int sv_attention(mia_sensevoice* sv, int B, int T, int H, const int32_t* seq_len) {
  const int D = H * 128;
  Attn128Args a;
  a.q = sv->qkv; a.k = sv->qkv + D; a.v = sv->qkv + 2 * D; a.ldq = a.ldk = a.ldv = 3 * D; a.out = sv->att; a.ldo = D;
  a.B = B; a.T = T; a.H = H; a.scale = 0.08838834764831845f; a.seq_len = seq_len; a.dtype = sv->dtype;       // 128^-0.5
  if (const char* e = mia_attn128_check(a)) return mia_fail(sv->ctx, MIA_ERR_INVALID_ARGUMENT, "sensevoice: %s", e);
  const int rec = mia_prof_begin(sv->ctx, MIA_PROF_ENC_ATTN, 4.0 * B * H * (double)T * T * 128);
  const int rc = mia_attn128_launch(a, sv->ctx->stream);
  mia_prof_end(sv->ctx, rec);
  return rc ? mia_fail(sv->ctx, MIA_ERR_DEVICE, "sensevoice: attention launch failed") : MIA_OK;
}

// ragged feats [sum T_b][ld_in] -> padded [B][T][D] * scale; padding rows zero
__global__ __launch_bounds__(256) void sv_pad_scale(const float* __restrict__ in, int64_t ld_in, const int32_t* __restrict__ lens, float* __restrict__ out,
                                                    int B, int T, int D, float scale) {
  const int b = blockIdx.y;
  int64_t row0 = 0;
  for (int i = 0; i < b; ++i) row0 += lens[i];
  const int Tb = lens[b];
  const int64_t total = (int64_t)T * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int t = (int)(e / D), c = (int)(e - (int64_t)t * D);
    out[((int64_t)b * T + t) * D + c] = t < Tb ? in[(row0 + t) * ld_in + c] * scale : 0.f;
  }
}

// encoder output, padded fp32 [B][T][D] -> the adaptor's operand [B][N k][D] in the 16-bit type, zero rows at and beyond a sequence's length
template <typename Tp>
__global__ __launch_bounds__(256) void sv_adaptor_in(const float* __restrict__ enc, const int32_t* __restrict__ lens, uint16_t* __restrict__ out,
                                                     int T, int Tk, int D) {
  const int b = blockIdx.y;
  const int Tb = lens[b];
  const int64_t total = (int64_t)Tk * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int t = (int)(e / D), c = (int)(e - (int64_t)t * D);
    out[((int64_t)b * Tk + t) * D + c] = t < Tb ? Tp::from_f32(enc[((int64_t)b * T + t) * D + c]) : (uint16_t)0;
  }
}

// padded fp32 [B][T][D] -> ragged [sum len_b][D]
__global__ __launch_bounds__(256) void sv_unpad(const float* __restrict__ in, const int32_t* __restrict__ lens, float* __restrict__ out, int T, int D) {
  const int b = blockIdx.y;
  int64_t row0 = 0;
  for (int i = 0; i < b; ++i) row0 += lens[i];
  const int64_t total = (int64_t)lens[b] * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256)
    out[row0 * D + e] = in[(int64_t)b * T * D + e];
}

inline unsigned grid_for(int64_t total) { return (unsigned)std::min<int64_t>((total + 255) / 256, 2048); }

// feats_dev: ragged fp32 [sum t_lfr][ld_feats] on the device; enc_dev (nullable) / emb_dev: ragged device outputs
int sv_encode_device(mia_sensevoice* sv, const float* feats_dev, int64_t ld_feats, const int32_t* t_lfr, int B, float* enc_dev, float* emb_dev, int32_t* n_out) {
  mia_ctx* ctx = sv->ctx;
  const mia_sensevoice_config& c = sv->cfg;
  hipStream_t s = ctx->stream;
  const int D = c.encoder_dim, F = c.ffn_dim, IN = c.input_dim, INP = (IN + 63) / 64 * 64, k = c.adaptor_k, L = c.llm_dim;
  const int FA = std::max(c.adaptor_ffn_dim, L / 4);
  int T = 0;
  std::vector<int32_t> lens(2 * (size_t)B);
  for (int b = 0; b < B; ++b) {
    MIA_CHECK_ARG(ctx, t_lfr[b] > 0, "sensevoice_encode: utterance %d has %d feature rows", b, t_lfr[b]);
    lens[b] = t_lfr[b];
    lens[B + b] = n_out[b] = (t_lfr[b] - 1) / k + 1;
    T = std::max(T, t_lfr[b]);
  }
  const int N = (T - 1) / k + 1, Tk = N * k;
  MIA_CHECK_ARG(ctx, (int64_t)B * Tk < (1ll << 30), "sensevoice_encode: too many rows");
  const size_t M = (size_t)B * T, Ma = (size_t)B * N;
  int rc;
  if ((rc = mia_grow(ctx, sv->fin, sv->fin_cap, M * IN, "sensevoice: out of memory")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, sv->x, sv->x_cap, std::max(M * D, Ma * L), "sensevoice: out of memory")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, sv->xb, sv->xb_cap, std::max(M * D, Ma * L), "sensevoice: out of memory")) != MIA_OK) return rc;   // x and xb trade places
  if ((rc = mia_grow(ctx, sv->h, sv->h_cap, std::max({M * (size_t)INP, M * (size_t)D, (size_t)B * Tk * D, Ma * (size_t)L}), "sensevoice: out of memory")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, sv->qkv, sv->qkv_cap, std::max(M * 3 * D, Ma * 3 * L), "sensevoice: out of memory")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, sv->att, sv->att_cap, std::max(M * D, Ma * L), "sensevoice: out of memory")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, sv->g, sv->g_cap, std::max(M * F, Ma * (size_t)FA), "sensevoice: out of memory")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, sv->lens, sv->lens_cap, 2 * (size_t)B, "sensevoice: out of memory")) != MIA_OK) return rc;
  HostIo io = HostIo::device(ctx);                     // lens[] lives on this call's stack: no return before its upload has been read
  const int32_t* d_T = io.table(lens.data(), sv->lens, lens.size() * 4);
  const int32_t* d_N = sv->lens + B;

  // ---- encoder
  hipLaunchKernelGGL(sv_pad_scale, dim3(grid_for((int64_t)T * IN), (unsigned)B), dim3(256), 0, s, feats_dev, ld_feats, d_T, sv->fin, B, T, IN, sqrtf((float)D));
  if (INP != IN) MIA_HIP(ctx, hipMemsetAsync(sv->h, 0, M * INP * 2, s));     // the operand tail of layer 0: columns IN .. INP - 1 stay zero
  const int left = funasr::fsmn_left(c.kernel_size, c.sanm_shift);
  const int n_main = c.n_encoders0 + c.n_encoders;
  for (size_t l = 0; l < sv->enc.size(); ++l) {
    const SvLayer& ly = sv->enc[l];
    const bool first = ly.in_dim != D;                 // inSize != size: no attention residual
    if ((int)l == n_main) {                            // after_norm sits between the two stacks
      if ((rc = sv_norm(sv, sv->x, D, sv->after_norm, sv->xb, D, (int)M, MIA_F32)) != MIA_OK) return rc;
      std::swap(sv->x, sv->xb); std::swap(sv->x_cap, sv->xb_cap);
    }
    if ((rc = sv_norm(sv, first ? sv->fin : sv->x, ly.in_dim, ly.norm1, sv->h, ly.qkv.K, (int)M, sv->dtype)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->h, ly.qkv, (int)M, MIA_ACT_NONE, nullptr, sv->qkv, false)) != MIA_OK) return rc;
    if ((rc = sv_attention(sv, B, T, c.n_heads, d_T)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->att, ly.out, (int)M, MIA_ACT_NONE, first ? nullptr : sv->x, sv->x, true)) != MIA_OK) return rc;
    {
      FsmnArgs a;
      a.x = sv->x; a.ldx = D; a.v = sv->qkv + 2 * D; a.ldv = 3 * D; a.w = ly.fsmn; a.B = B; a.T = T; a.D = D; a.K = c.kernel_size; a.left = left;
      a.seq_len = d_T; a.dtype = sv->dtype;
      if (const char* e = mia_fsmn_check(a)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "sensevoice: %s", e);
      const int rec = mia_prof_begin(ctx, MIA_PROF_FSMN, (double)M * D * (8.0 + 2.0 * (c.kernel_size + 1)));
      const int frc = mia_fsmn_launch(a, s);
      mia_prof_end(ctx, rec);
      if (frc) return mia_fail(ctx, MIA_ERR_DEVICE, "sensevoice: fsmn launch failed");
    }
    if ((rc = sv_norm(sv, sv->x, D, ly.norm2, sv->h, D, (int)M, sv->dtype)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->h, ly.w1, (int)M, MIA_ACT_RELU, nullptr, sv->g, false)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->g, ly.w2, (int)M, MIA_ACT_NONE, sv->x, sv->x, true)) != MIA_OK) return rc;
  }
  if ((int)sv->enc.size() == n_main) {                 // no tp_encoders: after_norm still runs
    if ((rc = sv_norm(sv, sv->x, D, sv->after_norm, sv->xb, D, (int)M, MIA_F32)) != MIA_OK) return rc;
    std::swap(sv->x, sv->xb); std::swap(sv->x_cap, sv->xb_cap);
  }
  if ((rc = sv_norm(sv, sv->x, D, sv->tp_norm, sv->xb, D, (int)M, MIA_F32)) != MIA_OK) return rc;
  if (enc_dev) hipLaunchKernelGGL(sv_unpad, dim3(grid_for((int64_t)T * D), (unsigned)B), dim3(256), 0, s, sv->xb, d_T, enc_dev, T, D);

  // ---- adaptor: rows [B][N], operand [B * N][D k]
  if (sv->dtype == MIA_F16) hipLaunchKernelGGL(sv_adaptor_in<F16>, dim3(grid_for((int64_t)Tk * D), (unsigned)B), dim3(256), 0, s, sv->xb, d_T, sv->h, T, Tk, D);
  else hipLaunchKernelGGL(sv_adaptor_in<BF16>, dim3(grid_for((int64_t)Tk * D), (unsigned)B), dim3(256), 0, s, sv->xb, d_T, sv->h, T, Tk, D);
  if ((rc = sv_linear(sv, sv->h, sv->lin1, (int)Ma, MIA_ACT_RELU, nullptr, sv->g, false)) != MIA_OK) return rc;
  if ((rc = sv_linear(sv, sv->g, sv->lin2, (int)Ma, MIA_ACT_NONE, nullptr, sv->x, true)) != MIA_OK) return rc;
  for (const SvLayer& ly : sv->blocks) {                // FunASREncoderLayer (EncoderLayerSANM.swift:144-158)
    if ((rc = sv_norm(sv, sv->x, L, ly.norm1, sv->h, L, (int)Ma, sv->dtype)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->h, ly.qkv, (int)Ma, MIA_ACT_NONE, nullptr, sv->qkv, false)) != MIA_OK) return rc;
    if ((rc = sv_attention(sv, B, N, c.adaptor_heads, d_N)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->att, ly.out, (int)Ma, MIA_ACT_NONE, sv->x, sv->x, true)) != MIA_OK) return rc;
    if ((rc = sv_norm(sv, sv->x, L, ly.norm2, sv->h, L, (int)Ma, sv->dtype)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->h, ly.w1, (int)Ma, MIA_ACT_RELU, nullptr, sv->g, false)) != MIA_OK) return rc;
    if ((rc = sv_linear(sv, sv->g, ly.w2, (int)Ma, MIA_ACT_NONE, sv->x, sv->x, true)) != MIA_OK) return rc;
  }
  hipLaunchKernelGGL(sv_unpad, dim3(grid_for((int64_t)N * L), (unsigned)B), dim3(256), 0, s, sv->x, d_N, emb_dev, N, L);
  MIA_HIP(ctx, hipGetLastError());
  return io.finish();
}

}  // namespace

extern "C" mia_sensevoice* mia_sensevoice_load(mia_ctx* ctx, const mia_sensevoice_config* cfg, const mia_tensor_view* tensors, int n_tensors, int dtype) {
  if (!ctx) return nullptr;
  if (!cfg || !tensors || n_tensors <= 0) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "sensevoice_load: null argument"); return nullptr; }
  if (dtype != MIA_BF16 && dtype != MIA_F16) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "sensevoice_load: dtype must be MIA_BF16 or MIA_F16"); return nullptr; }
  if (const char* e = funasr::config_check(*cfg)) { mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "sensevoice_load: %s", e); return nullptr; }
  if (hipSetDevice(ctx->device) != hipSuccess) { mia_fail(ctx, MIA_ERR_DEVICE, "sensevoice_load: hipSetDevice failed"); return nullptr; }
  mia_sensevoice* sv = new mia_sensevoice();
  sv->ctx = ctx; sv->cfg = *cfg; sv->dtype = dtype;
  const mia_sensevoice_config& c = sv->cfg;
  SvLoader L;
  L.allocs = &sv->allocs; L.dtype = dtype;
  L.index(tensors, n_tensors);
  bool ok = true;
  const int D = c.encoder_dim, LL = c.llm_dim;
  struct { const char* name; int n; } stacks[3] = {{"encoders0", c.n_encoders0}, {"encoders", c.n_encoders}, {"tp_encoders", c.n_tp_encoders}};
  for (int st = 0; st < 3 && ok; ++st)
    for (int i = 0; i < stacks[st].n && ok; ++i) {
      sv->enc.emplace_back();
      ok = load_sanm(L, std::string("audio_encoder.") + stacks[st].name + "." + std::to_string(i), sv->enc.back(), st == 0 && i == 0 ? c.input_dim : D, c);
    }
  ok = ok && L.norm("audio_encoder.after_norm", sv->after_norm, D) && L.norm("audio_encoder.tp_norm", sv->tp_norm, D);
  ok = ok && L.linear("audio_adaptor.linear1", sv->lin1, c.adaptor_ffn_dim, D * c.adaptor_k) && L.linear("audio_adaptor.linear2", sv->lin2, LL, c.adaptor_ffn_dim);
  for (int i = 0; i < c.adaptor_layers && ok; ++i) {
    sv->blocks.emplace_back();
    SvLayer& b = sv->blocks.back();
    const std::string p = "audio_adaptor.blocks." + std::to_string(i);
    b.in_dim = LL;
    ok = L.norm(p + ".norm1", b.norm1, LL) && L.linear3(p + ".self_attn", b.qkv, LL) && L.linear(p + ".self_attn.linear_out", b.out, LL, LL) &&
         L.norm(p + ".norm2", b.norm2, LL) && L.linear(p + ".feed_forward.w_1", b.w1, LL / 4, LL) && L.linear(p + ".feed_forward.w_2", b.w2, LL, LL / 4);
  }
  if (!ok || !L.err.empty()) {
    mia_fail(ctx, L.err.empty() ? MIA_ERR_INVALID_ARGUMENT : L.code, "sensevoice_load: %s", L.err.empty() ? "load failed" : L.err.c_str());
    mia_sensevoice_free(sv);
    return nullptr;
  }
  return sv;
}

extern "C" void mia_sensevoice_free(mia_sensevoice* sv) {
  if (!sv) return;
  (void)hipSetDevice(sv->ctx->device);
  (void)hipStreamSynchronize(sv->ctx->stream);
  for (void* p : sv->allocs) (void)hipFree(p);
  for (void* p : {(void*)sv->fin, (void*)sv->x, (void*)sv->xb, (void*)sv->h, (void*)sv->qkv, (void*)sv->att, (void*)sv->g, (void*)sv->lens,
                  (void*)sv->feats, (void*)sv->fscratch, (void*)sv->stage})
    if (p) (void)hipFree(p);
  delete sv;
}

extern "C" int mia_sensevoice_encode(mia_sensevoice* sv, const float* feats, const int32_t* t_lfr, int B, float* enc_out, float* emb_out, int32_t* n_out, int mem) {
  if (!sv) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = sv->ctx;
  MIA_CHECK_ARG(ctx, feats && t_lfr && emb_out && n_out && B > 0, "sensevoice_encode: null pointer or B <= 0");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "sensevoice_encode: bad mem");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io(ctx, mem);
  if (!io.host()) return sv_encode_device(sv, feats, sv->cfg.input_dim, t_lfr, B, enc_out, emb_out, n_out);
  const mia_sensevoice_config& c = sv->cfg;
  size_t rows = 0, rows_out = 0;
  for (int b = 0; b < B; ++b) {
    MIA_CHECK_ARG(ctx, t_lfr[b] > 0, "sensevoice_encode: utterance %d has %d feature rows", b, t_lfr[b]);
    rows += (size_t)t_lfr[b]; rows_out += (size_t)((t_lfr[b] - 1) / c.adaptor_k + 1);
  }
  const size_t n_f = rows * c.input_dim, n_e = rows * c.encoder_dim, n_o = rows_out * c.llm_dim;
  int rc = mia_grow(ctx, sv->stage, sv->stage_cap, n_f + n_e + n_o, "sensevoice: out of memory");
  if (rc != MIA_OK) return rc;
  const float* d_f = io.in(feats, sv->stage, n_f * 4);
  float* d_e = io.out(enc_out, sv->stage + n_f, n_e * 4);
  float* d_o = io.out(emb_out, sv->stage + n_f + n_e, n_o * 4);
  if ((rc = sv_encode_device(sv, d_f, c.input_dim, t_lfr, B, d_e, d_o, n_out)) != MIA_OK) return rc;
  return io.finish();
}

extern "C" int mia_sensevoice_encode_audio(mia_sensevoice* sv, const float* pcm, const int64_t* offs, int B, float* emb_out, int32_t* n_out, int mem) {
  if (!sv) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = sv->ctx;
  MIA_CHECK_ARG(ctx, pcm && offs && emb_out && n_out && B > 0, "sensevoice_encode_audio: null pointer or B <= 0");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "sensevoice_encode_audio: bad mem");
  MIA_CHECK_ARG(ctx, sv->cfg.input_dim == funasr::NMEL * funasr::LFR_M, "sensevoice_encode_audio: the front end emits %d columns, input_dim is %d",
                funasr::NMEL * funasr::LFR_M, sv->cfg.input_dim);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  FunasrPlan plan;
  int rc = funasr_plan(ctx, offs, B, plan);
  if (rc != MIA_OK) return rc;
  const mia_sensevoice_config& c = sv->cfg;
  size_t rows_out = 0;
  for (int b = 0; b < B; ++b) rows_out += (size_t)((plan.t_lfr[b] - 1) / c.adaptor_k + 1);
  if ((rc = mia_grow(ctx, sv->feats, sv->feats_cap, (size_t)plan.rows * c.input_dim, "sensevoice: out of memory")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, sv->fscratch, sv->fscratch_cap, funasr_scratch_bytes(plan), "sensevoice: out of memory")) != MIA_OK) return rc;
  HostIo io(ctx, mem);
  const size_t n_p = (size_t)offs[B], n_o = rows_out * c.llm_dim;
  if ((rc = mia_grow(ctx, sv->stage, sv->stage_cap, io.staged(n_p + n_o), "sensevoice: out of memory")) != MIA_OK) return rc;
  const float* d_pcm = io.in(pcm, sv->stage, n_p * 4);
  float* d_o = io.out(emb_out, io.host() ? sv->stage + n_p : nullptr, n_o * 4);
  if ((rc = funasr_features_device(ctx, d_pcm, offs, plan, sv->feats, c.input_dim, sv->fscratch)) != MIA_OK) return rc;
  if ((rc = sv_encode_device(sv, sv->feats, c.input_dim, plan.t_lfr.data(), B, nullptr, d_o, n_out)) != MIA_OK) return rc;
  return io.finish();
}
