// ops_abi.hip -- operator-level C ABI entry points (include/mia.h "operator level").
#include "gemm.h"
#include "mia_internal.h"
#include "ops.h"

extern "C" int mia_op_linear(mia_ctx* ctx, const void* x, int64_t lda, const void* w, const float* bias, const float* r, int64_t ldr,
                             void* y, int64_t ldy, int M, int N, int K, int act, int dtype, int out_f32, int variant, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, x && w && y, "op_linear: null pointer");
  MIA_CHECK_ARG(ctx, dtype == MIA_BF16 || dtype == MIA_F16, "op_linear: dtype must be MIA_BF16 or MIA_F16");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "op_linear: bad mem");
  MIA_CHECK_ARG(ctx, M > 0 && N > 0 && K > 0 && lda >= K && ldy >= N && (!r || ldr >= N), "op_linear: bad shape");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io(ctx, mem);
  GemmArgs g;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldy; g.ldr = ldr; g.act = act; g.out_f32 = out_f32 ? 1 : 0; g.variant = variant;
  const size_t xb = (size_t)M * lda * 2, wb = (size_t)N * K * 2, yb = (size_t)M * ldy * (out_f32 ? 4 : 2);
  const size_t bb = bias ? (size_t)N * 4 : 0, rb = r ? (size_t)M * ldr * 4 : 0;
  Carve cv;
  const size_t o_x = cv.add(io.staged(xb)), o_w = cv.add(io.staged(wb)), o_y = cv.add(io.staged(yb)), o_b = cv.add(io.staged(bb)), o_r = cv.add(io.staged(rb));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  g.A = io.in(x, ws + o_x, xb); g.W = io.in(w, ws + o_w, wb); g.bias = io.in(bias, ws + o_b, bb); g.R = io.in(r, ws + o_r, rb);
  g.C = io.out(y, ws + o_y, yb);
  if (const char* e = mia_gemm_check(g)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
  if (mia_gemm_launch(g, dtype, ctx->stream) != 0) return mia_fail(ctx, MIA_ERR_DEVICE, "op_linear: launch failed");
  return io.finish();
}

// mia_op_linear with the two special store layouts of gemm.hip (test hook): epi 1 = MIA_EPI_QKV_VT (q|k rows into y, V transposed per head
// into vt), epi 2 = MIA_EPI_HEADMAJOR (y [B][H][T][64]).  mia_gemm_check is the gatekeeper; what it leaves to the model in front of it -- that
// m = b*T + t covers whole clips and that the row stride covers the q|k row, i.e. that every store lands inside y / vt -- is checked here.
extern "C" int mia_op_linear_epi(mia_ctx* ctx, const void* x, int64_t lda, const void* w, const float* bias, void* y, int64_t ldy, void* vt, int M,
                                 int N, int K, int epi, int T, int H, int Tpad, int batch, int dtype, int out_f32, int variant, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, x && w && y && (vt || epi != MIA_EPI_QKV_VT), "op_linear_epi: null pointer");
  MIA_CHECK_ARG(ctx, dtype == MIA_BF16 || dtype == MIA_F16, "op_linear_epi: dtype must be MIA_BF16 or MIA_F16");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "op_linear_epi: bad mem");
  HostIo io(ctx, mem);
  MIA_CHECK_ARG(ctx, epi == MIA_EPI_QKV_VT || epi == MIA_EPI_HEADMAJOR, "op_linear_epi: epi must be 1 (QKV_VT) or 2 (HEADMAJOR)");
  MIA_CHECK_ARG(ctx, variant >= 0 && variant <= 4, "op_linear_epi: variant must be 0 .. 4");
  MIA_CHECK_ARG(ctx, M > 0 && N > 0 && K > 0 && T > 0 && H > 0 && lda >= K, "op_linear_epi: bad shape");
  MIA_CHECK_ARG(ctx, M % T == 0, "op_linear_epi: M must be B * T");
  const int64_t B = M / T, D2 = 2 * (int64_t)H * 64;
  if (epi == MIA_EPI_QKV_VT) {
    MIA_CHECK_ARG(ctx, ldy >= D2, "op_linear_epi: ldy must cover the q|k row (2 * H * 64)");
    MIA_CHECK_ARG(ctx, Tpad >= T, "op_linear_epi: Tpad must be >= T");
    MIA_CHECK_ARG(ctx, (((uintptr_t)y | (uintptr_t)vt) & 7) == 0 || io.host(), "op_linear_epi: y and vt must be 8-byte aligned");
  } else {
    MIA_CHECK_ARG(ctx, ((uintptr_t)y & 7) == 0 || io.host(), "op_linear_epi: y must be 8-byte aligned");
  }
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  GemmArgs g;
  g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldc = ldy; g.out_f32 = out_f32 ? 1 : 0; g.variant = variant; g.batch = batch;
  g.epi = epi; g.T = T; g.H = H; g.Tpad = Tpad;
  const size_t xb = (size_t)M * lda * 2, wb = (size_t)N * K * 2, bb = bias ? (size_t)N * 4 : 0;
  const size_t yb = epi == MIA_EPI_QKV_VT ? (size_t)(((int64_t)M - 1) * ldy + D2) * 2 : (size_t)B * H * T * 64 * 2;
  const size_t vb = epi == MIA_EPI_QKV_VT ? (size_t)B * H * 64 * Tpad * 2 : 0;
  Carve cv;
  const size_t o_x = cv.add(io.staged(xb)), o_w = cv.add(io.staged(wb)), o_y = cv.add(io.staged(yb)), o_v = cv.add(io.staged(vb)), o_b = cv.add(io.staged(bb));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  auto place = [&](const void* p, size_t off) -> void* { return p && io.host() ? ws + off : const_cast<void*>(p); };    // where in / inout will put it
  g.A = place(x, o_x); g.W = place(w, o_w); g.C = place(y, o_y); g.C2 = vb ? place(vt, o_v) : (io.host() ? nullptr : vt); g.bias = (const float*)place(bias, o_b);
  if (const char* e = mia_gemm_check(g)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);     // before anything is copied or launched
  io.in(x, ws + o_x, xb); io.in(w, ws + o_w, wb); io.in(bias, ws + o_b, bb);
  io.inout(y, ws + o_y, yb);                                                                          // untouched bytes survive the round trip
  if (vb) io.inout(vt, ws + o_v, vb);
  if (mia_gemm_launch(g, dtype, ctx->stream) != 0) return mia_fail(ctx, MIA_ERR_DEVICE, "op_linear_epi: launch failed");
  return io.finish();
}

// The Whisper encoder's attention (attention.hip) in its native layout (test hook): qk [B*T][ld_qk] with q of head h in columns h*64.. and k
// in columns H*64 + h*64.., vt [B][H][64][Tpad] (what MIA_EPI_QKV_VT stores), out [B*T][ld_out].  mia_enc_attention_check covers what the
// kernel's loads need; the sizes a model guarantees by construction (strides that cover the row, a 32-bit row count) are checked here.
// variant: one of attention.hip's kernel forms (ops.h MIA_ATT_*), or -1 for the form the encoder itself launches at this shape
static int op_attention_h64(mia_ctx* ctx, const void* qk, int64_t ld_qk, const void* vt, void* out, int64_t ld_out, int B, int T, int H,
                            int Tpad, int dtype, int variant, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, variant >= -1 && variant < MIA_ATT_NVARIANTS, "op_attention_h64: unknown kernel variant");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "op_attention_h64: bad mem");
  HostIo io(ctx, mem);
  MIA_CHECK_ARG(ctx, qk && vt && out, "op_attention_h64: null pointer");
  MIA_CHECK_ARG(ctx, dtype == MIA_BF16 || dtype == MIA_F16, "op_attention_h64: dtype must be MIA_BF16 or MIA_F16");
  if (const char* e = mia_enc_attention_check(B, T, H, Tpad, ld_qk, ld_out)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
  const int64_t rows = (int64_t)B * T, D = (int64_t)H * 64;
  MIA_CHECK_ARG(ctx, rows < (1ll << 31) && (int64_t)B * H * ((T + 127) / 128) < (1ll << 31), "op_attention_h64: B * T must stay below 2^31");
  MIA_CHECK_ARG(ctx, ld_qk >= 2 * D && ld_out >= D, "op_attention_h64: row strides must cover the row (ld_qk >= 2 * H * 64, ld_out >= H * 64)");
  MIA_CHECK_ARG(ctx, io.host() || ((((uintptr_t)qk | (uintptr_t)vt) & 15) == 0 && ((uintptr_t)out & 7) == 0),
                "op_attention_h64: qk and vt must be 16-byte aligned, out 8-byte aligned");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const size_t qb = (size_t)((rows - 1) * ld_qk + 2 * D) * 2, vb = (size_t)B * H * 64 * Tpad * 2, ob = (size_t)((rows - 1) * ld_out + D) * 2;
  Carve cv;
  const size_t o_q = cv.add(io.staged(qb)), o_v = cv.add(io.staged(vb)), o_o = cv.add(io.staged(ob));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  void* d_out = io.inout(out, ws + o_o, ob);                                                  // unwritten elements keep the caller's bytes
  const void* d_qk = io.in(qk, ws + o_q, qb); const void* d_vt = io.in(vt, ws + o_v, vb);
  if (variant < 0 ? mia_enc_attention_launch(d_qk, ld_qk, d_vt, d_out, ld_out, B, T, H, Tpad, dtype, ctx->stream)
                  : mia_enc_attention_launch_variant(d_qk, ld_qk, d_vt, d_out, ld_out, B, T, H, Tpad, dtype, variant, ctx->stream))
    return mia_fail(ctx, MIA_ERR_DEVICE, "op_attention_h64: launch failed");
  return io.finish();
}
extern "C" int mia_op_attention_h64(mia_ctx* ctx, const void* qk, int64_t ld_qk, const void* vt, void* out, int64_t ld_out, int B, int T, int H,
                                    int Tpad, int dtype, int mem) {
  return op_attention_h64(ctx, qk, ld_qk, vt, out, ld_out, B, T, H, Tpad, dtype, -1, mem);
}
extern "C" int mia_op_attention_h64_variant(mia_ctx* ctx, const void* qk, int64_t ld_qk, const void* vt, void* out, int64_t ld_out, int B, int T,
                                            int H, int Tpad, int dtype, int variant, int mem) {
  return op_attention_h64(ctx, qk, ld_qk, vt, out, ld_out, B, T, H, Tpad, dtype, variant, mem);
}

// fp32 Conv1d / Linear on the exact-fp32 matrix cores (device pointers only): y[t][n] = act(b[n] + sum_{k,c} x[t*stride + k*dil - pad][c] w[n][k][c]) (+ r)
#include "codec.h"
// what the public fp32 GEMM entry points add to codec_conv_gemm_check: the kernel clamps row offsets, so its loads and stores stay inside
// X / Y / R only when a row holds all Cin channels / N columns, and a public caller has no layer program in front of it that guarantees so
static const char* conv_gemm_abi_check(const ConvGemmArgs& g, int phases) {
  if (!g.X || !g.W || !g.Y) return "null pointer";
  if (phases <= 0 || g.T_in <= 0 || g.T_out <= 0 || g.dil <= 0 || g.x_row_mul <= 0) return "bad argument";
  if (g.ldx < g.Cin || g.ldy < g.N || ((g.R || g.R2) && g.ldr < g.N)) return "row strides must cover the row";
  if (g.gelu < 0 || g.gelu > 6) return "unknown activation";
  return nullptr;
}

extern "C" int mia_op_conv1d_f32(mia_ctx* ctx, const float* x, int64_t ldx, int T_in, const float* w, const float* bias, const float* r, float* y,
                                 int64_t ldy, int T_out, int N, int Cin, int taps, int stride, int dil, int pad, int act) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, x && w && y && T_in > 0 && T_out > 0 && N > 0 && taps > 0 && stride > 0 && dil > 0, "op_conv1d_f32: bad argument");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  ConvGemmArgs g;
  g.X = x; g.ldx = ldx; g.T_in = T_in; g.W = w; g.bias = bias; g.Y = y; g.ldy = ldy; g.T_out = T_out; g.R = r; g.ldr = ldy;
  g.M = T_out; g.N = N; g.Cin = Cin; g.taps = taps; g.dil = dil; g.pad = pad; g.x_row_mul = stride; g.gelu = act;
  if (const char* e = conv_gemm_abi_check(g, 1)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_conv1d_f32: %s", e);
  if (const char* e = codec_conv_gemm_check(g)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
  if (codec_conv_gemm_launch(g, 1, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_conv1d_f32: launch failed");
  return MIA_OK;
}

// the tap GEMM with every launch argument exposed (test hook; the formula is at the top of codec.h and in include/mia.h)
extern "C" int mia_op_conv_gemm_f32(mia_ctx* ctx, const mia_conv_gemm_desc* d, int phases) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, d, "op_conv_gemm_f32: null descriptor");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  ConvGemmArgs g;
  g.X = d->X; g.ldx = d->ldx; g.T_in = d->T_in; g.W = d->W; g.ldw = d->ldw; g.w_phase_stride = d->w_phase_stride; g.bias = d->bias;
  g.alpha = d->alpha; g.ralpha = d->ralpha; g.lrelu_slope = d->lrelu_slope; g.Y = d->Y; g.ldy = d->ldy; g.T_out = d->T_out;
  g.y_row_mul = d->y_row_mul; g.y_row_off = d->y_row_off; g.y_phase_step = d->y_phase_step; g.R = d->R; g.R2 = d->R2; g.ldr = d->ldr;
  g.noise = d->noise; g.out_scale = d->out_scale; g.M = d->M; g.N = d->N; g.Cin = d->Cin; g.taps = d->taps; g.dil = d->dil; g.pad = d->pad;
  g.x_row_mul = d->x_row_mul; g.gelu = d->act; g.tanh_out = d->tanh_out; g.phase_len = d->phase_len; g.x_phase_step = d->x_phase_step;
  g.n_seq = d->n_seq; g.x_seq_step = d->x_seq_step; g.y_seq_step = d->y_seq_step; g.seq_len = d->seq_len; g.noise_seq_off = d->noise_seq_off;
  if (const char* e = conv_gemm_abi_check(g, phases)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_conv_gemm_f32: %s", e);
  return codec_conv_gemm_run(ctx, g, phases, "op_conv_gemm_f32");
}

// The LM step's skinny GEMMs with every launch argument exposed (test hook; formulas in skinny.h and include/mia.h).  The launchers'
// own checks cover what lm.hip cannot get wrong by construction; a public caller has no model in front of it, so the sizes, strides,
// pointers and alignments the kernels rely on are checked here.
#include "skinny.h"
static const char* skinny_abi_check(const mia_skinny_desc& d) {
  if (d.dtype != MIA_BF16 && d.dtype != MIA_F16) return "dtype must be MIA_BF16 or MIA_F16";
  if (d.mode != SK_OUTF32 && d.mode != SK_PARTIAL && d.mode != SK_SWIGLU && d.mode != SK_RESID) return "mode must be 1 (OUTF32), 2 (PARTIAL), 4 (SWIGLU) or 5 (RESID)";
  if (!d.A || !d.out) return "null pointer";
  if (d.wfrag ? !d.stfrag : !d.W) return "null weights";
  if (d.lda < d.K) return "lda must cover the row";
  if (d.mode != SK_PARTIAL && d.S != 1) return "only PARTIAL takes S > 1";      // the other epilogues own their output: one K slice only
  if ((d.mode == SK_OUTF32 || d.mode == SK_RESID) && d.ldo < d.N) return "ldo must cover the row";
  if (d.mode == SK_SWIGLU && d.ldo < d.N / 2) return "ldo must cover the row";
  if (d.mode == SK_RESID && (!d.xres || !d.nw || !d.ss_out)) return "RESID needs xres, nw and ss_out";
  if (d.M_cap < 0) return "bad M_cap";
  auto misaligned = [](const void* p) { return ((uintptr_t)p & 15) != 0; };
  if (misaligned(d.A) || misaligned(d.W) || misaligned(d.wfrag) || misaligned(d.stfrag) || misaligned(d.out) || misaligned(d.xres) || misaligned(d.nw) ||
      (d.mode == SK_RESID && misaligned(d.bias)))
    return "operands must be 16-byte aligned";
  // (non-positive sizes and what the kernels hold in 32 bits -- operands of 4 GiB or more -- are refused by the launchers themselves)
  return nullptr;
}

extern "C" int mia_op_skinny_gemm(mia_ctx* ctx, const mia_skinny_desc* d) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, d, "op_skinny_gemm: null descriptor");
  if (const char* e = skinny_abi_check(*d)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_skinny_gemm: %s", e);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  SkinnyArgs a{(const uint16_t*)d->A, d->lda, (const uint16_t*)d->W, d->bias, d->out, d->ldo, nullptr, nullptr, nullptr, d->M, d->N, d->K, d->S, MIA_ACT_NONE, 0, 0, 0};
  a.xres = d->xres; a.nw = d->nw; a.ss_out = d->ss_out;
  a.ss_in = d->ss_in; a.ss_tiles = d->ss_tiles; a.ss_dim = d->ss_dim; a.eps = d->eps; a.rs_scale = d->rs_scale;
  int rc;
  if (d->wfrag) rc = skinny_gemm_q_launch(a, d->wfrag, d->stfrag, d->bits, d->mode, d->dtype, ctx->stream, d->M_cap);
  else {
    if (d->w_frag) {
      // (before the repack allocates and launches anything: what the launcher would refuse afterwards)
      MIA_CHECK_ARG(ctx, d->N > 0 && d->K > 0 && d->K % 32 == 0 && ((uint64_t)d->N + 15) / 16 * 16 * (uint64_t)d->K * 2 <= 0xffffffffull,
                    "op_skinny_gemm: N, K must be positive, K a multiple of 32, W below 4 GiB");
      void* wf = mia_workspace(ctx, (size_t)((d->N + 15) / 16) * 16 * d->K * 2);
      if (!wf) return MIA_ERR_OUT_OF_MEMORY;
      if (dec_launch_repack_wfrag(d->W, wf, d->N, d->K, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_skinny_gemm: fragment repack failed");
      a.W = (const uint16_t*)wf; a.w_frag = 1;
    }
    rc = skinny_gemm_launch(a, d->mode, d->dtype, ctx->stream);
  }
  if (rc) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_skinny_gemm: the launcher refused the arguments (K %d, S %d, lda %lld, N %d, ldo %lld, mode %d, bits %d, ss_tiles %d)",
                          d->K, d->S, (long long)d->lda, d->N, (long long)d->ldo, d->mode, d->bits, d->ss_tiles);
  if (hipGetLastError() != hipSuccess) return mia_fail(ctx, MIA_ERR_DEVICE, "op_skinny_gemm: launch failed");
  return MIA_OK;
}

// The packed prompt pass's GEMM (gemm_quant.hip) on caller-provided device arrays; gemm_quant_check is the gatekeeper.
#include "../../include/mia_gemm_quant.h"
extern "C" int mia_op_gemm_quant(mia_ctx* ctx, const mia_gemm_quant_desc* d) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, d, "op_gemm_quant: null descriptor");
  GemmQuantArgs a;
  a.A = (const uint16_t*)d->A; a.lda = d->lda; a.wfrag = d->wfrag; a.stfrag = d->stfrag; a.C = d->C; a.ldc = d->ldc; a.R = d->R; a.ldr = d->ldr;
  a.M = d->M; a.N = d->N; a.K = d->K;
  if (const char* e = gemm_quant_check(a, d->bits, d->dtype)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_%s", e);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  if (gemm_quant_launch(a, d->bits, d->dtype, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_gemm_quant: launch failed");
  return MIA_OK;
}

// fp32 attention, head dim 64, with every mode of attn_f32.hip (test hook): positional keys p with bias_u / bias_v, seq_len, chunk; device
// pointers, q/k/v [B*T][ld] with head h in columns h*64.., out [B*T][ldo]
extern "C" int mia_op_attention_f32_ex(mia_ctx* ctx, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                       const float* p, int64_t ldp, const float* bias_u, const float* bias_v, float* out, int64_t ldo, int B, int T,
                                       int H, float scale, const int32_t* seq_len, int chunk) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, chunk >= 0 && (int64_t)B * T < (1ll << 31), "op_attention_f32: bad argument");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  AttnF32Args a;
  a.q = q; a.ldq = ldq; a.k = k; a.ldk = ldk; a.v = v; a.ldv = ldv; a.out = out; a.ldo = ldo; a.B = B; a.T = T; a.H = H; a.scale = scale;
  a.p = p; a.ldp = ldp; a.bias_u = bias_u; a.bias_v = bias_v; a.seq_len = seq_len; a.chunk = chunk;
  if (const char* e = mia_attn_f32_check(a)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);     // B, T, H > 0 and the null checks live there
  if (mia_attn_f32_launch(a, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_attention_f32: launch failed");
  return MIA_OK;
}
// full (unmasked) softmax (MLXFast.scaledDotProductAttention as used by Codec/S3Gen/Matcha/MatchaTransformer.swift:58-66)
extern "C" int mia_op_attention_f32(mia_ctx* ctx, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                                    int64_t ldo, int B, int T, int H, float scale) {
  return mia_op_attention_f32_ex(ctx, q, ldq, k, ldk, v, ldv, nullptr, 0, nullptr, nullptr, out, ldo, B, T, H, scale, nullptr, 0);
}

// 16-bit scaled-dot-product attention, head dim 128, full softmax (attn128.hip): q / k / v [B*T][ld] with head h in columns h*128.., out [B*T][ldo]
// in `dtype`; seq_len int32 [B] or NULL.  Buffers live in `mem`; with host pointers every operand is copied on its own, so q, k and v may
// be three views of one fused buffer.
extern "C" int mia_op_attention_h128(mia_ctx* ctx, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out,
                                     int64_t ldo, int B, int T, int H, float scale, const int32_t* seq_len, int dtype, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "op_attention_h128: bad mem");
  MIA_CHECK_ARG(ctx, q && k && v && out && B > 0 && T > 0 && H > 0 && (int64_t)B * T < (1ll << 31), "op_attention_h128: bad argument");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  Attn128Args a;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo; a.B = B; a.T = T; a.H = H; a.scale = scale; a.dtype = dtype;
  const int64_t rows = (int64_t)B * T, D = (int64_t)H * 128;
  HostIo io(ctx, mem);
  MIA_CHECK_ARG(ctx, !io.host() || (ldq >= D && ldk >= D && ldv >= D && ldo >= D), "op_attention_h128: row strides must be >= H * 128");
  const size_t qb = (size_t)((rows - 1) * ldq + D) * 2, kb = (size_t)((rows - 1) * ldk + D) * 2, vb = (size_t)((rows - 1) * ldv + D) * 2;
  const size_t ob = (size_t)((rows - 1) * ldo + D) * 2, sb = (size_t)B * 4;
  Carve cv;
  const size_t o_q = cv.add(io.staged(qb)), o_k = cv.add(io.staged(kb)), o_v = cv.add(io.staged(vb)), o_o = cv.add(io.staged(ob)), o_s = cv.add(io.staged(sb));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  a.q = io.in(q, ws + o_q, qb); a.k = io.in(k, ws + o_k, kb); a.v = io.in(v, ws + o_v, vb);
  a.out = io.inout(out, ws + o_o, ob);                                                        // rows beyond seq_len keep the caller's bytes
  a.seq_len = io.in(seq_len, ws + o_s, sb);
  if (const char* e = mia_attn128_check(a)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
  if (mia_attn128_launch(a, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_attention_h128: launch failed");
  return io.finish();
}

// The SANM memory (fsmn.hip): x[t][c] += v[t][c] + sum_k w[k][c] v[t + k - left][c] per sequence of a [B][T] stack.
extern "C" int mia_op_fsmn_add(mia_ctx* ctx, float* x, int64_t ldx, const void* v, int64_t ldv, const float* w, int B, int T, int D, int K, int left,
                               const int32_t* seq_len, int dtype, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "op_fsmn_add: bad mem");
  MIA_CHECK_ARG(ctx, x && v && w && B > 0 && T > 0 && D > 0 && K > 0 && (int64_t)B * T < (1ll << 31), "op_fsmn_add: bad argument");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  FsmnArgs a;
  a.ldx = ldx; a.ldv = ldv; a.B = B; a.T = T; a.D = D; a.K = K; a.left = left; a.dtype = dtype;
  const int64_t rows = (int64_t)B * T;
  HostIo io(ctx, mem);
  MIA_CHECK_ARG(ctx, !io.host() || (ldx >= D && ldv >= D), "op_fsmn_add: row strides must be >= D");
  const size_t xb = (size_t)((rows - 1) * ldx + D) * 4, vb = (size_t)((rows - 1) * ldv + D) * 2, wb = (size_t)K * D * 4, sb = (size_t)B * 4;
  Carve cv;
  const size_t o_x = cv.add(io.staged(xb)), o_v = cv.add(io.staged(vb)), o_w = cv.add(io.staged(wb)), o_s = cv.add(io.staged(sb));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  a.x = io.inout(x, ws + o_x, xb);
  a.v = io.in(v, ws + o_v, vb); a.w = io.in(w, ws + o_w, wb); a.seq_len = io.in(seq_len, ws + o_s, sb);
  if (const char* e = mia_fsmn_check(a)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
  if (mia_fsmn_launch(a, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_fsmn_add: launch failed");
  return io.finish();
}

// The LM's single-token GQA attention over a cache it fills itself, without a model around it: K / V rows [Hkv][T][dh] (16 bit, taken
// as already rotated) go through the prompt pass's cache writer -- lm_rope_cache, or lm_kvq_rope_cache for bits 4 | 8 (QuantizedKVCache,
// TransformerBlock.swift:182-201) -- with all rotation angles zero, which leaves a 16-bit value unchanged; then the non-fused attention
// kernel of that cache mode runs q [Hq][dh] at position T - 1 over keys [0, T).  out fp32 [Hq][dh].  Host pointers.
#include "lm.h"
namespace {

float widen16(uint16_t x, int dtype) {
  if (dtype == MIA_F16) { _Float16 h; memcpy(&h, &x, 2); return (float)h; }
  const uint32_t u = (uint32_t)x << 16; float f; memcpy(&f, &u, 4); return f;
}

// What mia_op_kvq_attention and mia_op_lm_prompt_attention share: the q|k|v rows a prompt pass would hand the cache writer, row t =
// [q (last n rows only) | K[.][t] | V[.][t]], their row map, the workspace [part | map | freq | q | att | extra] with freq .. att (and the
// first `zeroed` bytes of extra) cleared, and a bare handle holding what the launch sites read of one.  Declare it before the call's HostIo:
// its vectors are uploaded through io.table and must outlive it.
struct LmOpRows {
  std::vector<float> part;
  std::vector<int2> rowmap;
  int Nq = 0, N = 0;
  float* d_part = nullptr; int2* d_map = nullptr; uint16_t* d_q = nullptr; uint16_t* d_att = nullptr; char* extra = nullptr;
  mia_lm sh;

  void build(const void* q, const void* k, const void* v, int Hq, int Hkv, int T, int n, int dh, int dtype) {
    const int Nk = Hkv * dh;
    Nq = Hq * dh; N = Nq + 2 * Nk;
    part.assign((size_t)T * N, 0.f);
    rowmap.resize(T);
    const uint16_t* q16 = (const uint16_t*)q; const uint16_t* k16 = (const uint16_t*)k; const uint16_t* v16 = (const uint16_t*)v;
    for (int r = 0; r < n; ++r)
      for (int i = 0; i < Nq; ++i) part[(size_t)(T - n + r) * N + i] = widen16(q16[(size_t)r * Nq + i], dtype);
    for (int t = 0; t < T; ++t) {
      rowmap[t] = make_int2(0, t);
      for (int h = 0; h < Hkv; ++h)
        for (int d = 0; d < dh; ++d) {
          part[(size_t)t * N + Nq + h * dh + d] = widen16(k16[((size_t)h * T + t) * dh + d], dtype);
          part[(size_t)t * N + Nq + Nk + h * dh + d] = widen16(v16[((size_t)h * T + t) * dh + d], dtype);
        }
    }
  }
  int stage(mia_ctx* ctx, HostIo& io, int Hq, int Hkv, int T, int n, int dh, int dtype, size_t extra_bytes, size_t zeroed) {
    Carve cv;
    const size_t o_part = cv.add(part.size() * 4), o_map = cv.add((size_t)T * sizeof(int2)), o_freq = cv.add((size_t)dh / 2 * 4),
                 o_q = cv.add((size_t)T * Nq * 2), o_att = cv.add((size_t)n * Nq * 2), o_extra = cv.add(extra_bytes);
    char* ws = (char*)mia_workspace(ctx, cv.bytes);
    if (!ws) return MIA_ERR_OUT_OF_MEMORY;
    d_q = (uint16_t*)(ws + o_q); d_att = (uint16_t*)(ws + o_att); extra = ws + o_extra;
    d_part = const_cast<float*>(io.table(part.data(), ws + o_part, part.size() * 4));
    d_map = const_cast<int2*>(io.table(rowmap.data(), ws + o_map, (size_t)T * sizeof(int2)));
    MIA_HIP(ctx, hipMemsetAsync(ws + o_freq, 0, o_extra - o_freq + zeroed, ctx->stream));
    sh.ctx = ctx; sh.dtype = dtype; sh.B_cap = 1; sh.inv_freq = (float*)(ws + o_freq);
    sh.cfg.n_layers = 1; sh.cfg.n_heads = Hq; sh.cfg.n_kv_heads = Hkv; sh.cfg.head_dim = dh; sh.cfg.max_ctx = T;
    return MIA_OK;
  }
  // the attention rows [n][Nq] back as fp32
  int read(HostIo& io, float* out, int n, int dtype) {
    std::vector<uint16_t> att((size_t)n * Nq);
    io.fetch(att.data(), d_att, att.size() * 2);
    if (int rc = io.finish()) return rc;
    for (size_t i = 0; i < att.size(); ++i) out[i] = widen16(att[i], dtype);
    return MIA_OK;
  }
};

}  // namespace

extern "C" int mia_op_kvq_attention(mia_ctx* ctx, const void* q, const void* k, const void* v, float* out, int Hq, int Hkv, int T, int dh, int bits, int dtype) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, q && k && v && out, "op_kvq_attention: null pointer");
  MIA_CHECK_ARG(ctx, dtype == MIA_BF16 || dtype == MIA_F16, "op_kvq_attention: dtype must be MIA_BF16 or MIA_F16");
  MIA_CHECK_ARG(ctx, Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Hq <= 1024 && T > 0 && T <= 8192, "op_kvq_attention: bad shape (Hq %% Hkv == 0, 1 <= T <= 8192)");
  int code = MIA_OK;
  if (const char* e = lm_kvq_check(bits, 64, dh, &code)) return mia_fail(ctx, code, "op_kvq_attention: %s (bits %d, head_dim %d)", e, bits, dh);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  LmOpRows f;
  f.build(q, k, v, Hq, Hkv, T, 1, dh, dtype);
  HostIo io = HostIo::device(ctx);
  const size_t rows = (size_t)Hkv * T;
  const size_t b_st = align_up(sizeof(LmState), 256), b_codes = align_up(bits ? rows * dh * bits / 8 : rows * dh * 2, 256), b_pairs = align_up(rows * (dh / 64) * 4, 256);
  if (int rc = f.stage(ctx, io, Hq, Hkv, T, 1, dh, dtype, b_st + 2 * b_codes + 2 * b_pairs, b_st)) return rc;
  char* d_kc = f.extra + b_st; char* d_vc = d_kc + b_codes; char* d_kp = d_vc + b_codes; char* d_vp = d_kp + b_pairs;
  mia_lm& sh = f.sh;
  sh.kv_bits = bits; sh.state = (LmState*)f.extra;
  if (bits) { sh.kq_codes = (uint32_t*)d_kc; sh.vq_codes = (uint32_t*)d_vc; sh.kq_pairs = (uint32_t*)d_kp; sh.vq_pairs = (uint32_t*)d_vp; }
  else { sh.k_cache = d_kc; sh.v_cache = d_vc; }
  lm_launch_rope_cache(&sh, 0, f.d_part, nullptr, f.d_q, f.d_map, T);
  lm_launch_attention(&sh, false, 1, f.d_q + (size_t)(T - 1) * f.Nq, 0, f.d_att, f.d_map + (T - 1), nullptr, 0, nullptr);
  if (hipGetLastError() != hipSuccess) return mia_fail(ctx, MIA_ERR_DEVICE, "op_kvq_attention: launch failed");
  return f.read(io, out, 1, dtype);
}

// lm_prefill_attn.hip without a model around it: K / V rows [Hkv][T][dh] (16 bit, taken as already rotated) go through the prompt pass's
// 16-bit cache writer (lm_rope_cache with all rotation angles zero, which leaves a 16-bit value unchanged), then the tiled kernel runs the
// q rows [n][Hq][dh] at positions T - n .. T - 1, each over keys [0, its position].  out fp32 [n][Hq][dh].  Host pointers.
extern "C" int mia_op_lm_prompt_attention(mia_ctx* ctx, const void* q, const void* k, const void* v, float* out, int Hq, int Hkv, int T, int n, int dh, int dtype) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, q && k && v && out, "op_lm_prompt_attention: null pointer");
  MIA_CHECK_ARG(ctx, dtype == MIA_BF16 || dtype == MIA_F16, "op_lm_prompt_attention: dtype must be MIA_BF16 or MIA_F16");
  MIA_CHECK_ARG(ctx, Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Hq <= 1024 && n >= 1 && n <= T && T <= 8192, "op_lm_prompt_attention: bad shape (Hq %% Hkv == 0, 1 <= n <= T <= 8192)");
  if (dh != 64 && dh != 128) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "op_lm_prompt_attention: head_dim %d (64 or 128)", dh);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  LmOpRows f;
  f.build(q, k, v, Hq, Hkv, T, n, dh, dtype);
  std::vector<int4> tiles;
  lm_prefill_attn_tiles(f.rowmap.data() + (T - n), n, lm_prefill_attn_qtile(Hq, Hkv), tiles);     // rows 0 .. n - 1 of q / att below
  HostIo io = HostIo::device(ctx);
  const size_t b_tiles = align_up(tiles.size() * sizeof(int4), 256), b_cache = align_up((size_t)Hkv * T * dh * 2, 256);
  if (int rc = f.stage(ctx, io, Hq, Hkv, T, n, dh, dtype, b_tiles + 2 * b_cache, 0)) return rc;
  const int4* d_tiles = io.table(tiles.data(), f.extra, tiles.size() * sizeof(int4));
  mia_lm& sh = f.sh;
  sh.k_cache = f.extra + b_tiles; sh.v_cache = f.extra + b_tiles + b_cache;
  lm_launch_rope_cache(&sh, 0, f.d_part, nullptr, f.d_q, f.d_map, T);
  LmPromptAttn a;
  a.q = f.d_q + (size_t)(T - n) * f.Nq; a.kc = (const uint16_t*)sh.k_cache; a.vc = (const uint16_t*)sh.v_cache; a.out = f.d_att; a.tiles = d_tiles; a.n_tiles = (int)tiles.size();
  a.Hq = Hq; a.Hkv = Hkv; a.dh = dh; a.max_ctx = T; a.seq_stride = (int64_t)Hkv * T * dh; a.dtype = dtype;
  if (const char* e = lm_prefill_attn_check(a)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
  if (lm_prefill_attn_launch(a, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_lm_prompt_attention: launch failed");
  return f.read(io, out, n, dtype);
}
