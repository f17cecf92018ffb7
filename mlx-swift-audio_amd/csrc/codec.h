// codec.h -- internal interface of the fp32 codec-decoder kernels (codec_kernels.hip) and the layer programs (codec.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mia.h"
#include "mia_internal.h"

// Tap-structured fp32 GEMM: Y[row(m)][n] = epi( sum_{tap,c} pre(X[m + tap*dil - pad][c]) * W[n][tap*Cin + c] + bias[n] )
//   row(m) = m*y_row_mul + y_row_off + z*y_phase_step (rows outside [0,T_out) are dropped); z = grid.z phase, W += z*w_phase_stride
// (mia_conv_gemm_desc in include/mia.h mirrors this struct field for field: the test hook mia_op_conv_gemm_f32 copies it and launches)
struct ConvGemmArgs {
  const float* X = nullptr; int64_t ldx = 0; int T_in = 0;
  const float* W = nullptr; int64_t w_phase_stride = 0;
  const float* bias = nullptr;
  const float* alpha = nullptr;        // snake prologue on X (per input channel), or null
  const float* ralpha = nullptr;       // snake multiplier (per channel); null -> 1/(alpha + 1e-9) (SNAC / DAC form)
  float lrelu_slope = 0.f;             // > 0: leaky-ReLU prologue on X instead of snake
  float* Y = nullptr; int64_t ldy = 0; int T_out = 0;
  int y_row_mul = 1, y_row_off = 0, y_phase_step = 0;
  const float* R = nullptr; int64_t ldr = 0;   // residual (same row mapping as Y)
  const float* noise = nullptr;        // if set: Y = R + noise[row] * (acc + bias)
  float out_scale = 0.f;               // != 0: Y = out_scale * (act(acc + bias) + R) + R2
  const float* R2 = nullptr;           // second residual, added after the scale (row stride ldr)
  int M = 0, N = 0, Cin = 0, taps = 1, dil = 1, pad = 0;
  int tanh_out = 0;
  int x_row_mul = 1;                   // convolution stride: A(m, tap, c) = X[m*x_row_mul + tap*dil - pad][c]
  int gelu = 0;                        // activation on acc + bias (before the residual): 1 = exact-erf GELU, 2 = ELU, 3 = abs, 4 = SiLU, 5 = leaky-ReLU(0.01), 6 = ReLU,
                                       // 7 = tanh-form GELU (Mimi)
  int64_t ldw = 0;                     // row stride of W (0 = taps*Cin, i.e. dense)
  const int32_t* phase_len = nullptr;  // device [phases], optional (with x_phase_step): sequence z holds phase_len[z] <= T_in valid rows, rows at or
                                       // beyond it read as zero like rows past T_in (padded stacked sequences under a forward-looking window)
  int x_phase_step = 0;                // rows of X skipped per grid.z phase: stacked sequences of T_in rows each (taps never cross
                                       // a sequence; pair with w_phase_stride = 0, y_row_mul = 1, y_phase_step = rows per sequence)
  // Stacked sequences under ANY row mapping (HiFT batches: plain, strided and transposed convolutions): grid.z = n_seq x phases,
  // sequence u = z / phases reads X + u * x_seq_step rows (T_in = rows per sequence, seq_len[u] <= T_in of them valid, the rest read
  // as zero like rows past T_in) and writes rows u * y_seq_step + row(m) of Y (R and R2 likewise); row(m) is tested against T_out
  // per sequence.  n_seq = 1: everything above is unchanged.
  int n_seq = 1;
  int64_t x_seq_step = 0, y_seq_step = 0;
  const int32_t* seq_len = nullptr;    // device [n_seq], optional
  // noise term under stacked sequences (needs seq_len, T_out rows == T_in rows): sequence u's value for row r is
  // noise[noise_seq_off[u] + r]; its rows at or past seq_len[u] have no noise value and are not written
  const int32_t* noise_seq_off = nullptr;   // device [n_seq]
  // ELU(alpha = 1) prologue on X instead of snake / leaky-ReLU (Mimi's SEANet).  elu_pre and gelu == 7 are served by a second set of
  // instantiations of the kernel (template flag MIMI): the launches without them run the code they ran before the flag existed.
  // (Not mirrored in mia_conv_gemm_desc: the operator-level hook has no Mimi case; tests/test_mimi_gpu.py covers it end to end.)
  int elu_pre = 0;
};

constexpr int MIA_MAX_LEVELS = 4;
struct EmbedArgs {
  const int32_t* codes[MIA_MAX_LEVELS];   // device, null = level absent
  const float* codebook[MIA_MAX_LEVELS];  // [size][cb_dim]
  const float* weff[MIA_MAX_LEVELS];      // folded weight-normed out_proj [C][cb_dim]
  const float* bias[MIA_MAX_LEVELS];      // [C]
  int stride[MIA_MAX_LEVELS];
  int n_levels, cb_dim;
  // stacked sequences: level l of sequence u reads codes_base + seq_code_off[u * MIA_MAX_LEVELS + l] (negative = skipped for that
  // sequence); codes[] is then unused
  const int32_t* codes_base;
  const int64_t* seq_code_off;            // device [n_seq][MIA_MAX_LEVELS], or null
};

// Stacked sequences for the element-wise kernels, in the tap GEMM's layout: n sequences side by side, sequence u at row u * step of the
// buffer (step = 0: T, the launch's rows per sequence), len[u] <= T of them valid.  Rows at or past len[u] read as zero, like rows past T in a single call,
// and are never written.  n = 1 with len = null: the single-sequence launch, unchanged.
struct SeqArgs {
  int n = 1;
  const int32_t* len = nullptr;           // device [n]
  int64_t step = 0;                       // rows between sequences (>= T), 0 = T
  const int32_t* noise_off = nullptr;     // device [n]: sequence u's noise values start at noise + noise_off[u]   (noise_mod1)
  const int64_t* out_off = nullptr;       // device [n]: sequence u's samples go to out + out_off[u]                (conv_out1)
};

const char* codec_conv_gemm_check(const ConvGemmArgs& g);
// algorithmic bytes of the fp32 conv / elementwise launches issued by the calling host thread since the last reset (profiling aid)
double codec_alg_bytes(bool reset);
int codec_conv_gemm_launch(const ConvGemmArgs& g, int phases, hipStream_t s);
// the checked launch every host file goes through: the arguments are checked, the GEMM goes to the context's stream, and a failure of either
// is recorded as "<who>: <text>"
static inline int codec_conv_gemm_run(mia_ctx* ctx, const ConvGemmArgs& g, int phases, const char* who) {
  if (const char* e = codec_conv_gemm_check(g)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s: %s", who, e);
  if (codec_conv_gemm_launch(g, phases, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "%s: conv_gemm launch failed", who);
  return MIA_OK;
}
int codec_dwconv_launch(const float* x, float* y, const float* w, const float* bias, const float* a_pre, const float* a_post, int T, int C,
                        int K, int dil, hipStream_t s, const SeqArgs& q = SeqArgs());
int codec_conv_out1_launch(const float* x, float* out, const float* w, const float* bias, const float* alpha, int T, int C, int K, hipStream_t s,
                           const SeqArgs& q = SeqArgs());
int codec_embed_launch(const EmbedArgs& a, float* z, int T, int C, hipStream_t s, const SeqArgs& q = SeqArgs());
int codec_noise1_launch(float* x, const float* w, const float* noise, int T, int C, hipStream_t s, const SeqArgs& q = SeqArgs());
int codec_conv_in1_launch(const float* x, float* y, const float* w, const float* bias, int64_t T, int C, int K, int pad, hipStream_t s);
int codec_vq_assign_launch(const float* zE, const float* cbn, const float* cbn_sq, const float* cb, const float* weff, const float* bias,
                           float* residual, int32_t* codes, int T, int C, int cs, int cd, hipStream_t s);
