// skinny.h -- the skinny (M <= 32 rows per block-z) MFMA GEMMs of the per-token decode steps: modes, operand layouts, arguments and the
// model-independent launchers.  Used by the LM step (lm.hip; fragment repack at load in lm_load.hip) and the Whisper step (decode.h); includes no model header.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mia.h"
#include "tensor_loader.h"

enum { SK_OUT16 = 0, SK_OUTF32 = 1, SK_PARTIAL = 2, SK_QKV = 3, SK_SWIGLU = 4, SK_RESID = 5 };

// ---- MFMA-fragment order (the Whisper decode step's GEMM operands) -------------------------------------------------------------
// v_mfma_f32_16x16x32 takes, per lane (r = lane & 15, c = lane >> 4), the 8 consecutive K-values 8c..8c+7 of row r.  Stored row-major,
// one wave instruction gathers 16 rows x 64 B (16 half cache lines whose 2560-byte stride maps them onto a few L2 channels); stored in
// fragment order it is ONE contiguous 1 KB.  tools/micro/skinny_probe.hip measures the difference on the decoder's fc1 shape
// (N 5120, K 1280, 32 rows): 11.9 us row-major -> 10.0 us with the weights in fragment order -> 8.3 us with the activations too.
//   activations [32 z][K]:  element (m, k) -> ((((m >> 5) * (K >> 5) + (k >> 5)) * 2 + ((m >> 4) & 1)) * 64 + ((k >> 3) & 3) * 16 + (m & 15)) * 8 + (k & 7)
//   weights     [N][K]:     element (n, k) -> (((n >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k >> 3) & 3) * 16 + (n & 15)) * 8 + (k & 7), rows padded to 16
__host__ __device__ inline int64_t afrag_index(int m, int k, int K) {
  return ((((int64_t)(m >> 5) * (K >> 5) + (k >> 5)) * 2 + ((m >> 4) & 1)) * 64 + ((k >> 3) & 3) * 16 + (m & 15)) * 8 + (k & 7);
}
__host__ __device__ inline int64_t wfrag_index(int n, int k, int K) {
  return (((int64_t)(n >> 4) * (K >> 5) + (k >> 5)) * 64 + ((k >> 3) & 3) * 16 + (n & 15)) * 8 + (k & 7);
}

struct SkinnyArgs {
  const uint16_t* A; int64_t lda;        // [M][K]
  const uint16_t* W;                     // [N][K]
  const float* bias;
  void* out; int64_t ldo;                // OUT16 / OUTF32: [M][ldo];  PARTIAL: [S][M][N];  QKV: q [M][D]
  uint16_t* cache_k; uint16_t* cache_v;  // QKV: [B][H][n_ctx][64] of this layer
  const int32_t* pos;                    // QKV: per-row (clip) cache position
  int M, N, K, S, act, D, H, n_ctx;
  int out_frag = 0;                      // fragment-order kernels, OUT16: write `out` in activation fragment order (row length N)
  int w_frag = 0;                        // row-major-activation kernels (the LM step): W is in weight fragment order
  int w_keep = 0;                        // fragment-order kernels (the Whisper step): load W with the default cache policy instead of
                                         // non-temporal -- set per launch by the step (whisper_decode.hip: dec_cache_policy)
  // ---- RMSNorm carried across the GEMM chain of the LM step (no separate reduce + norm launch):
  // SK_RESID (needs S == 1): xres[m][n] += acc (+ bias) in place (the fp32 residual stream, row stride N); out[m][n] (16-bit, row stride
  //   ldo) = (x_new * nw[n]) rounded -- the NEXT block's activation, not yet divided by its rms; ss_out[tile][m] = sum of x_new^2 over the
  //   tile's 16 columns (tile = n / 16), one value per (tile, row), written by exactly one lane: a fixed-order partial sum.
  // consumers of such an activation (any mode) pass ss_in / ss_tiles / ss_dim / eps: the accumulator of row m is multiplied by
  //   rstd[m] = rsqrt(sum_t ss_in[t][m] / ss_dim + eps) before bias and activation -- linear, so it commutes with the contraction.
  float* xres = nullptr; const float* nw = nullptr; float* ss_out = nullptr;
  const float* ss_in = nullptr; int ss_tiles = 0; int ss_dim = 0; float eps = 0.f;
  // range of the carried operand (mia_carry_prescale below): the producer's nw is the norm gain times a power of two p, the consumer
  // multiplies rstd by rs_scale = 1 / p (exact, so inside the normal range of the 16-bit type nothing changes)
  float rs_scale = 1.f;
  // LayerNorm form (the Whisper step, fragment-order kernels): ss_* hold PAIRS (sum x, sum x^2) per (tile, row); a consumer passes the
  // Linear's folded constants c1[n] = sum_k W[n][k] gamma[k], c2[n] = sum_k W[n][k] beta[k] and its epilogue computes
  //   LN(x) W^T = rstd (acc - mean c1) + c2      with acc = W (x * gamma), the activation the SK_RESID producer stored
  const float* c1 = nullptr; const float* c2 = nullptr;
};

// Pre-scale p = 2^-k of a carried operand x * gain (RMSNorm and LayerNorm chains, the encoder's hand-over).  The operand is rounded to
// 16 bit BEFORE the division by rms / std, so on F16 handles its range is the residual's, not the normalised row's: a residual of 3e4
// under a gain of 4 is inf (max 65504).  F16: k = 3 + ilogb(max |gain|), i.e. the stored |x * gain * p| < |x| / 4 whatever the gains
// are -- finite for residuals up to 2.6e5, and a residual as small as 1e-3 (where eps starts to matter) still lands above the f16
// subnormals' resolution: 2^-24 against 1e-4 is the 16-bit rounding of a normal value.  BF16 has fp32's range: p = 1.
inline float mia_carry_prescale(const float* gain, int n, int dtype) {
  if (dtype != MIA_F16) return 1.f;
  float mx = 0.f;
  for (int i = 0; i < n; ++i) { const float a = fabsf(gain[i]); if (a > mx) mx = a; }
  if (!(mx > 0.f) || !std::isfinite(mx)) return 1.f;
  int k = 3 + ilogbf(mx);
  k = k < -24 ? -24 : (k > 40 ? 40 : k);
  return ldexpf(1.f, -k);
}

// The gain of a carried norm as its producer stores with it: g x mia_carry_prescale, uploaded through L; *rs = 1 / that scale for the
// consumer.  `plain` (the unscaled gain already on the device) when the scale is 1.
inline float* mia_carry_gain(TensorLoader& L, const std::vector<float>& g, int dtype, float* plain, float* rs) {
  const float p = mia_carry_prescale(g.data(), (int)g.size(), dtype);
  *rs = 1.f / p;
  if (p == 1.f) return plain;
  std::vector<float> v(g);
  for (float& x : v) x *= p;
  return L.up(v);
}

// row-major [N][K] 16-bit -> weight fragment order (dst holds ceil(N/16)*16*K elements; rows past N are zero)
int dec_launch_repack_wfrag(const void* src, void* dst, int N, int K, hipStream_t s);
// The loaders' form: *dst = a fragment-order copy of src in a new buffer appended to `allocs` (one device repack per matrix).  A null src
// (a matrix the model does not have) gives a null copy.  false: K % 32 != 0, a refused hipMalloc or a failed launch.
bool dec_wfrag_copy(const void* src, int N, int K, std::vector<void*>& allocs, hipStream_t s, void** dst);
// row-major activations (the LM step; skinny_rowmajor.hip), dtype = MIA_BF16 | MIA_F16; modes SK_OUTF32 / SK_PARTIAL / SK_SWIGLU / SK_RESID.
// SK_SWIGLU: W rows interleaved gate/up, out[m][n/2] = silu(g)*u (16-bit)
// Both launchers also refuse (-1) non-positive sizes and a W (16 bit: an A too) or packed code array of 4 GiB or more: the kernels address
// them through buffer resources with 32-bit sizes and byte offsets (WFragBuf), and a loader can get there (a 262144 x 8192 vocabulary
// head is exactly 4 GiB).
// The kernel form is chosen from the shape alone; tests/_skinny_cases.py restates the rule (dispatch16) -- change the two together.
int skinny_gemm_launch(const SkinnyArgs& a, int mode, int dtype, hipStream_t s);
// MLX-affine 4- / 6- / 8-bit weights in fragment order (skinny_quant.hip: skinny_gemm_qi); modes SK_OUTF32 / SK_PARTIAL / SK_SWIGLU / SK_RESID
// M_cap: the rows the caller's handle can hold (0 = M).  The launcher chooses between kernel forms that split K differently -- four
// tiles per wave above 16 rows, the one-wave vocabulary head up to 16 -- and so sum in a different order.  It chooses from
// max(M, M_cap): with M_cap = the handle's batch capacity a row's result does not depend on how many rows this call carries
// (lm.hip: lm_enqueue_step).  Without it the form follows M, and these shapes change their K split between M <= 16 and M > 16:
//   * ceil(N / 64) * S >= 192 with K / S / 128 in {2, 6, 9, 10, 14, ...} (several waves below, one above; Qwen3-0.6B q|k|v: N 4096, K 1024, S 4;
//     Orpheus-3B q|k|v: N 5120, K 3072, S 4);
//   * ceil(N / 64) * S >= 192 with K / S / 128 == 4: four waves above 16 rows, two below;
//   * the OUTF32 head with N >= 65536 and K / 128 a multiple of 4: one wave up to 16 rows, four above (Qwen3-0.6B, Llama-3.2-1B,
//     Orpheus-3B vocabulary heads).
// tests/test_skinny_gpu.py asserts the derived bound only across the boundary for those, and bit-equality of rows everywhere else.
// (form rule restated in tests/_skinny_cases.py: dispatch_q)
int skinny_gemm_q_launch(const SkinnyArgs& a, const uint32_t* wfrag, const float* stfrag, int bits, int mode, int dtype, hipStream_t s, int M_cap = 0);

// ---- the many-row form on the same packed arrays (gemm_quant.hip): the LM's batched prompt pass on packed weights -----------------
// C[M][N] fp32 = A[M][K] (16 bit, row stride lda) . Wq^T (+ R[M][N] fp32; R may alias C), wfrag / stfrag exactly as skinny_gemm_q_launch
// reads them.  Any M, N >= 1, K % 128 == 0, lda % 8 == 0; no bias, no K split: a row's result depends on its own A row alone, whatever M.
struct GemmQuantArgs {
  const uint16_t* A = nullptr; int64_t lda = 0;
  const uint32_t* wfrag = nullptr; const float* stfrag = nullptr;
  float* C = nullptr; int64_t ldc = 0;
  const float* R = nullptr; int64_t ldr = 0;
  int M = 0, N = 0, K = 0;
};
// nullptr when the arguments satisfy the kernel's shape / alignment assumptions, else a message
const char* gemm_quant_check(const GemmQuantArgs& a, int bits, int dtype);
int gemm_quant_launch(const GemmQuantArgs& a, int bits, int dtype, hipStream_t s);
