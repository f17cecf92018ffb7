// mimi.h -- launch interface of Mimi's own kernels: the decoder's (mimi_kernels.hip; layer program and C ABI in mimi.hip) and the
// encoder's (mimi_encode_kernels.hip; layer program and C ABI in mimi_encode.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// z[t][:] = WfT^T e0[c0[t]] + WrT^T sum_{i >= 1} e_i[c_i[t]]     codes: device [n_q][n]; cb: [nq][bins][dq]; WfT / WrT: [dq][D]
int mimi_embed_launch(const int32_t* codes, int n_q, int64_t n, const float* cb, int bins, int dq, const float* wfT, const float* wrT, float* z,
                      int D, hipStream_t s);
// depthwise causal transposed convolution, kernel 2 * stride: y[t * stride + r][c] = z[t][c] w[r][c] + z[t - 1][c] w[r + stride][c];
// zp: [1 + n][D], row 0 = z[-1] (the carried row, zeros at the start of a clip)
int mimi_upsample_launch(const float* zp, const float* w, float* y, int64_t n, int D, int stride, hipStream_t s);
// split in_proj's [P][3 D] into q | k | v, interleaved-pair RoPE at position pos0 + row on q and k; k / v rows go to k_new / v_new (row stride D)
int mimi_qkv_finish_launch(const float* qkv, float* q, float* k_new, float* v_new, int64_t P, int D, int64_t pos0, const double* inv_freq, hipStream_t s);
// pair-windowed attention against a key history: queries are P rows at positions pos0 .. pos0 + P - 1 (pos0 and P even); the pair
// (2 f, 2 f + 1) sees the keys at positions [max(0, 2 f - ctx), 2 f + 2).  K / V: row r holds position row0_pos + r.
int mimi_window_attn_launch(const float* q, const float* K, const float* V, float* out, int64_t P, int D, int H, int64_t pos0, int64_t row0_pos,
                            int ctx, float scale, hipStream_t s);
// out[t] = bias + sum_{k, c} w[k * C + c] * elu(x[t + k][c])      x: [K - 1 + T][C], the first K - 1 rows are the left context
int mimi_conv_out1_launch(const float* x, const float* w, const float* bias, float* out, int64_t T, int C, int K, hipStream_t s);

// ---- encode side (mimi_encode_kernels.hip)
// edge padding of the latent downsample: y = [front copies of x[0] | the P rows of x | back copies of x[P - 1]], rows of D floats
int mimi_edge_rows_launch(const float* x, float* y, int64_t P, int D, int front, int back, hipStream_t s);

constexpr int MIMI_RVQ_TILE = 32;      // frames per workgroup of the chain stage
constexpr int MIMI_RVQ_SLICE = 128;    // codebook entries per workgroup
// One stage of one residual chain for the launch below.  r_in: the residual the PREVIOUS stage saw, [n_tiles * 32][ld_in] (rows at or
// past T are never read).  If prev_pd is set, the stage's prologue first finishes the previous stage: it reduces that stage's partials
// (prev_slices per frame, lexicographic on (distance, index)), writes the code to prev_codes[frame], and continues on
// r = r_in - e_prev[code]; the workgroups of slice 0 also store r to r_out ([n_tiles * 32][dq]).  Without prev_pd, r = r_in.
// Then every workgroup forms d[j] = c2[j] - r . e[j] over its slice of entries and writes its best (d, j) per frame to pd / pi
// ([slices][n_tiles * 32]).
struct MimiRvqChain {
  const float* r_in = nullptr; int64_t ld_in = 0;
  const float* e = nullptr; const float* c2 = nullptr;           // this stage's entries [bins][dq] and ||e||^2 / 2
  float* pd = nullptr; int32_t* pi = nullptr;
  const float* prev_pd = nullptr; const int32_t* prev_pi = nullptr; const float* e_prev = nullptr;
  int32_t* prev_codes = nullptr; float* r_out = nullptr;
};
// grid = (frame tiles, slices of `a` + slices of `b`): chain b (optional, b.e == nullptr: absent) rides in the same launch
int mimi_rvq_stage_launch(const MimiRvqChain& a, const MimiRvqChain& b, int64_t T, int bins, int dq, hipStream_t s);
// the reduction of a chain's last stage: codes[frame] from its partials, for up to two chains (pd_b == nullptr: one)
int mimi_rvq_finish_launch(const float* pd_a, const int32_t* pi_a, int32_t* codes_a, const float* pd_b, const int32_t* pi_b, int32_t* codes_b,
                           int64_t T, int bins, hipStream_t s);
static inline int mimi_rvq_slices(int bins) { return (bins + MIMI_RVQ_SLICE - 1) / MIMI_RVQ_SLICE; }
