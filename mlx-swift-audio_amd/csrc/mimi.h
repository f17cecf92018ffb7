// mimi.h -- launch interface of the Mimi decoder's own kernels (mimi_kernels.hip); the layer program and the C ABI are in mimi.hip.
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
