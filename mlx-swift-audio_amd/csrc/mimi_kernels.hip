// mimi_kernels.hip -- the Mimi decoder's own fp32 kernels on gfx950 (the GEMMs and convolutions run on conv_gemm_f32, the whole-clip
// attention on attn_f32).
//
//  * mimi_embed        split-RVQ decode (Quantization.swift:212-219): gather of up to 32 codebook rows per frame, the sum over the
//                      "rest" rows in codebook order, and the two 256 -> 512 projections.  One workgroup per frame; the projection
//                      weights are stored transposed so that the 256 threads read consecutive output channels.
//  * mimi_upsample     the depthwise k = 2 s, stride s causal transposed convolution in front of the transformer.
//  * mimi_qkv_finish   q | k | v split, interleaved-pair RoPE at the absolute position (angle in double: the position grows without
//                      bound over a stream), k / v written straight into the stream's history rows.
//  * mimi_window_attn  the streamed step's attention.  The reference feeds one frame = 2 positions per step with mask nil against
//                      its trimmed cache, so both rows of pair f see the keys [max(0, 2 f - ctx), 2 f + 2).  One workgroup = one pair
//                      of one head, one wave per query row; it walks exactly its hi - lo <= ctx + 2 keys, so keys outside a pair's
//                      range are never read (a stream costs O(T (ctx + 2)), not O(T^2)).  With at most 252 keys of 64 floats per
//                      query the scores are plain FMAs (lane = key), the softmax is one wave reduction, and the value sum has
//                      lane = output column, so V rows are read coalesced.
//  * mimi_conv_out1    ELU -> causal conv k (C -> 1), no tanh: the SEANet's last layer.
#include "mia_device.h"
#include "mimi.h"

namespace {

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }

__global__ __launch_bounds__(256) void mimi_embed(const int32_t* __restrict__ codes, int n_q, int64_t n, const float* __restrict__ cb, int bins,
                                                  int dq, const float* __restrict__ wfT, const float* __restrict__ wrT, float* __restrict__ z, int D) {
  extern __shared__ float sm[];          // e0[dq] | rest[dq]
  float* e0 = sm;
  float* er = sm + dq;
  const int64_t t = blockIdx.x;
  for (int j = threadIdx.x; j < dq; j += 256) {
    e0[j] = cb[(int64_t)codes[t] * dq + j];
    float acc = 0.f;
    for (int i = 1; i < n_q; ++i) {
      const float e = cb[((int64_t)i * bins + codes[(int64_t)i * n + t]) * dq + j];
      acc = i == 1 ? e : acc + e;
    }
    er[j] = acc;
  }
  __syncthreads();
  for (int ch = threadIdx.x; ch < D; ch += 256) {
    float a = 0.f, b = 0.f;
    for (int j = 0; j < dq; ++j) a = fmaf(wfT[(int64_t)j * D + ch], e0[j], a);
    if (n_q > 1) {
      for (int j = 0; j < dq; ++j) b = fmaf(wrT[(int64_t)j * D + ch], er[j], b);
      a += b;
    }
    z[t * D + ch] = a;
  }
}

__global__ __launch_bounds__(256) void mimi_upsample(const float* __restrict__ zp, const float* __restrict__ w, float* __restrict__ y, int64_t n, int D,
                                                     int stride) {
  const int64_t total = n * stride * D;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / D;
    const int c = (int)(e - row * D);
    const int64_t t = row / stride;
    const int r = (int)(row - t * stride);
    // zp row t + 1 = z[t], row t = z[t - 1]
    y[e] = zp[(t + 1) * D + c] * w[(int64_t)r * D + c] + zp[t * D + c] * w[(int64_t)(r + stride) * D + c];
  }
}

__global__ __launch_bounds__(256) void mimi_qkv_finish(const float* __restrict__ qkv, float* __restrict__ q, float* __restrict__ kn, float* __restrict__ vn,
                                                       int64_t P, int D, int64_t pos0, const double* __restrict__ inv_freq) {
  const int half = D >> 1;
  const int64_t total = P * half;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t p = e / half;
    const int col = (int)(e - p * half) * 2;
    const int i = (col & 63) >> 1;
    double sd, cd;
    sincos((double)(pos0 + p) * inv_freq[i], &sd, &cd);
    const float sn = (float)sd, cs = (float)cd;
    const float* src = qkv + p * 3 * D + col;
    const float2 qa = *reinterpret_cast<const float2*>(src);
    const float2 ka = *reinterpret_cast<const float2*>(src + D);
    const float2 va = *reinterpret_cast<const float2*>(src + 2 * D);
    *reinterpret_cast<float2*>(q + p * D + col) = make_float2(qa.x * cs - qa.y * sn, qa.x * sn + qa.y * cs);
    *reinterpret_cast<float2*>(kn + p * D + col) = make_float2(ka.x * cs - ka.y * sn, ka.x * sn + ka.y * cs);
    *reinterpret_cast<float2*>(vn + p * D + col) = va;
  }
}

__global__ __launch_bounds__(128) void mimi_window_attn(const float* __restrict__ q, const float* __restrict__ K, const float* __restrict__ V,
                                                        float* __restrict__ out, int D, int64_t pos0, int64_t row0_pos, int ctx, float scale) {
  extern __shared__ float sm[];          // [2][ctx + 2] scores, then probabilities, of the pair's two rows
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t pair = blockIdx.x;
  const int h = blockIdx.y;
  const int64_t p_abs = pos0 + 2 * pair;
  const int64_t lo = p_abs > ctx ? p_abs - ctx : 0;
  const int nk = (int)(p_abs + 2 - lo);                      // <= ctx + 2
  const float* Kb = K + (lo - row0_pos) * D + h * 64;
  const float* Vb = V + (lo - row0_pos) * D + h * 64;
  const float* qp = q + (2 * pair + w) * D + h * 64;
  float* pr = sm + w * (ctx + 2);
  f32x4 qv[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) qv[i] = *reinterpret_cast<const f32x4*>(qp + 4 * i);
  float mloc = -INFINITY;
  for (int j = lane; j < nk; j += 64) {
    const float* kr = Kb + (int64_t)j * D;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kr + 4 * i);
      a0 = fmaf(qv[i][0], kv[0], a0); a1 = fmaf(qv[i][1], kv[1], a1);
      a2 = fmaf(qv[i][2], kv[2], a2); a3 = fmaf(qv[i][3], kv[3], a3);
    }
    const float sc = ((a0 + a1) + (a2 + a3)) * scale;
    pr[j] = sc;
    mloc = fmaxf(mloc, sc);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mloc = fmaxf(mloc, __shfl_xor(mloc, o, 64));
  float lsum = 0.f;
  for (int j = lane; j < nk; j += 64) {
    const float e = expf(pr[j] - mloc);
    pr[j] = e;
    lsum += e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lsum += __shfl_xor(lsum, o, 64);
  __syncthreads();                                           // the row's probabilities are visible to all of its lanes
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int j = 0;
  for (; j + 4 <= nk; j += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(pr[j + u], Vb[(int64_t)(j + u) * D + lane], acc[u]);
  }
  for (; j < nk; ++j) acc[0] = fmaf(pr[j], Vb[(int64_t)j * D + lane], acc[0]);
  out[(2 * pair + w) * D + h * 64 + lane] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) / lsum;
}

__global__ __launch_bounds__(256) void mimi_conv_out1(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, int64_t T, int C, int K) {
  extern __shared__ float sw[];          // w[K * C]
  for (int i = threadIdx.x; i < K * C; i += 256) sw[i] = w[i];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  float acc = bias ? bias[0] : 0.f;
  for (int k = 0; k < K; ++k) {
    const float* xr = x + (t + k) * C;
    for (int c = 0; c < C; c += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = fmaf(sw[k * C + c + u], elu1(v[u]), acc);
    }
  }
  out[t] = acc;
}

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

}  // namespace

int mimi_embed_launch(const int32_t* codes, int n_q, int64_t n, const float* cb, int bins, int dq, const float* wfT, const float* wrT, float* z,
                      int D, hipStream_t s) {
  if (n <= 0 || n > 0x7fffffff || n_q < 1 || dq <= 0 || dq > 4096 || D <= 0) return -1;
  hipLaunchKernelGGL(mimi_embed, dim3((unsigned)n), dim3(256), (size_t)2 * dq * 4, s, codes, n_q, n, cb, bins, dq, wfT, wrT, z, D);
  return ok();
}

int mimi_upsample_launch(const float* zp, const float* w, float* y, int64_t n, int D, int stride, hipStream_t s) {
  if (n <= 0 || D <= 0 || stride <= 0) return -1;
  const int64_t total = n * stride * D;
  hipLaunchKernelGGL(mimi_upsample, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, s, zp, w, y, n, D, stride);
  return ok();
}

int mimi_qkv_finish_launch(const float* qkv, float* q, float* k_new, float* v_new, int64_t P, int D, int64_t pos0, const double* inv_freq, hipStream_t s) {
  if (P <= 0 || D <= 0 || D % 64 || pos0 < 0) return -1;
  const int64_t total = P * (D / 2);
  hipLaunchKernelGGL(mimi_qkv_finish, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, s, qkv, q, k_new, v_new, P, D, pos0, inv_freq);
  return ok();
}

int mimi_window_attn_launch(const float* q, const float* K, const float* V, float* out, int64_t P, int D, int H, int64_t pos0, int64_t row0_pos,
                            int ctx, float scale, hipStream_t s) {
  // every pair's lowest key must be a row of the history: lo(first pair) = max(0, pos0 - ctx) >= row0_pos
  if (P <= 0 || (P & 1) || (pos0 & 1) || pos0 < 0 || D != H * 64 || ctx < 0 || ctx > 8190 || P / 2 > 0x7fffffff || H > 65535) return -1;
  if ((pos0 > ctx ? pos0 - ctx : 0) < row0_pos || row0_pos < 0) return -1;
  hipLaunchKernelGGL(mimi_window_attn, dim3((unsigned)(P / 2), (unsigned)H), dim3(128), (size_t)2 * (ctx + 2) * 4, s, q, K, V, out, D, pos0, row0_pos, ctx, scale);
  return ok();
}

int mimi_conv_out1_launch(const float* x, const float* w, const float* bias, float* out, int64_t T, int C, int K, hipStream_t s) {
  if (T <= 0 || C <= 0 || C % 4 || K <= 0 || (size_t)K * C * 4 > 48 * 1024) return -1;
  hipLaunchKernelGGL(mimi_conv_out1, dim3((unsigned)((T + 255) / 256)), dim3(256), (size_t)K * C * 4, s, x, w, bias, out, T, C, K);
  return ok();
}
