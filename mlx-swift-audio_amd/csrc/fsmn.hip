// fsmn.hip -- the SANM memory: a depthwise Conv1d over time on the un-projected values, plus the values themselves, added into the fp32
// residual stream (MultiHeadAttentionSANM.forwardFSMN, STT/FunASR/Layers/MultiHeadAttentionSANM.swift:90-116, added after the attention
// at :174):   x[t][c] += v[t][c] + sum_k w[k][c] * v[t + k - left][c],   taps outside [0, len) read zero,
// with left = (K - 1) / 2 + sanm_shift (:73-79).  v is the 16-bit q | k | v GEMM output (any row stride), w fp32 [K][D], K a runtime value.
// Sequences are stacked [B][T] with an optional per-sequence length: no tap crosses a sequence's end (the reference masks v before
// the convolution, :101), and rows at or beyond the length are left alone.  One thread = 4 channels of one row; the taps are summed in
// k order into one fp32 accumulator, so a row's bits do not depend on the stack it sits in.
#include "mia_device.h"
#include "ops.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void fsmn_add_kernel(FsmnArgs a) {
  const int c4n = a.D >> 2;
  const int64_t total = (int64_t)a.B * a.T * c4n;
  const uint16_t* V = reinterpret_cast<const uint16_t*>(a.v);
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / c4n;
    const int c = (int)(e - row * c4n) * 4;
    const int b = (int)(row / a.T), t = (int)(row - (int64_t)b * a.T);
    const int Tb = a.seq_len ? min(a.T, a.seq_len[b]) : a.T;
    if (t >= Tb) continue;
    const uint16_t* vb = V + (int64_t)b * a.T * a.ldv + c;
    auto load4 = [&](int ts, float (&o)[4]) {
      const u32x2 p = *reinterpret_cast<const u32x2*>(vb + (int64_t)ts * a.ldv);
      o[0] = T::to_f32((uint16_t)(p[0] & 0xffffu)); o[1] = T::to_f32((uint16_t)(p[0] >> 16));
      o[2] = T::to_f32((uint16_t)(p[1] & 0xffffu)); o[3] = T::to_f32((uint16_t)(p[1] >> 16));
    };
    float acc[4];
    load4(t, acc);
    const int k_lo = max(0, a.left - t), k_hi = min(a.K, Tb - t + a.left);     // 0 <= t + k - left < Tb
    for (int k = k_lo; k < k_hi; ++k) {
      float vv[4];
      load4(t + k - a.left, vv);
      const f32x4 wk = *reinterpret_cast<const f32x4*>(a.w + (int64_t)k * a.D + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = fmaf(wk[j], vv[j], acc[j]);
    }
    f32x4* xp = reinterpret_cast<f32x4*>(a.x + row * a.ldx + c);
    f32x4 xv = *xp;
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[j] += acc[j];
    *xp = xv;
  }
}

}  // namespace

const char* mia_fsmn_check(const FsmnArgs& a) {
  if (a.B <= 0 || a.T <= 0 || a.D <= 0 || a.K <= 0) return "fsmn_add: B, T, D, K must be > 0";
  if (!a.x || !a.v || !a.w) return "fsmn_add: null operand";
  if (a.dtype != MIA_BF16 && a.dtype != MIA_F16) return "fsmn_add: dtype must be MIA_BF16 or MIA_F16";
  if (a.left < 0 || a.left > a.K - 1) return "fsmn_add: left context must lie in [0, K - 1] (right = K - 1 - left >= 0)";
  if (a.D % 4 || a.ldx % 4 || a.ldv % 4 || a.ldx < a.D || a.ldv < a.D) return "fsmn_add: D and the row strides must be multiples of 4, strides >= D";
  if (((uintptr_t)a.x & 15) || ((uintptr_t)a.w & 15) || ((uintptr_t)a.v & 7)) return "fsmn_add: x, w must be 16-byte and v 8-byte aligned";
  return nullptr;
}

int mia_fsmn_launch(const FsmnArgs& a, hipStream_t s) {
  const int64_t total = (int64_t)a.B * a.T * (a.D >> 2);
  const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  if (a.dtype == MIA_F16) hipLaunchKernelGGL((fsmn_add_kernel<F16>), dim3(blocks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((fsmn_add_kernel<BF16>), dim3(blocks), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
