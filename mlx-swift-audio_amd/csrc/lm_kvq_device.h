// lm_kvq_device.h -- device code the quantised KV cache's kernels share: the quantiser of one 64-group (lm_kvq.hip states the rule), the
// loaders of a lane's code dwords and the two ways a lane's 8 codes are read -- as values (scale * code + bias, lm_kvq.hip) or as the
// 16-bit numbers equal to the codes, the matrix-core operands of lm_prefill_attn_kvq.hip and lm_step_attn_kvq.hip.
#pragma once
#include "mia_device.h"

// One group of 64 values, one per lane of a full wave: returns the value read back; `word` = the code dword this lane's 32 / BITS
// neighbours share (identical in all of them), `pair` = scale | bias << 16.
template <typename T, int BITS>
__device__ __forceinline__ float kvq_group(float x, int lane, uint32_t& word, uint32_t& pair) {
  constexpr float n = (float)((1 << BITS) - 1);
  const float hi = wave_max(x), lo = -wave_max(-x);
  const float sc = hi == lo ? 1.0f : (hi - lo) / n;
  const uint16_t s16 = T::from_f32(sc), b16 = T::from_f32(lo);
  const float s = T::to_f32(s16), b = T::to_f32(b16);
  const float code = fminf(fmaxf(rintf((x - b) / s), 0.0f), n);
  int w = (int)code << (BITS * (lane & (32 / BITS - 1)));
  w |= dpp_i32<0xB1>(w);                        // lanes xor 1, xor 2: the quad's codes
  w |= dpp_i32<0x4E>(w);
  if (BITS == 4) w |= dpp_i32<0x141>(w);        // half-row mirror: the other quad of the 8 lanes
  word = (uint32_t)w;
  pair = (uint32_t)s16 | ((uint32_t)b16 << 16);
  return s * code + b;
}

// a lane's 8 consecutive elements of one cached row
template <typename T, int BITS>
__device__ __forceinline__ void kvq_dq8(const uint32_t (&w)[BITS / 4], uint32_t pair, float (&x)[8]) {
  const float s = T::to_f32((uint16_t)(pair & 0xffffu)), b = T::to_f32((uint16_t)(pair >> 16));
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t code = BITS == 4 ? (w[0] >> (4 * j)) & 15u : (w[j >> 2] >> (8 * (j & 3))) & 255u;
    x[j] = s * (float)code + b;
  }
}

template <int BITS>
__device__ __forceinline__ void kvq_load(const uint32_t* __restrict__ row, int c, uint32_t (&w)[BITS / 4]) {
  if constexpr (BITS == 4) w[0] = row[c];
  else { const u32x2 v = *reinterpret_cast<const u32x2*>(row + 2 * c); w[0] = v[0]; w[1] = v[1]; }
}

// a thread's 8 consecutive codes of a row as fp32
template <int BITS>
__device__ __forceinline__ void codes8(const uint32_t (&w)[BITS / 4], float (&x)[8]) {
  if constexpr (BITS == 4) {
    const uint32_t lo = w[0] & 0x0f0f0f0fu, hi = (w[0] >> 4) & 0x0f0f0f0fu;      // even / odd elements, one per byte
#pragma unroll
    for (int i = 0; i < 4; ++i) { x[2 * i] = (float)((lo >> (8 * i)) & 255u); x[2 * i + 1] = (float)((hi >> (8 * i)) & 255u); }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (float)((w[j >> 2] >> (8 * (j & 3))) & 255u);
  }
}

// two integers 0 .. 255 -> two 16-bit numbers (exact: bf16 is the fp32's high half, f16 rounds nothing below 2048)
template <typename T>
__device__ __forceinline__ uint32_t pack_codes(float lo, float hi);
template <>
__device__ __forceinline__ uint32_t pack_codes<BF16>(float lo, float hi) { return (__float_as_uint(lo) >> 16) | (__float_as_uint(hi) & 0xffff0000u); }
template <>
__device__ __forceinline__ uint32_t pack_codes<F16>(float lo, float hi) { return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(lo, hi)); }

template <int BITS>
__device__ __forceinline__ void load_codes(const uint32_t* __restrict__ p, uint32_t (&w)[BITS / 4]) {
  if constexpr (BITS == 4) w[0] = *p;
  else { const u32x2 v = *reinterpret_cast<const u32x2*>(p); w[0] = v[0]; w[1] = v[1]; }
}

// a thread's 8 consecutive codes of a row as the four dwords of 16-bit numbers equal to them: one MFMA operand fragment
template <typename T, int BITS>
__device__ __forceinline__ u32x4 codes8_pack(const uint32_t (&w)[BITS / 4]) {
  float x[8];
  codes8<BITS>(w, x);
  u32x4 r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = pack_codes<T>(x[2 * j], x[2 * j + 1]);
  return r;
}
