// host_convert.h -- the host's conversions between fp32 and the two 16-bit formats: the only copy.  Plain C++ (no HIP header); the
// loaders reach it through tensor_loader.h.  tests/test_tensor_loader.py pins all four against numpy / torch.
#pragma once
#include <stdint.h>
#include <string.h>

// round to nearest even; a NaN stays a NaN (the quiet bit is set, so a payload in the low half cannot round to inf or zero)
inline uint16_t f32_to_bf16(float f) {
  uint32_t u; memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1);
  return (uint16_t)(u >> 16);
}
inline uint16_t f32_to_f16(float f) { const _Float16 h = (_Float16)f; uint16_t r; memcpy(&r, &h, 2); return r; }   // RNE
inline float f16_to_f32(uint16_t h) { _Float16 x; memcpy(&x, &h, 2); return (float)x; }
inline float bf16_to_f32(uint16_t h) { const uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }
