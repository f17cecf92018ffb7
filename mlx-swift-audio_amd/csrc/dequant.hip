// dequant.hip -- MLX affine 4 / 6 / 8-bit (group 64) de-quantisation of checkpoint tensors at load time.
//
// The reference's default checkpoints are quantised (`quantize(model:) { (64, bits, .affine) }`, STT/Whisper/WhisperModel.swift:189-196;
// TTS/Orpheus/TTSEngine/OrpheusWeightLoader.swift): a Linear / Embedding stores `weight` as uint32 words holding 32/bits codes each
// (code j of a word in bits [j*bits, (j+1)*bits), little end first, along the input axis), plus per-group `scales` and `biases`
// (group = 64 consecutive inputs):  w[o][i] = scales[o][i/64] * code[o][i] + biases[o][i/64].
// 6-bit codes (Marvis' published checkpoints) do not divide a word: a row is one little-endian bit stream, code k in bits [6 k, 6 k + 6)
// of the row's bytes -- 16 codes per 3 words, a group of 64 in 12 whole words.
// MLX evaluates this inside its quantised matmul; here the weights are expanded ONCE to the 16-bit (or fp32) storage type the GEMMs
// stream -- HBM-bound, one pass: 0.5 / 1 byte read and 2 bytes written per weight.
#include "mia_device.h"
#include "mia_internal.h"

namespace {

__device__ __forceinline__ float load_scale(const void* p, int64_t i, int dt) {
  if (dt == MIA_F32) return reinterpret_cast<const float*>(p)[i];
  const uint16_t v = reinterpret_cast<const uint16_t*>(p)[i];
  return dt == MIA_F16 ? F16::to_f32(v) : BF16::to_f32(v);
}

// one thread per uint32 word: 8 (4-bit) or 4 (8-bit) outputs, all in one group (64 % (32/bits) == 0)
template <int BITS>
__global__ __launch_bounds__(256) void dequant_affine_kernel(const uint32_t* __restrict__ wq, const void* __restrict__ scales,
                                                             const void* __restrict__ biases, int64_t rows, int64_t cols, int group,
                                                             int sdt, void* __restrict__ out, int odt) {
  constexpr int PER = 32 / BITS;
  const int64_t words_per_row = cols / PER;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * words_per_row) return;
  const int64_t r = e / words_per_row, wi = e % words_per_row;
  const uint32_t word = wq[e];
  const int64_t c0 = wi * PER;
  const int64_t g = r * (cols / group) + c0 / group;
  const float sc = load_scale(scales, g, sdt), bs = load_scale(biases, g, sdt);
  float v[PER];
#pragma unroll
  for (int j = 0; j < PER; ++j) v[j] = fmaf(sc, (float)((word >> (j * BITS)) & ((1u << BITS) - 1u)), bs);
  const int64_t o = r * cols + c0;
  if (odt == MIA_F32) {
#pragma unroll
    for (int j = 0; j < PER; ++j) reinterpret_cast<float*>(out)[o + j] = v[j];
  } else {
    uint16_t* op = reinterpret_cast<uint16_t*>(out) + o;
#pragma unroll
    for (int j = 0; j < PER; ++j) op[j] = odt == MIA_F16 ? F16::from_f32(v[j]) : BF16::from_f32(v[j]);
  }
}

// 6 bit: one thread per 3 words = 16 codes (96 bits), all in one group (64 % 16 == 0); code j of the triple starts at bit 6 j
__global__ __launch_bounds__(256) void dequant_affine6_kernel(const uint32_t* __restrict__ wq, const void* __restrict__ scales,
                                                              const void* __restrict__ biases, int64_t rows, int64_t cols, int group,
                                                              int sdt, void* __restrict__ out, int odt) {
  const int64_t per_row = cols / 16;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * per_row) return;
  const int64_t r = e / per_row, c0 = (e % per_row) * 16;
  const uint32_t w0 = wq[3 * e], w1 = wq[3 * e + 1], w2 = wq[3 * e + 2];
  const uint64_t lo = (uint64_t)w0 | ((uint64_t)w1 << 32), hi = (uint64_t)w1 | ((uint64_t)w2 << 32);     // bits [0, 64) and [32, 96)
  const int64_t g = r * (cols / group) + c0 / group;
  const float sc = load_scale(scales, g, sdt), bs = load_scale(biases, g, sdt);
  const int64_t o = r * cols + c0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t q = (uint32_t)(6 * j + 6 <= 64 ? lo >> (6 * j) : hi >> (6 * j - 32)) & 63u;
    const float v = fmaf(sc, (float)q, bs);
    if (odt == MIA_F32) reinterpret_cast<float*>(out)[o + j] = v;
    else reinterpret_cast<uint16_t*>(out)[o + j] = odt == MIA_F16 ? F16::from_f32(v) : BF16::from_f32(v);
  }
}

}  // namespace

extern "C" int mia_dequant_affine(mia_ctx* ctx, const uint32_t* wq, const void* scales, const void* biases, int64_t rows, int64_t cols,
                                  int group_size, int bits, int scale_dtype, void* out, int out_dtype, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, wq && scales && biases && out && rows > 0 && cols > 0, "dequant_affine: null / empty argument");
  MIA_CHECK_ARG(ctx, bits == 4 || bits == 6 || bits == 8, "dequant_affine: bits must be 4, 6 or 8");
  MIA_CHECK_ARG(ctx, group_size > 0 && group_size % (bits == 6 ? 16 : 32 / bits) == 0 && cols % group_size == 0, "dequant_affine: cols must be a multiple of group_size");
  MIA_CHECK_ARG(ctx, bits != 6 || cols % 64 == 0, "dequant_affine: 6-bit rows must be a multiple of 64 codes");
  MIA_CHECK_ARG(ctx, (scale_dtype == MIA_F32 || scale_dtype == MIA_F16 || scale_dtype == MIA_BF16) &&
                         (out_dtype == MIA_F32 || out_dtype == MIA_F16 || out_dtype == MIA_BF16), "dequant_affine: bad dtype");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "dequant_affine: bad mem");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  HostIo io(ctx, mem);
  const int64_t words = rows * cols * bits / 32, groups = rows * (cols / group_size);
  const size_t ssz = scale_dtype == MIA_F32 ? 4 : 2, osz = out_dtype == MIA_F32 ? 4 : 2;
  const size_t w_bytes = (size_t)words * 4, s_bytes = groups * ssz, o_bytes = (size_t)rows * cols * osz;
  Carve cv;
  const size_t o_w = cv.add(io.staged(w_bytes)), o_s = cv.add(io.staged(s_bytes)), o_b = cv.add(io.staged(s_bytes)), o_o = cv.add(io.staged(o_bytes));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  const uint32_t* d_w = io.in(wq, ws + o_w, w_bytes);
  const void* d_s = io.in(scales, ws + o_s, s_bytes);
  const void* d_b = io.in(biases, ws + o_b, s_bytes);
  void* d_o = io.out(out, ws + o_o, o_bytes);
  const unsigned grid = (unsigned)((words + 255) / 256);
  if (bits == 6) hipLaunchKernelGGL(dequant_affine6_kernel, dim3((unsigned)((words / 3 + 255) / 256)), dim3(256), 0, s, d_w, d_s, d_b, rows, cols, group_size, scale_dtype, d_o, out_dtype);
  else if (bits == 4) hipLaunchKernelGGL(dequant_affine_kernel<4>, dim3(grid), dim3(256), 0, s, d_w, d_s, d_b, rows, cols, group_size, scale_dtype, d_o, out_dtype);
  else hipLaunchKernelGGL(dequant_affine_kernel<8>, dim3(grid), dim3(256), 0, s, d_w, d_s, d_b, rows, cols, group_size, scale_dtype, d_o, out_dtype);
  MIA_HIP(ctx, hipGetLastError());
  return io.finish();
}
