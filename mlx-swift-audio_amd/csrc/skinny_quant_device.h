// skinny_quant_device.h -- what the packed-weight skinny GEMMs share (skinny_quant.hip: the LM step, row-major activations;
// skinny_frag_quant.hip: the Whisper step, fragment-order activations): the fragment-ordered arrays and the magic constants, used by both;
// and the magic-constant unpack, the per-block code arithmetic and the three-block register ring in the form the Whisper kernel calls.
// skinny_gemm_qi keeps its own copy of those three as lambdas: calling these instead changes its register allocation in 118 of its 208
// variants (+-4 VGPRs, other spill counts in the 16-wave ones), and the LM step's time rests on them -- merge only with an A/B of the LM step.
#pragma once
#include "skinny_device.h"

struct QFrag { const uint32_t* wfrag; const float* stfrag; };

template <typename T> struct QMagic;
template <> struct QMagic<BF16> { static constexpr uint32_t pair = 0x43004300u; static constexpr uint32_t one = 0x3f803f80u; };   // 128 + q; 1.0
template <> struct QMagic<F16> { static constexpr uint32_t pair = 0x64006400u; static constexpr uint32_t one = 0x3c003c00u; };    // 1024 + q; 1.0

// one 128-input block of a wave's operands: NT tiles x NP nibble planes of code words, the tiles' (s, t) of the block's two groups, and
// the activation fragments of its 4 K-steps (a1: rows 16..31, unused when M16)
template <int NT, int NP>
struct QBlk { u32x4 w[NT][NP]; f32x4 st[NT]; s16x8 a0[4], a1[4]; };

template <typename T>
__device__ __forceinline__ s16x8 q_unpack(uint32_t word) {     // 8 codes -> 8 x (MAG + q) in K order
  return __builtin_bit_cast(s16x8, (u32x4){(word & 0x000f000fu) | QMagic<T>::pair, ((word >> 4) & 0x000f000fu) | QMagic<T>::pair,
                                           ((word >> 8) & 0x000f000fu) | QMagic<T>::pair, ((word >> 12) & 0x000f000fu) | QMagic<T>::pair});
}

// acc += the block's contribution: per group, integer-code MFMAs into P (one accumulator per nibble plane), the activation sum A through
// an all-ones operand, then acc += s P + t A (P = P_lo + 16 P_hi with two planes).  Activations are the MFMA's ROW operand.
template <typename T, int NT, int NP, bool M16>
__device__ __forceinline__ void q_mma_blk(const QBlk<NT, NP>& b, f32x4 (&acc)[NT][2]) {
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  const s16x8 ones = __builtin_bit_cast(s16x8, (u32x4){QMagic<T>::one, QMagic<T>::one, QMagic<T>::one, QMagic<T>::one});
#pragma unroll
  for (int g = 0; g < 2; ++g) {
    // A[i] = sum of the group's 64 activations of row 4 c + i
    f32x4 A0 = T::mfma16(b.a0[2 * g], ones, zero4), A1 = zero4;
    A0 = T::mfma16(b.a0[2 * g + 1], ones, A0);
    if (!M16) { A1 = T::mfma16(b.a1[2 * g], ones, zero4); A1 = T::mfma16(b.a1[2 * g + 1], ones, A1); }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      f32x4 P0[NP], P1[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const s16x8 f0 = q_unpack<T>(b.w[t][p][2 * g]), f1 = q_unpack<T>(b.w[t][p][2 * g + 1]);
        P0[p] = T::mfma16(b.a0[2 * g], f0, zero4);
        P0[p] = T::mfma16(b.a0[2 * g + 1], f1, P0[p]);
        if (!M16) { P1[p] = T::mfma16(b.a1[2 * g], f0, zero4); P1[p] = T::mfma16(b.a1[2 * g + 1], f1, P1[p]); }
      }
      const float sc = b.st[t][2 * g], tt = b.st[t][2 * g + 1];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p0 = NP == 2 ? __builtin_fmaf(16.0f, P0[NP - 1][i], P0[0][i]) : P0[0][i];
        acc[t][0][i] = __builtin_fmaf(sc, p0, __builtin_fmaf(tt, A0[i], acc[t][0][i]));
        if (!M16) {
          const float p1 = NP == 2 ? __builtin_fmaf(16.0f, P1[NP - 1][i], P1[0][i]) : P1[0][i];
          acc[t][1][i] = __builtin_fmaf(sc, p1, __builtin_fmaf(tt, A1[i], acc[t][1][i]));
        }
      }
    }
  }
}

// blocks b0 .. b0 + bc - 1 of a wave through a ring of three register blocks (each 4 K-steps = two groups deep): two blocks of loads in
// flight behind the one being multiplied.  load(blk_regs, block index) issues a block's loads; behind_first_loads() runs once, after the
// first two blocks are in flight (small loads of the epilogue ride under the weight stream there).
template <typename T, int NT, int NP, bool M16, typename Load, typename Behind>
__device__ __forceinline__ void q_block_ring(int b0, int bc, f32x4 (&acc)[NT][2], Load&& load, Behind&& behind_first_loads) {
  QBlk<NT, NP> k0, k1, k2;
  if (bc > 0) load(k0, b0);
  if (bc > 1) load(k1, b0 + 1);
  behind_first_loads();
  for (int i = 0; i < bc; i += 3) {
    if (i + 2 < bc) load(k2, b0 + i + 2);
    q_mma_blk<T, NT, NP, M16>(k0, acc);
    if (i + 1 >= bc) break;
    if (i + 3 < bc) load(k0, b0 + i + 3);
    q_mma_blk<T, NT, NP, M16>(k1, acc);
    if (i + 2 >= bc) break;
    if (i + 4 < bc) load(k1, b0 + i + 4);
    q_mma_blk<T, NT, NP, M16>(k2, acc);
  }
}
