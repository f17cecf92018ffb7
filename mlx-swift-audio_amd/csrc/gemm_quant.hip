// gemm_quant.hip -- the many-row GEMM on packed 4- / 6- / 8-bit weights (skinny.h: gemm_quant_launch): the LM's batched prompt pass on
// the SAME fragment-ordered arrays the step streams (layout: top of skinny_quant.hip; built once by quant_repack.hip).
#include "skinny_device.h"
#include "skinny_quant_device.h"

// ------------------------------------------------------------------------------------------------
// C[M][N] fp32 = A[M][K] (16 bit, row stride lda) . Wq^T (+ R[M][N]),  w = scale * code + bias per 64-input group, never formed:
//     y[m][n] = sum_g ( s[n][g] * sum_{k in g} code[n][k] a[m][k]  +  t'[n][g] * sum_{k in g} a[m][k] )
// -- the step kernel's arithmetic (skinny_gemm_qi), instruction for instruction within a group: the codes enter the MFMA as the exact
// 16-bit values MAG + q (magic-constant OR; the hi plane of a 6- / 8-bit code in a second accumulator), the group's activation sum comes
// from an MFMA with an all-ones operand, and acc = fma(s, P, fma(t, A, acc)) with t = b - MAG s (resp. b - 17 MAG s) as stored in stfrag.
// What differs is the shape of the work.  skinny_gemm_qi gives a wave 32 rows and splits K over waves and workgroups; here a wave (= a
// workgroup, no LDS, no barrier) owns 16 MT rows x 32 columns (MT = 4 above 32 rows) and walks the WHOLE K range in ascending group
// order:
//   * an unpacked weight fragment (7 VALU instructions) feeds MT = 4 row tiles, and the ones-operand MFMAs of a row tile (2 per group) are
//     shared by the wave's 2 column tiles: per group 16 NP code MFMAs + 8 for the sums, 28 NP unpack + 64 (96 with two planes) fix-up
//     VALU instructions.  The fix-up is two FMAs (three with two planes) per accumulator value against 2 NP MFMAs of 16 cycles per
//     accumulator tile -- 32 (48) VALU cycles against 32 (64) MFMA cycles, so it does not dominate; with the unpack the loop issues
//     92 (152) VALU instructions of 4 cycles beside 24 (40) MFMAs of 16: about balanced at every width.  (Four column tiles per wave
//     halve the share of the ones-operand MFMAs but need more than 256 registers: the MFMA results then sit in AGPRs and every one is
//     copied out before its fix-up, which costs more than it saves);
//   * activations are MFMA ROW fragments loaded straight from the row-major A (16 B per lane), codes and (s, t) pairs 8 B per lane and
//     group from the block's 16 B -- a second wave of the same rows (the next column tile) finds A in L2, the next row tile finds the codes;
//   * a row's result is a function of its own A row only and the K order is fixed, so it does not depend on M, on the row tile it falls
//     into or on MT (tests/test_gemm_quant_gpu.py: rows of an M = 200 call equal the same rows of an M = 33 call bit for bit).
// Rows past M re-read row M - 1 and column tiles past the end re-read the last tile; neither is stored.  R may alias C: every element is
// read and written by the same lane.
// ------------------------------------------------------------------------------------------------
namespace {

constexpr int GQ_NT = 2;      // 16-column tiles per wave

// one 64-input group of a wave's operands
template <int MT, int NP, int HB>
struct GqGrp {
  u32x2 w[GQ_NT];                         // lo plane: K-steps 2 g, 2 g + 1
  u32x2 h4[HB == 4 && NP == 2 ? GQ_NT : 1];   // 8 bit: the hi nibble plane
  uint32_t h2[HB == 2 ? GQ_NT : 1];       // 6 bit: the group's 2-bit hi parts
  f32x2 st[GQ_NT];                        // (s, t) of column r
  s16x8 a[MT][2];
};

// register budget: one plane fits two waves per SIMD (208 VGPRs at MT = 4, accumulators in plain VGPRs).  Two planes at MT = 4 need a few
// registers more than 256 -- capped there the compiler spills 12 to 36 bytes -- so those run one wave per SIMD with the MFMA results in
// AGPRs (160 v_accvgpr_read per two groups on top of the fix-up: the next thing to remove)
template <typename T, int MT, int NP, int HB>
__global__ __launch_bounds__(64, NP == 1 ? 2 : 1) void gemm_quant_k(GemmQuantArgs a) {
  constexpr int NT = GQ_NT;
  constexpr uint32_t BLKB = HB == 2 ? 1536u : 1024u * NP;      // bytes of codes per (tile, 128-input block)
  const int lane = threadIdx.x;
  const int r = lane & 15, c = lane >> 4;
  const int tile0 = blockIdx.x * NT;
  const int m0 = blockIdx.y * (16 * MT);
  const int nblk = a.K >> 7, ngrp = a.K >> 6;
  const int n_tiles = (a.N + 15) >> 4;
  const char* wb[NT];
  const char* sb[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tl = tile0 + t < n_tiles ? tile0 + t : n_tiles - 1;
    wb[t] = reinterpret_cast<const char*>(a.wfrag) + (int64_t)tl * nblk * BLKB;
    sb[t] = reinterpret_cast<const char*>(a.stfrag) + (int64_t)tl * nblk * 256;
  }
  // activations at a wave-uniform base + a 32-bit byte offset per lane (host-checked: A below 4 GiB)
  uint32_t ao[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = m0 + 16 * mt + r;
    ao[mt] = (uint32_t)(((int64_t)(m < a.M ? m : a.M - 1) * a.lda + 8 * c) * 2);
  }
  using Grp = GqGrp<MT, NP, HB>;
  auto load_grp = [&](Grp& b, int gi) {
    const int64_t blk = gi >> 1;
    const uint32_t g = gi & 1;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const char* wp = wb[t] + blk * BLKB;
      b.w[t] = *reinterpret_cast<const u32x2*>(wp + 16u * lane + 8u * g);
      if (HB == 4 && NP == 2) b.h4[NP == 2 && HB == 4 ? t : 0] = *reinterpret_cast<const u32x2*>(wp + 1024u + 16u * lane + 8u * g);
      if (HB == 2) b.h2[HB == 2 ? t : 0] = *reinterpret_cast<const uint32_t*>(wp + 1024u + 8u * lane + 4u * g);
      b.st[t] = *reinterpret_cast<const f32x2*>(sb[t] + blk * 256 + 16u * r + 8u * g);
    }
    const char* ab = reinterpret_cast<const char*>(a.A) + (int64_t)gi * 128;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      b.a[mt][0] = *reinterpret_cast<const s16x8*>(ab + ao[mt]);
      b.a[mt][1] = *reinterpret_cast<const s16x8*>(ab + ao[mt] + 64);
    }
  };
  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  const s16x8 ones = __builtin_bit_cast(s16x8, (u32x4){QMagic<T>::one, QMagic<T>::one, QMagic<T>::one, QMagic<T>::one});
  auto unpack2 = [](uint32_t word) -> s16x8 {    // 8 hi parts of 2 bits (the word already shifted to the K-step's four pair slots) -> 8 x (MAG + hi)
    return __builtin_bit_cast(s16x8, (u32x4){(word & 0x00030003u) | QMagic<T>::pair, ((word >> 2) & 0x00030003u) | QMagic<T>::pair,
                                             ((word >> 4) & 0x00030003u) | QMagic<T>::pair, ((word >> 6) & 0x00030003u) | QMagic<T>::pair});
  };
  auto mma_grp = [&](const Grp& b) {
    f32x4 As[MT];      // As[mt][i] = sum of the group's 64 activations of row 16 mt + 4 c + i
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) { As[mt] = T::mfma16(b.a[mt][0], ones, zero4); As[mt] = T::mfma16(b.a[mt][1], ones, As[mt]); }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      s16x8 f0[NP], f1[NP];
      f0[0] = q_unpack<T>(b.w[t][0]); f1[0] = q_unpack<T>(b.w[t][1]);
      if (NP == 2) {
        if (HB == 2) { const uint32_t hw = b.h2[HB == 2 ? t : 0]; f0[NP - 1] = unpack2(hw); f1[NP - 1] = unpack2(hw >> 8); }
        else { f0[NP - 1] = q_unpack<T>(b.h4[NP == 2 && HB == 4 ? t : 0][0]); f1[NP - 1] = q_unpack<T>(b.h4[NP == 2 && HB == 4 ? t : 0][1]); }
      }
      const float sc = b.st[t][0], tt = b.st[t][1];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        f32x4 P[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) { P[p] = T::mfma16(b.a[mt][0], f0[p], zero4); P[p] = T::mfma16(b.a[mt][1], f1[p], P[p]); }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float pv = NP == 2 ? __builtin_fmaf(16.0f, P[NP - 1][i], P[0][i]) : P[0][i];
          acc[t][mt][i] = __builtin_fmaf(sc, pv, __builtin_fmaf(tt, As[mt][i], acc[t][mt][i]));
        }
      }
    }
  };
  // two register groups: the next group's loads are in flight behind the one being multiplied (K % 128 == 0: an even number of groups)
  Grp g0, g1;
  load_grp(g0, 0);
  for (int i = 0; i < ngrp; i += 2) {
    load_grp(g1, i + 1);
    mma_grp(g0);
    if (i + 2 < ngrp) load_grp(g0, i + 2);
    mma_grp(g1);
  }
  // lane (r, c) holds C[m0 + 16 mt + 4 c + i][16 (tile0 + t) + r]
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = 16 * (tile0 + t) + r;
    if (n >= a.N) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * mt + 4 * c + i;
        if (m >= a.M) continue;
        float v = acc[t][mt][i];
        if (a.R) v += a.R[(int64_t)m * a.ldr + n];
        a.C[(int64_t)m * a.ldc + n] = v;
      }
  }
}

template <typename T, int NP, int HB>
void gemm_quant_go(const GemmQuantArgs& a, hipStream_t s) {
  const unsigned gx = (unsigned)(((a.N + 15) / 16 + GQ_NT - 1) / GQ_NT);
  // the row tile follows M only to skip MFMAs on rows that do not exist: a row's result is the same in every form
  if (a.M > 32) hipLaunchKernelGGL((gemm_quant_k<T, 4, NP, HB>), dim3(gx, (unsigned)((a.M + 63) / 64)), dim3(64), 0, s, a);
  else if (a.M > 16) hipLaunchKernelGGL((gemm_quant_k<T, 2, NP, HB>), dim3(gx, 1), dim3(64), 0, s, a);
  else hipLaunchKernelGGL((gemm_quant_k<T, 1, NP, HB>), dim3(gx, 1), dim3(64), 0, s, a);
}

template <typename T>
void gemm_quant_go_t(const GemmQuantArgs& a, int bits, hipStream_t s) {
  if (bits == 8) gemm_quant_go<T, 2, 4>(a, s);
  else if (bits == 6) gemm_quant_go<T, 2, 2>(a, s);
  else gemm_quant_go<T, 1, 4>(a, s);
}

}  // namespace

const char* gemm_quant_check(const GemmQuantArgs& a, int bits, int dtype) {
  if (dtype != MIA_BF16 && dtype != MIA_F16) return "gemm_quant: dtype must be MIA_BF16 or MIA_F16";
  if (bits != 4 && bits != 6 && bits != 8) return "gemm_quant: bits must be 4, 6 or 8";
  if (!a.A || !a.wfrag || !a.stfrag || !a.C) return "gemm_quant: null pointer";
  if (a.M <= 0 || a.N <= 0 || a.K <= 0) return "gemm_quant: M, N, K must be positive";
  if (a.K % 128 != 0) return "gemm_quant: K must be a multiple of 128";
  if (a.M > 65535 * 64) return "gemm_quant: M must stay below 65535 * 64";
  if (a.lda < a.K || a.lda % 8 != 0) return "gemm_quant: lda must cover the row and be a multiple of 8";
  if (a.ldc < a.N || (a.R && a.ldr < a.N)) return "gemm_quant: ldc / ldr must cover the row";
  if ((uint64_t)a.M * (uint64_t)a.lda * 2 > 0xffffffffull) return "gemm_quant: A must stay below 4 GiB";      // 32-bit byte offsets into A
  if (((uintptr_t)a.A | (uintptr_t)a.wfrag | (uintptr_t)a.stfrag) & 15) return "gemm_quant: A, wfrag and stfrag must be 16-byte aligned";
  if (((uintptr_t)a.C | (uintptr_t)a.R) & 3) return "gemm_quant: C and R must be 4-byte aligned";
  return nullptr;
}

int gemm_quant_launch(const GemmQuantArgs& a, int bits, int dtype, hipStream_t s) {
  if (gemm_quant_check(a, bits, dtype)) return -1;
  if (dtype == MIA_F16) gemm_quant_go_t<F16>(a, bits, s); else gemm_quant_go_t<BF16>(a, bits, s);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
