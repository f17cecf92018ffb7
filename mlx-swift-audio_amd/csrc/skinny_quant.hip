// skinny_quant.hip -- the LM step's skinny GEMM on packed 4- / 6- / 8-bit weights (skinny.h: skinny_gemm_q_launch).
#include "skinny_device.h"
#include "skinny_quant_device.h"

// ------------------------------------------------------------------------------------------------
// The same skinny GEMM on MLX-affine quantised weights (group 64: w = scale * code + bias; 4-, 6- or 8-bit codes), multiplied PACKED: the
// step streams ~5 (or ~7, ~9) bits per weight from HBM instead of 16.  Replaces MLX's quantizedMatmul on the reference's default
// checkpoints (TTS/Orpheus/TTSEngine/OrpheusWeightLoader.swift:28-60, STT/Whisper/WhisperModel.swift:189-200; 4- and 8-bit:
// Models/TranscriptionResult.swift:162-198).
//
// Arithmetic (the one MLX's own qmv / qmm kernels use: scale * sum(code * x) + bias * sum(x) per group): the MFMA runs on the integer
// CODES, which are exact in 16-bit floating point, and scale / bias are applied once per 64-input group to the group's partial sums:
//     y[m][n] = sum_g ( s[n][g] * sum_{k in g} code[n][k] a[m][k]  +  b[n][g] * sum_{k in g} a[m][k] )
// -- no per-weight de-quantisation at all.  A 4-bit code becomes a 16-bit float by OR-ing it into the mantissa of a magic constant
// (bf16 0x4300 | q = 128 + q, f16 0x6400 | q = 1024 + q): with the nibbles stored so that (word >> 4 i) & 0x000f000f isolates the
// codes of K-values 2 i and 2 i + 1, a lane's 8 MFMA operand values cost 7 VALU instructions (the first form of this kernel expanded
// fmaf(scale, code, bias) and re-rounded per weight: 28 to 32 instructions per MFMA, and at one wave per SIMD the kernel ran at the VALU
// issue latency -- 14 us for the 27 MB gate|up matrix of Orpheus-3B, 1.9 TB/s).  The magic offset is removed in the group fix-up:
// sum (MAG + q) a = MAG A + sum q a, so y += s P + t A with t = b - MAG s (fp32, built at attach time) and A = sum_k a[m][k] -- itself
// an MFMA with an all-ones operand, shared by the tiles of a wave.  An 8-bit code is two 4-bit planes, q = 16 hi + lo: the hi plane goes
// through the same unpack + MFMA into its own accumulator, P = P_lo + 16 P_hi and t = b - 17 MAG s.  A 6-bit code (Marvis' published
// checkpoints, TTS/Marvis/MarvisTTS.swift:220-226) is the same with a hi plane of 2 bits, hi = q >> 4 in 0..3: stored sixteen to a word so
// that (word >> 2 i) & 0x00030003 isolates the hi parts of two adjacent K-values, a lane's 8 operand values again cost 7 VALU
// instructions; everything behind the unpack is the 8-bit arithmetic (two accumulators, fma(16, P_hi, P_lo), t = b - 17 MAG s), and the
// codes streamed are 6 bits per weight exactly.
//
// HBM layout (built once at attach, lm_load.hip:q_repack):
//   wfrag  [tile = n/16][blk = k/128][plane][lane = 16 c + r][4 words]: word st of lane (r, c) = the plane's nibbles of
//          W[16 tile + r][128 blk + 32 st + 8 c .. +7], nibble of K-value 2 i at bits [4 i, 4 i + 4), of 2 i + 1 at bits [16 + 4 i, ..)
//   6 bit: [tile][blk] is 1536 B -- the lo plane as above (1024 B), then the hi plane [lane = 16 c + r][2 words] (512 B): word g of lane
//          (r, c) = the 2-bit hi parts of the lane's 16 K-values of group g (K-steps st = 2 g and 2 g + 1), pair slot j = 4 (st & 1) + i:
//          W[16 tile + r][128 blk + 32 st + 8 c + 2 i] at bits [2 j, 2 j + 2), its neighbour 2 i + 1 at bits [16 + 2 j, ..)
//   stfrag [tile][blk][row r][4] fp32: (s, t) of the block's two groups -- the weights are the MFMA's COLUMN operand, so a lane's four
//          accumulator values share one output column and one 16-byte load per block brings its scale and offset
// Results agree with the 16-bit step on the de-quantised checkpoint to the rounding of the de-quantised weights to 16 bit (this form
// does not round them at all); tests/test_lm_gpu.py compares both with the fp32 oracle.
// ------------------------------------------------------------------------------------------------
// Epilogue of the transposed accumulator layout (activations are the MFMA's row operand here): lane (r, c) holds
// C[m = m0 + 16 mt + 4 c + i][n = n0 + 16 t + r], i = 0..3 -- one output column per lane, so scale / offset are per-lane scalars.
template <typename T, int MODE, int NT>
__device__ __forceinline__ void skinny_store_tr(const SkinnyArgs& a, const f32x4 (&acc)[NT][2], int n0, int m0, int split, int lane, const float* rs) {
  const int r = lane & 15, c = lane >> 4;
  const bool scaled = a.ss_in != nullptr;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + r;
    const bool nv = n < a.N;
    const float bs = (MODE != SK_PARTIAL && a.bias && nv) ? a.bias[n] : 0.f;
    const float wn = (MODE == SK_RESID && nv) ? a.nw[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int mr = 16 * mt + 4 * c + i, m = m0 + mr;
        const bool mv = m < a.M;
        const float raw = scaled ? acc[t][mt][i] * (mv ? rs[mr] : 0.f) : acc[t][mt][i];
        float v = raw + bs;
        if (MODE == SK_SWIGLU) {                 // interleaved rows: even column = gate, odd column = up (the neighbouring lane)
          const float u = dpp_f32<0xB1>(v);      // quad_perm [1, 0, 3, 2]: every lane executes the exchange
          if (nv && mv && !(r & 1)) reinterpret_cast<uint16_t*>(a.out)[(int64_t)m * a.ldo + (n >> 1)] = T::from_f32((v / (1.0f + __expf(-v))) * u);
          continue;
        }
        if (MODE == SK_RESID) {                  // x += acc; next activation = x * norm weight; the tile's sum of squares (16 lanes of a DPP row)
          float x = 0.f;
          if (nv && mv) {
            float* xp = a.xres + (int64_t)m * a.N + n;
            x = *xp + v;
            *xp = x;
            reinterpret_cast<uint16_t*>(a.out)[(int64_t)m * a.ldo + n] = T::from_f32(x * wn);
          }
          float q = x * x;
          q += dpp_f32<0xB1>(q); q += dpp_f32<0x4E>(q); q += dpp_f32<0x141>(q); q += dpp_f32<0x140>(q);     // fixed butterfly: every lane of the row holds the sum
          if (r == 0 && mv) a.ss_out[(int64_t)((n0 >> 4) + t) * a.M + m] = q;
          continue;
        }
        if (!nv || !mv) continue;
        if (MODE == SK_PARTIAL) reinterpret_cast<float*>(a.out)[((int64_t)split * a.M + m) * a.N + n] = raw;
        else if (MODE == SK_OUTF32) reinterpret_cast<float*>(a.out)[(int64_t)m * a.ldo + n] = v;
        else reinterpret_cast<uint16_t*>(a.out)[(int64_t)m * a.ldo + n] = T::from_f32(v);
      }
    }
  }
}

// M16: at most 16 rows (single-sequence decode, small batches): the second 16-row MFMA half and its activation loads are skipped
// NP: planes per code (1 = 4-bit, 2 = 6- and 8-bit); HB: bits per code of the hi plane (4 = a nibble plane like the lo one, 16 B per lane
// and block; 2 = the 6-bit form's, 8 B per lane and block)
template <typename T, int MODE, int NT, int NW, bool M16, int NP, int HB>
__global__ __launch_bounds__(64 * NW) void skinny_gemm_qi(SkinnyArgs a, QFrag q) {
  __shared__ float rs[32];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile0 = blockIdx.x * NT;
  const int n0 = tile0 * 16;
  const int split = blockIdx.y;
  const int m0 = blockIdx.z * 32;
  const int nblk = a.K >> 7;                      // 128-input blocks per row
  const int bc = nblk / (a.S * NW);               // blocks per wave
  const int b0 = (split * NW + wave) * bc;
  const int n_tiles = (a.N + 15) >> 4;
  const int r = lane & 15, c = lane >> 4;
  // activations are the MFMA's ROW operand (lane r = row m0 + r): only lanes whose row exists fetch them (dec_skinny_gemm)
  const bool av0 = m0 + r < a.M, av1 = !M16 && m0 + 16 + r < a.M;
  const uint16_t* ap0 = a.A + (int64_t)(av0 ? m0 + r : 0) * a.lda + 8 * c;
  const uint16_t* ap1 = a.A + (int64_t)(av1 ? m0 + 16 + r : 0) * a.lda + 8 * c;
  const u32x4* wp[NT];
  const f32x4* sp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tl = tile0 + t < n_tiles ? tile0 + t : n_tiles - 1;      // tiles past the end re-read the last one and are never stored
    wp[t] = reinterpret_cast<const u32x4*>(q.wfrag) + ((int64_t)tl * nblk) * (HB == 2 ? 96 : NP * 64) + lane;
    sp[t] = reinterpret_cast<const f32x4*>(q.stfrag) + ((int64_t)tl * nblk) * 16 + r;      // (s, t) of the block's two groups for column r
  }
  // codes and (scale, offset) pairs as buffer loads at 32-bit byte offsets, non-temporal (aux 2): see dec_skinny_fflat
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(q.wfrag), (short)0, (int)((unsigned)n_tiles * (unsigned)nblk * (HB == 2 ? 1536u : NP * 64 * 16u)), 0x00020000);
  const __amdgpu_buffer_rsrc_t rst = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.stfrag), (short)0, (int)((unsigned)n_tiles * (unsigned)nblk * 256u), 0x00020000);
  uint32_t wo[NT], so[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    wo[t] = (uint32_t)((const char*)wp[t] - (const char*)q.wfrag);
    so[t] = (uint32_t)((const char*)sp[t] - (const char*)q.stfrag);
  }
  f32x4 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) { acc[t][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[t][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  const s16x8 zfrag = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
  struct Blk { u32x4 w[NT][HB == 2 ? 1 : NP]; u32x2 h2[HB == 2 ? NT : 1]; f32x4 st[NT]; s16x8 a0[4], a1[4]; };      // h2: the 2-bit hi plane (HB == 2 only)
  auto load_blk = [&](Blk& b, int blk) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (HB == 2) {    // lo plane at the block's start, the lane's 8 B of the hi plane 1024 B in (wo holds 16 lane; the hi plane's rows are 8 lane)
        b.w[t][0] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(wo[t] + (uint32_t)blk * 1536u), 0, 2));
        b.h2[HB == 2 ? t : 0] = __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(rw, (int)(wo[t] - 8u * (uint32_t)lane + (uint32_t)blk * 1536u + 1024u), 0, 2));
      } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) b.w[t][HB == 2 ? 0 : p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(wo[t] + (uint32_t)(blk * NP + p) * 1024u), 0, 2));
      }
      b.st[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rst, (int)(so[t] + (uint32_t)blk * 256u), 0, 2));
    }
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      b.a0[st] = zfrag;
      if (av0) b.a0[st] = *reinterpret_cast<const s16x8*>(ap0 + (int64_t)blk * 128 + 32 * st);
      if (!M16) { b.a1[st] = zfrag; if (av1) b.a1[st] = *reinterpret_cast<const s16x8*>(ap1 + (int64_t)blk * 128 + 32 * st); }
    }
  };
  const f32x4 zero4 = (f32x4){0.f, 0.f, 0.f, 0.f};
  const s16x8 ones = __builtin_bit_cast(s16x8, (u32x4){QMagic<T>::one, QMagic<T>::one, QMagic<T>::one, QMagic<T>::one});
  auto unpack = [](uint32_t word) -> s16x8 {     // 8 codes -> 8 x (MAG + q) in K order
    return __builtin_bit_cast(s16x8, (u32x4){(word & 0x000f000fu) | QMagic<T>::pair, ((word >> 4) & 0x000f000fu) | QMagic<T>::pair,
                                             ((word >> 8) & 0x000f000fu) | QMagic<T>::pair, ((word >> 12) & 0x000f000fu) | QMagic<T>::pair});
  };
  auto unpack2 = [](uint32_t word) -> s16x8 {    // 8 hi parts of 2 bits (the word already shifted to the K-step's four pair slots) -> 8 x (MAG + hi)
    return __builtin_bit_cast(s16x8, (u32x4){(word & 0x00030003u) | QMagic<T>::pair, ((word >> 2) & 0x00030003u) | QMagic<T>::pair,
                                             ((word >> 4) & 0x00030003u) | QMagic<T>::pair, ((word >> 6) & 0x00030003u) | QMagic<T>::pair});
  };
  auto mma_blk = [&](const Blk& b) {
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
          s16x8 f0, f1;
          if (HB == 2 && p == 1) { const uint32_t hw = b.h2[HB == 2 ? t : 0][g]; f0 = unpack2(hw); f1 = unpack2(hw >> 8); }
          else { f0 = unpack(b.w[t][HB == 2 ? 0 : p][2 * g]); f1 = unpack(b.w[t][HB == 2 ? 0 : p][2 * g + 1]); }
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
  };
  // ring of three register blocks (each 4 K-steps = two groups deep): two blocks of loads in flight behind the one being multiplied
  Blk k0, k1, k2;
  if (bc > 0) load_blk(k0, b0);
  if (bc > 1) load_blk(k1, b0 + 1);
  skinny_rstd_prepare(a, rs, m0, wave, lane);        // behind the first two blocks of loads: its own loads ride under the weight stream
  for (int i = 0; i < bc; i += 3) {
    if (i + 2 < bc) load_blk(k2, b0 + i + 2);
    mma_blk(k0);
    if (i + 1 >= bc) break;
    if (i + 3 < bc) load_blk(k0, b0 + i + 3);
    mma_blk(k1);
    if (i + 2 >= bc) break;
    if (i + 4 < bc) load_blk(k1, b0 + i + 4);
    mma_blk(k2);
  }
  if (!skinny_wave_reduce<NT, NW>(acc, wave, lane)) return;
  skinny_store_tr<T, MODE, NT>(a, acc, n0, m0, split, lane, rs);
}

template <typename T, bool M16, int NP, int HB>
static void skinny_qi_launch_m(const SkinnyArgs& a, const QFrag& q, int mode, hipStream_t s, int M_cap) {
  const int tiles = (a.N + 15) / 16, nblk = a.K / 128;
  const int zb = (a.M + 31) / 32;
  // the FORM follows the rows the handle can hold (M_cap, skinny.h), the grid the rows of this call
  const int Mf = M_cap > a.M ? M_cap : a.M, zf = (Mf + 31) / 32;
  const int per_split = nblk / a.S;               // 128-input blocks per cross-workgroup split
  // 4 tiles per wave only when one tile per wave would put more than ~16 waves on every SIMD anyway (the vocabulary-wide head): the
  // activation fragments and group sums are then reused four times.  Otherwise one tile per wave and as many waves per workgroup
  // (1..4, splitting the K range) as keep 2+ blocks per wave -- the kernel hides its memory latency by occupancy.
  // ... and whenever more than 16 rows are multiplied: every wave then loads 32 activation rows per K-step (8 KB per 128-input block against
  // 1 KB of codes), which four tiles share (32 sequences side by side, Orpheus-3B: 4 900 tokens/s with one tile per wave, 11 000 with four)
  const bool nt4 = (int64_t)tiles * a.S * zf >= 16384 || (Mf > 16 && (int64_t)((tiles + 3) / 4) * a.S * zf >= 192);
  int nw = 1;
  for (int cand : {4, 3, 2}) if (per_split % cand == 0 && (per_split / cand >= 2 || cand == 2)) { nw = cand; break; }
  // the vocabulary-wide head at <= 16 rows: 4 tiles per ONE-wave workgroup, the whole K range in the wave (no LDS reduction, a quarter
  // of the workgroups) -- Orpheus-3B, V 156 940: 75.4 us as 9 809 four-wave workgroups, 72.6 as one-wave ones, 67.8 in this form
  // (4 tiles x 4 waves: 107.6)
  const bool head41 = mode == SK_OUTF32 && tiles >= 4096 && Mf <= 16;
#define QI_GO(MODE_, NT_, NW_) hipLaunchKernelGGL((skinny_gemm_qi<T, MODE_, NT_, NW_, M16, NP, HB>), dim3((tiles + NT_ - 1) / NT_, a.S, zb), dim3(64 * NW_), 0, s, a, q)
#define QI_LAUNCH(MODE_)                                                                                   \
  do {                                                                                                     \
    if (head41) QI_GO(MODE_, 4, 1);                                                                        \
    else if (nt4) { if (per_split % 4 == 0) QI_GO(MODE_, 4, 4); else QI_GO(MODE_, 4, 1); }                  \
    else if (nw == 4) QI_GO(MODE_, 1, 4); else if (nw == 3) QI_GO(MODE_, 1, 3);                             \
    else if (nw == 2) QI_GO(MODE_, 1, 2); else QI_GO(MODE_, 1, 1);                                          \
  } while (0)
  switch (mode) {
    case SK_OUTF32: QI_LAUNCH(SK_OUTF32); break;
    case SK_SWIGLU: QI_LAUNCH(SK_SWIGLU); break;
    case SK_PARTIAL: QI_LAUNCH(SK_PARTIAL); break;
    default:   // SK_RESID (skinny_gemm_q_launch admits no other mode)
      if (!nt4 && per_split % 16 == 0 && per_split >= 64) QI_GO(SK_RESID, 1, 16);            // N / 16 workgroups only: K over 8 or 16 waves
      else if (!nt4 && per_split % 8 == 0) QI_GO(SK_RESID, 1, 8);
      else QI_LAUNCH(SK_RESID);
      break;
  }
#undef QI_LAUNCH
#undef QI_GO
}

template <typename T>
static void skinny_qi_launch_t(const SkinnyArgs& a, const QFrag& q, int bits, int mode, hipStream_t s, int M_cap) {
  if (bits == 8) { if (a.M <= 16) skinny_qi_launch_m<T, true, 2, 4>(a, q, mode, s, M_cap); else skinny_qi_launch_m<T, false, 2, 4>(a, q, mode, s, M_cap); }
  else if (bits == 6) { if (a.M <= 16) skinny_qi_launch_m<T, true, 2, 2>(a, q, mode, s, M_cap); else skinny_qi_launch_m<T, false, 2, 2>(a, q, mode, s, M_cap); }      // the 8-bit form rule
  else { if (a.M <= 16) skinny_qi_launch_m<T, true, 1, 4>(a, q, mode, s, M_cap); else skinny_qi_launch_m<T, false, 1, 4>(a, q, mode, s, M_cap); }
}

// quantised form of skinny_gemm_launch: a.W is ignored, the weights come from the fragment-ordered arrays (see skinny_gemm_qi)
// (the form rule -- skinny_qi_launch_m / _t -- is restated in tests/_skinny_cases.py: dispatch_q; change the two together)
int skinny_gemm_q_launch(const SkinnyArgs& a, const uint32_t* wfrag, const float* stfrag, int bits, int mode, int dtype, hipStream_t s, int M_cap) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || a.S <= 0 || a.K % (128 * a.S) != 0 || a.lda % 8 != 0 || !wfrag || !stfrag) return -1;
  if (bits != 4 && bits != 6 && bits != 8) return -1;
  // the kernel's buffer resources and byte offsets are 32 bit: codes [tiles][K / 128][bits / 4] KB, 1536 B per block at 6 bits (the
  // (scale, offset) array is smaller; A is loaded through 64-bit pointers here and needs no such limit)
  if ((uint64_t)((a.N + 15) / 16) * (uint64_t)(a.K / 128) * (bits == 6 ? 1536u : 1024u * (uint64_t)(bits / 4)) > 0xffffffffull) return -1;
  if (mode != SK_OUTF32 && mode != SK_PARTIAL && mode != SK_SWIGLU && mode != SK_RESID) return -1;
  if (mode == SK_SWIGLU && (a.N & 3)) return -1;
  if (mode == SK_RESID && (a.S != 1 || (a.N & 15) || !a.xres || !a.nw || !a.ss_out)) return -1;
  if (a.ss_in && (a.ss_tiles <= 0 || a.ss_tiles > 512 || a.ss_dim <= 0)) return -1;    // skinny_rstd_prepare sums at most 512 tiles
  const QFrag q{wfrag, stfrag};
  if (dtype == MIA_F16) skinny_qi_launch_t<F16>(a, q, bits, mode, s, M_cap); else skinny_qi_launch_t<BF16>(a, q, bits, mode, s, M_cap);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
