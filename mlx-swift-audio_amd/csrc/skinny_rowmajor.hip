// skinny_rowmajor.hip -- the LM step's 16-bit skinny GEMMs: row-major activations, weights row-major or in fragment order (skinny.h).
#include "skinny_device.h"

// ------------------------------------------------------------------------------------------------
// Skinny GEMM for decode (M <= 32 rows per block-z): out[m][n] = sum_k A[m][k] W[n][k].
// One wave per 16 output columns and K-slice; weights go HBM -> VGPR (each weight byte is read exactly once),
// activations come from L2; v_mfma_f32_16x16x32 with W as the row operand so a lane owns 4 consecutive n.
// ------------------------------------------------------------------------------------------------
// NT = 16-column tiles per wave (activation fragments are reused NT times: NT=4 for the 51866-wide logits GEMM,
// where the L2->CU activation traffic would otherwise be twice the HBM weight traffic); KB = K-steps per batch.
// NW = waves per workgroup, each taking 1/NW of the K range (intra-block split-K, summed through LDS in wave order: deterministic).
// With one wave per CU the weight stream is latency-bound (12 KB in flight per CU); NW = 4 quadruples the loads in flight.
// (Cross-workgroup tickets were tried for fusing the split-K reduction + LayerNorm into this kernel: same-address device-scope atomics
// from ~640 workgroups on 8 XCDs cost ~60 us per launch -- far more than the 5 us kernel boundary they would remove.)
template <typename T, int MODE, int NT, int KB, int NW>
__global__ __launch_bounds__(64 * NW) void dec_skinny_gemm(SkinnyArgs a) {
  __shared__ float rs[32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * (16 * NT);
  const int split = blockIdx.y;
  const int m0 = blockIdx.z * 32;
  const int Kc = a.K / (a.S * NW);
  const int kbeg = (split * NW + wave) * Kc;
  const int r = lane & 15, c = lane >> 4;
  // weights: row-major [N][K] (a K-step of a lane = 16 bytes of row r at column 8 c: 16 rows x 64 B per wave instruction), or in
  // fragment order (skinny.h: one contiguous 1 KB per wave instruction); ws = elements between two K-steps of a lane
  const int ws = a.w_frag ? 512 : 32;
  const uint16_t* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (a.w_frag) {
      const int tiles = (a.N + 15) >> 4;
      int tile = (n0 >> 4) + t; tile = tile < tiles ? tile : tiles - 1;
      wp[t] = a.W + (((int64_t)tile * (a.K >> 5) + (kbeg >> 5)) * 64 + lane) * 8;
    } else {
      int wn = n0 + 16 * t + r; wn = wn < a.N ? wn : a.N - 1;
      wp[t] = a.W + (int64_t)wn * a.K + kbeg + 8 * c;
    }
  }
  // weight loads as buffer loads at 32-bit byte offsets (no 64-bit address arithmetic per load; see dec_skinny_fflat)
  const WFragBuf wbuf(a, a.w_frag != 0);
  uint32_t wo[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wo[t] = wbuf.offset(wp[t]);
  const uint32_t wsb = (uint32_t)ws * 2u;
  int am0 = m0 + r; am0 = am0 < a.M ? am0 : a.M - 1;
  int am1 = m0 + 16 + r; am1 = am1 < a.M ? am1 : a.M - 1;
  const uint16_t* ap0 = a.A + (int64_t)am0 * a.lda + kbeg + 8 * c;
  const uint16_t* ap1 = a.A + (int64_t)am1 * a.lda + kbeg + 8 * c;
  // Only the lanes whose row exists fetch activations (the others feed zeros: their accumulator columns are never stored).  At one
  // sequence that is 4 of 64 lanes in the first MFMA half and none in the second: a 16-byte wave load costs the address unit per
  // ACTIVE lane, and with every lane fetching (rows clamped to the last one) the activation fragments were two of the three load
  // instructions of every K-step.
  const bool av0 = m0 + r < a.M, av1 = m0 + 16 + r < a.M;
  const s16x8 zfrag = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
  const WFragBuf abuf(a, WFragBuf::RowMajorA{});
  const uint32_t ab0 = abuf.offset(ap0), ab1 = abuf.offset(ap1);
  auto lda0 = [&](int k) -> s16x8 { s16x8 v = zfrag; if (av0) v = abuf.template load<0>(ab0 + 2u * (uint32_t)k); return v; };
  auto lda1 = [&](int k) -> s16x8 { s16x8 v = zfrag; if (av1) v = abuf.template load<0>(ab1 + 2u * (uint32_t)k); return v; };
  f32x4 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) { acc[t][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[t][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  // Software-pipelined register double buffer: batch i+1 (KB K-steps) is issued before the MFMAs of batch i, so two
  // batches of independent 16-byte loads stay in flight per lane (weights are HBM-once traffic).
  struct Batch { s16x8 w[KB][NT], a0[KB], a1[KB]; };
  auto load_batch = [&](Batch& t, int k) {
#pragma unroll
    for (int u = 0; u < KB; ++u) {
#pragma unroll
      for (int n = 0; n < NT; ++n) t.w[u][n] = wbuf.template load<0>(wo[n] + (uint32_t)((k >> 5) + u) * wsb);
      t.a0[u] = lda0(k + 32 * u);
      t.a1[u] = lda1(k + 32 * u);
    }
  };
  auto mma_batch = [&](const Batch& t) {
#pragma unroll
    for (int u = 0; u < KB; ++u)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        acc[n][0] = T::mfma16(t.w[u][n], t.a0[u], acc[n][0]);
        acc[n][1] = T::mfma16(t.w[u][n], t.a1[u], acc[n][1]);
      }
  };
  constexpr int KSTEP = 32 * KB;
  const int nb = Kc / KSTEP;
  // The K-steps left over after the whole batches (< KB of them).  On a SHORT slice (at most 3 batches: the ring's fourth register
  // batch is idle) their loads are issued up front into that batch -- fetched after the main loop, one step at a time, they were up
  // to KB - 1 extra dependent memory round trips at the end of every launch (Qwen2-0.5B: K / S = 224 = one batch of 4 steps + 3 such
  // steps, in each of its 72 projection launches per token: 0.876 -> 0.80 ms per token).  Long slices keep the trailing loop: a fifth
  // register batch would cost the 64-thread form its occupancy (measured on Orpheus-3B: 1.96 -> 2.15 ms per token).
  const int ktail = nb * KSTEP, rem = (Kc - ktail) >> 5;
  const bool early_tail = nb <= 3 && rem > 0;
  Batch b0, b1, b2, b3;
  if (early_tail) {
#pragma unroll
    for (int u = 0; u < KB; ++u)
      if (u < rem) {
#pragma unroll
        for (int n = 0; n < NT; ++n) b3.w[u][n] = wbuf.template load<0>(wo[n] + (uint32_t)((ktail >> 5) + u) * wsb);
        b3.a0[u] = lda0(ktail + 32 * u);
        b3.a1[u] = lda1(ktail + 32 * u);
      }
  }
  if (nb > 0) {
    // ring of four register batches (static names: runtime-indexed vector arrays would go to scratch): three batches of
    // loads are always in flight behind the batch being multiplied
    load_batch(b0, 0);
    if (nb > 1) load_batch(b1, KSTEP);
    if (nb > 2) load_batch(b2, 2 * KSTEP);
    skinny_rstd_prepare(a, rs, m0, wave, lane);      // behind the first three batches of loads: its own loads ride under the weight stream
    for (int i = 0; i < nb; i += 4) {
      if (i + 3 < nb) load_batch(b3, (i + 3) * KSTEP);
      mma_batch(b0);
      if (i + 1 >= nb) break;
      if (i + 4 < nb) load_batch(b0, (i + 4) * KSTEP);
      mma_batch(b1);
      if (i + 2 >= nb) break;
      if (i + 5 < nb) load_batch(b1, (i + 5) * KSTEP);
      mma_batch(b2);
      if (i + 3 >= nb) break;
      if (i + 6 < nb) load_batch(b2, (i + 6) * KSTEP);
      mma_batch(b3);
    }
  } else skinny_rstd_prepare(a, rs, m0, wave, lane);
  if (early_tail) {
#pragma unroll
    for (int u = 0; u < KB; ++u)
      if (u < rem) {
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          acc[n][0] = T::mfma16(b3.w[u][n], b3.a0[u], acc[n][0]);
          acc[n][1] = T::mfma16(b3.w[u][n], b3.a1[u], acc[n][1]);
        }
      }
  } else {
    for (int k = ktail; k < Kc; k += 32) {
      const s16x8 fa0 = lda0(k);
      const s16x8 fa1 = lda1(k);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const s16x8 fw = wbuf.template load<0>(wo[n] + (uint32_t)(k >> 5) * wsb);
        acc[n][0] = T::mfma16(fw, fa0, acc[n][0]);
        acc[n][1] = T::mfma16(fw, fa1, acc[n][1]);
      }
    }
  }
  if (!skinny_wave_reduce<NT, NW>(acc, wave, lane)) return;
  skinny_store<T, MODE, NT>(a, acc, n0, m0, split, lane, rs);
}

// The same GEMM for a SHORT K-slice per wave (exactly NSTEP K-steps of 32, host-checked: K == S * NW * 32 * NSTEP): every operand
// load of the wave is issued before the first MFMA, so the kernel pays ONE memory round trip (the ring above pays one per refill:
// two to three on a 160- or 320-wide slice, ~1.5 us each on a step that is a chain of such kernels).  Weights are read once per
// step and never again before 1.3 GB of other traffic has passed: non-temporal loads keep them from displacing the activations in
// L2 / MALL.  Same K order per wave and same wave-order reduction as dec_skinny_gemm: results are bit-identical to it.
template <typename T, int MODE, int NT, int NSTEP, int NW>
__global__ __launch_bounds__(64 * NW) void dec_skinny_flat(SkinnyArgs a) {
  __shared__ float rs[32];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * (16 * NT);
  const int split = blockIdx.y;
  const int m0 = blockIdx.z * 32;
  constexpr int Kc = 32 * NSTEP;
  const int kbeg = (split * NW + wave) * Kc;
  const int r = lane & 15, c = lane >> 4;
  const int ws = a.w_frag ? 512 : 32;     // weights row-major or in fragment order: see dec_skinny_gemm
  const uint16_t* wp[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    if (a.w_frag) {
      const int tiles = (a.N + 15) >> 4;
      int tile = (n0 >> 4) + t; tile = tile < tiles ? tile : tiles - 1;
      wp[t] = a.W + (((int64_t)tile * (a.K >> 5) + (kbeg >> 5)) * 64 + lane) * 8;
    } else {
      int wn = n0 + 16 * t + r; wn = wn < a.N ? wn : a.N - 1;
      wp[t] = a.W + (int64_t)wn * a.K + kbeg + 8 * c;
    }
  }
  const WFragBuf wbuf(a, a.w_frag != 0);
  uint32_t wo[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wo[t] = wbuf.offset(wp[t]);
  const uint32_t wsb = (uint32_t)ws * 2u;
  int am0 = m0 + r; am0 = am0 < a.M ? am0 : a.M - 1;
  int am1 = m0 + 16 + r; am1 = am1 < a.M ? am1 : a.M - 1;
  const uint16_t* ap0 = a.A + (int64_t)am0 * a.lda + kbeg + 8 * c;
  const uint16_t* ap1 = a.A + (int64_t)am1 * a.lda + kbeg + 8 * c;
  const bool av0 = m0 + r < a.M, av1 = m0 + 16 + r < a.M;     // only lanes whose row exists fetch activations (see dec_skinny_gemm)
  const s16x8 zfrag = (s16x8){0, 0, 0, 0, 0, 0, 0, 0};
  s16x8 fw[NSTEP][NT], fa0[NSTEP], fa1[NSTEP];
#pragma unroll
  for (int u = 0; u < NSTEP; ++u) {
#pragma unroll
    for (int n = 0; n < NT; ++n) fw[u][n] = wbuf.template load<2>(wo[n] + (uint32_t)u * wsb);
    fa0[u] = zfrag; fa1[u] = zfrag;
    if (av0) fa0[u] = *reinterpret_cast<const s16x8*>(ap0 + 32 * u);
    if (av1) fa1[u] = *reinterpret_cast<const s16x8*>(ap1 + 32 * u);
  }
  __builtin_amdgcn_sched_barrier(0);   // keep every load ahead of the first MFMA (the scheduler would otherwise trade them for registers)
  skinny_rstd_prepare(a, rs, m0, wave, lane);
  f32x4 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) { acc[t][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[t][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int u = 0; u < NSTEP; ++u)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      acc[n][0] = T::mfma16(fw[u][n], fa0[u], acc[n][0]);
      acc[n][1] = T::mfma16(fw[u][n], fa1[u], acc[n][1]);
    }
  if (!skinny_wave_reduce<NT, NW>(acc, wave, lane)) return;
  skinny_store<T, MODE, NT>(a, acc, n0, m0, split, lane, rs);
}

// short-K-slice form (dec_skinny_flat) of the row-major kernel, taken only where it keeps the ring kernel's 4-wave split of K:
// the LM step's packed-weight twin (skinny_gemm_qi) must sum in the same order as its 16-bit form
template <typename T, int MODE>
static bool skinny_flat_try(const SkinnyArgs& a, hipStream_t s) {
  const int tiles = (a.N + 15) / 16, zb = (a.M + 31) / 32;
  // (the row blocks do not enter the form: a row's result must not depend on how many rows the call carries -- the LM step has one block)
  const int64_t wgs = (int64_t)tiles * a.S;
  if (a.K % (128 * a.S) != 0 || wgs > 1024 || a.K / a.S < 512) return false;
  const int per_split = a.K / a.S;
  const dim3 grid(tiles, a.S, zb);
#define FLAT(NSTEP_)                                                                                                  \
  if (per_split == 4 * 32 * NSTEP_) {                                                                                 \
    hipLaunchKernelGGL((dec_skinny_flat<T, MODE, 1, NSTEP_, 4>), grid, dim3(256), 0, s, a);                            \
    return true;                                                                                                      \
  }
  FLAT(10) FLAT(5) FLAT(8) FLAT(6) FLAT(4)
#undef FLAT
  return false;
}

template <typename T>
static void skinny_launch_t(const SkinnyArgs& a, int mode, hipStream_t s) {
  switch (mode) {
    case SK_OUTF32: break;   // bandwidth-bound: the ring kernel (measured: flat forms are 11-14 us slower on the 51866-wide head)
    case SK_PARTIAL: if (skinny_flat_try<T, SK_PARTIAL>(a, s)) return; break;
    case SK_SWIGLU: if (skinny_flat_try<T, SK_SWIGLU>(a, s)) return; break;
    default: break;          // SK_RESID: N / 16 workgroups only, always the ring kernel with K over 4 / 8 / 16 waves (below)
  }
  if (mode == SK_OUTF32) {   // the vocabulary-wide logits GEMM: 64 columns per wave
    dim3 grid((a.N + 63) / 64, a.S, (a.M + 31) / 32);
    hipLaunchKernelGGL((dec_skinny_gemm<T, SK_OUTF32, 4, 2, 1>), grid, dim3(64), 0, s, a);
    return;
  }
  dim3 grid((a.N + 15) / 16, a.S, (a.M + 31) / 32);
  // few workgroups and a long K per wave -> split K over 4 waves of the workgroup (K per wave stays a multiple of 32)
  // (counted per 32-row block, as in skinny_flat_try: with grid.z in the count a row of a 33-row call was summed in another order than alone)
  const bool wide = (int64_t)grid.x * grid.y <= 1024 && a.K % (128 * a.S) == 0 && a.K / a.S >= 512;
#define SK_LAUNCH(MODE_)                                                                                              \
  do {                                                                                                                \
    if (wide) hipLaunchKernelGGL((dec_skinny_gemm<T, MODE_, 1, 2, 4>), grid, dim3(256), 0, s, a);                      \
    else hipLaunchKernelGGL((dec_skinny_gemm<T, MODE_, 1, 4, 1>), grid, dim3(64), 0, s, a);                            \
  } while (0)
  switch (mode) {
    case SK_PARTIAL: SK_LAUNCH(SK_PARTIAL); break;
    case SK_SWIGLU: SK_LAUNCH(SK_SWIGLU); break;
    default:   // SK_RESID
      // no cross-workgroup split here (the epilogue owns the residual row slice): N / 16 workgroups only, so K goes over 8 waves
      if (a.K % 1024 == 0 && a.K >= 8192) hipLaunchKernelGGL((dec_skinny_gemm<T, SK_RESID, 1, 2, 16>), grid, dim3(1024), 0, s, a);
      else if (a.K % 256 == 0 && a.K >= 2048) hipLaunchKernelGGL((dec_skinny_gemm<T, SK_RESID, 1, 2, 8>), grid, dim3(512), 0, s, a);
      else SK_LAUNCH(SK_RESID);
      break;
  }
#undef SK_LAUNCH
}

// (the form rule below -- skinny_flat_try and skinny_launch_t -- is restated in tests/_skinny_cases.py: dispatch16; change the two together)
int skinny_gemm_launch(const SkinnyArgs& a, int mode, int dtype, hipStream_t s) {
  if (a.M <= 0 || a.N <= 0 || a.K <= 0 || a.S <= 0 || a.K % (32 * a.S) != 0 || a.lda % 8 != 0) return -1;
  // WFragBuf holds sizes and byte offsets in 32 bits (fragment order pads the rows to 16)
  if ((uint64_t)((a.N + 15) / 16) * 16 * (uint64_t)a.K * 2 > 0xffffffffull || (uint64_t)a.M * (uint64_t)a.lda * 2 > 0xffffffffull) return -1;
  if (mode != SK_OUTF32 && mode != SK_PARTIAL && mode != SK_SWIGLU && mode != SK_RESID) return -1;    // the LM step's modes
  if (mode == SK_SWIGLU && (a.N & 3)) return -1;
  if (mode == SK_RESID && (a.S != 1 || (a.N & 15) || (a.ldo & 3) || !a.xres || !a.nw || !a.ss_out)) return -1;
  if (a.ss_in && (a.ss_tiles <= 0 || a.ss_tiles > 512 || a.ss_dim <= 0)) return -1;    // skinny_rstd_prepare sums at most 512 tiles
  if (dtype == MIA_F16) skinny_launch_t<F16>(a, mode, s); else skinny_launch_t<BF16>(a, mode, s);
  return 0;
}
