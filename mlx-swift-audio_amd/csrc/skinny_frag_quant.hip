// skinny_frag_quant.hip -- the Whisper step's skinny GEMMs on packed 4- / 8-bit weights (decode.h: dec_launch_skinny_q): the packed
// counterpart of skinny_frag.hip, for handles with attached MLX-affine weights (mia_whisper_attach_quantized / mia_whisper_use_packed).
#include "decode.h"
#include "skinny_quant_device.h"

// ------------------------------------------------------------------------------------------------
// Weights: the wfrag / stfrag arrays of skinny_quant.hip (same repack, quant_repack.h) and the same arithmetic -- integer-code MFMAs,
// one fix-up y += s P + t A per 64-input group (P = sum code a, A = sum a; t = b - MAG s), two nibble planes for 8 bit.  Nothing is
// de-quantised and no weight is rounded.
// Activations: the step's fragment order (skinny.h: afrag_index), so a wave's operand load is one contiguous 1 KB per 16 rows; the
// buffers are whole zero-padded 32-row blocks (whisper_reserve), so the loads need no row mask.
// The activations are the MFMA's ROW operand (as in skinny_gemm_qi): lane (r, c) holds C[m = 16 mt + 4 c + i][n = 16 t + r], one output
// column per lane, so a group's (s, t) are per-lane scalars from one 16-byte load.  The price is an epilogue of 2- / 4-byte stores
// (skinny_frag.hip stores 8 / 16 bytes per lane); the modes are the split chain's: SK_QKV, SK_OUT16 (+ out_frag, GELU), SK_PARTIAL, SK_OUTF32.
// The carried-LayerNorm modes (SK_RESID, c1 / c2 consumers) have no packed form: the step runs the reduce + LayerNorm chain when packed.
//
// Resources (gfx950, hipcc -O3; launch bounds 64 NW): LDS = the cross-wave reduction only, (NW - 1) NT 2 KB (NW 5, NT 1: 8 KB; NW 1: none).
// Registers (VGPR + AGPR, as compiled; three blocks in flight, each NT NP 4 code words + NT 4 (s, t) + 16 (M16) or 32 activation
// registers): NT 1, at most 16 rows: 4 bit 106..116, 8 bit 126..138 (3 waves per SIMD); NT 1, 32 rows: 4 bit 178..196, 8 bit 206..228,
// SK_QKV 8 bit 256 (2 waves per SIMD); NT 4 (the logits GEMM above 16 rows, one-wave workgroups): 4 bit 352, 8 bit 444 of the 512 a
// lone wave may hold.  No scratch in any variant (tests/test_whisper_packed_resources.py).
// ------------------------------------------------------------------------------------------------
template <typename T, int MODE, int NT>
__device__ __forceinline__ void fq_store(const SkinnyArgs& a, const f32x4 (&acc)[NT][2], const int (&ps)[2][4], int n0, int m0, int split, int lane) {
  const int r = lane & 15, c = lane >> 4;
  uint16_t* o16 = reinterpret_cast<uint16_t*>(a.out);
  float* o32 = reinterpret_cast<float*>(a.out);
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + r;
    if (n >= a.N) continue;
    const float bs = (MODE != SK_PARTIAL && a.bias) ? a.bias[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = m0 + 16 * mt + 4 * c + i;
        if (m >= a.M) continue;
        float v = acc[t][mt][i];
        if (MODE == SK_PARTIAL) { o32[((int64_t)split * a.M + m) * a.N + n] = v; continue; }
        v += bs;
        if (a.act == MIA_ACT_GELU) v = gelu_erf(v);
        if (MODE == SK_OUTF32) { o32[(int64_t)m * a.ldo + n] = v; continue; }
        const uint16_t h = T::from_f32(v);
        if (MODE == SK_OUT16) { o16[a.out_frag ? afrag_index(m, n, a.N) : (int64_t)m * a.ldo + n] = h; continue; }
        // SK_QKV (host-checked: D % 64 == 0, N == 3 D): [0,D) -> q row-major, [D,2D) -> self K cache, [2D,3D) -> self V cache at pos[m]
        if (n < a.D) { o16[(int64_t)m * a.ldo + n] = h; continue; }
        const int hd = (n - a.D) % a.D, hh = hd >> 6, d = hd & 63;
        uint16_t* cache = n < 2 * a.D ? a.cache_k : a.cache_v;
        cache[(((int64_t)m * a.H + hh) * a.n_ctx + ps[mt][i]) * 64 + d] = h;
      }
    }
  }
}

// M16: at most 16 rows (the reference's own batch sizes): the second 16-row MFMA half and its activation loads are skipped
// NP: nibble planes per code (1 = 4-bit, 2 = 8-bit)
template <typename T, int MODE, int NT, int NW, bool M16, int NP>
__global__ __launch_bounds__(64 * NW) void dec_skinny_fq(SkinnyArgs a, QFrag q) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile0 = blockIdx.x * NT;
  const int n0 = tile0 * 16;
  const int split = blockIdx.y;
  const int z = blockIdx.z, m0 = z * 32;
  const int nblk = a.K >> 7;                      // 128-input blocks per row
  const int bc = nblk / (a.S * NW);               // blocks per wave (host-checked: exact)
  const int b0 = (split * NW + wave) * bc;
  const int n_tiles = (a.N + 15) >> 4;
  const int r = lane & 15, c = lane >> 4;
  // the epilogue's cache positions, ahead of the operand stream (rows 16 mt + 4 c + i)
  int ps[2][4];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int m = m0 + 16 * mt + 4 * c + i; ps[mt][i] = (MODE == SK_QKV && m < a.M) ? a.pos[m] : 0; }
  // activation fragments of this 32-row block: K-step ks, half mt at ap + 1024 ks + 512 mt (elements)
  const uint16_t* ap = a.A + ((int64_t)z * (a.K >> 5) * 128 + lane) * 8;
  // codes and (scale, offset) pairs as buffer loads at 32-bit byte offsets; cache policy = the immediate aux operand (dec_skinny_fflat)
  const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(q.wfrag), (short)0, (int)((unsigned)n_tiles * (unsigned)nblk * (NP * 64 * 16u)), 0x00020000);
  const __amdgpu_buffer_rsrc_t rst = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(q.stfrag), (short)0, (int)((unsigned)n_tiles * (unsigned)nblk * 256u), 0x00020000);
  uint32_t wo[NT], so[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tl = tile0 + t < n_tiles ? tile0 + t : n_tiles - 1;      // tiles past the end re-read the last one and are never stored
    wo[t] = ((uint32_t)tl * (uint32_t)nblk * (NP * 64) + (uint32_t)lane) * 16u;
    so[t] = ((uint32_t)tl * (uint32_t)nblk * 16 + (uint32_t)r) * 16u;   // (s, t) of the block's two groups for column r
  }
  f32x4 acc[NT][2];
#pragma unroll
  for (int t = 0; t < NT; ++t) { acc[t][0] = (f32x4){0.f, 0.f, 0.f, 0.f}; acc[t][1] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
  using Blk = QBlk<NT, NP>;
  const bool keep = a.w_keep != 0;                // wave-uniform: one test per block of loads
  auto load_blk = [&](Blk& b, int blk) {
    auto go = [&](auto keep_tag) {
      constexpr int AUX = decltype(keep_tag)::value ? 0 : 2;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int p = 0; p < NP; ++p) b.w[t][p] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (int)(wo[t] + (uint32_t)(blk * NP + p) * 1024u), 0, AUX));
        b.st[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rst, (int)(so[t] + (uint32_t)blk * 256u), 0, AUX));
      }
    };
    if (keep) go(std::true_type{}); else go(std::false_type{});
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      b.a0[st] = *reinterpret_cast<const s16x8*>(ap + (int64_t)(blk * 4 + st) * 1024);
      if (!M16) b.a1[st] = *reinterpret_cast<const s16x8*>(ap + (int64_t)(blk * 4 + st) * 1024 + 512);
    }
  };
  q_block_ring<T, NT, NP, M16>(b0, bc, acc, load_blk, [] {});      // the block arithmetic and the three-block ring: skinny_quant_device.h
  if (!skinny_wave_reduce<NT, NW>(acc, wave, lane)) return;
  fq_store<T, MODE, NT>(a, acc, ps, n0, m0, split, lane);
}

template <typename T, int MODE, bool M16, int NP>
static void skinny_fq_launch_m(const SkinnyArgs& a, const QFrag& q, hipStream_t s) {
  const int tiles = (a.N + 15) / 16, zb = (a.M + 31) / 32;
  const int per_split = (a.K / 128) / a.S;        // 128-input blocks per cross-workgroup split
#define FQ_GO(NT_, NW_) hipLaunchKernelGGL((dec_skinny_fq<T, MODE, NT_, NW_, M16, NP>), dim3((tiles + NT_ - 1) / NT_, a.S, zb), dim3(64 * NW_), 0, s, a, q)
  if constexpr (MODE == SK_OUTF32 && !M16) {
    // the vocabulary-wide logits GEMM above 16 rows: every wave loads 8 KB of activations per block against 1 KB of codes per tile, so
    // four tiles share them (skinny_quant.hip: the same choice, measured there)
    FQ_GO(4, 1);
  } else {
    // one tile per wave; K of a split over the most waves of {5, 4, 3, 2} that take whole blocks (summed through LDS in wave order):
    // D 1280 = 10 blocks -> 5 waves x 2, 4 D = 4 splits x 5 waves x 2; the kernel hides its memory latency by occupancy
    if (per_split % 5 == 0) FQ_GO(1, 5);
    else if (per_split % 4 == 0) FQ_GO(1, 4);
    else if (per_split % 3 == 0) FQ_GO(1, 3);
    else if (per_split % 2 == 0) FQ_GO(1, 2);
    else FQ_GO(1, 1);
  }
#undef FQ_GO
}

template <typename T, bool M16, int NP>
static int skinny_fq_launch_t(const SkinnyArgs& a, const QFrag& q, int mode, hipStream_t s) {
  switch (mode) {
    case SK_OUT16: skinny_fq_launch_m<T, SK_OUT16, M16, NP>(a, q, s); return 0;
    case SK_OUTF32: skinny_fq_launch_m<T, SK_OUTF32, M16, NP>(a, q, s); return 0;
    case SK_PARTIAL: skinny_fq_launch_m<T, SK_PARTIAL, M16, NP>(a, q, s); return 0;
    case SK_QKV: skinny_fq_launch_m<T, SK_QKV, M16, NP>(a, q, s); return 0;
    default: return -1;
  }
}

template <typename T>
static int skinny_fq_launch_b(const SkinnyArgs& a, const QFrag& q, int bits, int mode, hipStream_t s) {
  if (bits == 8) return a.M <= 16 ? skinny_fq_launch_t<T, true, 2>(a, q, mode, s) : skinny_fq_launch_t<T, false, 2>(a, q, mode, s);
  return a.M <= 16 ? skinny_fq_launch_t<T, true, 1>(a, q, mode, s) : skinny_fq_launch_t<T, false, 1>(a, q, mode, s);
}

int dec_launch_skinny_q(mia_whisper* w, const SkinnyArgs& a, const uint32_t* wfrag, const float* stfrag, int bits, int mode, hipStream_t s) {
  if (!a.A || !wfrag || !stfrag || !a.out || a.M <= 0 || a.N <= 0 || a.S <= 0 || a.K <= 0 || a.K % (128 * a.S) != 0) return -1;
  if (bits != 4 && bits != 8) return -1;
  if (a.ss_in || a.c1) return -1;                 // no carried LayerNorm in packed form
  if (mode == SK_QKV && (a.D % 64 != 0 || a.N != 3 * a.D || !a.cache_k || !a.cache_v || !a.pos)) return -1;
  if (mode == SK_OUT16 && a.out_frag && a.N % 32 != 0) return -1;
  // 32-bit byte offsets of the buffer loads
  const uint64_t tiles = (uint64_t)(a.N + 15) / 16, nblk = (uint64_t)a.K / 128;
  if (tiles * nblk * (uint64_t)(bits / 4) * 1024u >= (1ull << 31)) return -1;
  const QFrag q{wfrag, stfrag};
  const int rc = w->dtype == MIA_F16 ? skinny_fq_launch_b<F16>(a, q, bits, mode, s) : skinny_fq_launch_b<BF16>(a, q, bits, mode, s);
  if (rc != 0) return rc;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
