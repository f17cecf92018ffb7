// lm_prefill_attn.hip -- tiled causal grouped-query attention for the LM's batched prompt pass, head dim 64 / 128, bf16 / f16 operands,
// fp32 online softmax, Q K^T and P V on the matrix cores, gfx950.
//
// Serves lm_prefill_rows (lm.hip) when mia_lm_set_prompt_attention(lm, 1) is set: the rows of a chunk -- (sequence, position) pairs, q
// already rotated (and q/k-normalised) by lm_rope_cache, the layer's 16-bit K/V cache [B_cap][Hkv][max_ctx][dh] already holding the chunk's
// rows -- attend causally: the row at (s, p) sees keys [0, p] of sequence s.  It replaces one lm_attention<.., FUSED = false> workgroup per
// (query head, row), each of which re-reads its head's K/V from key 0 on the VALU (OuteTTS's ~1 900-token speaker prompt, OuteTTS.swift:
// 327-340: 61 000 workgroups and 15 GB of cache reads per layer of a Llama-3.2-1B).
//
// The structure is attn128.hip's, with the head dim a template parameter, a causal mask and the GQA group folded into the query tile:
//   * the host cuts every run of a chunk (one sequence's contiguous positions) into QUERY TILES of 128 / GW positions, GW = 4, 2 or 1
//     query heads of one KV group (4 when the group size is a multiple of 4, else 2 when even, else 1): a 256-thread workgroup owns one
//     query tile of GW heads of one KV head, one wave = 32 positions of one head (the WAVE WIDTH), and the GW heads share every staged
//     K / V tile.  Llama-3.2-1B (group of 4): 32 positions x 4 heads; a group of 2: 64 x 2; no grouping: 128 x 1;
//   * keys are walked in KEY TILES of 64, anchored at key 0 of the sequence whatever the chunk or the tile start; a wave stops computing
//     at the tile that holds its own last position, and masks (key > position, an exact zero probability) only in tiles that reach
//     past its first position;
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (dh / 16 k-steps): a lane owns ONE query and 32 keys of it, so the online softmax is in-lane plus
//     one cross-half shuffle, and the S^T accumulator is, register for register, the B operand of O^T += V^T P^T (K rows are fed with
//     bits 2 <-> 3 of the row index swapped so that the register order is natural key order);
//   * K tiles [64 keys][dh] (16-B chunk index XOR (row & 15) at dh 128, XOR (row >> 1) & 7 at dh 64) and V^T tiles [dh][64 keys] (128-B
//     rows, chunk XOR (row >> 1) & 7) are staged cache -> registers -> LDS, double buffered; V is transposed in the staging write, as
//     in attn128.hip.  Loads are clamped to the workgroup's own last position: nothing past it, and so nothing past the sequence's
//     position or max_ctx, is read.
// Row independence: a lane's arithmetic involves its own q row, the staged keys and its own position only.  The reference point of the
// softmax moves per lane (a lane that stays multiplies by an exact 1), tiles wholly past a lane's position add exact zeros, and the key
// tiles do not depend on the query tiling -- so a row's bits do not depend on the chunk start, on its tile mates or on the other
// sequences of the chunk.  Sums run in a fixed order (no atomics): a repeat call returns the same bits.
//
// Per (row, head) the kernel does 4 dh (p + 1) flop; per workgroup it reads (p_last + 1) dh 2 x 2 bytes of cache for 128 (row, head)
// pairs, where the row kernel reads as much for one.
#include <algorithm>
#include <type_traits>

#include "lm.h"
#include "mia_device.h"

namespace {

constexpr int KV_TILE = 64;

__device__ __forceinline__ int swap23(int r) {  // swap bits 2 and 3
  return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1);
}

template <typename T, int DH, int GW>
__global__ __launch_bounds__(256) void lm_prefill_attn_kernel(LmPromptAttn a, float scale_log2) {
  constexpr int CH = DH / 8;                      // 16-B chunks per K row
  constexpr int RPI = 256 / CH;                   // K rows (V key pairs) staged per pass of the workgroup
  constexpr int NK = KV_TILE / RPI, NV = 32 / RPI;
  constexpr int K_BYTES = KV_TILE * DH * 2;       // [64 keys][DH]
  constexpr int V_BYTES = DH * 128;               // [DH][64 keys]
  constexpr int BUF_BYTES = K_BYTES + V_BYTES;
  __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int lin = blockIdx.x;
  {  // every XCD gets a contiguous run of the linear index: the query tiles of a (sequence, KV head) re-read the same K / V
    const int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, xcd = lin % 8;
    lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + lin / 8;
  }
  const int G = a.Hq / a.Hkv, gpk = G / GW;       // head chunks per KV head
  const int4 td = a.tiles[lin % a.n_tiles];       // (sequence, first position, first row, positions)
  const int hc = lin / a.n_tiles;
  const int kvh = hc / gpk, head = kvh * G + (hc % gpk) * GW + wave % GW;
  const int qs = (wave / GW) * 32;                // the wave's first position inside the tile
  const int seq = td.x, pos0 = td.y, row0 = td.z, cnt = td.w;
  const bool wave_on = qs < cnt;                  // wave-uniform
  const int kmax = pos0 + cnt - 1;                // the workgroup's last position: no key beyond it is read
  const int pmin = pos0 + qs, pmax = pos0 + min(qs + 31, cnt - 1);
  const int lq = lane & 31, lh = lane >> 5;
  const int qi = min(qs + lq, cnt - 1);           // rows past the tile repeat its last row and are not stored
  const int p_lane = pos0 + qi;
  const uint16_t* Kg = a.kc + (int64_t)seq * a.seq_stride + (int64_t)kvh * a.max_ctx * DH;
  const uint16_t* Vg = a.vc + (int64_t)seq * a.seq_stride + (int64_t)kvh * a.max_ctx * DH;

  // ---- Q^T fragments (B operand): lane holds Q[row][16 ks + 8 lh + 0..7]
  s16x8 qf[DH / 16];
  {
    const uint16_t* qp = a.q + (int64_t)(row0 + qi) * a.Hq * DH + head * DH + 8 * lh;
#pragma unroll
    for (int ks = 0; ks < DH / 16; ++ks) qf[ks] = *reinterpret_cast<const s16x8*>(qp + 16 * ks);
  }

  // ---- staging.  K: 64 rows x CH chunks of 16 B, NK per thread (rows s_row + RPI i).  V: 32 key pairs x CH chunks, NV per thread.
  const int s_chk = tid % CH, s_row = tid / CH;
  const uint16_t* kbase = Kg + s_chk * 8;
  const uint16_t* vbase = Vg + s_chk * 8;
  u32x4 rk[NK], rv[NV][2];
  auto load_regs = [&](int key0) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int key = min(key0 + s_row + RPI * i, kmax);                     // masked below; the clamped row is the sequence's own
      rk[i] = *reinterpret_cast<const u32x4*>(kbase + (int64_t)key * DH);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = min(key0 + 2 * (s_row + RPI * i) + e, kmax);
        rv[i][e] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)key * DH);
      }
  };
  auto kswz = [](int row) { return DH == 128 ? (row & 15) : ((row >> 1) & 7); };
  auto write_lds = [&](int buf) {
    char* kd = lds + buf * BUF_BYTES;
    char* vd = kd + K_BYTES;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int row = s_row + RPI * i;
      *reinterpret_cast<u32x4*>(kd + row * (DH * 2) + ((s_chk ^ kswz(row)) << 4)) = rk[i];
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int pair = s_row + RPI * i;                  // keys 2 pair, 2 pair + 1 of the tile
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = 8 * s_chk + j;
        const uint32_t lo = rv[i][0][j >> 1], hi = rv[i][1][j >> 1];
        const uint32_t w = (j & 1) ? (lo >> 16) | (hi & 0xffff0000u) : (lo & 0xffffu) | (hi << 16);
        *reinterpret_cast<uint32_t*>(vd + d * 128 + (((pair >> 2) ^ ((d >> 1) & 7)) << 4) + (pair & 3) * 4) = w;
      }
    }
  };

  f32x16 acc_o[DH / 32];
#pragma unroll
  for (int i = 0; i < DH / 32; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_o[i][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int krow = swap23(lq);   // K row fed to MFMA row lq
  // One K / V tile of one wave; MASK (tiles that reach past the wave's first position) gives the keys above the lane's own position
  // -inf, an exact zero probability.  The softmax works on the raw scores: p = exp2(fma(s, c, -m c)), c = scale * log2(e) > 0.
  auto compute = [&](int key0, int cur, auto mask_tag) {
    constexpr bool MASK = decltype(mask_tag)::value;
    const char* sk = lds + cur * BUF_BYTES;
    const char* sv = sk + K_BYTES;
    // ---- S^T = K Q^T : two 32-key blocks, DH / 16 k-steps
    f32x16 acc_s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_s[kb][r] = 0.f;
      const int row = kb * 32 + krow;
#pragma unroll
      for (int ks = 0; ks < DH / 16; ++ks) {
        const s16x8 kf = *reinterpret_cast<const s16x8*>(sk + row * (DH * 2) + (((2 * ks + lh) ^ kswz(row)) << 4));
        acc_s[kb] = T::mfma32(kf, qf[ks], acc_s[kb]);
      }
    }
    // ---- online softmax (base 2), lane = one query, registers = keys
    float mloc = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (MASK) {
          const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (key0 + kb * 32 + swap23(i) > p_lane) acc_s[kb][r] = -INFINITY;
        }
        mloc = fmaxf(mloc, acc_s[kb][r]);
      }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    // bounded-growth lazy rescaling (attention.hip), decided per lane = per query row: the reference point moves only when the tile's
    // maximum exceeds it by more than 2^LAZY_LOG2.  The ballot only skips the multiplies when no lane moves; a lane that stays
    // multiplies by an exact 1.  A lane whose keys are all masked here (mloc = -inf) stays: key 0 made its m_run finite in tile 0.
    constexpr float LAZY_LOG2 = 8.0f;
    const bool grow = (mloc - m_run) * scale_log2 > LAZY_LOG2;
    if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {
      const float m_new = grow ? mloc : m_run;
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < DH / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[db][r] *= alpha;
    }
    const float neg_mc = -m_run * scale_log2;
    float lsum = 0.f;
    s16x8 pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = __builtin_amdgcn_exp2f(fmaf(acc_s[kb][r], scale_log2, neg_mc));
        lsum += p[r];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        u32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = pack2<T>(p[8 * s + 2 * j], p[8 * s + 2 * j + 1]);
        pf[kb][s] = __builtin_bit_cast(s16x8, w);
      }
    }
    l_run += lsum;
    // ---- O^T += V^T P^T : DH / 32 channel blocks
#pragma unroll
    for (int db = 0; db < DH / 32; ++db) {
      const int row = db * 32 + lq;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const int chk = kb * 4 + 2 * s + lh;
          const s16x8 vf = *reinterpret_cast<const s16x8*>(sv + row * 128 + ((chk ^ ((row >> 1) & 7)) << 4));
          acc_o[db] = T::mfma32(vf, pf[kb][s], acc_o[db]);
        }
    }
  };

  const int ntiles = kmax / KV_TILE + 1;          // workgroup-uniform: every wave stages and meets every barrier
  load_regs(0);
  write_lds(0);
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int key0 = kt * KV_TILE;
    if (kt + 1 < ntiles) load_regs(key0 + KV_TILE);
    if (wave_on && key0 <= pmax) {                // wave-uniform
      if (key0 + KV_TILE - 1 <= pmin) compute(key0, cur, std::false_type{});
      else compute(key0, cur, std::true_type{});
    }
    if (kt + 1 < ntiles) write_lds(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // ---- normalise and store: lane owns row row0 + qs + lq, d = db * 32 + (r & 3) + 8 (r >> 2) + 4 lh
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_run;
  if (qs + lq < cnt) {
    uint16_t* op = a.out + (int64_t)(row0 + qs + lq) * a.Hq * DH + head * DH + 4 * lh;
#pragma unroll
    for (int db = 0; db < DH / 32; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float o0 = acc_o[db][4 * g + 0] * inv, o1 = acc_o[db][4 * g + 1] * inv;
        const float o2 = acc_o[db][4 * g + 2] * inv, o3 = acc_o[db][4 * g + 3] * inv;
        *reinterpret_cast<u32x2*>(op + db * 32 + 8 * g) = (u32x2){pack2<T>(o0, o1), pack2<T>(o2, o3)};
      }
  }
}

int group_width(int Hq, int Hkv) {
  const int G = Hq / Hkv;
  return G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1;
}

}  // namespace

int lm_prefill_attn_qtile(int Hq, int Hkv) { return 128 / group_width(Hq, Hkv); }

// rows: (sequence, position) pairs with every sequence's positions ascending and contiguous; row r of the chunk is row `r` of q / out
void lm_prefill_attn_tiles(const int2* rows, int M, int qtile, std::vector<int4>& tiles) {
  tiles.clear();
  for (int r = 0; r < M;) {
    int n = 1;                                    // the run: one sequence's contiguous positions
    while (r + n < M && rows[r + n].x == rows[r].x && rows[r + n].y == rows[r].y + n) ++n;
    for (int o = 0; o < n; o += qtile) tiles.push_back(make_int4(rows[r].x, rows[r].y + o, r + o, std::min(qtile, n - o)));
    r += n;
  }
}

const char* lm_prefill_attn_check(const LmPromptAttn& a) {
  if (!a.q || !a.kc || !a.vc || !a.out || !a.tiles) return "lm_prefill_attn: null operand";
  if (a.dtype != MIA_BF16 && a.dtype != MIA_F16) return "lm_prefill_attn: dtype must be MIA_BF16 or MIA_F16";
  if (a.dh != 64 && a.dh != 128) return "lm_prefill_attn: head_dim must be 64 or 128";
  if (a.Hq <= 0 || a.Hkv <= 0 || a.Hq % a.Hkv) return "lm_prefill_attn: n_heads must be a positive multiple of n_kv_heads";
  if (a.n_tiles <= 0 || a.max_ctx <= 0) return "lm_prefill_attn: nothing to do";
  if ((((uintptr_t)a.q | (uintptr_t)a.kc | (uintptr_t)a.vc) & 15) || ((uintptr_t)a.out & 7)) return "lm_prefill_attn: operands must be 16-byte (q, k, v) / 8-byte (out) aligned";
  if ((int64_t)a.n_tiles * (a.Hq / group_width(a.Hq, a.Hkv)) > 0x7fffffffll) return "lm_prefill_attn: too many workgroups";
  return nullptr;
}

int lm_prefill_attn_launch(const LmPromptAttn& a, hipStream_t s) {
  const int gw = group_width(a.Hq, a.Hkv);
  const dim3 grid(a.n_tiles * (a.Hq / gw)), block(256);
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)a.dh);
#define PA_GO(TT, DD, GG) hipLaunchKernelGGL((lm_prefill_attn_kernel<TT, DD, GG>), grid, block, 0, s, a, scale_log2)
#define PA_G(TT, DD) do { if (gw == 4) PA_GO(TT, DD, 4); else if (gw == 2) PA_GO(TT, DD, 2); else PA_GO(TT, DD, 1); } while (0)
  if (a.dtype == MIA_F16) { if (a.dh == 128) PA_G(F16, 128); else PA_G(F16, 64); }
  else                    { if (a.dh == 128) PA_G(BF16, 128); else PA_G(BF16, 64); }
#undef PA_G
#undef PA_GO
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
