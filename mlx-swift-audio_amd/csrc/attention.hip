// attention.hip -- fused (flash-style) multi-head attention for the Whisper encoder, head dim 64, gfx950.
//
// Replaces WhisperMultiHeadAttention.qkvAttention (STT/Whisper/Layers/MultiHeadAttention.swift:85-135) for the
// encoder's full (unmasked) self-attention: softmax((q s)(k s)^T) v with s = d_h^-1/4 on both operands, fp32
// softmax ("precise").  The raw qk tensor the Swift returns is only used by word timestamps, not on this path.
//
// Structure (one 256-thread workgroup = 128 or 256 queries of one (clip, head); one wave = one or two blocks of 32 queries):
//   * S^T = K Q^T on v_mfma_f32_32x32x16 ("swapped" product): a lane then owns ONE query column and 32 keys of
//     it in registers, so the row max / row sum of the online softmax are in-lane plus one cross-half shuffle;
//   * the S^T accumulator is consumed directly as the B operand of O^T = V^T P^T (no LDS round trip): K rows are
//     fed with bits 2<->3 of the row index swapped so the accumulator's register order equals natural key order;
//   * K tiles [64 keys][64] and V^T tiles [64 d][64 keys] arrive by LDS-DMA into a ring of three slots, two tiles ahead of the
//     compute, behind counted vmcnt waits and one s_barrier per tile (enc_attention_body has the order and why it is safe); 128-B rows
//     with the 16-B chunk index XOR-swizzled by (row>>1)&7 so all fragment reads (ds_read_b128) are bank-conflict free;
//   * with two query blocks per wave (enc_attn_q64_kernel, T >= 256) a K / V^T fragment read from LDS feeds both blocks' MFMAs and one
//     block's softmax is issued between the other block's MFMAs;
//   * V arrives pre-transposed ([B][H][64][Tpad], zero padded) from the QKV GEMM epilogue (gemm.hip QKV_VT).
// The register-staged form (HBM -> registers -> LDS, two buffers) that preceded the ring stays compiled as the reference of the
// operator-level tests (tests/test_enc_attn_variants_gpu.py): every form must produce its bits.
#include <type_traits>

#include "mia_device.h"
#include "ops.h"

namespace {

constexpr int KV_TILE = 64;
constexpr int TILE_BYTES = 64 * 128;  // 8 KB

__device__ __forceinline__ int swap23(int r) {  // swap bits 2 and 3
  return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1);
}

// LDS-DMA destination of one wave-instruction: wave-uniform base + lane * 16 B (1 KB = 8 tile rows)
__device__ __forceinline__ void glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, 0, 0);
}

#define ATT_BAR()                                 \
  do {                                            \
    asm volatile("" ::: "memory");                \
    __builtin_amdgcn_s_barrier();                 \
    asm volatile("" ::: "memory");                \
  } while (0)

constexpr int SLOT_BYTES = 2 * TILE_BYTES;   // one key tile: [K | V^T]

// NQ   = 32-query blocks per wave (workgroup = 4 waves = 128 * NQ queries).  NQ = 2 reads every K / V^T fragment from LDS once for both
//        blocks and runs block 0's softmax between block 1's MFMAs (and block 1's between block 0's P V MFMAs).
// DMA  = false: K / V^T tiles staged HBM -> registers -> LDS, two buffers (issue early, write after the compute, one __syncthreads()).
//        true:  LDS-DMA (global_load_lds_dwordx4) into a ring of three slots, K and V^T of tile t + 2 issued at the head of tile t.  The
//        LDS image is lane-linear per wave-instruction, so the (row >> 1) & 7 chunk swizzle sits on the per-lane SOURCE address.
//        Per tile t:  s_waitcnt vmcnt(4 | 0)  (tile t landed; only tile t + 1's four loads may stay in flight)  ->  s_barrier  (every
//        wave's part of tile t is visible, and every wave has finished reading tile t - 1, whose slot is (t + 2) % 3)  ->  issue tile
//        t + 2  ->  read and compute tile t.  So a slot is first read one barrier after the wait that retires it, and re-staged only
//        after the barrier that follows its last read.  No wait here spins on memory: the kernel cannot hang.
// Per query the arithmetic is the same in every form (key-tile order, raw-max softmax, lazy rescale, fp32 accumulation): a lane that
// does not grow multiplies by exp2(0) = 1, so a query's result does not depend on the queries it shares a wave with.
template <typename T, int NQ, bool DMA>
__device__ __forceinline__ void enc_attention_body(char* lds, const uint16_t* __restrict__ qk, int64_t ld_qk,
                                                   const uint16_t* __restrict__ vt, uint16_t* __restrict__ out, int64_t ld_out,
                                                   int T_len, int Tpad, int H, float scale_log2) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // XCD-aware mapping: the q-blocks of one (clip, head) re-read the same K / V^T; consecutive block ids are dealt round-robin to
  // the 8 XCDs, so give every XCD a contiguous run of the linear index and keep the q-blocks of a (clip, head) adjacent in it.
  constexpr int QWG = 128 * NQ;
  const int nqb = (T_len + QWG - 1) / QWG;               // launch is 1-D: gridDim.x = nqb * H * B
  int lin = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, xcd = lin % 8;
    lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + lin / 8;
  }
  const int qb = lin % nqb, hb = lin / nqb;
  const int h = hb % H, b = hb / H;
  const int D = H * 64;
  const int q0 = qb * QWG + wave * (32 * NQ);            // block n of this wave: queries q0 + 32 n ..
  const int lq = lane & 31, lh = lane >> 5;

  // ---- Q^T fragments (B operand): lane holds Q[q0+32n+lq][16*ks + 8*lh + 0..7]
  s16x8 qf[NQ][4];
  auto load_q = [&]() {
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      int q = q0 + 32 * n + lq; q = q < T_len ? q : T_len - 1;
      const uint16_t* qp = qk + ((int64_t)b * T_len + q) * ld_qk + h * 64 + 8 * lh;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) qf[n][ks] = *reinterpret_cast<const s16x8*>(qp + 16 * ks);
    }
  };
  if (!DMA) load_q();

  // ---- staging: 2 x 16 B of K and 2 x 16 B of V^T per thread per tile (tile rows s_row and s_row + 32, which share (row >> 1) & 7)
  const int s_row = tid >> 3, s_pos = tid & 7;
  // register staging: the thread holds logical chunk s_pos and writes it to its swizzled place.  LDS-DMA: the thread's bytes land at
  // position s_pos of the row, so it fetches the logical chunk that lives there.
  const int s_chk = DMA ? (s_pos ^ ((s_row >> 1) & 7)) : s_pos;
  const uint16_t* kbase = qk + (int64_t)b * T_len * ld_qk + D + h * 64 + s_chk * 8;
  const uint16_t* vbase = vt + ((int64_t)b * H + h) * 64 * Tpad + s_chk * 8;
  const int ntiles = (T_len + KV_TILE - 1) / KV_TILE;
  const int nfull = T_len / KV_TILE;

  // -- register staging
  int s_dst[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = s_row + 32 * i;
    s_dst[i] = row * 128 + ((s_pos ^ ((row >> 1) & 7)) << 4);
  }
  u32x4 rk[2], rv[2];
  auto load_regs = [&](int key0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int row = s_row + 32 * i;
      int key = key0 + row; key = key < T_len ? key : T_len - 1;   // masked below; any finite value will do
      rk[i] = *reinterpret_cast<const u32x4*>(kbase + (int64_t)key * ld_qk);
      rv[i] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)row * Tpad + key0);
    }
  };
  auto write_lds = [&](int buf) {
    char* base = lds + buf * SLOT_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      *reinterpret_cast<u32x4*>(base + s_dst[i]) = rk[i];
      *reinterpret_cast<u32x4*>(base + TILE_BYTES + s_dst[i]) = rv[i];
    }
  };

  // -- LDS-DMA staging: per-lane sources of the NEXT tile to issue, advanced by a constant per tile.  Full tiles (all 64 keys < T_len)
  // need no clamp; the tail tile's K rows are clamped to the last key (masked in the softmax).  V^T reads columns below
  // align_up(T_len, 64) <= Tpad only, whose pad columns are zero by contract.  Issue order is tile 0, 1, 2, ...
  const uint16_t* kp[2];
  const uint16_t* vp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    kp[i] = kbase + (int64_t)(s_row + 32 * i) * ld_qk;
    vp[i] = vbase + (int64_t)(s_row + 32 * i) * Tpad;
  }
  const int64_t k_step = (int64_t)KV_TILE * ld_qk;
  int slot_issue = 0;                                                 // wave-uniform: tile % 3 of the next tile to issue
  char* const lds_wave = lds + __builtin_amdgcn_readfirstlane(wave) * 1024;   // rows 8 * wave .. + 7 (and + 32) of every tile
  auto issue_full = [&]() {
    char* dst = lds_wave + slot_issue * SLOT_BYTES;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      glds16(kp[i], dst + i * 4096);
      glds16(vp[i], dst + TILE_BYTES + i * 4096);
      kp[i] += k_step;
      vp[i] += KV_TILE;
    }
    slot_issue = slot_issue == 2 ? 0 : slot_issue + 1;
  };
  auto issue = [&](int kt) {                                          // kt < ntiles, called in tile order
    if (kt < nfull) {
      issue_full();
    } else {
      char* dst = lds_wave + slot_issue * SLOT_BYTES;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        int key = kt * KV_TILE + s_row + 32 * i; key = key < T_len ? key : T_len - 1;
        glds16(kbase + (int64_t)key * ld_qk, dst + i * 4096);
        glds16(vp[i], dst + TILE_BYTES + i * 4096);
      }
      slot_issue = slot_issue == 2 ? 0 : slot_issue + 1;
    }
  };

  f32x16 acc_o[NQ][2];
  float m_run[NQ], l_run[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_o[n][i][r] = 0.f;
    m_run[n] = -INFINITY; l_run[n] = 0.f;
  }

  const int krow = swap23(lq);   // K row fed to MFMA row lq
  // One K/V tile.  TAIL (the last, partial tile only) masks the keys at or beyond T_len: in the full tiles the masking selects are
  // not compiled at all (as a runtime `if (tail)` hipcc if-converted them into ~170 of the tile's ~480 instructions, every tile).
  // The softmax works on the RAW scores: max over s, then p = exp2(fma(s, c, -m c)) with c = scale * log2(e) > 0 -- one fma + one
  // exp per score instead of mul, sub, exp; the reference point m is kept raw.
  auto tile = [&](int kt, int cur, auto tail_tag, auto steady_tag) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    constexpr bool STEADY = decltype(steady_tag)::value;   // DMA only: tile kt + 2 exists and is a full tile -- no run-time choices
    const int key0 = kt * KV_TILE;
    if (DMA) {
      // tile kt has landed (the wave's own part; the barrier makes it every wave's); at most tile kt + 1 stays in flight
      if (STEADY || kt + 1 < ntiles) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      ATT_BAR();
      if (STEADY) issue_full();                    // into the slot tile kt - 1 was read from, before this barrier
      else if (kt + 2 < ntiles) issue(kt + 2);
    } else {
      if (kt + 1 < ntiles) load_regs(key0 + KV_TILE);
    }
    const char* sk = lds + cur * SLOT_BYTES;
    const char* sv = sk + TILE_BYTES;

    f32x16 acc_s[NQ][2];
    s16x8 kf[2][4], vf[2][4], pf[NQ][2][2];
    // ---- S^T = K Q^T : two 32-key blocks
    auto read_k = [&]() {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        const int row = kb * 32 + krow;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          kf[kb][ks] = *reinterpret_cast<const s16x8*>(sk + row * 128 + (((2 * ks + lh) ^ ((row >> 1) & 7)) << 4));
      }
    };
    auto read_v = [&]() {
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const int row = db * 32 + lq;
#pragma unroll
        for (int c = 0; c < 4; ++c) {               // c = kb * 2 + s
          const int chk = 2 * c + lh;
          vf[db][c] = *reinterpret_cast<const s16x8*>(sv + row * 128 + ((chk ^ ((row >> 1) & 7)) << 4));
        }
      }
    };
    auto s_mma = [&](int n, int kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_s[n][kb][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) acc_s[n][kb] = T::mfma32(kf[kb][ks], qf[n][ks], acc_s[n][kb]);
    };
    // ---- online softmax (base-2), lane = one query, registers = keys
    auto soft_max = [&](int n) {
      float mloc = -INFINITY;
      int left = T_len - key0;                       // valid keys of the tail tile
      // (opaque per block: shared between two blocks, the 32 compare masks stay live in 64 scalar registers and spill)
      if (TAIL && NQ > 1) asm volatile("" : "+v"(left));
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (TAIL) {
            const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (kb * 32 + swap23(i) >= left) acc_s[n][kb][r] = -INFINITY;
          }
          mloc = fmaxf(mloc, acc_s[n][kb][r]);
        }
      return fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    };
    // Bounded-growth lazy rescaling: the reference point m_run of a query moves only when the tile's maximum exceeds it by more than
    // 2^LAZY_LOG2 (in the exponent's units), so p = exp2(c (s - m_run)) <= 2^LAZY_LOG2 and the O / l rescale -- 32 multiplies + one exp
    // per tile, ~12 % of the loop's vector issue -- runs in the first tile and then almost never (softmax is invariant to the reference
    // point; the 16-bit P keeps its relative precision at any scale, O and l accumulate in fp32).  The test is wave-uniform.
    auto rescale = [&](int n, float mloc) {
      constexpr float LAZY_LOG2 = 8.0f;
      const bool grow = (mloc - m_run[n]) * scale_log2 > LAZY_LOG2;   // first tile: m_run = -inf; every tile holds >= 1 valid key
      if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {
        const float m_new = grow ? mloc : m_run[n];
        const float alpha = __builtin_amdgcn_exp2f((m_run[n] - m_new) * scale_log2);       // 1 for the lanes that stay
        m_run[n] = m_new;
        l_run[n] *= alpha;
#pragma unroll
        for (int db = 0; db < 2; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc_o[n][db][r] *= alpha;
      }
    };
    // (pairing the scores through v_pk_fma_f32 / v_pk_add_f32 was measured: 231 instead of 256 instructions per tile, 16.5-16.6 ms
    // per pass against 16.3-16.4 in alternating runs on one box -- the packed fp32 ops are not double rate here)
    auto soft_exp = [&](int n) {
      const float neg_mc = -m_run[n] * scale_log2;
      float lsum = 0.f;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        float p[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          p[r] = __builtin_amdgcn_exp2f(fmaf(acc_s[n][kb][r], scale_log2, neg_mc));
          lsum += p[r];
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          u32x4 w;
#pragma unroll
          for (int j = 0; j < 4; ++j) w[j] = pack2<T>(p[8 * s + 2 * j], p[8 * s + 2 * j + 1]);
          pf[n][kb][s] = __builtin_bit_cast(s16x8, w);
        }
      }
      l_run[n] += lsum;
    };
    // ---- O^T += V^T P^T
    auto pv_mma = [&](int n, int db) {
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int s = 0; s < 2; ++s) acc_o[n][db] = T::mfma32(vf[db][kb * 2 + s], pf[n][kb][s], acc_o[n][db]);
    };

    read_k();
    if (NQ == 1) {
      s_mma(0, 0); s_mma(0, 1);
      rescale(0, soft_max(0));
      soft_exp(0);
      read_v();
      pv_mma(0, 0); pv_mma(0, 1);
    } else {
      // two independent chains, interleaved by hand between the basic blocks the rescale branches cut:
      //   S0 | S1[keys 0..31] + max0 | branch0 | S1[keys 32..63] + exp0 ; P0 V[d 0..31] + max1 | branch1 | P0 V[d 32..63] + exp1 | P1 V
      constexpr int N1 = NQ - 1;
      s_mma(0, 0); s_mma(0, 1);
      s_mma(N1, 0);
      const float m0 = soft_max(0);
      rescale(0, m0);
      s_mma(N1, 1);
      soft_exp(0);
      read_v();
      pv_mma(0, 0);
      const float m1 = soft_max(N1);
      rescale(N1, m1);
      pv_mma(0, 1);
      soft_exp(N1);
      pv_mma(N1, 0); pv_mma(N1, 1);
    }
    if (!DMA) {
      if (kt + 1 < ntiles) write_lds(cur ^ 1);
      __syncthreads();
    }
  };
  if (DMA) {
    issue(0);
    if (ntiles > 1) issue(1);
    // Q after the first two tiles' DMA, and pinned here: an ordinary load still pending at the loop's head would make the compiler
    // wait vmcnt(0) -- every DMA in flight -- at the first MFMA of every tile
    load_q();
#pragma unroll
    for (int n = 0; n < NQ; ++n)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qf[n][ks]));
    int cur = 0, kt = 0;
    for (; kt + 2 < nfull; ++kt) { tile(kt, cur, std::false_type{}, std::true_type{}); cur = cur == 2 ? 0 : cur + 1; }
    for (; kt < nfull; ++kt) { tile(kt, cur, std::false_type{}, std::false_type{}); cur = cur == 2 ? 0 : cur + 1; }
    if (nfull < ntiles) tile(nfull, cur, std::true_type{}, std::false_type{});
  } else {
    load_regs(0);
    write_lds(0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nfull; ++kt) { tile(kt, cur, std::false_type{}, std::false_type{}); cur ^= 1; }
    if (nfull < ntiles) tile(nfull, cur, std::true_type{}, std::false_type{});
  }

  // ---- normalise and store: lane owns query q0+32n+lq, d = db*32 + (r&3) + 8*(r>>2) + 4*lh
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    l_run[n] += __shfl_xor(l_run[n], 32, 64);
    const float inv = 1.0f / l_run[n];
    int q = q0 + 32 * n + lq;
    // (opaque: shared with the Q load's row address, the 64-bit row offset is carried across the tile loop and spills)
    if (NQ > 1) asm volatile("" : "+v"(q));
    if (q < T_len) {
      uint16_t* op = out + ((int64_t)b * T_len + q) * ld_out + h * 64 + 4 * lh;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float o0 = acc_o[n][db][4 * g + 0] * inv, o1 = acc_o[n][db][4 * g + 1] * inv;
          const float o2 = acc_o[n][db][4 * g + 2] * inv, o3 = acc_o[n][db][4 * g + 3] * inv;
          *reinterpret_cast<u32x2*>(op + db * 32 + 8 * g) = (u32x2){pack2<T>(o0, o1), pack2<T>(o2, o3)};
        }
    }
  }
}

// 128 queries per workgroup, 32 per wave: <= 168 VGPRs, three workgroups per CU (48 KB of LDS each with the ring).
template <typename T, bool DMA>
__global__ __launch_bounds__(256, 2) void enc_attention_kernel(const uint16_t* __restrict__ qk, int64_t ld_qk,
                                                               const uint16_t* __restrict__ vt, uint16_t* __restrict__ out,
                                                               int64_t ld_out, int T_len, int Tpad, int H, float scale_log2) {
  __shared__ __attribute__((aligned(16))) char lds[(DMA ? 3 : 2) * SLOT_BYTES];
  enc_attention_body<T, 1, DMA>(lds, qk, ld_qk, vt, out, ld_out, T_len, Tpad, H, scale_log2);
}

// 256 queries per workgroup, 64 per wave (two 32-query blocks), LDS-DMA ring: ~255 VGPRs, two workgroups per CU, 128 queries in flight
// per SIMD instead of 96.  (Register-staged, this form was measured too: slower than the ring, and its 16 staging registers spill.)
template <typename T>
__global__ __launch_bounds__(256, 2) void enc_attn_q64_kernel(const uint16_t* __restrict__ qk, int64_t ld_qk,
                                                              const uint16_t* __restrict__ vt, uint16_t* __restrict__ out,
                                                              int64_t ld_out, int T_len, int Tpad, int H, float scale_log2) {
  __shared__ __attribute__((aligned(16))) char lds[3 * SLOT_BYTES];
  enc_attention_body<T, 2, true>(lds, qk, ld_qk, vt, out, ld_out, T_len, Tpad, H, scale_log2);
}

}  // namespace

const char* mia_enc_attention_check(int B, int T, int H, int Tpad, int64_t ld_qk, int64_t ld_out) {
  if (B <= 0 || T <= 0 || H <= 0) return "attention: B, T, H must be > 0";
  if (Tpad % 64 || Tpad < T) return "attention: Tpad must be a multiple of 64 and >= T";
  if (ld_qk % 8 || ld_out % 4) return "attention: row strides must keep 16-byte (qk) / 8-byte (out) alignment";
  return nullptr;
}

template <typename E>
static void launch_variant(int variant, dim3 block, hipStream_t s, const uint16_t* qk, int64_t ld_qk, const uint16_t* vt, uint16_t* out,
                           int64_t ld_out, int B, int T, int H, int Tpad, float scale_log2) {
  const dim3 g128(((T + 127) / 128) * H * B), g256(((T + 255) / 256) * H * B);
  switch (variant) {
    case MIA_ATT_REG128: hipLaunchKernelGGL((enc_attention_kernel<E, false>), g128, block, 0, s, qk, ld_qk, vt, out, ld_out, T, Tpad, H, scale_log2); break;
    case MIA_ATT_DMA128: hipLaunchKernelGGL((enc_attention_kernel<E, true>), g128, block, 0, s, qk, ld_qk, vt, out, ld_out, T, Tpad, H, scale_log2); break;
    default: hipLaunchKernelGGL((enc_attn_q64_kernel<E>), g256, block, 0, s, qk, ld_qk, vt, out, ld_out, T, Tpad, H, scale_log2); break;
  }
}

int mia_enc_attention_launch_variant(const void* qk, int64_t ld_qk, const void* vt, void* out, int64_t ld_out, int B, int T, int H,
                                     int Tpad, int dtype, int variant, hipStream_t s) {
  if (variant < 0 || variant >= MIA_ATT_NVARIANTS) return -1;
  const float scale_log2 = 0.125f * 1.4426950408889634f;  // (64^-1/4)^2 * log2(e)
  if (dtype == MIA_F16)
    launch_variant<F16>(variant, dim3(256), s, (const uint16_t*)qk, ld_qk, (const uint16_t*)vt, (uint16_t*)out, ld_out, B, T, H, Tpad, scale_log2);
  else
    launch_variant<BF16>(variant, dim3(256), s, (const uint16_t*)qk, ld_qk, (const uint16_t*)vt, (uint16_t*)out, ld_out, B, T, H, Tpad, scale_log2);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int mia_enc_attention_launch(const void* qk, int64_t ld_qk, const void* vt, void* out, int64_t ld_out, int B, int T, int H,
                             int Tpad, int dtype, hipStream_t s) {
  // Measured on one MI355X (bf16, H = 20; LABNOTES): at 32 clips the 64-query form loses below T = 768 (a short sequence leaves its
  // second query block half empty and its few key tiles do not repay the longer prologue), ties there and wins from T = 1024 on; at
  // T = 1500 it loses at 120 workgroups (one clip: 256 CUs, half of them idle), ties at 240 and wins from 480 on.
  const int64_t nwg256 = (int64_t)((T + 255) / 256) * H * B;
  const int variant = T >= 1024 && nwg256 >= 480 ? MIA_ATT_DMA256 : MIA_ATT_DMA128;
  return mia_enc_attention_launch_variant(qk, ld_qk, vt, out, ld_out, B, T, H, Tpad, dtype, variant, s);
}
