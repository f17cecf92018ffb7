// attn128.hip -- fused (flash-style) full multi-head attention, head dim 128, bf16 / f16 operands, fp32 online softmax, gfx950.
//
// Serves Fun-ASR's two attention shapes: MultiHeadAttentionSANM (STT/FunASR/Layers/MultiHeadAttentionSANM.swift:124-175, 512 / 4 heads,
// q | k | v fused in one [M][3 D] buffer) and the adaptor's FunASRMultiHeadAttention (:221-260, 1024 / 8 heads, three Linears), both
// softmax(q k^T d_k^-0.5) v over the whole utterance.  q, k and v come with their own pointer and row stride, so one kernel reads both.
//
// The structure is attention.hip's (head dim 64) with the contraction doubled:
//   * one 256-thread workgroup = Q_TILE = 128 queries of one (sequence, head), one wave = 32 of them; keys are walked in KV_TILE = 64;
//   * S^T = K Q^T on v_mfma_f32_32x32x16 (8 k-steps): a lane owns ONE query column and 32 keys of it, so the online softmax is in-lane
//     plus one cross-half shuffle, and the S^T accumulator is, register for register, the B operand of O^T += V^T P^T (K rows are fed
//     with bits 2 <-> 3 of the row index swapped so that the register order is natural key order);
//   * K tiles [64 keys][128] (256-B rows, 16-B chunk index XOR (row & 15)) and V^T tiles [128 d][64 keys] (128-B rows, chunk index XOR
//     (row >> 1) & 7, the layout attention.hip reads conflict free) are staged HBM -> registers -> LDS, double buffered.  V arrives
//     row-major like q and k; it is transposed HERE, in the staging write: a thread holds 8 channels of two neighbouring keys and
//     writes one (key, key + 1) word per channel.  Those ds_write_b32 land 8 to a bank (16 per tile and thread, against 48 MFMAs per
//     wave); the 64-wide QKV_VT GEMM epilogue is not involved;
//   * a sequence of a stacked call walks ceil(seq_len[b] / 64) tiles and reads no row at or beyond seq_len[b] (loads are clamped to its
//     last row, the clamped keys masked to an exact zero probability), so its result is that of its own B = 1, T = seq_len[b] call bit
//     for bit; rows at or beyond seq_len[b] of `out` are not written.
// Sums run in a fixed order (no atomics): a repeat call returns the same bits.
#include <type_traits>

#include "mia_device.h"
#include "ops.h"

namespace {

constexpr int Q_TILE = 128;
constexpr int KV_TILE = 64;
constexpr int K_BYTES = KV_TILE * 256;          // [64 keys][128 d] x 2 B
constexpr int V_BYTES = 128 * 128;              // [128 d][64 keys] x 2 B
constexpr int BUF_BYTES = K_BYTES + V_BYTES;    // 32 KB, two of them

__device__ __forceinline__ int swap23(int r) {  // swap bits 2 and 3
  return (r & ~12) | ((r & 4) << 1) | ((r & 8) >> 1);
}

template <typename T>
__global__ __launch_bounds__(256) void attn128_kernel(Attn128Args a, float scale_log2) {
  __shared__ __attribute__((aligned(16))) char lds[2 * BUF_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nqb = (a.T + Q_TILE - 1) / Q_TILE;          // launch is 1-D: gridDim.x = nqb * H * B
  int lin = blockIdx.x;
  {  // every XCD gets a contiguous run of the linear index: the q-blocks of a (sequence, head) re-read the same K / V
    const int nwg = gridDim.x, q = nwg / 8, r = nwg % 8, xcd = lin % 8;
    lin = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + lin / 8;
  }
  const int qb = lin % nqb, hb = lin / nqb;
  const int h = hb % a.H, b = hb / a.H;
  const int Tb = a.seq_len ? min(a.T, max(1, a.seq_len[b])) : a.T;
  if (qb * Q_TILE >= Tb) return;                        // workgroup-uniform, ahead of every barrier
  const int q0 = qb * Q_TILE + wave * 32;
  const int lq = lane & 31, lh = lane >> 5;
  const int64_t row0 = (int64_t)b * a.T;
  const uint16_t* Qg = reinterpret_cast<const uint16_t*>(a.q) + row0 * a.ldq + h * 128;
  const uint16_t* Kg = reinterpret_cast<const uint16_t*>(a.k) + row0 * a.ldk + h * 128;
  const uint16_t* Vg = reinterpret_cast<const uint16_t*>(a.v) + row0 * a.ldv + h * 128;

  // ---- Q^T fragments (B operand): lane holds Q[q0 + lq][16 ks + 8 lh + 0..7]
  s16x8 qf[8];
  {
    int q = q0 + lq; q = q < Tb ? q : Tb - 1;
    const uint16_t* qp = Qg + (int64_t)q * a.ldq + 8 * lh;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[ks] = *reinterpret_cast<const s16x8*>(qp + 16 * ks);
  }

  // ---- staging.  K: 64 rows x 16 chunks of 16 B, 4 per thread (rows s_row + 16 i).  V: 32 key pairs x 16 chunks, 2 per thread.
  const int s_chk = tid & 15, s_row = tid >> 4;
  const uint16_t* kbase = Kg + s_chk * 8;
  const uint16_t* vbase = Vg + s_chk * 8;
  u32x4 rk[4], rv[2][2];
  auto load_regs = [&](int key0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int key = key0 + s_row + 16 * i; key = key < Tb ? key : Tb - 1;        // masked below; the clamped row is the sequence's own
      rk[i] = *reinterpret_cast<const u32x4*>(kbase + (int64_t)key * a.ldk);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        int key = key0 + 2 * (s_row + 16 * i) + e; key = key < Tb ? key : Tb - 1;
        rv[i][e] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)key * a.ldv);
      }
  };
  auto write_lds = [&](int buf) {
    char* kd = lds + buf * BUF_BYTES;
    char* vd = kd + K_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = s_row + 16 * i;
      *reinterpret_cast<u32x4*>(kd + row * 256 + ((s_chk ^ (row & 15)) << 4)) = rk[i];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int pair = s_row + 16 * i;                   // keys 2 pair, 2 pair + 1 of the tile
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = 8 * s_chk + j;
        const uint32_t lo = rv[i][0][j >> 1], hi = rv[i][1][j >> 1];
        const uint32_t w = (j & 1) ? (lo >> 16) | (hi & 0xffff0000u) : (lo & 0xffffu) | (hi << 16);
        *reinterpret_cast<uint32_t*>(vd + d * 128 + (((pair >> 2) ^ ((d >> 1) & 7)) << 4) + (pair & 3) * 4) = w;
      }
    }
  };

  f32x16 acc_o[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_o[i][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;

  const int krow = swap23(lq);   // K row fed to MFMA row lq
  const int ntiles = (Tb + KV_TILE - 1) / KV_TILE;
  // One K / V tile; TAIL (the last, partial tile only) masks the keys at or beyond Tb.  The softmax works on the raw scores:
  // p = exp2(fma(s, c, -m c)) with c = scale * log2(e) > 0 and the reference point m kept raw.
  auto tile = [&](int kt, int cur, auto tail_tag) {
    constexpr bool TAIL = decltype(tail_tag)::value;
    const int key0 = kt * KV_TILE;
    if (kt + 1 < ntiles) load_regs(key0 + KV_TILE);
    const char* sk = lds + cur * BUF_BYTES;
    const char* sv = sk + K_BYTES;

    // ---- S^T = K Q^T : two 32-key blocks, 8 k-steps of 16
    f32x16 acc_s[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc_s[kb][r] = 0.f;
      const int row = kb * 32 + krow;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const s16x8 kf = *reinterpret_cast<const s16x8*>(sk + row * 256 + (((2 * ks + lh) ^ (row & 15)) << 4));
        acc_s[kb] = T::mfma32(kf, qf[ks], acc_s[kb]);
      }
    }
    // ---- online softmax (base 2), lane = one query, registers = keys
    float mloc = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (TAIL) {
          const int i = (r & 3) + 8 * (r >> 2) + 4 * lh;
          if (key0 + kb * 32 + swap23(i) >= Tb) acc_s[kb][r] = -INFINITY;
        }
        mloc = fmaxf(mloc, acc_s[kb][r]);
      }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    // bounded-growth lazy rescaling (attention.hip): the reference point moves only when the tile's maximum exceeds it by more than
    // 2^LAZY_LOG2, so p <= 2^LAZY_LOG2 -- in range for f16, and the 16-bit P keeps its relative precision at any scale.  A lane that
    // stays multiplies by an exact 1, so a query's bits do not depend on what the other lanes of its wave hold.
    constexpr float LAZY_LOG2 = 8.0f;
    const bool grow = (mloc - m_run) * scale_log2 > LAZY_LOG2;   // first tile: m_run = -inf; every tile holds >= 1 valid key
    if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {
      const float m_new = grow ? mloc : m_run;
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int db = 0; db < 4; ++db)
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

    // ---- O^T += V^T P^T : four 32-channel blocks
#pragma unroll
    for (int db = 0; db < 4; ++db) {
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
    if (kt + 1 < ntiles) write_lds(cur ^ 1);
    __syncthreads();
  };
  load_regs(0);
  write_lds(0);
  __syncthreads();
  const int nfull = Tb / KV_TILE;
  int cur = 0;
  for (int kt = 0; kt < nfull; ++kt) { tile(kt, cur, std::false_type{}); cur ^= 1; }
  if (nfull < ntiles) tile(nfull, cur, std::true_type{});

  // ---- normalise and store: lane owns query q0 + lq, d = db * 32 + (r & 3) + 8 (r >> 2) + 4 lh
  l_run += __shfl_xor(l_run, 32, 64);
  const float inv = 1.0f / l_run;
  const int q = q0 + lq;
  if (q < Tb) {
    uint16_t* op = reinterpret_cast<uint16_t*>(a.out) + (row0 + q) * a.ldo + h * 128 + 4 * lh;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float o0 = acc_o[db][4 * g + 0] * inv, o1 = acc_o[db][4 * g + 1] * inv;
        const float o2 = acc_o[db][4 * g + 2] * inv, o3 = acc_o[db][4 * g + 3] * inv;
        *reinterpret_cast<u32x2*>(op + db * 32 + 8 * g) = (u32x2){pack2<T>(o0, o1), pack2<T>(o2, o3)};
      }
  }
}

}  // namespace

const char* mia_attn128_check(const Attn128Args& a) {
  if (a.B <= 0 || a.T <= 0 || a.H <= 0) return "attn128: B, T, H must be > 0";
  if (!a.q || !a.k || !a.v || !a.out) return "attn128: null operand";
  if (a.dtype != MIA_BF16 && a.dtype != MIA_F16) return "attn128: dtype must be MIA_BF16 or MIA_F16";
  const int64_t D = (int64_t)a.H * 128;
  if (a.ldq < D || a.ldk < D || a.ldv < D || a.ldo < D) return "attn128: row strides must be >= H * 128";
  if (a.ldq % 8 || a.ldk % 8 || a.ldv % 8 || a.ldo % 4) return "attn128: row strides must keep 16-byte (q, k, v) / 8-byte (out) alignment";
  if ((((uintptr_t)a.q | (uintptr_t)a.k | (uintptr_t)a.v) & 15) || ((uintptr_t)a.out & 7)) return "attn128: operands must be 16-byte (q, k, v) / 8-byte (out) aligned";
  if (!(a.scale > 0.f)) return "attn128: scale must be > 0";
  if ((int64_t)((a.T + Q_TILE - 1) / Q_TILE) * a.H * a.B > 0x7fffffffll) return "attn128: too many workgroups";
  return nullptr;
}

int mia_attn128_launch(const Attn128Args& a, hipStream_t s) {
  dim3 grid(((a.T + Q_TILE - 1) / Q_TILE) * a.H * a.B), block(256);
  const float scale_log2 = a.scale * 1.4426950408889634f;
  if (a.dtype == MIA_F16) hipLaunchKernelGGL((attn128_kernel<F16>), grid, block, 0, s, a, scale_log2);
  else hipLaunchKernelGGL((attn128_kernel<BF16>), grid, block, 0, s, a, scale_log2);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
