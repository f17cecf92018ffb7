// lm_prefill_attn_kvq.hip -- lm_prefill_attn.hip's tiled causal grouped-query attention over the QUANTISED KV cache (lm_kvq.hip: 4- / 8-bit
// codes plus a 16-bit (scale, bias) pair per 64 values), head dim 64 / 128, bf16 / f16 handles, gfx950.  The codes themselves are the
// matrix-core operands; scale and bias are applied in fp32 around the MFMAs.
//
// Serves lm_prefill_rows (lm.hip) when mia_lm_set_kvq_prompt_attention(lm, 1) is set and the cache is packed.  It replaces one
// lm_kvq_attention<.., FUSED = false> workgroup per (query head, row), each of which re-reads and de-quantises its head's cache from key 0
// on the VALU.
//
// Work split, mask rule, lazy rescale, clamped loads and double buffering are lm_prefill_attn.hip's: query tiles of 128 / GW positions of
// GW = 4 | 2 | 1 heads of one KV group (lm_prefill_attn_tiles / _qtile), 256 threads, one wave = 32 positions of one head, key tiles of 64
// anchored at key 0, nothing past the workgroup's last position is read.  What differs:
//   * staging.  A thread's 8 elements of a cached row are one code dword (4 bit) or two (8 bit).  They are unpacked ONCE per workgroup
//     into the 16-bit numbers equal to the codes (0 .. 255 are exact in bf16 and f16) and written to the same swizzled K [64 keys][dh]
//     and V^T [dh][64 keys] tiles, so the compute loop's LDS reads and MFMA operand order are unchanged.  Next to them go the tile's
//     pairs as fp32: scale_K, bias_K, 2^BITS scale_V, bias_V, each [dh / 64][64 keys];
//   * scores.  Per 64-element group g of the head dim, S_g^T = Code_g Q_g^T on v_mfma_f32_32x32x16 (integer-valued code x 16-bit q:
//     exact products), then in fp32  s[k][q] = sum_g scale_K[k][g] S_g[k][q] + bias_K[k][g] qsum_g[q],  qsum_g = the fp32 sum of the
//     lane's own q row over the group (in-lane half + one cross-half shuffle, once per kernel);
//   * output.  O[q][d] = sum_k code_V[k][d] (p[k] scale_V[k][g(d)]) + sum_k p[k] bias_V[k][g(d)].  The first term is the V^T P^T MFMA
//     with P multiplied by the key's V scale of that group before it is packed to 16 bits (its own P fragments per group); the second
//     is one fp32 scalar per (lane, group), summed in-lane over the lane's keys of the tile, rescaled with l_run, joined across the
//     half-waves at the end and added to the group's channels before the division by l.
//     p scale_V goes in as a hi + lo pair of 16-bit numbers, two MFMAs per V fragment.  One 16-bit number is not enough here: its
//     rounding multiplies code scale_V, the value's distance from its group's MINIMUM -- for values around zero several times |v|,
//     where the 16-bit kernel's rounding of p multiplies v itself -- and the K/V rows the next layer forms from such an output sat up
//     to 1.18 of (half a quantisation step + the 16-bit path's own error) away from the oracle's.  With the pair the product carries
//     16 (bf16) / 22 (f16) significant bits and the kernel's only 16-bit rounding that matters is its output's.
// Nothing is de-quantised to 16 bits: rounding scale * code + bias to bf16 would be a second quantisation that the step kernel
// (lm_kvq_attention, fp32 read-back) does not make, and prompt rows and stepped rows would attend over different keys.
//
// f16 range.  p scale_V is below f16's normal range for small p (scale_V = range / 255 at 8 bits), so P carries a factor 2^BITS into the
// MFMA, taken out of the accumulator exactly in the epilogue.  The lazy rescale lets p reach 2^8, so the packed value is at most
// 2^8 * 2^BITS / (2^BITS - 1) * R with R = max - min of the key's V group: it stays finite in f16 (65504) for R < 239 at 4 bits and
// R < 254 at 8 bits -- 2^-8 of the type's range, where the 16-bit kernel has 2^-8 of it for p alone -- and always in bf16.
//
// Row independence (lm_prefill_attn.hip's argument, restated): a lane's arithmetic involves its own q row (qsum included), the staged
// codes and pairs of keys [0, its position] and its own position only.  The softmax's reference point moves per lane (a lane that stays
// multiplies l, O and the bias sums by an exact 1), keys above the lane's position have p = 0 exactly and add exact zeros to all three,
// and the key tiles do not depend on the query tiling -- so a row's bits depend on its own q row and on keys and values [0, p] only,
// not on the chunk, its tile mates or the other sequences.  Sums run in a fixed order (no atomics): a repeat call returns the same bits.
#include <type_traits>

#include "lm.h"
#include "lm_kvq_device.h"
#include "mia_device.h"

namespace {

constexpr int KV_TILE = 64;

struct KvqPromptAttn {
  const uint16_t* q; uint16_t* out;               // [M][Hq * dh]
  const uint32_t* kq; const uint32_t* vq; const uint32_t* kp; const uint32_t* vp;      // the layer's packed cache, all sequences
  const int4* tiles; int n_tiles;
  int Hq, Hkv, max_ctx;
};

template <typename T, int DH, int GW, int BITS>
__global__ __launch_bounds__(256) void lm_prefill_attn_kvq_kernel(KvqPromptAttn a, float scale_log2) {
  constexpr int CH = DH / 8;                      // 8-element chunks per row
  constexpr int RPI = 256 / CH;                   // K rows (V key pairs) staged per pass of the workgroup
  constexpr int NK = KV_TILE / RPI, NV = 32 / RPI;
  constexpr int WPL = BITS / 4;                   // code dwords per chunk
  constexpr int WPR = DH * BITS / 32, GPR = DH / 64;
  constexpr int K_BYTES = KV_TILE * DH * 2;       // [64 keys][DH], the codes as 16-bit numbers
  constexpr int V_BYTES = DH * 128;               // [DH][64 keys]
  constexpr int P_FLOATS = 4 * GPR * KV_TILE;     // scale_K | bias_K | 2^BITS scale_V | bias_V, each [GPR][64 keys]
  constexpr int BUF_BYTES = K_BYTES + V_BYTES + P_FLOATS * 4;
  constexpr float PSCALE = (float)(1 << BITS);
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
  const int64_t r0 = ((int64_t)seq * a.Hkv + kvh) * a.max_ctx;      // first row of this sequence's K/V head

  // ---- Q^T fragments (B operand): lane holds Q[row][16 ks + 8 lh + 0..7]; qsum[g] = the row's sum over group g
  s16x8 qf[DH / 16];
  float qsum[GPR];
  {
    const uint16_t* qp = a.q + (int64_t)(row0 + qi) * a.Hq * DH + head * DH + 8 * lh;
#pragma unroll
    for (int ks = 0; ks < DH / 16; ++ks) qf[ks] = *reinterpret_cast<const s16x8*>(qp + 16 * ks);
#pragma unroll
    for (int g = 0; g < GPR; ++g) {
      float t = 0.f;
#pragma unroll
      for (int ks = 4 * g; ks < 4 * g + 4; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) t += T::to_f32((uint16_t)qf[ks][j]);
      qsum[g] = t + __shfl_xor(t, 32, 64);        // (a + b in one half, b + a in the other: the same bits)
    }
  }

  // ---- staging.  Codes: 64 K rows x CH chunks, NK per thread (rows s_row + RPI i); 32 V key pairs x CH chunks, NV per thread.
  // Pairs: one dword per thread, (K | V) x 64 keys x GPR groups (threads [0, 128 GPR)).
  const int s_chk = tid % CH, s_row = tid / CH;
  const uint32_t* kbase = a.kq + r0 * WPR + s_chk * WPL;
  const uint32_t* vbase = a.vq + r0 * WPR + s_chk * WPL;
  const bool p_on = tid < 2 * KV_TILE * GPR;
  const int p_v = tid / (KV_TILE * GPR), p_key = (tid / GPR) % KV_TILE, p_g = tid % GPR;
  const uint32_t* pbase = (p_v ? a.vp : a.kp) + r0 * GPR + p_g;
  uint32_t rk[NK][WPL], rv[NV][2][WPL], rp = 0;
  auto load_regs = [&](int key0) {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int key = min(key0 + s_row + RPI * i, kmax);                     // masked below; the clamped row is the sequence's own
      load_codes<BITS>(kbase + (int64_t)key * WPR, rk[i]);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = min(key0 + 2 * (s_row + RPI * i) + e, kmax);
        load_codes<BITS>(vbase + (int64_t)key * WPR, rv[i][e]);
      }
    if (p_on) rp = pbase[(int64_t)min(key0 + p_key, kmax) * GPR];
  };
  auto kswz = [](int row) { return DH == 128 ? (row & 15) : ((row >> 1) & 7); };
  auto write_lds = [&](int buf) {
    char* kd = lds + buf * BUF_BYTES;
    char* vd = kd + K_BYTES;
    float* pd = reinterpret_cast<float*>(vd + V_BYTES);
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int row = s_row + RPI * i;
      float x[8];
      codes8<BITS>(rk[i], x);
      u32x4 w;
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = pack_codes<T>(x[2 * j], x[2 * j + 1]);
      *reinterpret_cast<u32x4*>(kd + row * (DH * 2) + ((s_chk ^ kswz(row)) << 4)) = w;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int pair = s_row + RPI * i;                  // keys 2 pair, 2 pair + 1 of the tile
      float x0[8], x1[8];
      codes8<BITS>(rv[i][0], x0);
      codes8<BITS>(rv[i][1], x1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = 8 * s_chk + j;
        *reinterpret_cast<uint32_t*>(vd + d * 128 + (((pair >> 2) ^ ((d >> 1) & 7)) << 4) + (pair & 3) * 4) = pack_codes<T>(x0[j], x1[j]);
      }
    }
    if (p_on) {
      const float sc = T::to_f32((uint16_t)(rp & 0xffffu)), bi = T::to_f32((uint16_t)(rp >> 16));
      pd[((2 * p_v) * GPR + p_g) * KV_TILE + p_key] = p_v ? sc * PSCALE : sc;      // (a power of two: exact)
      pd[((2 * p_v + 1) * GPR + p_g) * KV_TILE + p_key] = bi;
    }
  };

  f32x16 acc_o[DH / 32];
#pragma unroll
  for (int i = 0; i < DH / 32; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc_o[i][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f, ob[GPR];
#pragma unroll
  for (int g = 0; g < GPR; ++g) ob[g] = 0.f;

  // K row fed to MFMA row lq: bits 2 and 3 of the row index swapped, so that accumulator register r of 32-key block kb is key
  // kb * 32 + 16 (r >> 3) + 8 lh + (r & 7): two runs of 8 consecutive keys per lane
  const int krow = (lq & ~12) | ((lq & 4) << 1) | ((lq & 8) >> 1);
  // the lane's 16 keys of block kb from one of the pair arrays: arr 0 scale_K, 1 bias_K, 2 scale_V 2^BITS, 3 bias_V
  auto pair16 = [&](const float* pp, int arr, int g, int kb, float (&v)[16]) {
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(pp + (arr * GPR + g) * KV_TILE + kb * 32 + 16 * h2 + 8 * lh + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[8 * h2 + 4 * c + j] = t[j];
      }
  };
  // One K / V tile of one wave; MASK (tiles that reach past the wave's first position) gives the keys above the lane's own position
  // -inf, an exact zero probability.  The softmax works on the raw scores: p = exp2(fma(s, c, -m c)), c = scale * log2(e) > 0.
  auto compute = [&](int key0, int cur, auto mask_tag) {
    constexpr bool MASK = decltype(mask_tag)::value;
    const char* sk = lds + cur * BUF_BYTES;
    const char* sv = sk + K_BYTES;
    const float* pp = reinterpret_cast<const float*>(sv + V_BYTES);
    // ---- S_g^T = Code_g Q_g^T per group (4 k-steps), folded into the scores in fp32 in group order
    float sc_[2][16];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      const int row = kb * 32 + krow;
#pragma unroll
      for (int g = 0; g < GPR; ++g) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int ks = 4 * g; ks < 4 * g + 4; ++ks) {
          const s16x8 kf = *reinterpret_cast<const s16x8*>(sk + row * (DH * 2) + (((2 * ks + lh) ^ kswz(row)) << 4));
          acc = T::mfma32(kf, qf[ks], acc);
        }
        float ksc[16], kbi[16];
        pair16(pp, 0, g, kb, ksc);
        pair16(pp, 1, g, kb, kbi);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float t = kbi[r] * qsum[g];
          sc_[kb][r] = fmaf(ksc[r], acc[r], g == 0 ? t : sc_[kb][r] + t);
        }
      }
    }
    // ---- online softmax (base 2), lane = one query, registers = keys
    float mloc = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (MASK) {
          if (key0 + kb * 32 + 16 * (r >> 3) + 8 * lh + (r & 7) > p_lane) sc_[kb][r] = -INFINITY;
        }
        mloc = fmaxf(mloc, sc_[kb][r]);
      }
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    // bounded-growth lazy rescaling, decided per lane = per query row, as in lm_prefill_attn.hip: the reference point moves only when
    // the tile's maximum exceeds it by more than 2^LAZY_LOG2; a lane that stays multiplies by an exact 1.  A lane whose keys are all
    // masked here (mloc = -inf) stays: key 0 made its m_run finite in tile 0.
    constexpr float LAZY_LOG2 = 8.0f;
    const bool grow = (mloc - m_run) * scale_log2 > LAZY_LOG2;
    if (__builtin_amdgcn_ballot_w64(grow) != 0ull) {
      const float m_new = grow ? mloc : m_run;
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2);
      m_run = m_new;
      l_run *= alpha;
#pragma unroll
      for (int g = 0; g < GPR; ++g) ob[g] *= alpha;
#pragma unroll
      for (int db = 0; db < DH / 32; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc_o[db][r] *= alpha;
    }
    const float neg_mc = -m_run * scale_log2;
    float lsum = 0.f;
    // ---- per 32-key block and group: the bias sum, then O^T += Code_V^T (P scale_V)^T with P scale_V as a hi + lo pair of 16-bit
    // numbers (hi = the product rounded, lo = the exactly representable rest, rounded), one MFMA each, on the group's two channel blocks
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      float p[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = __builtin_amdgcn_exp2f(fmaf(sc_[kb][r], scale_log2, neg_mc));
        lsum += p[r];
      }
#pragma unroll
      for (int g = 0; g < GPR; ++g) {
        float vsc[16], vbi[16];
        pair16(pp, 2, g, kb, vsc);
        pair16(pp, 3, g, kb, vbi);
#pragma unroll
        for (int r = 0; r < 16; ++r) ob[g] = fmaf(p[r], vbi[r], ob[g]);
        s16x8 pf_hi[2], pf_lo[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          u32x4 wh, wl;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float xa = p[8 * s + 2 * j] * vsc[8 * s + 2 * j], xb = p[8 * s + 2 * j + 1] * vsc[8 * s + 2 * j + 1];
            wh[j] = pack2<T>(xa, xb);
            wl[j] = pack2<T>(xa - T::to_f32((uint16_t)(wh[j] & 0xffffu)), xb - T::to_f32((uint16_t)(wh[j] >> 16)));
          }
          pf_hi[s] = __builtin_bit_cast(s16x8, wh);
          pf_lo[s] = __builtin_bit_cast(s16x8, wl);
        }
#pragma unroll
        for (int db = 2 * g; db < 2 * g + 2; ++db) {
          const int row = db * 32 + lq;
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            const int chk = kb * 4 + 2 * s + lh;
            const s16x8 vf = *reinterpret_cast<const s16x8*>(sv + row * 128 + ((chk ^ ((row >> 1) & 7)) << 4));
            acc_o[db] = T::mfma32(vf, pf_hi[s], acc_o[db]);
            acc_o[db] = T::mfma32(vf, pf_lo[s], acc_o[db]);
          }
        }
      }
    }
    l_run += lsum;
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

  // ---- join the half-waves, take 2^BITS out, add the bias sums, normalise and store: lane owns row row0 + qs + lq,
  // d = db * 32 + (r & 3) + 8 (r >> 2) + 4 lh
  l_run += __shfl_xor(l_run, 32, 64);
#pragma unroll
  for (int g = 0; g < GPR; ++g) ob[g] += __shfl_xor(ob[g], 32, 64);
  const float inv = 1.0f / l_run;
  if (qs + lq < cnt) {
    uint16_t* op = a.out + (int64_t)(row0 + qs + lq) * a.Hq * DH + head * DH + 4 * lh;
#pragma unroll
    for (int db = 0; db < DH / 32; ++db)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (acc_o[db][4 * g4 + j] * (1.0f / PSCALE) + ob[db / 2]) * inv;
        *reinterpret_cast<u32x2*>(op + db * 32 + 8 * g4) = (u32x2){pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3])};
      }
  }
}

}  // namespace

const char* lm_prefill_attn_kvq_check(const LmKvq& a, const uint16_t* q, const uint16_t* out, const int4* tiles, int n_tiles) {
  if (!q || !out || !tiles || !a.kq || !a.vq || !a.kp || !a.vp) return "lm_prefill_attn_kvq: null operand";
  if (a.dtype != MIA_BF16 && a.dtype != MIA_F16) return "lm_prefill_attn_kvq: dtype must be MIA_BF16 or MIA_F16";
  if (a.dh != 64 && a.dh != 128) return "lm_prefill_attn_kvq: head_dim must be 64 or 128";
  if (a.bits != 4 && a.bits != 8) return "lm_prefill_attn_kvq: bits must be 4 or 8";
  if (a.Hq <= 0 || a.Hkv <= 0 || a.Hq % a.Hkv) return "lm_prefill_attn_kvq: n_heads must be a positive multiple of n_kv_heads";
  if (n_tiles <= 0 || a.max_ctx <= 0) return "lm_prefill_attn_kvq: nothing to do";
  if (((uintptr_t)q & 15) || (((uintptr_t)out | (uintptr_t)a.kq | (uintptr_t)a.vq) & 7)) return "lm_prefill_attn_kvq: operands must be 16-byte (q) / 8-byte (out, codes) aligned";
  if ((int64_t)n_tiles * a.Hq * lm_prefill_attn_qtile(a.Hq, a.Hkv) / 128 > 0x7fffffffll) return "lm_prefill_attn_kvq: too many workgroups";
  return nullptr;
}

int lm_prefill_attn_kvq_launch(const LmKvq& a, const uint16_t* q, uint16_t* out, const int4* tiles, int n_tiles, hipStream_t s) {
  const int gw = 128 / lm_prefill_attn_qtile(a.Hq, a.Hkv);      // query heads per workgroup
  const dim3 grid(n_tiles * (a.Hq / gw)), block(256);
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)a.dh);
  const KvqPromptAttn k{q, out, a.kq, a.vq, a.kp, a.vp, tiles, n_tiles, a.Hq, a.Hkv, a.max_ctx};
#define PQ_GO(TT, DD, GG, BB) hipLaunchKernelGGL((lm_prefill_attn_kvq_kernel<TT, DD, GG, BB>), grid, block, 0, s, k, scale_log2)
#define PQ_G(TT, DD, BB) do { if (gw == 4) PQ_GO(TT, DD, 4, BB); else if (gw == 2) PQ_GO(TT, DD, 2, BB); else PQ_GO(TT, DD, 1, BB); } while (0)
#define PQ_B(TT, DD) do { if (a.bits == 4) PQ_G(TT, DD, 4); else PQ_G(TT, DD, 8); } while (0)
  if (a.dtype == MIA_F16) { if (a.dh == 128) PQ_B(F16, 128); else PQ_B(F16, 64); }
  else                    { if (a.dh == 128) PQ_B(BF16, 128); else PQ_B(BF16, 64); }
#undef PQ_B
#undef PQ_G
#undef PQ_GO
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
