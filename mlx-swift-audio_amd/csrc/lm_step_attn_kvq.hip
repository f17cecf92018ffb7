// lm_step_attn_kvq.hip -- the LM decode step's attention on the QUANTISED KV cache (lm_kvq.hip: 4- / 8-bit codes plus a 16-bit (scale,
// bias) pair per 64 values), split over the keys and shared across a KV group: head dim 64 / 128, bf16 / f16 handles, gfx950.  The work
// split is lm_step_attn.hip's, the arithmetic on the codes is lm_prefill_attn_kvq.hip's: the codes themselves are the operands of
// v_mfma_f32_16x16x32, scale and bias are applied in fp32 around the MFMAs.  Serves lm_launch_attention (lm.hip) when
// mia_lm_set_kvq_step_attention(lm, 1) is set and the cache is packed; it replaces lm_kvq_attention<.., FUSED = true>, which runs one
// workgroup per (query head, sequence), each de-quantising its head's whole cache on the vector pipe -- once per query head of the group.
//
// lm_step_attn_kvq_split: grid (Hkv, nb, ceil(max_ctx / 256)), 256 threads.  A workgroup owns keys [256 s, 256 s + 256) of one KV head of
// one sequence and attends for all G = Hq / Hkv <= 16 query heads at once (the 16 MFMA columns).  It reads st[seq].pos on the device and
// returns, writing nothing, when the sequence is frozen or the slice starts beyond pos; slices are anchored at key 0, so what a workgroup
// computes depends on (sequence state, KV head, slice) only -- not on the batch, the capacity or graph versus direct launch.
//   * preamble (every live workgroup): the step's q rows of the G heads from the q|k|v GEMM's split-K slices -- sum of S <= 4 partials,
//     bias, RoPE, one 16-bit rounding: lm_kvq_attention<FUSED>'s preamble, operation for operation (no q/k-norm variant:
//     mia_lm_set_kv_quant refuses such handles) -- into LDS as 16-bit rows [16][DH], rows >= G zero.  Every wave then holds, per lane
//     (= head lane & 15), qsum_g = the fp32 sum of the rounded row over each 64-group: 16 elements in-lane, then xor 16 / xor 32.
//   * writer: the workgroup whose slice holds pos also finishes the new K and V row, rounds it to 16 bits and quantises it with kvq_group,
//     one full wave per 64-group (waves 0 .. 2 DH / 64 - 1).  It is the row's only writer; codes and pairs also go to LDS, and the new
//     row enters the scores and the output from there, as the values read back.
//   * scores.  The four waves own 64 keys each as four 16-key MFMA tiles with lm_step_attn_split's tile-to-key mapping (tile t, MFMA
//     row m = key 32 (t >> 1) + 8 (m >> 2) + 4 (t & 1) + (m & 3) of the wave), so the score accumulators of tiles (2 u, 2 u + 1) are,
//     register for register, keys 8 (lane >> 4) + 0..7 of k-step u: P^T of the V MFMA in natural key order.  A lane's 8 elements of a K
//     row are one code dword (4 bit) or two (8 bit), loaded cache -> registers and unpacked to the 16-bit numbers equal to the codes
//     (exact in bf16 and f16): the row-major A operand of S_g = Code_g Q_g^T, one accumulator per 64-group g of the head dim.  Then in
//     fp32  s[k][h] = sum_g scale_K[k][g] S_g[k][h] + bias_K[k][g] qsum_g[h].  Integer x 16-bit products are exact: only fp32 summation.
//   * softmax over the wave's 64 keys per head as in lm_step_attn_split (keys > pos at -inf, the wave-local maximum is exact, p <= 1).
//   * output.  O[h][d] = sum_k code_V[k][d] (p[k] scale_V[k][g(d)]) + sum_k p[k] bias_V[k][g(d)].  The first term is the V^T P^T MFMA:
//     the V codes are staged cache -> registers -> LDS, transposed, as 16-bit integers (lm_step_attn.hip's [DH][32 keys] tile and
//     swizzle; rows past pos are zeros); p scale_V 2^BITS gets its own P fragments per group and goes in as a hi + lo pair of 16-bit
//     numbers (lm_prefill_attn_kvq.hip's header says why one term is not enough on codes), small term first.  The second term is one
//     fp32 scalar per (head, group): in-lane over the lane's 16 keys in key order, then xor 16 / xor 32; it is added to the group's
//     channels when the wave partials are merged, after 2^-BITS has taken the factor out of the accumulator (exact).
//   * the waves' (m, l, acc, bias sums) are merged through LDS in wave order and the workgroup writes one fp32 partial (m, l, acc[DH])
//     per head to ws [seq][head][slice][DH + 2] -- lm_step_attn.hip's layout, so the second launch is its lm_step_attn_combine.
// No atomics, no workgroup waits on another, every sum runs in a fixed order, loads are clamped so that nothing at or past pos is read
// from the cache; pairs of keys past pos are replaced by zeros before they meet p = 0.
//
// f16 range.  p scale_V is below f16's normal range for small p, so P carries the factor 2^BITS as in the prompt kernel.  Here p <= 1
// (the maximum is the wave's own), so the packed value is at most 2^BITS / (2^BITS - 1) R with R = max - min of the key's V group: finite
// in f16 (65504) for R < 61 410 at 4 bits and R < 65 248 at 8 bits -- wider than any group whose scale R / (2^BITS - 1) and values are
// themselves finite f16 numbers needs in practice, and 2^8 times the prompt kernel's limit (239 / 254).  bf16 has no such limit.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; VGPRs / AGPRs / scratch bytes per lane / LDS bytes, no spills):
//   bf16 dh 64  q4  98 / 16 / 0 / 19 784      bf16 dh 128 q4 170 / 32 / 0 / 39 056      f16 dh 64  q4  96 / 16 / 0 / 19 784      f16 dh 128 q4 167 / 32 / 0 / 39 056
//   bf16 dh 64  q8 100 / 16 / 0 / 19 848      bf16 dh 128 q8 176 / 32 / 0 / 39 184      f16 dh 64  q8 101 / 16 / 0 / 19 848      f16 dh 128 q8 177 / 32 / 0 / 39 184
#include "lm.h"
#include "lm_kvq_device.h"
#include "mia_device.h"

namespace {

constexpr int SLICE = LM_STEP_SLICE;
constexpr int WAVE_KEYS = 64;
constexpr int PTERMS = 2;                         // 16-bit terms of p scale_V: hi + lo

template <typename T, int DH, int BITS>
__global__ __launch_bounds__(256) void lm_step_attn_kvq_split(LmStepAttnKvq a, float scale_log2) {
  constexpr int half = DH / 2;
  constexpr int KS = DH / 32;                     // k-steps of S = Code Q^T, two per 64-group
  constexpr int DB = DH / 16;                     // 16-channel blocks of O^T, four per 64-group
  constexpr int CH = DH / 8;                      // 8-element chunks per cache row
  constexpr int GPR = DH / 64;                    // 64-groups (pairs) per row
  constexpr int WPL = BITS / 4;                   // code dwords per chunk
  constexpr int WPR = DH * BITS / 32;             // code dwords per row
  constexpr int CPW = 32 / BITS;                  // codes per dword
  constexpr int VT_BYTES = DH * 64;               // one wave's V^T [DH][32 keys]; later its merge rows [16 heads][DH] fp32 -- the same size
  constexpr float PSCALE = (float)(1 << BITS);
  __shared__ __attribute__((aligned(16))) uint16_t q16[16 * DH];
  __shared__ float knf[DH];                       // the new K / V row, 16-bit rounded (writer)
  __shared__ float vnf[DH];
  __shared__ __attribute__((aligned(16))) uint32_t ncode[2][WPR];      // its codes and pairs, K | V
  __shared__ uint32_t npair[2][GPR];
  __shared__ __attribute__((aligned(16))) char stage[4 * VT_BYTES];
  __shared__ float ml[4][16][2];
  __shared__ float obl[4][16][GPR];

  const int seq = blockIdx.y, kvh = blockIdx.x, slice = blockIdx.z;
  const LmState* st = a.st + seq;
  if (st->frozen) return;                         // (uniform over the workgroup, like everything up to the first barrier)
  const int pos = st->pos;
  const int k0s = slice * SLICE;
  if (pos < 0 || pos >= a.max_ctx || k0s > pos) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int G = a.Hq / a.Hkv;
  const int Nq = a.Hq * DH, Nk = a.Hkv * DH, N = Nq + 2 * Nk;
  const bool writer = (pos >> 8) == slice;        // this slice holds the new row
  const int64_t r0 = ((int64_t)seq * a.Hkv + kvh) * a.max_ctx;      // first row of this sequence's K/V head
  uint32_t* Kc = a.kq + r0 * WPR;
  uint32_t* Vc = a.vq + r0 * WPR;
  uint32_t* Kp = a.kp + r0 * GPR;
  uint32_t* Vp = a.vp + r0 * GPR;

  // ---- preamble: lm_kvq_attention<FUSED>'s, for the G query heads of the group (and, in the writer, the new K / V row)
  auto val = [&](int n) {                         // S <= 4 slices [S][nb][N], loads issued together
    float pv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pv[k] = a.part[((int64_t)(k < a.S ? k : a.S - 1) * a.nb + seq) * N + n];
    float r = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < a.S) r += pv[k];
    return r;
  };
  // one rotation pair (i, i + half) of the row that starts at `base`, rounded to 16 bits
  auto rope_pair = [&](int base, int i, uint16_t& y0, uint16_t& y1) {
    const float x0 = val(base + i), x1 = val(base + i + half);
    float sn, cs;
    sincosf((float)pos * a.inv_freq[i], &sn, &cs);
    y0 = T::from_f32(x0 * cs - x1 * sn); y1 = T::from_f32(x1 * cs + x0 * sn);
  };
  for (int e = tid; e < G * half; e += 256) {
    const int hl = e / half, i = e - hl * half;
    uint16_t y0, y1;
    rope_pair((kvh * G + hl) * DH, i, y0, y1);
    q16[hl * DH + i] = y0; q16[hl * DH + i + half] = y1;
  }
  for (int e = G * DH + tid; e < 16 * DH; e += 256) q16[e] = 0;
  if (writer) {
    if (tid < half) {
      uint16_t y0, y1;
      rope_pair(Nq + kvh * DH, tid, y0, y1);
      knf[tid] = T::to_f32(y0); knf[tid + half] = T::to_f32(y1);
    } else if (tid >= 64 && tid - 64 < DH) {
      const int d = tid - 64;
      vnf[d] = T::to_f32(T::from_f32(val(Nq + Nk + kvh * DH + d)));
    }
  }
  __syncthreads();
  if (writer) {
    if (wave < 2 * GPR) {                         // (wave-uniform: the reductions inside need all 64 lanes)
      const int is_v = wave >= GPR ? 1 : 0;
      const int grp = is_v ? wave - GPR : wave, e = grp * 64 + lane;
      uint32_t word, pair;
      (void)kvq_group<T, BITS>((is_v ? vnf : knf)[e], lane, word, pair);
      if ((lane & (CPW - 1)) == 0) {
        ncode[is_v][e / CPW] = word;
        ((is_v ? Vc : Kc) + (int64_t)pos * WPR)[e / CPW] = word;
      }
      if (lane == 0) {
        npair[is_v][grp] = pair;
        ((is_v ? Vp : Kp) + (int64_t)pos * GPR)[grp] = pair;
      }
    }
    __syncthreads();                              // (writer is uniform over the workgroup)
  }

  const int g = lane >> 4, lr = lane & 15;
  const int k0w = k0s + WAVE_KEYS * wave;
  const bool live = k0w <= pos;                   // wave-uniform; the live waves are 0 .. n_live - 1
  const int last_cached = pos > 0 ? pos - 1 : 0;  // loads are clamped to it: nothing at or past pos (and so past max_ctx) is read from the cache

  f32x4 oacc[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) oacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float p[2][8];                                  // the lane's probabilities: keys 8 g + 0..7 of k-step u, head lr
  float vsc[2][8][GPR];                           // 2^BITS scale_V of those keys
  float ob[GPR];                                  // sum_k p[k] bias_V[k][group]
  float m2 = -INFINITY, lsum = 0.f;

  // V rows of k-step u: lane -> key pair lr and chunks c = g + 4 i
  uint32_t rv[CH / 4][2][WPL];
  auto load_v = [&](int u) {
#pragma unroll
    for (int i = 0; i < CH / 4; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = k0w + 32 * u + 2 * lr + e, c = g + 4 * i;
        load_codes<BITS>(Vc + (int64_t)min(key, last_cached) * WPR + c * WPL, rv[i][e]);
#pragma unroll
        for (int w = 0; w < WPL; ++w) {
          if (key == pos) rv[i][e][w] = ncode[1][c * WPL + w];
          if (key > pos) rv[i][e][w] = 0u;
        }
      }
  };
  char* vt = stage + wave * VT_BYTES;
  auto vswz = [](int d) { return ((d >> 2) ^ (d >> 4)) & 3; };
  auto stage_v = [&]() {
#pragma unroll
    for (int i = 0; i < CH / 4; ++i) {
      float x0[8], x1[8];
      codes8<BITS>(rv[i][0], x0);
      codes8<BITS>(rv[i][1], x1);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = 8 * (g + 4 * i) + j;
        *reinterpret_cast<uint32_t*>(vt + d * 64 + (((lr >> 2) ^ vswz(d)) << 4) + (lr & 3) * 4) = pack_codes<T>(x0[j], x1[j]);
      }
    }
  };
  // O^T += Code_V^T (P scale_V)^T of k-step u: per group its own P fragments, PTERMS 16-bit terms, on the group's four channel blocks
  auto pv_step = [&](int u) {
#pragma unroll
    for (int gr = 0; gr < GPR; ++gr) {
      float x[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = p[u][j] * vsc[u][j][gr];
      s16x8 pf[PTERMS];
#pragma unroll
      for (int term = 0; term < PTERMS; ++term) {
        u32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          w[j] = pack2<T>(x[2 * j], x[2 * j + 1]);
          x[2 * j] -= T::to_f32((uint16_t)(w[j] & 0xffffu)); x[2 * j + 1] -= T::to_f32((uint16_t)(w[j] >> 16));      // exact: the remainder
        }
        pf[term] = __builtin_bit_cast(s16x8, w);
      }
#pragma unroll
      for (int db = 4 * gr; db < 4 * gr + 4; ++db) {
        const int d = 16 * db + lr;
        const s16x8 vf = *reinterpret_cast<const s16x8*>(vt + d * 64 + ((g ^ vswz(d)) << 4));
#pragma unroll
        for (int term = PTERMS - 1; term >= 0; --term) oacc[db] = T::mfma16(vf, pf[term], oacc[db]);      // small terms first
      }
    }
  };

  if (live) {
    // the pairs of the lane's 16 accumulator keys: key k0w + 32 u + 8 g + j = score register [2 u + (j >> 2)][j & 3]
    uint32_t kpr[2][8][GPR], vpr[2][8][GPR];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int key = k0w + 32 * u + 8 * g + j;
        const int64_t row = (int64_t)min(key, last_cached) * GPR;
#pragma unroll
        for (int gr = 0; gr < GPR; ++gr) {
          kpr[u][j][gr] = Kp[row + gr]; vpr[u][j][gr] = Vp[row + gr];
          if (key == pos) { kpr[u][j][gr] = npair[0][gr]; vpr[u][j][gr] = npair[1][gr]; }
          if (key > pos) vpr[u][j][gr] = 0u;      // scale 0, bias 0: whatever the clamped row holds never meets p = 0
        }
      }
    // ---- q fragments (B operand: lane & 15 = head) and the head's sums per 64-group
    s16x8 qf[KS];
    float qsum[GPR];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) qf[kk] = *reinterpret_cast<const s16x8*>(q16 + lr * DH + 32 * kk + 8 * g);
#pragma unroll
    for (int gr = 0; gr < GPR; ++gr) {
      float t = 0.f;
#pragma unroll
      for (int kk = 2 * gr; kk < 2 * gr + 2; ++kk)
#pragma unroll
        for (int j = 0; j < 8; ++j) t += T::to_f32((uint16_t)qf[kk][j]);
      t += __shfl_xor(t, 16, 64);                 // (a + b on one side, b + a on the other: the same bits in all four lane groups)
      qsum[gr] = t + __shfl_xor(t, 32, 64);
    }
    load_v(0);
    // ---- S_g = Code_g Q_g^T per tile and group: MFMA row lr of tile t is key k0w + 32 (t >> 1) + 8 (lr >> 2) + 4 (t & 1) + (lr & 3)
    float sc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = k0w + 32 * (t >> 1) + 8 * (lr >> 2) + 4 * (t & 1) + (lr & 3);
      const uint32_t* kr = Kc + (int64_t)min(key, last_cached) * WPR + g * WPL;
      s16x8 kf[KS];
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        uint32_t w[WPL];
        load_codes<BITS>(kr + 4 * kk * WPL, w);
#pragma unroll
        for (int i = 0; i < WPL; ++i) if (key == pos) w[i] = ncode[0][(4 * kk + g) * WPL + i];
        kf[kk] = __builtin_bit_cast(s16x8, codes8_pack<T, BITS>(w));
      }
#pragma unroll
      for (int gr = 0; gr < GPR; ++gr) {
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 2 * gr; kk < 2 * gr + 2; ++kk) acc = T::mfma16(kf[kk], qf[kk], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t pr = kpr[t >> 1][4 * (t & 1) + r][gr];
          const float ksc = T::to_f32((uint16_t)(pr & 0xffffu)), kbi = T::to_f32((uint16_t)(pr >> 16));
          const float tb = kbi * qsum[gr];
          sc[t][r] = fmaf(ksc, acc[r], gr == 0 ? tb : sc[t][r] + tb);
        }
      }
    }
    // ---- softmax of head lr over the wave's 64 keys (raw scores; p = exp2((s - m) c), c = dh^-0.5 log2 e)
    float mraw = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (k0w + 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r > pos) sc[t][r] = -INFINITY;
        mraw = fmaxf(mraw, sc[t][r]);
      }
    mraw = fmaxf(mraw, __shfl_xor(mraw, 16, 64));
    mraw = fmaxf(mraw, __shfl_xor(mraw, 32, 64));    // finite: key k0w <= pos is in every head's row
#pragma unroll
    for (int gr = 0; gr < GPR; ++gr) ob[gr] = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[u][j] = __builtin_amdgcn_exp2f((sc[2 * u + (j >> 2)][j & 3] - mraw) * scale_log2);
        lsum += p[u][j];
#pragma unroll
        for (int gr = 0; gr < GPR; ++gr) {
          const uint32_t pr = vpr[u][j][gr];
          vsc[u][j][gr] = T::to_f32((uint16_t)(pr & 0xffffu)) * PSCALE;      // (a power of two: exact)
          ob[gr] = fmaf(p[u][j], T::to_f32((uint16_t)(pr >> 16)), ob[gr]);
        }
      }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
#pragma unroll
    for (int gr = 0; gr < GPR; ++gr) {
      ob[gr] += __shfl_xor(ob[gr], 16, 64);
      ob[gr] += __shfl_xor(ob[gr], 32, 64);
    }
    m2 = mraw * scale_log2;
    stage_v();
  }
  __syncthreads();
  if (live) { load_v(1); pv_step(0); }
  __syncthreads();
  if (live) stage_v();
  __syncthreads();
  if (live) pv_step(1);
  __syncthreads();

  // ---- merge the live waves in wave order: lane holds O^T[d = 16 db + 4 g + r][head lr]
  if (live && lr < G) {
    float* red = reinterpret_cast<float*>(stage + wave * VT_BYTES);      // [16 heads][DH]
#pragma unroll
    for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4*>(red + lr * DH + 16 * db + 4 * g) = oacc[db];
    if (g == 0) {
      ml[wave][lr][0] = m2; ml[wave][lr][1] = lsum;
#pragma unroll
      for (int gr = 0; gr < GPR; ++gr) obl[wave][lr][gr] = ob[gr];
    }
  }
  __syncthreads();
  const int n_live = min(4, ((pos - k0s) >> 6) + 1);
  const int n_slices = (a.max_ctx + SLICE - 1) / SLICE;
  for (int e = tid; e < G * DH; e += 256) {
    const int hl = e / DH, d = e - hl * DH;
    float m = ml[0][hl][0];
    for (int w = 1; w < n_live; ++w) m = fmaxf(m, ml[w][hl][0]);
    float l = 0.f, o = 0.f;
    for (int w = 0; w < n_live; ++w) {
      const float f = __builtin_amdgcn_exp2f(ml[w][hl][0] - m);
      l += ml[w][hl][1] * f;
      o += (reinterpret_cast<const float*>(stage + w * VT_BYTES)[hl * DH + d] * (1.0f / PSCALE) + obl[w][hl][d >> 6]) * f;
    }
    float* dst = a.ws + (((int64_t)seq * a.Hq + kvh * G + hl) * n_slices + slice) * (DH + 2);
    if (d == 0) { dst[0] = m; dst[1] = l; }
    dst[2 + d] = o;
  }
}

}  // namespace

const char* lm_step_attn_kvq_check(int Hq, int Hkv, int dh, int bits) {
  if (bits != 4 && bits != 8) return "bits must be 4 or 8";
  return lm_step_attn_check(Hq, Hkv, dh);
}

int lm_step_attn_kvq_launch(const LmStepAttnKvq& a, hipStream_t s) {
  if (lm_step_attn_kvq_check(a.Hq, a.Hkv, a.dh, a.bits) || !a.kq || !a.vq || !a.kp || !a.vp || !a.out || !a.ws || !a.st || !a.part || !a.inv_freq || a.S < 1 || a.S > 4 ||
      a.nb <= 0 || a.max_ctx <= 0)
    return -1;
  const dim3 grid(a.Hkv, a.nb, lm_step_attn_slices(a.max_ctx));
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)a.dh);
#define SQ_GO(TT, DD, BB) hipLaunchKernelGGL((lm_step_attn_kvq_split<TT, DD, BB>), grid, dim3(256), 0, s, a, scale_log2)
#define SQ_B(TT, DD) do { if (a.bits == 4) SQ_GO(TT, DD, 4); else SQ_GO(TT, DD, 8); } while (0)
  if (a.dtype == MIA_F16) { if (a.dh == 128) SQ_B(F16, 128); else SQ_B(F16, 64); }
  else                    { if (a.dh == 128) SQ_B(BF16, 128); else SQ_B(BF16, 64); }
#undef SQ_B
#undef SQ_GO
  if (hipGetLastError() != hipSuccess) return -1;
  LmStepAttn c;                                   // the merge over the slices reads (st, ws) and writes out: lm_step_attn.hip's
  c.out = a.out; c.ws = a.ws; c.st = a.st; c.nb = a.nb; c.Hq = a.Hq; c.Hkv = a.Hkv; c.dh = a.dh; c.max_ctx = a.max_ctx; c.dtype = a.dtype;
  return lm_step_attn_combine_launch(c, s);
}
