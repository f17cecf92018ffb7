// lm_kvq.hip -- the LM's quantised KV cache on gfx950: QuantizedKVCache(groupSize: 64, bits: 4 | 8) of the reference
// (TTS/Orpheus/BuildingBlocks/TransformerBlock.swift:182-201, routed through attentionWithCacheUpdate at :91-99).
//
// The rule, restated from MLX's public documentation (mx.quantize, mode "affine"; PARITY UNPINNED against MLX, which is not in the
// tree).  Every K row (after RoPE) and V row is first rounded to the handle's 16-bit type exactly as the 16-bit cache does, then per
// group of 64 consecutive elements of the head dimension:
//   lo, hi = min, max;  n = 2^bits - 1;  scale = (hi - lo) / n in fp32 (1 when hi == lo);  bias = lo;
//   scale and bias are rounded to the 16-bit type (RNE: MLX stores them in the input's dtype);
//   code = clamp(rintf((x - bias) / scale), 0, n) with the ROUNDED pair: one fp32 subtract, one IEEE divide, rintf.  No reciprocal, no
//   fast divide: the build has no fast-math and -ffp-contract=off, and this file relies on both.  A scale that rounds to zero makes
//   the quotient +inf (code n) or NaN (code 0, through fmaxf); either way the value read back is `bias`.
//   value read back = scale * code + bias in fp32, a multiply then an add.
// MLX also nudges scale / bias so that zero is exactly representable; that detail is NOT reproduced (as in oracle/quant.py).
// Attention in this mode sees only values read back from the codes, the row of the token being processed included (MLX quantises the
// new keys / values before it attends, in the prompt pass and in the step alike).  The dot products run over de-quantised values
// (not MLX's packed form scale * sum(code * x) + bias * sum(x)): the same function up to fp32 summation order, and it keeps the
// error next to a large bias what it is in the 16-bit kernel.
//
// Layout (per layer, per sequence; DESIGN.md "HBM data layout"): codes [Hkv][max_ctx][dh * bits / 32] uint32, little end first (the
// packing of oracle/quant.py); pairs [Hkv][max_ctx][dh / 64] uint32 = scale (low half) | bias (high half).  With the 16-bit kernel's
// lane split -- dh / 8 lanes per key, 8 elements per lane -- a lane's share of a row is one dword at 4 bits, two at 8 bits, and 8
// lanes share one pair.  Bytes per cached row: dh * bits / 8 + dh / 16 against 2 * dh.
//
// Kernels: lm_kvq_rope_cache (prompt pass: lm_rope_cache's sum + bias + RoPE + 16-bit rounding, then quantise and store) and
// lm_kvq_attention (lm_attention's structure; FUSED = the decode step, which quantises its new row in LDS).  Grid: one workgroup per
// (query head, row), as lm_attention; the query heads of a GQA group each read their K/V head's rows (no shared read).
#include <cmath>
#include <type_traits>

#include "lm.h"
#include "mia_device.h"

namespace {

constexpr int KVQ_NW = 16;     // waves per attention workgroup (lm.hip: ATT_NW, same reasoning)

// One group of 64 values, one per lane of a full wave: returns the value read back; `word` = the code dword this lane's 32 / BITS
// neighbours share (identical in all of them), `pair` = scale | bias << 16.
template <typename T, int BITS>
__device__ __forceinline__ float kvq_group(float x, int lane, uint32_t& word, uint32_t& pair) {
  constexpr float n = (float)((1 << BITS) - 1);
  const float hi = wave_max(x), lo = -wave_max(-x);
  const float sc = hi == lo ? 1.0f : (hi - lo) / n;
  const uint16_t s16 = T::from_f32(sc), b16 = T::from_f32(lo);
  const float s = T::to_f32(s16), b = T::to_f32(b16);
  const float code = fminf(fmaxf(rintf((x - b) / s), 0.0f), n);
  int w = (int)code << (BITS * (lane & (32 / BITS - 1)));
  w |= dpp_i32<0xB1>(w);                        // lanes xor 1, xor 2: the quad's codes
  w |= dpp_i32<0x4E>(w);
  if (BITS == 4) w |= dpp_i32<0x141>(w);        // half-row mirror: the other quad of the 8 lanes
  word = (uint32_t)w;
  pair = (uint32_t)s16 | ((uint32_t)b16 << 16);
  return s * code + b;
}

// a lane's 8 consecutive elements of one cached row
template <typename T, int BITS>
__device__ __forceinline__ void kvq_dq8(const uint32_t (&w)[BITS / 4], uint32_t pair, float (&x)[8]) {
  const float s = T::to_f32((uint16_t)(pair & 0xffffu)), b = T::to_f32((uint16_t)(pair >> 16));
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t code = BITS == 4 ? (w[0] >> (4 * j)) & 15u : (w[j >> 2] >> (8 * (j & 3))) & 255u;
    x[j] = s * (float)code + b;
  }
}

template <int BITS>
__device__ __forceinline__ void kvq_load(const uint32_t* __restrict__ row, int c, uint32_t (&w)[BITS / 4]) {
  if constexpr (BITS == 4) w[0] = row[c];
  else { const u32x2 v = *reinterpret_cast<const u32x2*>(row + 2 * c); w[0] = v[0]; w[1] = v[1]; }
}

// q|k|v = sum_s partial[s] + bias; RoPE on q and k (lm_rope_cache's expressions); q -> qout; the K / V head's row -> 16 bit -> codes and
// pairs at cache[kv head][pos].  One workgroup of DH threads per (head slot, row): slots [0, Hq) query heads, [Hq, Hq + Hkv) key
// heads, then value heads; wave g of the workgroup owns group g of the row.
template <typename T, int DH, int BITS>
__global__ __launch_bounds__(DH) void lm_kvq_rope_cache(const float* __restrict__ part, int S, const float* __restrict__ bias, const float* __restrict__ inv_freq,
                                                        uint16_t* __restrict__ qout, uint32_t* __restrict__ kq, uint32_t* __restrict__ vq,
                                                        uint32_t* __restrict__ kp, uint32_t* __restrict__ vp, const int2* __restrict__ rowmap,
                                                        int Hq, int Hkv, int max_ctx) {
  __shared__ float row[DH];
  constexpr int half = DH / 2, WPR = DH * BITS / 32, GPR = DH / 64, CPW = 32 / BITS;
  const int Nq = Hq * DH, Nk = Hkv * DH, N = Nq + 2 * Nk;
  const int seq = rowmap[blockIdx.y].x, pos = rowmap[blockIdx.y].y;
  part += (int64_t)blockIdx.y * N; qout += (int64_t)blockIdx.y * Nq;
  const int slot = blockIdx.x, tid = threadIdx.x;
  auto val = [&](int n) {        // S <= 4 slices, loads issued together (see lm_reduce_norm)
    float p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = part[(int64_t)(k < S ? k : S - 1) * N + n];
    float a = bias ? bias[n] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < S) a += p[k];
    return a;
  };
  const bool is_v = slot >= Hq + Hkv;
  if (!is_v) {
    if (tid < half) {
      const int i = tid, base = slot * DH;                  // q and k sections are contiguous: [q heads | k heads]
      const float x0 = val(base + i), x1 = val(base + i + half);
      float sn, cs;
      sincosf((float)pos * inv_freq[i], &sn, &cs);
      const float y0 = x0 * cs - x1 * sn, y1 = x1 * cs + x0 * sn;
      if (slot < Hq) { qout[base + i] = T::from_f32(y0); qout[base + i + half] = T::from_f32(y1); }
      else { row[i] = T::to_f32(T::from_f32(y0)); row[i + half] = T::to_f32(T::from_f32(y1)); }
    }
    if (slot < Hq) return;                                  // (the whole workgroup)
  } else row[tid] = T::to_f32(T::from_f32(val(Nq + Nk + (slot - Hq - Hkv) * DH + tid)));
  __syncthreads();
  const int head = is_v ? slot - Hq - Hkv : slot - Hq;
  const int64_t r = ((int64_t)seq * Hkv + head) * max_ctx + pos;      // row of this sequence's cache
  uint32_t word, pair;
  (void)kvq_group<T, BITS>(row[tid], tid & 63, word, pair);
  uint32_t* codes = (is_v ? vq : kq) + r * WPR;
  uint32_t* pairs = (is_v ? vp : kp) + r * GPR;
  if ((tid & (CPW - 1)) == 0) codes[tid / CPW] = word;
  if ((tid & 63) == 0) pairs[tid >> 6] = pair;
}

// lm_attention over the packed cache.  Same workgroup / lane split, key loop, softmax and output reduction; a cached row is read as
// the lane's code dword(s) plus its group's pair and de-quantised in registers.  FUSED (the decode step): after the workgroup has
// finished its q head and its K/V head's new row (16-bit rounded, in LDS), waves 0 .. 2 * DH / 64 - 1 quantise one group each in
// place -- every workgroup of a GQA group derives the identical codes, the first query head's stores them -- and the new row enters
// the scores and the output as the values read back.  Not FUSED (prompt pass): keys [0, pos] all come from the cache, the row's own
// (written by lm_kvq_rope_cache) included.
template <typename T, int DH, int BITS, bool FUSED>
__global__ __launch_bounds__(64 * KVQ_NW) void lm_kvq_attention(const uint16_t* __restrict__ q, uint32_t* __restrict__ kq, uint32_t* __restrict__ vq,
                                                                uint32_t* __restrict__ kp, uint32_t* __restrict__ vp, uint16_t* __restrict__ out,
                                                                const LmState* __restrict__ st, int Hq, int Hkv, int max_ctx, float scale,
                                                                const float* __restrict__ part, int S, const float* __restrict__ bias,
                                                                const float* __restrict__ inv_freq, int B, const int2* __restrict__ rowmap) {
  extern __shared__ float sc[];            // [max_ctx] scores, then red[KVQ_NW][DH] + red2[2 * KVQ_NW] + q, k, v rows [3][DH] (FUSED)
  constexpr int LPK = DH / 8;              // lanes per key
  constexpr int KPW = 64 / LPK;            // keys per wave instruction
  constexpr int WPR = DH * BITS / 32, GPR = DH / 64, CPW = 32 / BITS, WPL = BITS / 4;
  const int seq = FUSED ? (int)blockIdx.y : rowmap[blockIdx.y].x;
  st += seq;
  float* red = sc + max_ctx;
  float* red2 = red + KVQ_NW * DH;
  float* qs = red2 + 2 * KVQ_NW;           // FUSED only
  float* kn = qs + DH;
  float* vn = kn + DH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, kvh = h / (Hq / Hkv);
  const int nk = (FUSED ? st->pos : rowmap[blockIdx.y].y) + 1;
  const int nkc = FUSED ? nk - 1 : nk;     // keys read from the cache
  q += (int64_t)blockIdx.y * Hq * DH; out += (int64_t)blockIdx.y * Hq * DH;
  const int c = lane % LPK, g = lane / LPK;
  const int64_t r0 = ((int64_t)seq * Hkv + kvh) * max_ctx;      // first row of this sequence's K/V head
  const uint32_t* kcb = kq + r0 * WPR;
  const uint32_t* vcb = vq + r0 * WPR;
  const uint32_t* kpb = kp + r0 * GPR + c / 8;                  // the lane's group
  const uint32_t* vpb = vp + r0 * GPR + c / 8;
  if (FUSED) {
    constexpr int half = DH / 2;
    const int Nq = Hq * DH, Nk = Hkv * DH, N = Nq + 2 * Nk, pos = nk - 1;
    const bool writer = h % (Hq / Hkv) == 0;
    auto val = [&](int n) {                // S <= 4 slices, loads issued together
      float pv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) pv[k] = part[((int64_t)(k < S ? k : S - 1) * B + blockIdx.y) * N + n];   // slices [S][B][N]
      float a = bias ? bias[n] : 0.f;
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < S) a += pv[k];
      return a;
    };
    if (tid < DH) {                        // rotation pairs (i, i + half): the q head, then the k head
      const bool is_k = tid >= half;
      const int i = is_k ? tid - half : tid;
      const int base = is_k ? Nq + kvh * DH : h * DH;
      const float x0 = val(base + i), x1 = val(base + i + half);
      float sn, cs;
      sincosf((float)pos * inv_freq[i], &sn, &cs);
      const uint16_t a0 = T::from_f32(x0 * cs - x1 * sn), a1 = T::from_f32(x1 * cs + x0 * sn);
      float* dst = is_k ? kn : qs;
      dst[i] = T::to_f32(a0); dst[i + half] = T::to_f32(a1);
    } else if (tid < 2 * DH) {
      const int d = tid - DH;
      vn[d] = T::to_f32(T::from_f32(val(Nq + Nk + kvh * DH + d)));
    }
    __syncthreads();
    if (wave < 2 * GPR) {                  // (wave-uniform: the reductions inside need all 64 lanes)
      const bool is_v = wave >= GPR;
      const int grp = is_v ? wave - GPR : wave, e = grp * 64 + lane;
      float* rowp = is_v ? vn : kn;
      uint32_t word, pair;
      rowp[e] = kvq_group<T, BITS>(rowp[e], lane, word, pair);
      if (writer) {
        const int64_t r = r0 + pos;
        if ((lane & (CPW - 1)) == 0) ((is_v ? vq : kq) + r * WPR)[e / CPW] = word;
        if (lane == 0) ((is_v ? vp : kp) + r * GPR)[grp] = pair;
      }
    }
    __syncthreads();
  }
  float qf[8];
  if (FUSED) {
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = qs[c * 8 + j];
  } else {
    const s16x8 qv = *reinterpret_cast<const s16x8*>(q + h * DH + c * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = T::to_f32((uint16_t)qv[j]);
  }
  for (int k0 = wave * KPW * 4; k0 < nkc; k0 += KVQ_NW * KPW * 4) {
    uint32_t kw[4][WPL], pr[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      int key = k0 + KPW * u + g; key = key < nkc ? key : nkc - 1;
      kvq_load<BITS>(kcb + (int64_t)key * WPR, c, kw[u]);
      pr[u] = kpb[(int64_t)key * GPR];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float x[8];
      kvq_dq8<T, BITS>(kw[u], pr[u], x);
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) dot += qf[j] * x[j];
#pragma unroll
      for (int o = 1; o < LPK; o <<= 1) dot += __shfl_xor(dot, o, 64);
      const int key = k0 + KPW * u + g;
      if (c == 0 && key < nkc) sc[key] = dot * scale;
    }
  }
  if (FUSED && wave == 0) {                // the new key, from LDS (same lane split and summation order as a cached key)
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) dot += qf[j] * kn[c * 8 + j];
#pragma unroll
    for (int o = 1; o < LPK; o <<= 1) dot += __shfl_xor(dot, o, 64);
    if (lane == 0) sc[nk - 1] = dot * scale;
  }
  __syncthreads();
  float m = -INFINITY;
  for (int i = tid; i < nk; i += 64 * KVQ_NW) m = fmaxf(m, sc[i]);
  m = wave_max(m);
  if (lane == 0) red2[wave] = m;
  __syncthreads();
  m = red2[0];
#pragma unroll
  for (int i = 1; i < KVQ_NW; ++i) m = fmaxf(m, red2[i]);
  float sum = 0.f;
  for (int i = tid; i < nk; i += 64 * KVQ_NW) { const float p = __expf(sc[i] - m); sc[i] = p; sum += p; }
  sum = wave_sum(sum);
  if (lane == 0) red2[KVQ_NW + wave] = sum;
  __syncthreads();
  sum = 0.f;
#pragma unroll
  for (int i = 0; i < KVQ_NW; ++i) sum += red2[KVQ_NW + i];
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int k0 = wave * KPW * 4; k0 < nkc; k0 += KVQ_NW * KPW * 4) {
    uint32_t vw[4][WPL], pr[4]; float pw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = k0 + KPW * u + g; const int k2 = key < nkc ? key : nkc - 1;
      kvq_load<BITS>(vcb + (int64_t)k2 * WPR, c, vw[u]);
      pr[u] = vpb[(int64_t)k2 * GPR];
      pw[u] = key < nkc ? sc[k2] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float x[8];
      kvq_dq8<T, BITS>(vw[u], pr[u], x);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += pw[u] * x[j];
    }
  }
  if (FUSED && wave == 0 && g == 0) {      // the new row's contribution
    const float pw = sc[nk - 1];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += pw * vn[c * 8 + j];
  }
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1) acc[j] += __shfl_xor(acc[j], o, 64);
  if (g == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave * DH + c * 8 + j] = acc[j];
  }
  __syncthreads();
  if (tid < DH) {
    float o = 0.f;
#pragma unroll
    for (int i = 0; i < KVQ_NW; ++i) o += red[i * DH + tid];
    out[h * DH + tid] = T::from_f32(o / sum);
  }
}

template <typename T, int DH, int BITS>
void kvq_rope_go(hipStream_t s, const LmKvq& a, const float* part, const float* bias, uint16_t* qout, const int2* rowmap, int M) {
  hipLaunchKernelGGL((lm_kvq_rope_cache<T, DH, BITS>), dim3(a.Hq + 2 * a.Hkv, M), dim3(DH), 0, s, part, 1, bias, a.inv_freq, qout, a.kq, a.vq, a.kp, a.vp, rowmap,
                     a.Hq, a.Hkv, a.max_ctx);
}

template <typename T, int DH, int BITS>
void kvq_att_go(hipStream_t s, const LmKvq& a, bool fused, int rows, const uint16_t* q, uint16_t* out, const int2* rowmap, const float* part, int S, const float* bias) {
  const size_t lds = (size_t)(a.max_ctx + KVQ_NW * DH + 2 * KVQ_NW + 3 * DH) * 4;
  const float scale = 1.0f / sqrtf((float)DH);
  const dim3 grid(a.Hq, rows), block(64 * KVQ_NW);
  if (fused) hipLaunchKernelGGL((lm_kvq_attention<T, DH, BITS, true>), grid, block, lds, s, q, a.kq, a.vq, a.kp, a.vp, out, a.st, a.Hq, a.Hkv, a.max_ctx, scale, part, S, bias, a.inv_freq, rows, rowmap);
  else hipLaunchKernelGGL((lm_kvq_attention<T, DH, BITS, false>), grid, block, lds, s, q, a.kq, a.vq, a.kp, a.vp, out, a.st, a.Hq, a.Hkv, a.max_ctx, scale, part, S, bias, a.inv_freq, rows, rowmap);
}

// one dispatch over (dtype, head_dim, bits) for both kernels
template <typename F>
void kvq_dispatch(const LmKvq& a, F&& f) {
#define KVQ_CASE(TT, DD, BB) f((TT*)nullptr, std::integral_constant<int, DD>(), std::integral_constant<int, BB>())
  const bool f16 = a.dtype == MIA_F16;
  if (a.dh == 128) { if (a.bits == 4) { if (f16) KVQ_CASE(F16, 128, 4); else KVQ_CASE(BF16, 128, 4); } else { if (f16) KVQ_CASE(F16, 128, 8); else KVQ_CASE(BF16, 128, 8); } }
  else             { if (a.bits == 4) { if (f16) KVQ_CASE(F16, 64, 4); else KVQ_CASE(BF16, 64, 4); } else { if (f16) KVQ_CASE(F16, 64, 8); else KVQ_CASE(BF16, 64, 8); } }
#undef KVQ_CASE
}

}  // namespace

const char* lm_kvq_check(int bits, int group_size, int head_dim, int* code) {
  if (bits != 0 && bits != 4 && bits != 8) { *code = MIA_ERR_INVALID_ARGUMENT; return "kv quantisation: bits must be 0 (16-bit cache), 4 or 8"; }
  if (bits != 0 && group_size != 64) { *code = MIA_ERR_UNSUPPORTED; return "kv quantisation: group_size must be 64"; }
  if (head_dim != 64 && head_dim != 128) { *code = MIA_ERR_UNSUPPORTED; return "kv quantisation: head_dim must be 64 or 128"; }
  return nullptr;
}

void lm_kvq_launch_rope_cache(hipStream_t s, const LmKvq& a, const float* part, const float* bias, uint16_t* qout, const int2* rowmap, int M) {
  kvq_dispatch(a, [&](auto* t, auto dh, auto bits) { kvq_rope_go<std::remove_pointer_t<decltype(t)>, decltype(dh)::value, decltype(bits)::value>(s, a, part, bias, qout, rowmap, M); });
}

void lm_kvq_launch_attention(hipStream_t s, const LmKvq& a, bool fused, int rows, const uint16_t* q, uint16_t* out, const int2* rowmap, const float* part, int S,
                             const float* bias) {
  kvq_dispatch(a, [&](auto* t, auto dh, auto bits) { kvq_att_go<std::remove_pointer_t<decltype(t)>, decltype(dh)::value, decltype(bits)::value>(s, a, fused, rows, q, out, rowmap, part, S, bias); });
}

void lm_kvq_read_rows(const uint32_t* codes, const uint32_t* pairs, int64_t n_rows, int dh, int bits, int dtype, float* out) {
  const int wpr = dh * bits / 32, gpr = dh / 64, cpw = 32 / bits;
  auto w16 = [&](uint16_t v) -> float {
    if (dtype == MIA_F16) { _Float16 hh; memcpy(&hh, &v, 2); return (float)hh; }
    const uint32_t u = (uint32_t)v << 16; float f; memcpy(&f, &u, 4); return f;
  };
  for (int64_t r = 0; r < n_rows; ++r)
    for (int d = 0; d < dh; ++d) {
      const uint32_t pr = pairs[r * gpr + d / 64];
      const float sc = w16((uint16_t)(pr & 0xffffu)), b = w16((uint16_t)(pr >> 16));
      const uint32_t code = (codes[r * wpr + d / cpw] >> ((d % cpw) * bits)) & ((1u << bits) - 1u);
      const float v = sc * (float)code;
      out[r * dh + d] = v + b;
    }
}
