// lm.hip -- autoregressive Llama-3 / Qwen2 style language-model decode on gfx950 (§8 a10-a12, a18).
//
// Replaces, per token, OrpheusModel / OrpheusLMHeadModel (TTS/Orpheus/BuildingBlocks/TransformerBlock.swift:70-105,129-139,
// 165-180,223-233), Llama3RoPE (TTS/Shared/Llama3RoPE.swift:27-66,104-114), SwiGLUMLP (TTS/Shared/SwiGLUMLP.swift:27-29),
// Qwen2Attention / Qwen2 blocks (TTS/CosyVoice2/LLM/Qwen2LM.swift:48-151), Qwen3Attention with its per-head q / k RMSNorm
// (STT/FunASR/Layers/Qwen3Model.swift:72-109); the samplers that end a step are lm_sample_*.hip.
//
// Decode at batch 1 is HBM-bound on the weights (Orpheus-3B: 6.6 GB bf16 per token).  Every projection is the skinny
// MFMA GEMM of skinny_rowmajor.hip (weights HBM -> VGPR once, split-K partials summed in a fixed order by the consumer
// kernel); RMSNorm / RoPE / KV-cache write / GQA attention / SwiGLU / sampling are fused around it; one hipGraph per token.
// The prompt is consumed one position per step through the same graph (identical maths to a causal prefill).
// This file: the step's row kernels next to their launch sites, the batched prompt pass, the step graph and the entry points; the
// loader and the packed-weight attach are lm_load.hip, the prompt pass's optional tiled attention is lm_prefill_attn.hip
// (mia_lm_set_prompt_attention), and lm.h is what the sources share.
#include <algorithm>
#include <cmath>
#include <vector>

#include "gemm.h"
#include "lm.h"
#include "mia_device.h"
#include "ops.h"
#include "skinny.h"

namespace {

constexpr int LM_NV = 4;   // float4 per thread of the 256-thread row kernels: hidden <= 4096

template <typename T>
__device__ __forceinline__ void rms_store(const f32x4 (&v)[LM_NV], int nv, int D, float eps, const float* __restrict__ w, uint16_t* __restrict__ h, float* sh) {
  const int tid = threadIdx.x;
  // the norm weights do not depend on the reduction: fetch them before it, so their L2 round trip overlaps the two barriers
  f32x4 g[LM_NV];
#pragma unroll
  for (int i = 0; i < LM_NV; ++i) g[i] = tid + 256 * i < nv ? *reinterpret_cast<const f32x4*>(w + 4 * (tid + 256 * i)) : (f32x4){0.f, 0.f, 0.f, 0.f};
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LM_NV; ++i) if (tid + 256 * i < nv) q += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
  const float rstd = rsqrtf(block256_sum(q, sh) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < LM_NV; ++i) {
    const int c = tid + 256 * i;
    if (c >= nv) continue;
    *reinterpret_cast<u32x2*>(h + 4 * c) = (u32x2){pack2<T>(v[i][0] * rstd * g[i][0], v[i][1] * rstd * g[i][1]), pack2<T>(v[i][2] * rstd * g[i][2], v[i][3] * rstd * g[i][3])};
  }
}

// x = E[token[pos]] (or a caller-provided embedding row);  h = RMSNorm(x) * w
// One workgroup per row.  Step graph (rowmap == nullptr): row b is SEQUENCE b at its own st[b].pos (tokens / embedding rows / state strided
// per sequence); batched prompt pass: row r is position rowmap[r].y of sequence rowmap[r].x -- rows of several prompts share a pass.
template <typename T>
__global__ __launch_bounds__(256) void lm_embed_norm(const int32_t* __restrict__ tokens, const uint16_t* __restrict__ emb, const uint16_t* __restrict__ gen_emb,
                                                     const float* __restrict__ embeds, const float* __restrict__ w,
                                                     float* __restrict__ x, uint16_t* __restrict__ h, const LmState* __restrict__ st, int D, float eps,
                                                     const int2* __restrict__ rowmap, int max_ctx, int emb_rows, int gen_rows) {
  __shared__ float sh[4];
  const int tid = threadIdx.x, nv = D >> 2;
  const int seq = rowmap ? rowmap[blockIdx.x].x : (int)blockIdx.x;         // prompt pass: row -> (sequence, position)
  st += seq; tokens += (int64_t)seq * max_ctx; embeds += (int64_t)seq * max_ctx * D;
  if (!rowmap && st->frozen) return;                       // (the same for every thread of the workgroup)
  const int pos = rowmap ? rowmap[blockIdx.x].y : st->pos;
  x += (int64_t)blockIdx.x * D; h += (int64_t)blockIdx.x * D;
  const bool from_rows = pos < st->n_embeds;               // prompt given as embedding rows
  const bool use_gen = st->n_embeds > 0 && gen_emb;
  int tok = from_rows ? 0 : tokens[pos];
  const int rows = use_gen ? gen_rows : emb_rows;
  tok = tok < 0 ? 0 : (tok < rows ? tok : rows - 1);       // an id outside the table (a corrupted sampler output) must never become a wild address
  const uint16_t* e = (use_gen ? gen_emb : emb) + (int64_t)tok * D;
  const float* er = embeds + (int64_t)pos * D;
  f32x4 v[LM_NV];
#pragma unroll
  for (int i = 0; i < LM_NV; ++i) {
    const int c = tid + 256 * i;
    if (c < nv) {
      if (from_rows) v[i] = *reinterpret_cast<const f32x4*>(er + 4 * c);
      else {
        const s16x4 ev = *reinterpret_cast<const s16x4*>(e + 4 * c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[i][j] = T::to_f32((uint16_t)ev[j]);
      }
      *reinterpret_cast<f32x4*>(x + 4 * c) = v[i];
    } else v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  rms_store<T>(v, nv, D, eps, w, h, sh);
}

// x += sum_s partial[s];  h = RMSNorm(x) * w        (one workgroup per row; the batched prompt pass runs it with S = 0)
template <typename T>
__global__ __launch_bounds__(256) void lm_reduce_norm(const float* __restrict__ partial, int S, const float* __restrict__ w, float* __restrict__ x,
                                                      uint16_t* __restrict__ h, int D, float eps, int B) {
  __shared__ float sh[4];
  const int tid = threadIdx.x, nv = D >> 2;
  x += (int64_t)blockIdx.x * D; h += (int64_t)blockIdx.x * D;
  f32x4 v[LM_NV];
#pragma unroll
  for (int i = 0; i < LM_NV; ++i) {
    const int c = tid + 256 * i;
    if (c < nv) {
      f32x4 a = *reinterpret_cast<const f32x4*>(x + 4 * c);
      // the slices were written by other XCDs (L2 misses): issue all loads before the first add.  S <= 8; slot k >= S re-reads
      // slice S-1 and is discarded, so the loads are unconditional and the sum keeps its fixed order.
      f32x4 p[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)                        // slices are [S][B][D]: row blockIdx.x of each
        p[k] = S > 0 ? *reinterpret_cast<const f32x4*>(partial + ((int64_t)(k < S ? k : S - 1) * B + blockIdx.x) * D + 4 * c) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (k < S) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += p[k][j];
        }
      v[i] = a;
      *reinterpret_cast<f32x4*>(x + 4 * c) = a;
    } else v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  rms_store<T>(v, nv, D, eps, w, h, sh);
}

// q|k|v = sum_s partial[s] + bias; RoPE (split-half pairs (i, i+dh/2), angle = pos * inv_freq[i]) on q and k; q -> qout,
// k, v -> cache[kv head][pos][:]          one thread per rotation pair / per v element; blockIdx.y = row of the batched prompt pass
// QKN (Qwen3Attention, STT/FunASR/Layers/Qwen3Model.swift:88-95): every q and k head goes through an RMSNorm over head_dim between the
// sum (+ bias) and the rotation, y = x * rsqrt(mean(x^2) + eps) * w with qkn = [q_norm | k_norm] gains [2][dh]; all fp32, the one 16-bit
// rounding stays where it is.  A head's dh/2 pairs are dh/2 consecutive threads, each holding both halves of its pair, and the segments
// are aligned to dh/2 (32 | 64) inside the 256-thread block, so the sum of squares is an xor-shuffle over those lanes: n_pairs is a
// multiple of dh/2, a segment never mixes with the V lanes of its wave, and every lane of the wave runs the shuffles.
template <typename T, bool QKN>
__global__ __launch_bounds__(256) void lm_rope_cache(const float* __restrict__ part, int S, const float* __restrict__ bias, const float* __restrict__ inv_freq,
                                                     uint16_t* __restrict__ qout, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                                                     const int2* __restrict__ rowmap, int Hq, int Hkv, int dh, int max_ctx, int64_t seq_stride,
                                                     const float* __restrict__ qkn, float qk_eps) {
  const int Nq = Hq * dh, Nk = Hkv * dh, N = Nq + 2 * Nk;
  const int half = dh >> 1;
  const int pos = rowmap[blockIdx.y].y;
  kc += (int64_t)rowmap[blockIdx.y].x * seq_stride; vc += (int64_t)rowmap[blockIdx.y].x * seq_stride;
  part += (int64_t)blockIdx.y * N; qout += (int64_t)blockIdx.y * Nq;      // prompt pass: S == 1, one GEMM output row per position
  const int n_pairs = (Hq + Hkv) * half;
  const int e = blockIdx.x * 256 + threadIdx.x;
  auto val = [&](int n) {        // S <= 4 slices, loads issued together (see lm_reduce_norm)
    float p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = part[(int64_t)(k < S ? k : S - 1) * N + n];
    float a = bias ? bias[n] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < S) a += p[k];
    return a;
  };
  float n0 = 0.f, n1 = 0.f, rstd = 0.f;
  if constexpr (QKN) {           // ahead of the divergence below, so that every lane of the wave reaches the shuffles
    if (e < n_pairs) { const int head = e / half, i = e - head * half; n0 = val(head * dh + i); n1 = val(head * dh + i + half); }
    float ss = n0 * n0 + n1 * n1;
    for (int o = 1; o < half; o <<= 1) ss += __shfl_xor(ss, o, 64);
    rstd = rsqrtf(ss / (float)dh + qk_eps);
  }
  if (e < n_pairs) {
    const int head = e / half, i = e - head * half;       // head < Hq: query head, else key head
    const int base = head * dh;                           // q and k sections are contiguous: [q heads | k heads]
    float x0, x1;
    if constexpr (QKN) { const float* w = qkn + (head < Hq ? 0 : dh); x0 = n0 * rstd * w[i]; x1 = n1 * rstd * w[i + half]; }
    else { x0 = val(base + i); x1 = val(base + i + half); }
    float sn, cs;
    sincosf((float)pos * inv_freq[i], &sn, &cs);
    const float y0 = x0 * cs - x1 * sn, y1 = x1 * cs + x0 * sn;
    if (head < Hq) { qout[base + i] = T::from_f32(y0); qout[base + i + half] = T::from_f32(y1); }
    else {
      uint16_t* k = kc + ((int64_t)(head - Hq) * max_ctx + pos) * dh;
      k[i] = T::from_f32(y0); k[i + half] = T::from_f32(y1);
    }
  } else if (e < n_pairs + Nk) {
    const int j = e - n_pairs, vh = j / dh, d = j - vh * dh;
    vc[((int64_t)vh * max_ctx + pos) * dh + d] = T::from_f32(val(Nq + Nk + j));
  }
}

// grouped-query single-token attention: one workgroup per (query head, row); DH/8 lanes share a key.  Row r of the batched
// prompt pass sits at position pos0 + r and sees keys [0, pos0 + r] -- causal by construction, same arithmetic as a decode step.
// 16 waves per workgroup: a decode step has only n_heads workgroups, so the key loop's memory latency is hidden by waves of
// the same workgroup (4 waves: +12 us per layer per 300 keys on Orpheus-3B; 16 waves: a quarter of that).
constexpr int ATT_NW = 16;
// FUSED (the decode step): the workgroup first finishes its own q head and its K/V head's new row from the split-K slices of the
// q|k|v GEMM (sum + bias + RoPE, exactly lm_rope_cache's arithmetic and 16-bit rounding), keeps them in LDS, and the first query
// head of each group writes the K/V row to the cache -- one kernel less per layer; the new row is used from LDS because the
// writer may be another workgroup.  QKN (FUSED only): lm_rope_cache's per-head RMSNorm of q and k before the rotation -- with DH 128 the q
// pairs are wave 0 and the k pairs wave 1, with DH 64 the two halves of wave 0; `tid < DH` is uniform over a wave, so every lane shuffles.
template <typename T, int DH, bool FUSED, bool QKN>
__global__ __launch_bounds__(64 * ATT_NW) void lm_attention(const uint16_t* __restrict__ q, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                                                    uint16_t* __restrict__ out, const LmState* __restrict__ st, int Hq, int Hkv, int max_ctx, float scale, int pos0,
                                                    const float* __restrict__ part, int S, const float* __restrict__ bias, const float* __restrict__ inv_freq,
                                                    int B, int64_t seq_stride, const int2* __restrict__ rowmap, const float* __restrict__ qkn, float qk_eps) {
  extern __shared__ float sc[];            // [max_ctx] scores, then red[ATT_NW][DH] + red2[2 * ATT_NW] (+ FUSED: q, k, v rows [3][DH])
  const int seq = FUSED ? (int)blockIdx.y : rowmap[blockIdx.y].x;          // FUSED: row = sequence; prompt pass: row -> (sequence, position)
  st += seq; kc += (int64_t)seq * seq_stride; vc += (int64_t)seq * seq_stride;
  if (FUSED && st->frozen) return;                          // a frozen sequence's step writes no cache row (uniform over the workgroup)
  constexpr int LPK = DH / 8;              // lanes per key
  constexpr int KPW = 64 / LPK;            // keys per wave instruction
  float* red = sc + max_ctx;
  float* red2 = red + ATT_NW * DH;
  float* qs = red2 + 2 * ATT_NW;           // FUSED only
  float* kn = qs + DH;
  float* vn = kn + DH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, kvh = h / (Hq / Hkv);
  const int nk = (FUSED ? st->pos : rowmap[blockIdx.y].y) + 1;
  const int nkc = FUSED ? nk - 1 : nk;     // keys read from the cache
  q += (int64_t)blockIdx.y * Hq * DH; out += (int64_t)blockIdx.y * Hq * DH;
  const int c = lane % LPK, g = lane / LPK;
  const uint16_t* kb = kc + (int64_t)kvh * max_ctx * DH;
  const uint16_t* vb = vc + (int64_t)kvh * max_ctx * DH;
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
      float x0 = val(base + i), x1 = val(base + i + half);
      if constexpr (QKN) {
        float ss = x0 * x0 + x1 * x1;
#pragma unroll
        for (int o = 1; o < half; o <<= 1) ss += __shfl_xor(ss, o, 64);
        const float rstd = rsqrtf(ss / (float)DH + qk_eps);
        const float* w = qkn + (is_k ? DH : 0);
        x0 = x0 * rstd * w[i]; x1 = x1 * rstd * w[i + half];
      }
      float sn, cs;
      sincosf((float)pos * inv_freq[i], &sn, &cs);
      const uint16_t r0 = T::from_f32(x0 * cs - x1 * sn), r1 = T::from_f32(x1 * cs + x0 * sn);
      float* dst = is_k ? kn : qs;
      dst[i] = T::to_f32(r0); dst[i + half] = T::to_f32(r1);
      if (is_k && writer) { uint16_t* k = kc + ((int64_t)kvh * max_ctx + pos) * DH; k[i] = r0; k[i + half] = r1; }
    } else if (tid < 2 * DH) {
      const int d = tid - DH;
      const uint16_t r = T::from_f32(val(Nq + Nk + kvh * DH + d));
      vn[d] = T::to_f32(r);
      if (writer) vc[((int64_t)kvh * max_ctx + pos) * DH + d] = r;
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
  for (int k0 = wave * KPW * 4; k0 < nkc; k0 += ATT_NW * KPW * 4) {
    s16x8 kv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { int key = k0 + KPW * u + g; key = key < nkc ? key : nkc - 1; kv[u] = *reinterpret_cast<const s16x8*>(kb + (int64_t)key * DH + c * 8); }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      float dot = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) dot += qf[j] * T::to_f32((uint16_t)kv[u][j]);
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
  for (int i = tid; i < nk; i += 64 * ATT_NW) m = fmaxf(m, sc[i]);
  m = wave_max(m);
  if (lane == 0) red2[wave] = m;
  __syncthreads();
  m = red2[0];
#pragma unroll
  for (int i = 1; i < ATT_NW; ++i) m = fmaxf(m, red2[i]);
  float sum = 0.f;
  for (int i = tid; i < nk; i += 64 * ATT_NW) { const float p = __expf(sc[i] - m); sc[i] = p; sum += p; }
  sum = wave_sum(sum);
  if (lane == 0) red2[ATT_NW + wave] = sum;
  __syncthreads();
  sum = 0.f;
#pragma unroll
  for (int i = 0; i < ATT_NW; ++i) sum += red2[ATT_NW + i];
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int k0 = wave * KPW * 4; k0 < nkc; k0 += ATT_NW * KPW * 4) {
    s16x8 vv[4]; float pw[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int key = k0 + KPW * u + g; const int k2 = key < nkc ? key : nkc - 1;
      vv[u] = *reinterpret_cast<const s16x8*>(vb + (int64_t)k2 * DH + c * 8);
      pw[u] = key < nkc ? sc[k2] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += pw[u] * T::to_f32((uint16_t)vv[u][j]);
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
    for (int i = 0; i < ATT_NW; ++i) o += red[i * DH + tid];
    out[h * DH + tid] = T::from_f32(o / sum);
  }
}

// greedy / plain path: advance only (logits are read back by the host)
__global__ void lm_advance(LmState* st) { if (!st[blockIdx.x].frozen) st[blockIdx.x].pos += 1; }
__global__ void lm_set_pos(LmState* st, int pos) { st->pos = pos; }

// batched prompt pass: act[r][j] = silu(gu[r][2j]) * gu[r][2j+1] from the fp32 GEMM output (same expression as the SK_SWIGLU epilogue)
template <typename T>
__global__ __launch_bounds__(256) void lm_swiglu_rows(const float* __restrict__ gu, uint16_t* __restrict__ act, int64_t n_pairs2) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;      // two outputs per thread
  if (e >= n_pairs2) return;
  const f32x4 v = *reinterpret_cast<const f32x4*>(gu + 4 * e);
  const float a = v[0] / (1.0f + __expf(-v[0])) * v[1], b = v[2] / (1.0f + __expf(-v[2])) * v[3];
  *reinterpret_cast<uint32_t*>(act + 2 * e) = pack2<T>(a, b);
}

// ---- host side ------------------------------------------------------------------------------------

}  // namespace

// the layer's packed cache, all sequences of the handle
static LmKvq lm_kvq_layer(const mia_lm* m, int layer) {
  const mia_lm_config& c = m->cfg;
  const size_t rows = ((size_t)layer * m->B_cap) * c.n_kv_heads * c.max_ctx, wpr = (size_t)c.head_dim * m->kv_bits / 32, gpr = c.head_dim / 64;
  return LmKvq{m->dtype, c.head_dim, m->kv_bits, c.n_heads, c.n_kv_heads, c.max_ctx, m->kq_codes + rows * wpr, m->vq_codes + rows * wpr,
               m->kq_pairs + rows * gpr, m->vq_pairs + rows * gpr, m->state, m->inv_freq};
}

void lm_launch_rope_cache(mia_lm* m, int layer, const float* qkv, const float* bias, void* q, const int2* rowmap, int M) {
  const mia_lm_config& c = m->cfg;
  hipStream_t s = m->ctx->stream;
  if (m->kv_bits) { lm_kvq_launch_rope_cache(s, lm_kvq_layer(m, layer), qkv, bias, (uint16_t*)q, rowmap, M); return; }
  const bool f16 = m->dtype == MIA_F16;
  const int dh = c.head_dim;
  const int64_t seq_stride = (int64_t)c.n_kv_heads * c.max_ctx * dh;
  uint16_t* kc = (uint16_t*)m->k_cache + (size_t)layer * m->B_cap * seq_stride;
  uint16_t* vc = (uint16_t*)m->v_cache + (size_t)layer * m->B_cap * seq_stride;
  const int n_el = (c.n_heads + c.n_kv_heads) * (dh / 2) + c.n_kv_heads * dh;
  const float* qkn = m->qk_norm ? m->qk_norm + (size_t)layer * 2 * dh : nullptr;
  const dim3 grid((n_el + 255) / 256, M);
#define ROPE_GO(TT, NN) hipLaunchKernelGGL((lm_rope_cache<TT, NN>), grid, dim3(256), 0, s, qkv, 1, bias, m->inv_freq, (uint16_t*)q, kc, vc, rowmap, c.n_heads, c.n_kv_heads, dh, c.max_ctx, seq_stride, qkn, c.rms_eps)
  if (qkn) { if (f16) ROPE_GO(F16, true); else ROPE_GO(BF16, true); }
  else     { if (f16) ROPE_GO(F16, false); else ROPE_GO(BF16, false); }
#undef ROPE_GO
}

// one launch site for the twelve (dtype, head_dim, fused, q/k norm) instances of the 16-bit cache -- the norm exists in the fused form only:
// the prompt pass's q and k rows were normalised by lm_rope_cache; the packed cache's are lm_kvq.hip's
int lm_launch_attention(mia_lm* m, bool fused, int rows, const void* q, int layer, void* att, const int2* rowmap, const float* part, int S, const float* bias) {
  // fused: rows = sequences (row b uses state b and the b-th cache of the layer); otherwise rows = (sequence, position) pairs
  const mia_lm_config& c = m->cfg;
  hipStream_t s = m->ctx->stream;
  if (m->kv_bits) { lm_kvq_launch_attention(s, lm_kvq_layer(m, layer), fused, rows, (const uint16_t*)q, (uint16_t*)att, rowmap, part, S, bias); return 0; }
  const int64_t seq_stride = (int64_t)c.n_kv_heads * c.max_ctx * c.head_dim;
  uint16_t* kc = (uint16_t*)m->k_cache + (size_t)layer * m->B_cap * seq_stride;
  uint16_t* vc = (uint16_t*)m->v_cache + (size_t)layer * m->B_cap * seq_stride;
  const int dh = c.head_dim;
  const size_t lds = (size_t)(c.max_ctx + ATT_NW * dh + 2 * ATT_NW + 3 * dh) * 4;
  const float scale = 1.0f / sqrtf((float)dh);
  const dim3 grid(c.n_heads, rows), block(64 * ATT_NW);
  const float* qkn = fused && m->qk_norm ? m->qk_norm + (size_t)layer * 2 * dh : nullptr;
#define ATT_GO_N(TT, DD, FF, NN) hipLaunchKernelGGL((lm_attention<TT, DD, FF, NN>), grid, block, lds, s, (const uint16_t*)q, kc, vc, (uint16_t*)att, m->state, c.n_heads, c.n_kv_heads, c.max_ctx, scale, 0, part, S, bias, m->inv_freq, rows, seq_stride, rowmap, qkn, c.rms_eps)
#define ATT_GO(TT, DD, FF) ATT_GO_N(TT, DD, FF, false)
  const bool f16 = m->dtype == MIA_F16;
  if (qkn) { if (dh == 128) { if (f16) ATT_GO_N(F16, 128, true, true); else ATT_GO_N(BF16, 128, true, true); } else { if (f16) ATT_GO_N(F16, 64, true, true); else ATT_GO_N(BF16, 64, true, true); } }
  else if (dh == 128) { if (fused) { if (f16) ATT_GO(F16, 128, true); else ATT_GO(BF16, 128, true); } else { if (f16) ATT_GO(F16, 128, false); else ATT_GO(BF16, 128, false); } }
  else           { if (fused) { if (f16) ATT_GO(F16, 64, true); else ATT_GO(BF16, 64, true); } else { if (f16) ATT_GO(F16, 64, false); else ATT_GO(BF16, 64, false); } }
#undef ATT_GO
#undef ATT_GO_N
  return 0;
}

// one skinny GEMM of the step chain on nb rows of the handle (16-bit or packed weights; fragment order when the handle has the copy)
static int lm_skinny(mia_lm* m, int nb, const void* A, int64_t lda, const void* W, const void* Wf, const float* bias, void* out, int64_t ldo, int N, int K, int S,
                     int mode, const Q4W* qw = nullptr, const float* ss_in = nullptr, const float* nw = nullptr, float* ss_out = nullptr, float rs_scale = 1.f) {
  const mia_lm_config& c = m->cfg;
  SkinnyArgs a{(const uint16_t*)A, lda, (const uint16_t*)W, bias, out, ldo, nullptr, nullptr, nullptr, nb, N, K, S, MIA_ACT_NONE, 0, 0, 0};
  if (ss_in) { a.ss_in = ss_in; a.ss_tiles = c.hidden / 16; a.ss_dim = c.hidden; a.eps = c.rms_eps; a.rs_scale = rs_scale; }
  if (mode == SK_RESID) { a.xres = m->x; a.nw = nw; a.ss_out = ss_out; }
  if (m->q4 && qw && qw->wfrag) return skinny_gemm_q_launch(a, qw->wfrag, qw->stfrag, m->q_bits, mode, m->dtype, m->ctx->stream, m->B_cap);      // the form follows the capacity (skinny.h)
  if (Wf) { a.W = (const uint16_t*)Wf; a.w_frag = 1; }      // same K order and partition as the row-major form: identical results
  return skinny_gemm_launch(a, mode, m->dtype, m->ctx->stream);
}

bool lm_fused_norm(const mia_lm* m) { return (m->cfg.hidden % 16) == 0 && m->cfg.hidden <= 8192 && m->B_cap <= 4; }

// nb sequences = nb rows of every skinny GEMM: the weights are still read once per step
// RMSNorm rides on the GEMMs (skinny.h, SkinnyArgs): the two residual-writing projections (o, down) add into x, emit the next block's
// activation x * norm weight (16 bit) and per-tile sums of squares; the GEMM that consumes it scales its accumulators by rstd.  Two
// launches less per layer than "GEMM -> split-K partials -> reduce + norm kernel" (5.1 us each on Orpheus-3B, 56 per token).
// Up to 4 sequences (the latency-critical case).  Wider batches keep the split-K + reduce / norm chain: without a cross-workgroup split the
// residual-writing projections run on hidden / 16 workgroups only (32 sentences side by side, Orpheus-3B: 6 400 tokens/s fused, 9 500 split).
// The choice follows the handle's CAPACITY (mia_lm_set_batch), not the rows of this call: within one capacity every call -- one sequence
// or many -- runs the same chain, so a sequence's ids do not depend on which batch it sits in.
int lm_enqueue_layers(mia_lm* m, int nb) {
  hipStream_t s = m->ctx->stream;
  const mia_lm_config& c = m->cfg;
  const int D = c.hidden, dh = c.head_dim, Nq = c.n_heads * dh, Nk = c.n_kv_heads * dh, Nqkv = Nq + 2 * Nk;
  const bool f16 = m->dtype == MIA_F16;
  const bool fused_norm = lm_fused_norm(m);
  const int ss_tiles = D / 16;
  float* ss_o = m->ss;                                   // written by o-proj, read by gate|up
  float* ss_d = m->ss + (size_t)ss_tiles * m->B_cap;     // written by down-proj, read by the next q|k|v (or the head)
  auto skinny = [&](const void* A, int64_t lda, const void* W, const void* Wf, const float* bias, void* out, int64_t ldo, int N, int K, int S, int mode,
                    const Q4W* qw = nullptr, const float* ss_in = nullptr, const float* nw = nullptr, float* ss_out = nullptr, float rs_scale = 1.f) {
    return lm_skinny(m, nb, A, lda, W, Wf, bias, out, ldo, N, K, S, mode, qw, ss_in, nw, ss_out, rs_scale);
  };
  LAUNCH_T(lm_embed_norm, dim3(nb), dim3(256), 0, m->tokens, (const uint16_t*)m->embed, (const uint16_t*)m->gen_embed, m->embeds, m->layers[0].in_norm, m->x, (uint16_t*)m->h, m->state, D, c.rms_eps, (const int2*)nullptr, c.max_ctx, c.vocab, m->gen_rows);
  for (int l = 0; l < c.n_layers; ++l) {
    const LmLayer& L = m->layers[l];
    const float* next_norm = l + 1 < c.n_layers ? m->layers[l + 1].in_norm : m->final_norm;
    const float* next_norm_c = l + 1 < c.n_layers ? m->layers[l + 1].in_norm_c : m->final_norm_c;
    if (fused_norm) {
      // layer 0 reads the embedding kernel's (normalised) h; later layers the previous down-proj's x * norm weight + its sums of squares
      if (skinny(m->h, D, L.wqkv, L.wqkv_f, nullptr, m->qkv_part, 0, Nqkv, D, m->S_qkv, SK_PARTIAL, &L.q_qkv, l > 0 ? ss_d : nullptr, nullptr, nullptr, L.in_rs)) return -1;
      lm_launch_attention(m, true, nb, nullptr, l, m->att, nullptr, m->qkv_part, m->S_qkv, L.bqkv);      // RoPE + cache row + attention
      if (skinny(m->att, Nq, L.wo, L.wo_f, nullptr, m->h, D, D, Nq, 1, SK_RESID, &L.q_o, nullptr, L.post_norm_c, ss_o)) return -1;
      if (skinny(m->h, D, L.wgu, L.wgu_f, nullptr, m->act, c.inter, 2 * c.inter, D, 1, SK_SWIGLU, &L.q_gu, ss_o, nullptr, nullptr, L.post_rs)) return -1;
      if (skinny(m->act, c.inter, L.wdown, L.wdown_f, nullptr, m->h, D, D, c.inter, 1, SK_RESID, &L.q_down, nullptr, next_norm_c, ss_d)) return -1;
      continue;
    }
    if (skinny(m->h, D, L.wqkv, L.wqkv_f, nullptr, m->qkv_part, 0, Nqkv, D, m->S_qkv, SK_PARTIAL, &L.q_qkv)) return -1;
    lm_launch_attention(m, true, nb, nullptr, l, m->att, nullptr, m->qkv_part, m->S_qkv, L.bqkv);      // RoPE + cache row + attention
    if (skinny(m->att, Nq, L.wo, L.wo_f, nullptr, m->partial, 0, D, Nq, m->S_o, SK_PARTIAL, &L.q_o)) return -1;
    LAUNCH_T(lm_reduce_norm, dim3(nb), dim3(256), 0, m->partial, m->S_o, L.post_norm, m->x, (uint16_t*)m->h, D, c.rms_eps, nb);
    if (skinny(m->h, D, L.wgu, L.wgu_f, nullptr, m->act, c.inter, 2 * c.inter, D, 1, SK_SWIGLU, &L.q_gu)) return -1;
    if (skinny(m->act, c.inter, L.wdown, L.wdown_f, nullptr, m->partial, 0, D, c.inter, m->S_down, SK_PARTIAL, &L.q_down)) return -1;
    LAUNCH_T(lm_reduce_norm, dim3(nb), dim3(256), 0, m->partial, m->S_down, next_norm, m->x, (uint16_t*)m->h, D, c.rms_eps, nb);
  }
  return 0;
}

// out [nb][ldo] (fp32) = final_norm(x) . W^T (+ bias): m->h is the last layer's carried activation (fused chain: still to be divided by its
// rms, which the GEMM does from the down-projection's sums of squares) or the normalised row (split-K chain)
int lm_enqueue_linear_of_last(mia_lm* m, int nb, const void* W, const void* Wf, const float* bias, const Q4W* qw, float* out, int64_t ldo, int N) {
  const mia_lm_config& c = m->cfg;
  const float* ss_d = m->ss + (size_t)(c.hidden / 16) * m->B_cap;
  return lm_skinny(m, nb, m->h, c.hidden, W, Wf, bias, out, ldo, N, c.hidden, 1, SK_OUTF32, qw, lm_fused_norm(m) && c.n_layers > 0 ? ss_d : nullptr, nullptr, nullptr, m->final_rs);
}

void lm_enqueue_advance(mia_lm* m, int nb) { hipLaunchKernelGGL(lm_advance, dim3(nb), dim3(1), 0, m->ctx->stream, m->state); }

namespace {

// (the samplers read each sequence's prompt length from its state: a captured and a directly launched step issue the same arguments)
// mode: LM_STEP_* (what ends the step); sp: the top-p sampler's arguments, the greedy one's stop ids, or the top-k one's temperature, top_p
// and stop ids with its effective k in top_k; ras: the RAS sampler's
int lm_enqueue_step(mia_lm* m, int mode, const mia_lm_sampler& sp, const RasParams* ras = nullptr, int nb = 1, int top_k = 0) {
  hipStream_t s = m->ctx->stream;
  const mia_lm_config& c = m->cfg;
  if (lm_enqueue_layers(m, nb)) return -1;
  const int HV = m->head_vocab > 0 ? m->head_vocab : c.vocab;
  if (lm_enqueue_linear_of_last(m, nb, m->lm_head, m->lm_head_f, m->head_bias, &m->q_head, m->logits, HV, HV)) return -1;
  if (mode == LM_STEP_RAS) lm_sample_ras_launch(s, m->logits, HV, m->tokens, m->out_tokens, m->uniforms, m->state, *ras, c.max_ctx, nb);
  else if (mode == LM_STEP_TOP_P) lm_sample_launch(s, m->logits, HV, m->tokens, m->hist, m->uniforms, m->state, m->smx, sp, -1, c.max_ctx, nb);
  else if (mode == LM_STEP_GREEDY) lm_sample_greedy_launch(s, m->logits, HV, m->tokens, m->out_tokens, m->state, m->smx, sp, c.max_ctx, nb);
  else if (mode == LM_STEP_TOPK) lm_sample_topk_launch(s, m->logits, HV, m->tokens, m->out_tokens, m->uniforms, m->state, m->smx, sp, top_k, c.max_ctx, nb);
  else lm_enqueue_advance(m, nb);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace

// ---- batched prompt pass ---------------------------------------------------------------------------
// Positions [pos0, pos0 + P) of the sequence (token ids already in m->tokens, or embedding rows in m->embeds) go through the
// layers as rows of bf16/f16 MFMA GEMMs (gemm.hip) instead of P single-row step graphs: one read of the weights per chunk of
// PF_ROWS positions instead of one per position.  Only the K/V caches are produced -- the caller runs the LAST prompt position
// through the ordinary step (which owns the head and the sampler), so P = n_prompt - 1.  Per-row arithmetic mirrors the step:
// fp32 residual stream, 16-bit RMSNorm output, fp32 q|k|v -> RoPE -> 16-bit, same attention kernel (row r sees keys [0, pos0+r]),
// fp32 gate/up -> silu(g)*u -> 16-bit.  (The reference does the same thing: model(promptIds, cache) is one batched call,
// OrpheusTTS.swift:262-279 / Qwen2LM.swift:353-361.)  With mia_lm_set_prompt_weights(1) the four GEMMs multiply the attached packed
// weights instead (gemm_quant.hip), as the reference's quantizedMatmul does for prompt and step alike; nothing else changes.
static constexpr int PF_ROWS = 512;
static constexpr int PF_MIN_ROWS = LM_PREFILL_MIN_ROWS;

bool lm_prefill_supported(const mia_lm* m) {
  const bool off = (m->debug_flags & 2) != 0;      // test hook (mia_lm_set_debug)
  const mia_lm_config& c = m->cfg;
  return !off && c.hidden % 64 == 0 && (c.n_heads * c.head_dim) % 64 == 0 && c.inter % 64 == 0;
}

// rows: (sequence, position) pairs, every sequence's positions ascending; after the pass set_pos[b] (if >= 0) becomes state b's position
int lm_prefill_rows(mia_lm* m, const std::vector<int2>& rows, const std::vector<int>& set_pos) {
  mia_ctx* ctx = m->ctx;
  hipStream_t s = ctx->stream;
  const mia_lm_config& c = m->cfg;
  const int D = c.hidden, dh = c.head_dim, Nq = c.n_heads * dh, Nk = c.n_kv_heads * dh, Nqkv = Nq + 2 * Nk, I = c.inter;
  const bool f16 = m->dtype == MIA_F16;
  const size_t b_x = align_up((size_t)PF_ROWS * D * 4, 256), b_h = align_up((size_t)PF_ROWS * D * 2, 256), b_qkv = align_up((size_t)PF_ROWS * Nqkv * 4, 256),
               b_q = align_up((size_t)PF_ROWS * Nq * 2, 256), b_gu = align_up((size_t)PF_ROWS * 2 * I * 4, 256), b_act = align_up((size_t)PF_ROWS * I * 2, 256),
               b_map = align_up((size_t)PF_ROWS * sizeof(int2), 256), b_tiles = align_up((size_t)PF_ROWS * sizeof(int4), 256);
  if (!m->pf_buf) {
    void* p = nullptr;
    if (hipMalloc(&p, b_x + b_h + b_qkv + 2 * b_q + b_gu + b_act + b_map + b_tiles) != hipSuccess) return mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "lm: prompt-pass buffers");
    m->allocs.push_back(p); m->pf_buf = (char*)p;
  }
  char* b = m->pf_buf;
  float* x = (float*)b; b += b_x;
  uint16_t* h = (uint16_t*)b; b += b_h;
  float* qkv = (float*)b; b += b_qkv;
  uint16_t* q = (uint16_t*)b; b += b_q;
  uint16_t* att = (uint16_t*)b; b += b_q;
  float* gu = (float*)b; b += b_gu;
  uint16_t* act = (uint16_t*)b; b += b_act;
  int2* rowmap = (int2*)b; b += b_map;
  int4* tiles = (int4*)b;                          // query tiles of the chunk (prompt_attn 1 only)
  // mia_lm_set_prompt_attention(1): the chunk's attention is lm_prefill_attn.hip's tiled kernel; the packed cache keeps lm_kvq's row kernel
  const bool tiled = m->prompt_attn == 1 && !m->kv_bits;
  const int qtile = lm_prefill_attn_qtile(c.n_heads, c.n_kv_heads);
  std::vector<std::vector<int4>> chunk_tiles(tiled ? (rows.size() + PF_ROWS - 1) / PF_ROWS : 0);    // alive until the call returns, like `rows`
  // mia_lm_set_prompt_weights(1): the four GEMMs read the packed weights the step streams (gemm_quant.hip) -- the prompt's K/V rows then
  // come from the same function of the weights as the generated tokens' -- and W is not touched (it may be gone: mia_lm_release_dense)
  const bool packed = m->prompt_packed != 0;
  auto gemm = [&](const void* A, int K, const void* W, const Q4W& qw, float* C, int N, int M, const float* R) {
    if (packed) {
      GemmQuantArgs g;
      g.A = (const uint16_t*)A; g.lda = K; g.wfrag = qw.wfrag; g.stfrag = qw.stfrag; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K;
      if (R) { g.R = R; g.ldr = N; }
      if (const char* e = gemm_quant_check(g, m->q_bits, m->dtype)) { ctx->err = e; return -1; }
      return gemm_quant_launch(g, m->q_bits, m->dtype, s);
    }
    GemmArgs g;
    g.A = A; g.lda = K; g.W = W; g.C = C; g.ldc = N; g.M = M; g.N = N; g.K = K; g.out_f32 = 1;
    if (R) { g.R = R; g.ldr = N; }
    if (const char* e = mia_gemm_check(g)) { ctx->err = e; return -1; }
    return mia_gemm_launch(g, m->dtype, s);
  };
  const int P = (int)rows.size();
  for (int r0 = 0; r0 < P; r0 += PF_ROWS) {
    const int M = std::min(PF_ROWS, P - r0);
    // (pageable source: the copy is staged before the call returns, and the stream orders it behind the previous chunk's kernels)
    MIA_HIP(ctx, hipMemcpyAsync(rowmap, rows.data() + r0, (size_t)M * sizeof(int2), hipMemcpyHostToDevice, s));
    LAUNCH_T(lm_embed_norm, dim3(M), dim3(256), 0, m->tokens, (const uint16_t*)m->embed, (const uint16_t*)m->gen_embed, m->embeds, m->layers[0].in_norm, x, h,
             m->state, D, c.rms_eps, (const int2*)rowmap, c.max_ctx, c.vocab, m->gen_rows);
    LmPromptAttn pa;
    if (tiled) {
      std::vector<int4>& t = chunk_tiles[r0 / PF_ROWS];
      lm_prefill_attn_tiles(rows.data() + r0, M, qtile, t);
      MIA_HIP(ctx, hipMemcpyAsync(tiles, t.data(), t.size() * sizeof(int4), hipMemcpyHostToDevice, s));
      pa.q = q; pa.out = att; pa.tiles = tiles; pa.n_tiles = (int)t.size(); pa.Hq = c.n_heads; pa.Hkv = c.n_kv_heads; pa.dh = dh; pa.max_ctx = c.max_ctx;
      pa.seq_stride = (int64_t)c.n_kv_heads * c.max_ctx * dh; pa.dtype = m->dtype;
    }
    for (int l = 0; l < c.n_layers; ++l) {
      const LmLayer& L = m->layers[l];
      if (gemm(h, D, L.wqkv, L.q_qkv, qkv, Nqkv, M, nullptr)) return MIA_ERR_DEVICE;
      lm_launch_rope_cache(m, l, qkv, L.bqkv, q, rowmap, M);
      if (l + 1 == c.n_layers) break;            // past its K/V rows the last layer feeds only the head, which the prompt pass skips
      if (tiled) {
        pa.kc = (const uint16_t*)m->k_cache + (size_t)l * m->B_cap * pa.seq_stride; pa.vc = (const uint16_t*)m->v_cache + (size_t)l * m->B_cap * pa.seq_stride;
        if (const char* e = lm_prefill_attn_check(pa)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "%s", e);
        if (lm_prefill_attn_launch(pa, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "lm: prompt attention launch failed");
      } else lm_launch_attention(m, false, M, q, l, att, rowmap, nullptr, 0, nullptr);
      if (gemm(att, Nq, L.wo, L.q_o, x, D, M, x)) return MIA_ERR_DEVICE;                   // x += att . Wo^T
      LAUNCH_T(lm_reduce_norm, dim3(M), dim3(256), 0, (const float*)nullptr, 0, L.post_norm, x, h, D, c.rms_eps, 1);
      if (gemm(h, D, L.wgu, L.q_gu, gu, 2 * I, M, nullptr)) return MIA_ERR_DEVICE;
      const int64_t n2 = (int64_t)M * I / 2;
      LAUNCH_T(lm_swiglu_rows, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, gu, act, n2);
      if (gemm(act, I, L.wdown, L.q_down, x, D, M, x)) return MIA_ERR_DEVICE;             // x += act . Wdown^T
      LAUNCH_T(lm_reduce_norm, dim3(M), dim3(256), 0, (const float*)nullptr, 0, m->layers[l + 1].in_norm, x, h, D, c.rms_eps, 1);
    }
  }
  for (size_t sq = 0; sq < set_pos.size(); ++sq)
    if (set_pos[sq] >= 0) hipLaunchKernelGGL(lm_set_pos, dim3(1), dim3(1), 0, s, m->state + sq, set_pos[sq]);
  if (hipGetLastError() != hipSuccess) return mia_fail(ctx, MIA_ERR_DEVICE, "lm: prompt-pass launch failed");
  return MIA_OK;
}

// positions [pos0, pos0 + P) of sequence 0
static int lm_prefill(mia_lm* m, int pos0, int P) {
  std::vector<int2> rows(P);
  for (int i = 0; i < P; ++i) rows[i] = make_int2(0, pos0 + i);
  return lm_prefill_rows(m, rows, {pos0 + P});
}

namespace {

int lm_graph(mia_lm* m, int mode, const mia_lm_sampler& sp, const RasParams* ras = nullptr, int nb = 1, int top_k = 0) {
  mia_ctx* ctx = m->ctx;
  if (m->debug_flags & 1) return 1;                  // test hook (mia_lm_set_debug): launch every step directly
  mia_lm_sampler key{}; RasParams rkey{};
  if (mode == LM_STEP_TOP_P || mode == LM_STEP_GREEDY || mode == LM_STEP_TOPK) key = sp;
  if (mode == LM_STEP_RAS) rkey = *ras;
  const int kkey = mode == LM_STEP_TOPK ? top_k : 0;
  if (m->graph && m->graph_mode == mode && m->graph_nb == nb && m->graph_top_k == kkey && memcmp(&m->graph_sampler, &key, sizeof(key)) == 0 &&
      memcmp(&m->graph_ras, &rkey, sizeof(rkey)) == 0) return 0;
  if (m->graph) { (void)hipGraphExecDestroy(m->graph); m->graph = nullptr; }
  hipGraph_t g = nullptr;
  MIA_HIP(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  const int erc = lm_enqueue_step(m, mode, sp, ras, nb, top_k);
  hipError_t ce = hipStreamEndCapture(ctx->stream, &g);
  if (erc != 0 || ce != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); return mia_fail(ctx, MIA_ERR_DEVICE, "lm: step graph capture failed"); }
  hipError_t ie = hipGraphInstantiate(&m->graph, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (ie != hipSuccess) { m->graph = nullptr; return mia_fail(ctx, MIA_ERR_DEVICE, "lm: hipGraphInstantiate failed"); }
  m->graph_sampler = key; m->graph_ras = rkey; m->graph_top_k = kkey; m->graph_mode = mode; m->graph_nb = nb;
  return 0;
}

}  // namespace

// test hook: bit 0 launches every step directly (no hipGraph), bit 1 walks prompts through the step (no batched prompt pass)
extern "C" int mia_lm_set_debug(mia_lm* m, int flags) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(m->ctx, flags >= 0 && flags <= 3, "lm_set_debug: flags must be 0..3 (got %d)", flags);
  m->debug_flags = flags;
  return MIA_OK;
}

// which attention the batched prompt pass runs on the 16-bit cache: 0 = lm_attention, one workgroup per (query head, row) -- the default;
// 1 = lm_prefill_attn.hip's tiled matrix-core kernel.  The step graph and the packed cache's prompt pass are not affected.
extern "C" int mia_lm_set_prompt_attention(mia_lm* m, int mode) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_CHECK_ARG(m->ctx, mode == 0 || mode == 1, "lm_set_prompt_attention: mode must be 0 or 1 (got %d)", mode);
  m->prompt_attn = mode;
  return MIA_OK;
}

extern "C" int mia_lm_reset(mia_lm* m) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  MIA_HIP(m->ctx, hipSetDevice(m->ctx->device));
  MIA_HIP(m->ctx, hipMemsetAsync(m->state, 0, sizeof(LmState), m->ctx->stream));
  return MIA_OK;
}

// Feed n tokens (appended at the current position) and return the logits after the last one (model(ids, cache) + [0,-1]).
extern "C" int mia_lm_forward(mia_lm* m, const int32_t* ids, int n, float* last_logits) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, ids && n > 0, "lm_forward: ids required");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  LmState st{};
  MIA_HIP(ctx, hipMemcpyAsync(&st, m->state, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  MIA_CHECK_ARG(ctx, st.pos + n <= m->cfg.max_ctx, "lm_forward: context overflow (%d + %d > %d)", st.pos, n, m->cfg.max_ctx);
  for (int i = 0; i < n; ++i) MIA_CHECK_ARG(ctx, ids[i] >= 0 && ids[i] < m->cfg.vocab, "lm_forward: token %d out of vocabulary", ids[i]);
  MIA_HIP(ctx, hipMemcpyAsync(m->tokens + st.pos, ids, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  mia_lm_sampler none{};
  const int gr = lm_graph(m, LM_STEP_FORWARD, none);
  if (gr < 0) return gr;
  int done = 0;
  if (n - 1 >= PF_MIN_ROWS && lm_prefill_supported(m)) {        // all but the last position: K/V only, batched
    if (const int rc = lm_prefill(m, st.pos, n - 1)) return rc;
    done = n - 1;
  }
  for (int i = done; i < n; ++i) {
    if (gr == 0) MIA_HIP(ctx, hipGraphLaunch(m->graph, ctx->stream));
    else if (lm_enqueue_step(m, LM_STEP_FORWARD, none)) return mia_fail(ctx, MIA_ERR_DEVICE, "lm_forward: launch failed");
  }
  if (last_logits) MIA_HIP(ctx, hipMemcpyAsync(last_logits, m->logits, (size_t)m->cfg.vocab * 4, hipMemcpyDeviceToHost, ctx->stream));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MIA_OK;
}

// Sequences side by side: every step reads the weights once for all of them (rows of the same skinny GEMMs), each sequence has
// its own K/V cache, repetition window, uniforms and stop state.  Re-allocates the per-sequence state; 1 restores the default.
extern "C" int mia_lm_set_batch(mia_lm* m, int max_batch) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, max_batch >= 1 && max_batch <= 32, "lm_set_batch: 1 <= max_batch <= 32 (one MFMA row tile)");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (max_batch == m->B_cap) return MIA_OK;
  if (lm_alloc_state(m, max_batch)) return mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "lm_set_batch: state buffers for %d sequences", max_batch);
  MIA_HIP(ctx, hipDeviceSynchronize());
  return MIA_OK;
}

// QuantizedKVCache(groupSize:bits:) in place of KVCacheSimple (OrpheusModel.newCache, TransformerBlock.swift:182-201): bits 4 | 8 keeps K/V
// as codes + per-64 (scale, bias) pairs (lm_kvq.hip), bits 0 restores the 16-bit caches.  Re-allocates the per-sequence state at the
// current capacity (either order with mia_lm_set_batch), drops the step graph and resets every sequence; cache contents are not converted.
extern "C" int mia_lm_set_kv_quant(mia_lm* m, int bits, int group_size) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  int code = MIA_OK;
  if (const char* e = lm_kvq_check(bits, group_size, m->cfg.head_dim, &code)) return mia_fail(ctx, code, "lm_set_kv_quant: %s (bits %d, group_size %d)", e, bits, group_size);
  // (the reference's Qwen3 decoder runs on KVCacheSimple only, FunASRSTT.swift:120; lm_kvq.hip's kernels do not carry the q/k norm)
  if (bits != 0 && m->qk_norm) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "lm_set_kv_quant: a quantised KV cache on a handle with q_norm / k_norm tensors is not supported");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int before = m->kv_bits;
  m->kv_bits = bits;
  if (lm_alloc_state(m, m->B_cap)) {
    m->kv_bits = before;
    (void)lm_alloc_state(m, m->B_cap);
    return mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "lm_set_kv_quant: state buffers for %d sequences", m->B_cap);
  }
  MIA_HIP(ctx, hipDeviceSynchronize());
  return MIA_OK;
}

// test hook: rows [pos0, pos0 + n) of every kv head of (layer, seq) as fp32 [Hkv][n][dh] -- scale * code + bias from the packed cache,
// widened from the 16-bit one.  Host pointers.
extern "C" int mia_lm_read_kv(mia_lm* m, int layer, int seq, int pos0, int n, float* k_out, float* v_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  const mia_lm_config& c = m->cfg;
  MIA_CHECK_ARG(ctx, k_out && v_out, "lm_read_kv: null output");
  MIA_CHECK_ARG(ctx, layer >= 0 && layer < c.n_layers && seq >= 0 && seq < m->B_cap, "lm_read_kv: layer %d / sequence %d out of range (%d layers, capacity %d)", layer, seq, c.n_layers, m->B_cap);
  MIA_CHECK_ARG(ctx, pos0 >= 0 && n > 0 && pos0 <= c.max_ctx - n, "lm_read_kv: rows [%d, %d + %d) outside [0, %d)", pos0, pos0, n, c.max_ctx);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const int dh = c.head_dim;
  const size_t wpr = m->kv_bits ? (size_t)dh * m->kv_bits / 32 : (size_t)dh / 2, gpr = dh / 64;      // dwords per row
  std::vector<uint32_t> rows((size_t)n * wpr), pairs((size_t)n * gpr);
  for (int kv = 0; kv < 2; ++kv)
    for (int hd = 0; hd < c.n_kv_heads; ++hd) {
      const size_t r0 = (((size_t)layer * m->B_cap + seq) * c.n_kv_heads + hd) * c.max_ctx + pos0;
      float* out = (kv ? v_out : k_out) + (size_t)hd * n * dh;
      if (m->kv_bits) {
        MIA_HIP(ctx, hipMemcpy(rows.data(), (kv ? m->vq_codes : m->kq_codes) + r0 * wpr, rows.size() * 4, hipMemcpyDeviceToHost));
        MIA_HIP(ctx, hipMemcpy(pairs.data(), (kv ? m->vq_pairs : m->kq_pairs) + r0 * gpr, pairs.size() * 4, hipMemcpyDeviceToHost));
        lm_kvq_read_rows(rows.data(), pairs.data(), n, dh, m->kv_bits, m->dtype, out);
      } else {
        MIA_HIP(ctx, hipMemcpy(rows.data(), (const uint32_t*)(kv ? m->v_cache : m->k_cache) + r0 * wpr, rows.size() * 4, hipMemcpyDeviceToHost));
        const uint16_t* src = (const uint16_t*)rows.data();
        for (size_t i = 0; i < (size_t)n * dh; ++i) {
          if (m->dtype == MIA_F16) { _Float16 hh; memcpy(&hh, &src[i], 2); out[i] = (float)hh; }
          else { const uint32_t u = (uint32_t)src[i] << 16; memcpy(&out[i], &u, 4); }
        }
      }
    }
  return MIA_OK;
}

// ---- the generate loop -----------------------------------------------------------------------------
namespace {

// One validated call of a generate entry point.  The samplers tie the two forms together: the top-p kernels count a prompt of ids
// (LmState::n_prompt) and append the drawn ids to `tokens` (n_gen of them); the RAS kernel counts a prompt of embedding rows (n_embeds)
// and emits to `out_tokens` (n_out ids), and so do the greedy kernel (embedding rows in, no uniforms) and the top-k kernels (embedding
// rows AND uniforms, top_k > 0).  A single-sequence call is
// n_seq = 1 with offsets {0, n_prompt}.
struct LmGenCall {
  const char* name;                       // entry point, for error messages
  int n_seq;
  const int32_t* offsets;                 // [n_seq + 1]: sequence b's prompt is ids / rows [offsets[b], offsets[b + 1])
  const int32_t* ids = nullptr;           // top-p: the prompts' ids ...
  const mia_lm_sampler* sp = nullptr;     // ... and the sampler
  const float* embeds = nullptr;          // RAS / greedy: the prompts' embedding rows [.][hidden] ...
  const mia_ras_params* ras = nullptr;    // ... RAS: [n_seq] parameters (min_len / max_len per sequence, the rest equal)
  const float* uniforms = nullptr;        // sequence b draws from uniforms[b * u_stride + i], i < n_uniforms (staged up to max_ctx of them); greedy: none
  int top_k = 0;                          // > 0: the top-k / top-p sampler on an embedding-row prompt, with this effective k and sp's temperature / top_p
  int u_stride = 0, n_uniforms = 0;
  int max_new = 0;                        // the most steps any sequence runs past its prompt
  // A prompt with at least this many positions before its last one goes through the batched prompt pass; a shorter one walks the step.
  // The pass builds K/V through gemm.hip, the step through the skinny kernels: different fp32 summation orders, so the threshold is part
  // of an entry point's results.  The single-sequence entries pass PF_MIN_ROWS (below it the step is as fast), the batch entries 1 (every
  // prompt row shares the GEMMs of one pass).  Two values on purpose: merging them changes ids.
  int pf_min_rows = 1;
  int32_t* out = nullptr; int out_stride = 0; int32_t* n_out = nullptr;   // sequence b's ids at out + b * out_stride, their count in n_out[b]
};

int lm_generate_run(mia_lm* m, const LmGenCall& g) {
  mia_ctx* ctx = m->ctx;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int C = m->cfg.max_ctx, D = m->cfg.hidden, B = g.n_seq;
  const int nu = std::min(g.n_uniforms, C);
  auto n_prompt = [&](int b) { return g.offsets[b + 1] - g.offsets[b]; };
  std::vector<LmState> st(B);
  for (int b = 0; b < B; ++b) {
    st[b] = LmState{};
    if (g.embeds) {
      st[b].n_embeds = n_prompt(b);
      if (g.ras) { st[b].min_len = g.ras[b].min_len; st[b].max_len = g.ras[b].max_len; }
      else st[b].max_len = g.max_new;
      MIA_HIP(ctx, hipMemcpyAsync(m->embeds + (size_t)b * C * D, g.embeds + (size_t)g.offsets[b] * D, (size_t)n_prompt(b) * D * 4, hipMemcpyHostToDevice, s));
    } else {
      st[b].n_prompt = n_prompt(b);
      MIA_HIP(ctx, hipMemcpyAsync(m->tokens + (size_t)b * C, g.ids + g.offsets[b], (size_t)n_prompt(b) * 4, hipMemcpyHostToDevice, s));
    }
    if (g.uniforms) MIA_HIP(ctx, hipMemcpyAsync(m->uniforms + (size_t)b * C, g.uniforms + (size_t)b * g.u_stride, (size_t)nu * 4, hipMemcpyHostToDevice, s));
  }
  MIA_HIP(ctx, hipMemcpyAsync(m->state, st.data(), sizeof(LmState) * B, hipMemcpyHostToDevice, s));
  MIA_HIP(ctx, hipStreamSynchronize(s));
  mia_lm_sampler sp{}; RasParams r{};
  if (g.ras) r = RasParams{g.ras[0].top_p, g.ras[0].top_k, g.ras[0].win, g.ras[0].tau, g.ras[0].eos, 0, 0, nu};   // (the length bounds travel in the state: one graph serves every text length)
  else sp = *g.sp;
  const RasParams* rp = g.ras ? &r : nullptr;
  const int mode = g.ras ? LM_STEP_RAS : g.embeds ? (g.top_k > 0 ? LM_STEP_TOPK : LM_STEP_GREEDY) : LM_STEP_TOP_P;
  const int gr = lm_graph(m, mode, sp, rp, B, g.top_k);
  if (gr < 0) return gr;
  // prompts: everything but a prompt's last position through the batched prompt pass (K/V only; the rows of all prompts share its
  // GEMMs), the last position takes the first step.  A prompt that does not take the pass walks the step instead -- its sampler idles
  // until the prompt is consumed -- and the longest such walk adds to everyone's step count.
  const bool pre = lm_prefill_supported(m);
  std::vector<int2> rows;
  std::vector<int> set_pos(B, -1);
  int walk = 0;
  for (int b = 0; b < B; ++b) {
    const int head = n_prompt(b) - 1;
    if (pre && head >= g.pf_min_rows) {
      for (int i = 0; i < head; ++i) rows.push_back(make_int2(b, i));
      set_pos[b] = head;
    } else walk = std::max(walk, head);
  }
  if (!rows.empty()) { if (const int rc = lm_prefill_rows(m, rows, set_pos)) return rc; }
  auto read_state = [&]() -> int {
    MIA_HIP(ctx, hipMemcpyAsync(st.data(), m->state, sizeof(LmState) * B, hipMemcpyDeviceToHost, s));
    MIA_HIP(ctx, hipStreamSynchronize(s));
    return MIA_OK;
  };
  const int total = walk + g.max_new;
  for (int step = 0; step < total; ++step) {
    if (gr == 0) MIA_HIP(ctx, hipGraphLaunch(m->graph, s));
    else if (lm_enqueue_step(m, mode, sp, rp, B, g.top_k)) return mia_fail(ctx, MIA_ERR_DEVICE, "%s: launch failed", g.name);
    if ((step & 15) == 15) {                               // after every 16th launched step: a finished sequence's further steps are no-ops
      if (const int rc = read_state()) return rc;
      bool all = true;
      for (int b = 0; b < B; ++b) all = all && st[b].finished;
      if (all) break;
    }
  }
  if (const int rc = read_state()) return rc;
  for (int b = 0; b < B; ++b) {
    const int n = g.embeds ? st[b].n_out : st[b].n_gen;
    const int32_t* src = g.embeds ? m->out_tokens + (size_t)b * C : m->tokens + (size_t)b * C + n_prompt(b);
    g.n_out[b] = n;
    if (n > 0) MIA_HIP(ctx, hipMemcpyAsync(g.out + (size_t)b * g.out_stride, src, (size_t)n * 4, hipMemcpyDeviceToHost, s));
  }
  MIA_HIP(ctx, hipStreamSynchronize(s));
  return MIA_OK;
}

}  // namespace

// prompt -> sampled continuation, all on device (OrpheusTTS.generateChunk's loop, OrpheusTTS.swift:245-348).
extern "C" int mia_lm_generate(mia_lm* m, const int32_t* prompt, int n_prompt, const mia_lm_sampler* sp, const float* uniforms,
                               int32_t* out_tokens, int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompt && n_prompt > 0 && sp && uniforms && out_tokens && n_out, "lm_generate: null arguments");
  MIA_CHECK_ARG(ctx, sp->max_new_tokens > 0 && n_prompt + sp->max_new_tokens <= m->cfg.max_ctx, "lm_generate: prompt + max_new_tokens exceeds max_ctx");
  MIA_CHECK_ARG(ctx, sp->rep_window >= 0 && sp->rep_window <= 64 && sp->n_stop >= 0 && sp->n_stop <= 4, "lm_generate: rep_window <= 64, n_stop <= 4");
  for (int i = 0; i < n_prompt; ++i) MIA_CHECK_ARG(ctx, prompt[i] >= 0 && prompt[i] < m->cfg.vocab, "lm_generate: token %d out of vocabulary", prompt[i]);
  const int32_t offsets[2] = {0, n_prompt};
  LmGenCall g{"lm_generate", 1, offsets};
  g.ids = prompt; g.sp = sp; g.uniforms = uniforms; g.n_uniforms = g.max_new = sp->max_new_tokens;
  g.pf_min_rows = PF_MIN_ROWS; g.out = out_tokens; g.n_out = n_out;
  return lm_generate_run(m, g);
}

// mia_lm_generate for n_seq independent prompts at once (sentence-level batching of OrpheusTTS.generate, OrpheusTTS.swift:179-191: the
// reference runs its sentences one after another).  prompts: the ids of all sequences back to back, prompt_offsets [n_seq + 1];
// uniforms [n_seq][max_new_tokens]; out_tokens [n_seq][max_new_tokens]; n_out [n_seq].  Sequence b's ids equal what mia_lm_generate
// returns for prompt b with uniforms row b (rows of a GEMM do not mix; asserted in tests/test_lm_gpu.py).
extern "C" int mia_lm_generate_batch(mia_lm* m, const int32_t* prompts, const int32_t* prompt_offsets, int n_seq, const mia_lm_sampler* sp,
                                     const float* uniforms, int32_t* out_tokens, int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompts && prompt_offsets && sp && uniforms && out_tokens && n_out, "lm_generate_batch: null arguments");
  MIA_CHECK_ARG(ctx, n_seq >= 1 && n_seq <= m->B_cap, "lm_generate_batch: n_seq %d exceeds the batch set with mia_lm_set_batch (%d)", n_seq, m->B_cap);
  MIA_CHECK_ARG(ctx, sp->max_new_tokens > 0 && sp->rep_window >= 0 && sp->rep_window <= 64 && sp->n_stop >= 0 && sp->n_stop <= 4, "lm_generate_batch: bad sampler");
  const int C = m->cfg.max_ctx, mn = sp->max_new_tokens;
  for (int b = 0; b < n_seq; ++b) {
    const int np_ = prompt_offsets[b + 1] - prompt_offsets[b];
    MIA_CHECK_ARG(ctx, np_ > 0 && np_ + mn <= C, "lm_generate_batch: prompt %d: length %d + max_new_tokens exceeds max_ctx", b, np_);
    for (int i = prompt_offsets[b]; i < prompt_offsets[b + 1]; ++i) MIA_CHECK_ARG(ctx, prompts[i] >= 0 && prompts[i] < m->cfg.vocab, "lm_generate_batch: token %d out of vocabulary", prompts[i]);
  }
  LmGenCall g{"lm_generate_batch", n_seq, prompt_offsets};
  g.ids = prompts; g.sp = sp; g.uniforms = uniforms; g.u_stride = g.n_uniforms = g.max_new = mn;
  g.out = out_tokens; g.out_stride = mn; g.n_out = n_out;
  return lm_generate_run(m, g);
}

// Qwen2LM.inference / inferenceLoop (TTS/CosyVoice2/LLM/Qwen2LM.swift:335-427) on device: prompt given as embedding rows
// [sos, text..., task, prompt speech...] (the caller gathers them from its three tables), generated ids embedded through
// speech_embedding, logits through llm_decoder, RAS sampling with explicit uniforms.
extern "C" int mia_lm_generate_ras(mia_lm* m, const float* prompt_embeds, int n_prompt, const mia_ras_params* rp, const float* uniforms, int n_uniforms,
                                   int32_t* out_tokens, int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompt_embeds && n_prompt > 0 && rp && uniforms && n_uniforms > 0 && out_tokens && n_out, "lm_generate_ras: null arguments");
  MIA_CHECK_ARG(ctx, m->gen_embed && m->head_vocab > 0, "lm_generate_ras: model has no speech_embedding / llm_decoder tensors");
  MIA_CHECK_ARG(ctx, rp->max_len > 0 && n_prompt + rp->max_len <= m->cfg.max_ctx, "lm_generate_ras: prompt + max_len exceeds max_ctx");
  MIA_CHECK_ARG(ctx, m->head_vocab <= LM_RAS_MAX_VOCAB && rp->top_k <= m->head_vocab, "lm_generate_ras: llm_decoder has %d rows; the RAS sampler holds at most %d", m->head_vocab, LM_RAS_MAX_VOCAB);
  MIA_CHECK_ARG(ctx, rp->top_k > 0 && rp->top_k <= 32 && rp->win >= 0 && rp->win <= 64 && rp->eos >= 0 && rp->eos < m->head_vocab, "lm_generate_ras: bad sampler parameters");
  const int32_t offsets[2] = {0, n_prompt};
  LmGenCall g{"lm_generate_ras", 1, offsets};
  g.embeds = prompt_embeds; g.ras = rp; g.uniforms = uniforms; g.n_uniforms = n_uniforms; g.max_new = rp->max_len;
  g.pf_min_rows = PF_MIN_ROWS; g.out = out_tokens; g.n_out = n_out;
  return lm_generate_run(m, g);
}

// mia_lm_generate_ras for n_seq utterances side by side (see mia_lm_generate_batch).  prompt_embeds: the rows of all prompts back to back
// [prompt_offsets[n_seq]][hidden]; rp [n_seq]: top_p / top_k / win / tau / eos must agree, min_len / max_len are per utterance;
// uniforms [n_seq][n_uniforms]; out_tokens [n_seq][out_stride] with out_stride >= max(max_len) + 1; n_out [n_seq].
extern "C" int mia_lm_generate_ras_batch(mia_lm* m, const float* prompt_embeds, const int32_t* prompt_offsets, int n_seq, const mia_ras_params* rp,
                                         const float* uniforms, int n_uniforms, int32_t* out_tokens, int out_stride, int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompt_embeds && prompt_offsets && rp && uniforms && n_uniforms > 0 && out_tokens && n_out, "lm_generate_ras_batch: null arguments");
  MIA_CHECK_ARG(ctx, n_seq >= 1 && n_seq <= m->B_cap, "lm_generate_ras_batch: n_seq %d exceeds the batch set with mia_lm_set_batch (%d)", n_seq, m->B_cap);
  MIA_CHECK_ARG(ctx, m->gen_embed && m->head_vocab > 0 && m->head_vocab <= LM_RAS_MAX_VOCAB, "lm_generate_ras_batch: model has no (or too large a) speech head");
  int max_len = 0;
  for (int b = 0; b < n_seq; ++b) {
    const int np_ = prompt_offsets[b + 1] - prompt_offsets[b];
    MIA_CHECK_ARG(ctx, np_ > 0 && rp[b].max_len > 0 && np_ + rp[b].max_len <= m->cfg.max_ctx, "lm_generate_ras_batch: utterance %d: prompt + max_len exceeds max_ctx", b);
    MIA_CHECK_ARG(ctx, rp[b].top_p == rp[0].top_p && rp[b].top_k == rp[0].top_k && rp[b].win == rp[0].win && rp[b].tau == rp[0].tau && rp[b].eos == rp[0].eos,
                  "lm_generate_ras_batch: top_p / top_k / win / tau / eos must be the same for all utterances");
    max_len = std::max(max_len, rp[b].max_len);
  }
  MIA_CHECK_ARG(ctx, rp[0].top_k > 0 && rp[0].top_k <= 32 && rp[0].top_k <= m->head_vocab && rp[0].win >= 0 && rp[0].win <= 64 && rp[0].eos >= 0 && rp[0].eos < m->head_vocab,
                "lm_generate_ras_batch: bad sampler parameters");
  MIA_CHECK_ARG(ctx, out_stride >= max_len + 1, "lm_generate_ras_batch: out_stride must hold max_len + 1 ids");
  LmGenCall g{"lm_generate_ras_batch", n_seq, prompt_offsets};
  g.embeds = prompt_embeds; g.ras = rp; g.uniforms = uniforms; g.u_stride = g.n_uniforms = n_uniforms; g.max_new = max_len;
  g.out = out_tokens; g.out_stride = out_stride; g.n_out = n_out;
  return lm_generate_run(m, g);
}

// ---- greedy decode from a prompt of embedding rows (Fun-ASR's decoder loop, STT/FunASR/FunASRSTT.swift:118-156) ----
namespace {

int lm_greedy_check(mia_lm* m, const char* name, const int32_t* stop_ids, int n_stop, int max_new_tokens, mia_lm_sampler* sp) {
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, !m->gen_embed && m->head_vocab == 0, "%s: the handle has speech_embedding / llm_decoder tensors (its loop is mia_lm_generate_ras)", name);
  MIA_CHECK_ARG(ctx, n_stop >= 1 && n_stop <= 4, "%s: n_stop must be 1..4 (got %d)", name, n_stop);
  MIA_CHECK_ARG(ctx, max_new_tokens > 0, "%s: max_new_tokens must be positive", name);
  *sp = mia_lm_sampler{};
  sp->n_stop = n_stop;
  for (int i = 0; i < n_stop; ++i) {
    MIA_CHECK_ARG(ctx, stop_ids[i] >= 0 && stop_ids[i] < m->cfg.vocab, "%s: stop id %d out of vocabulary", name, stop_ids[i]);
    sp->stop_ids[i] = stop_ids[i];
  }
  return MIA_OK;
}

}  // namespace

// The two greedy entries give a prompt of two or more rows to the batched prompt pass (pf_min_rows 1), alone or in a batch: sequence b of
// mia_lm_generate_greedy_batch goes through exactly the kernels of its single call.
extern "C" int mia_lm_generate_greedy(mia_lm* m, const float* prompt_embeds, int n_prompt, const int32_t* stop_ids, int n_stop, int max_new_tokens,
                                      int32_t* out_tokens, int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompt_embeds && stop_ids && out_tokens && n_out, "lm_generate_greedy: null arguments");
  mia_lm_sampler sp;
  if (const int rc = lm_greedy_check(m, "lm_generate_greedy", stop_ids, n_stop, max_new_tokens, &sp)) return rc;
  MIA_CHECK_ARG(ctx, n_prompt > 0 && n_prompt <= m->cfg.max_ctx - max_new_tokens, "lm_generate_greedy: prompt %d + max_new_tokens %d exceeds max_ctx %d", n_prompt, max_new_tokens, m->cfg.max_ctx);
  const int32_t offsets[2] = {0, n_prompt};
  LmGenCall g{"lm_generate_greedy", 1, offsets};
  g.embeds = prompt_embeds; g.sp = &sp; g.max_new = max_new_tokens; g.out = out_tokens; g.n_out = n_out;
  return lm_generate_run(m, g);
}

extern "C" int mia_lm_generate_greedy_batch(mia_lm* m, const float* prompt_embeds, const int32_t* prompt_offsets, int n_seq, const int32_t* stop_ids, int n_stop,
                                            int max_new_tokens, int32_t* out_tokens, int out_stride, int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompt_embeds && prompt_offsets && stop_ids && out_tokens && n_out, "lm_generate_greedy_batch: null arguments");
  MIA_CHECK_ARG(ctx, n_seq >= 1 && n_seq <= m->B_cap, "lm_generate_greedy_batch: n_seq %d exceeds the batch set with mia_lm_set_batch (%d)", n_seq, m->B_cap);
  mia_lm_sampler sp;
  if (const int rc = lm_greedy_check(m, "lm_generate_greedy_batch", stop_ids, n_stop, max_new_tokens, &sp)) return rc;
  MIA_CHECK_ARG(ctx, out_stride >= max_new_tokens, "lm_generate_greedy_batch: out_stride %d must hold max_new_tokens %d ids", out_stride, max_new_tokens);
  for (int b = 0; b < n_seq; ++b) {
    const int np_ = prompt_offsets[b + 1] - prompt_offsets[b];
    MIA_CHECK_ARG(ctx, np_ > 0 && np_ <= m->cfg.max_ctx - max_new_tokens, "lm_generate_greedy_batch: prompt %d: length %d + max_new_tokens exceeds max_ctx", b, np_);
  }
  LmGenCall g{"lm_generate_greedy_batch", n_seq, prompt_offsets};
  g.embeds = prompt_embeds; g.sp = &sp; g.max_new = max_new_tokens; g.out = out_tokens; g.out_stride = out_stride; g.n_out = n_out;
  return lm_generate_run(m, g);
}

// ---- the same loop with sampleNextToken's temperature > 0 branch (FunASRModel.swift:165-198; the rule is stated in mia.h) ----
namespace {

// the greedy checks plus the sampler's own; *k = the effective k
int lm_topk_check(mia_lm* m, const char* name, float temperature, int top_k, float top_p, const int32_t* stop_ids, int n_stop, int max_new_tokens, mia_lm_sampler* sp,
                  int* k) {
  mia_ctx* ctx = m->ctx;
  if (const int rc = lm_greedy_check(m, name, stop_ids, n_stop, max_new_tokens, sp)) return rc;
  MIA_CHECK_ARG(ctx, std::isfinite(temperature) && temperature > 0.f, "%s: temperature must be finite and positive (0 is mia_lm_generate_greedy)", name);
  MIA_CHECK_ARG(ctx, std::isfinite(top_p) && top_p > 0.f, "%s: top_p must be finite and positive", name);
  MIA_CHECK_ARG(ctx, top_k >= 0, "%s: top_k must not be negative (0 = the reference's 50)", name);
  *k = std::min(top_k > 0 ? top_k : 50, m->cfg.vocab);
  if (*k > LM_TOPK_MAX_K) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "%s: k %d exceeds %d", name, *k, LM_TOPK_MAX_K);
  sp->temperature = temperature; sp->top_p = top_p;
  return MIA_OK;
}

}  // namespace

extern "C" int mia_lm_generate_topk(mia_lm* m, const float* prompt_embeds, int n_prompt, float temperature, int top_k, float top_p, const int32_t* stop_ids, int n_stop,
                                    int max_new_tokens, const float* uniforms, int32_t* out_tokens, int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompt_embeds && stop_ids && uniforms && out_tokens && n_out, "lm_generate_topk: null arguments");
  mia_lm_sampler sp; int k = 0;
  if (const int rc = lm_topk_check(m, "lm_generate_topk", temperature, top_k, top_p, stop_ids, n_stop, max_new_tokens, &sp, &k)) return rc;
  MIA_CHECK_ARG(ctx, n_prompt > 0 && n_prompt <= m->cfg.max_ctx - max_new_tokens, "lm_generate_topk: prompt %d + max_new_tokens %d exceeds max_ctx %d", n_prompt, max_new_tokens, m->cfg.max_ctx);
  const int32_t offsets[2] = {0, n_prompt};
  LmGenCall g{"lm_generate_topk", 1, offsets};
  g.embeds = prompt_embeds; g.sp = &sp; g.top_k = k; g.uniforms = uniforms; g.n_uniforms = g.max_new = max_new_tokens; g.out = out_tokens; g.n_out = n_out;
  return lm_generate_run(m, g);
}

extern "C" int mia_lm_generate_topk_batch(mia_lm* m, const float* prompt_embeds, const int32_t* prompt_offsets, int n_seq, float temperature, int top_k, float top_p,
                                          const int32_t* stop_ids, int n_stop, int max_new_tokens, const float* uniforms, int32_t* out_tokens, int out_stride,
                                          int32_t* n_out) {
  if (!m) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = m->ctx;
  MIA_CHECK_ARG(ctx, prompt_embeds && prompt_offsets && stop_ids && uniforms && out_tokens && n_out, "lm_generate_topk_batch: null arguments");
  MIA_CHECK_ARG(ctx, n_seq >= 1 && n_seq <= m->B_cap, "lm_generate_topk_batch: n_seq %d exceeds the batch set with mia_lm_set_batch (%d)", n_seq, m->B_cap);
  mia_lm_sampler sp; int k = 0;
  if (const int rc = lm_topk_check(m, "lm_generate_topk_batch", temperature, top_k, top_p, stop_ids, n_stop, max_new_tokens, &sp, &k)) return rc;
  MIA_CHECK_ARG(ctx, out_stride >= max_new_tokens, "lm_generate_topk_batch: out_stride %d must hold max_new_tokens %d ids", out_stride, max_new_tokens);
  for (int b = 0; b < n_seq; ++b) {
    const int np_ = prompt_offsets[b + 1] - prompt_offsets[b];
    MIA_CHECK_ARG(ctx, np_ > 0 && np_ <= m->cfg.max_ctx - max_new_tokens, "lm_generate_topk_batch: prompt %d: length %d + max_new_tokens exceeds max_ctx", b, np_);
  }
  LmGenCall g{"lm_generate_topk_batch", n_seq, prompt_offsets};
  g.embeds = prompt_embeds; g.sp = &sp; g.top_k = k; g.uniforms = uniforms; g.u_stride = g.n_uniforms = g.max_new = max_new_tokens;
  g.out = out_tokens; g.out_stride = out_stride; g.n_out = n_out;
  return lm_generate_run(m, g);
}
