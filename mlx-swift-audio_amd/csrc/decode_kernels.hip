// decode_kernels.hip -- the per-token kernels of the batched Whisper greedy decoder (gfx950).
//
// Replaces, per step, TextDecoder.callAsFunction (STT/Whisper/Layers/TextDecoder.swift:53-96), the decoder half of
// ResidualAttentionBlock (ResidualAttentionBlock.swift:51-95), WhisperMultiHeadAttention with KV cache
// (MultiHeadAttention.swift:40-135) and the logit rules + argmax of GreedyDecoder.decode
// (STT/Whisper/WhisperDecoding.swift:186-358).  All state (position, tokens, rule state, log-prob sums) lives in
// HBM, every kernel reads the position from DecState, so one captured hipGraph replays for every step and the
// host never synchronises per token (the reference does >= 4 .item() syncs per token).
//
// Roofline: a decode step is HBM-bound -- weights are streamed once (skinny MFMA GEMM, M <= 32 rows), the
// cross-attention K/V of every clip is streamed once (dec_attention).
#include <cstdlib>

#include <type_traits>
#include "decode.h"

// ------------------------------------------------------------------------------------------------
// Row kernels of the decode step: one 256-thread workgroup per clip, the row (D <= 2048 floats) lives in
// registers as float4, statistics via wave shuffles + one LDS hop.
// ------------------------------------------------------------------------------------------------
constexpr int ROW_NV = 2;   // float4 per thread: D <= 256 * 4 * ROW_NV

// h is written in activation FRAGMENT order (skinny.h): the row is the A operand of the step's next skinny GEMM
template <typename T>
__device__ __forceinline__ void row_layernorm_store(const f32x4 (&v)[ROW_NV], int nv, int D, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, uint16_t* __restrict__ h, int row, float* sh) {
  const int tid = threadIdx.x;
  // gamma / beta do not depend on the statistics: fetch them first, so their L2 round trip overlaps the two block reductions
  f32x4 gm[ROW_NV], bt[ROW_NV];
#pragma unroll
  for (int i = 0; i < ROW_NV; ++i) {
    const bool in = tid + 256 * i < nv;
    gm[i] = in ? *reinterpret_cast<const f32x4*>(gamma + 4 * (tid + 256 * i)) : (f32x4){0.f, 0.f, 0.f, 0.f};
    bt[i] = in ? *reinterpret_cast<const f32x4*>(beta + 4 * (tid + 256 * i)) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < ROW_NV; ++i) if (tid + 256 * i < nv) s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  const float mean = block256_sum(s, sh) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < ROW_NV; ++i)
    if (tid + 256 * i < nv) {
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float d = v[i][j] - mean; q += d * d; }
    }
  const float rstd = rsqrtf(block256_sum(q, sh) / (float)D + 1e-5f);
#pragma unroll
  for (int i = 0; i < ROW_NV; ++i) {
    const int c = tid + 256 * i;
    if (c >= nv) continue;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[i][j] - mean) * rstd * gm[i][j] + bt[i][j];
    *reinterpret_cast<u32x2*>(h + afrag_index(row, 4 * c, D)) = (u32x2){pack2<T>(o[0], o[1]), pack2<T>(o[2], o[3])};
  }
}

// x[b] = E[token[b][pos]] + P[pos];  h[b] = LN(x[b])          (TextDecoder.swift:67 + first attn_ln)
template <typename T>
__global__ __launch_bounds__(256) void dec_embed_ln(const int32_t* __restrict__ tokens, const uint16_t* __restrict__ emb,
                                                    const float* __restrict__ pos_emb, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ x,
                                                    uint16_t* __restrict__ h, const int32_t* __restrict__ pos_arr, int D, int n_ctx) {
  __shared__ float sh[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int pos = pos_arr[b];
  const int tok = tokens[b * n_ctx + pos];
  const uint16_t* e = emb + (int64_t)tok * D;
  const float* p = pos_emb + (int64_t)pos * D;
  float* xr = x + (int64_t)b * D;
  const int nv = D >> 2;
  f32x4 v[ROW_NV];
#pragma unroll
  for (int i = 0; i < ROW_NV; ++i) {
    const int c = tid + 256 * i;
    if (c < nv) {
      const s16x4 ev = *reinterpret_cast<const s16x4*>(e + 4 * c);
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = T::to_f32((uint16_t)ev[j]) + pv[j];
      *reinterpret_cast<f32x4*>(xr + 4 * c) = v[i];
    } else v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  row_layernorm_store<T>(v, nv, D, gamma, beta, h, b, sh);
}

// x[b] += bias + sum_s partial[s][b];  h[b] = LN(x[b])        (residual add + next LayerNorm, fixed-order split-K sum)
// (A one-wave-per-row form -- no LDS hop, no barrier, the statistics as plain DPP wave reductions -- was measured: 1.6 us SLOWER per
// launch; a single wave issuing the row's 30-40 loads takes longer than four waves with two barriers.)
template <typename T>
__global__ __launch_bounds__(256) void dec_reduce_ln(const float* __restrict__ partial, int S, int B, const float* __restrict__ bias,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float* __restrict__ x, uint16_t* __restrict__ h, int D) {
  __shared__ float sh[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  float* xr = x + (int64_t)b * D;
  const int nv = D >> 2;
  f32x4 v[ROW_NV];
#pragma unroll
  for (int i = 0; i < ROW_NV; ++i) {
    const int c = tid + 256 * i;
    if (c < nv) {
      f32x4 a = *reinterpret_cast<const f32x4*>(xr + 4 * c);
      const f32x4 bs = *reinterpret_cast<const f32x4*>(bias + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += bs[j];
      // split-K slices come from other XCDs (L2 misses): issue every load before the first add.  S <= 4; a slot k >= S
      // re-reads slice S-1 and is dropped, so the loads are unconditional and the sum keeps its fixed order.
      f32x4 pv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) pv[k] = *reinterpret_cast<const f32x4*>(partial + ((int64_t)(k < S ? k : S - 1) * B + b) * D + 4 * c);
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < S) {
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] += pv[k][j];
        }
      v[i] = a;
      *reinterpret_cast<f32x4*>(xr + 4 * c) = a;
    } else v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  row_layernorm_store<T>(v, nv, D, gamma, beta, h, b, sh);
}

// ------------------------------------------------------------------------------------------------
// Single-query attention against a head-major K/V cache: one workgroup per (head, clip).
// 8 lanes share a key (16 B each, fully coalesced 1 KB per wave instruction); fp32 softmax.
// n_keys = pos[clip] + 1 (self attention) or the constant T (cross attention).
// ------------------------------------------------------------------------------------------------
constexpr int DEC_MAX_KEYS = 1536;

// U = independent 1 KB loads a wave keeps in flight per trip (8 U keys); NTL = non-temporal K/V loads (the cross K/V of a step is
// 1 GB read once: keep it from displacing the step's weights and activations in L2 / MALL)
template <typename T, int U, bool NTL>
__global__ __launch_bounds__(256) void dec_attention(const uint16_t* __restrict__ q, const uint16_t* __restrict__ kc,
                                                     const uint16_t* __restrict__ vc, uint16_t* __restrict__ out,
                                                     const int32_t* __restrict__ pos_arr, int fixed_keys, int cap_keys, int H,
                                                     float scale, float* __restrict__ qk_out, const int32_t* __restrict__ head_slot,
                                                     int n_slots, int qk_ctx) {
  __shared__ float sc[DEC_MAX_KEYS];
  __shared__ float red[4][64];
  __shared__ float red2[8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int h = blockIdx.x, b = blockIdx.y;
  const int D = H * 64;
  const int nk = fixed_keys > 0 ? fixed_keys : pos_arr[b] + 1;
  const int c = lane & 7, g = lane >> 3;
  const uint16_t* kb = kc + ((int64_t)b * H + h) * cap_keys * 64;
  const uint16_t* vb = vc + ((int64_t)b * H + h) * cap_keys * 64;
  float qf[8];
  {
    const s16x8 qv = *reinterpret_cast<const s16x8*>(q + (int64_t)b * D + h * 64 + c * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[j] = T::to_f32((uint16_t)qv[j]);
  }
  // K / V of this (clip, head) as buffer resources: 16-byte loads at 32-bit offsets (no 64-bit address arithmetic per load), the cache
  // policy in the instruction's aux immediate (2 = non-temporal)
  const __amdgpu_buffer_rsrc_t rk = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(kb), (short)0, cap_keys * 128, 0x00020000);
  const __amdgpu_buffer_rsrc_t rv = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(vb), (short)0, cap_keys * 128, 0x00020000);
  auto load_trip = [&](s16x8 (&dst)[U], const __amdgpu_buffer_rsrc_t& base, int k0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int key = k0 + 8 * u + g; key = key < nk ? key : nk - 1;
      dst[u] = __builtin_bit_cast(s16x8, __builtin_amdgcn_raw_buffer_load_b128(base, key * 128 + c * 16, 0, NTL ? 2 : 0));
    }
  };
  constexpr int TRIP = 32 * U;   // keys per workgroup trip; a wave owns 8 U consecutive keys of it
  // ---- scores: the next trip's U independent 1 KB loads are issued before the current trip's dot products (U .. 2U loads in flight)
  {
    int k0 = wave * (8 * U);
    s16x8 kv[U], kn[U];
    if (k0 < nk) load_trip(kv, rk, k0);
    for (; k0 < nk; k0 += TRIP) {
      const bool more = k0 + TRIP < nk;
      if (more) load_trip(kn, rk, k0 + TRIP);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += qf[j] * T::to_f32((uint16_t)kv[u][j]);
        dot += dpp_xor1(dot);            // 8-lane all-reduce on DPP (the lanes of a key): no LDS-crossbar round trips in the K loop
        dot += dpp_xor2(dot);
        dot += dpp_half_mirror(dot);
        const int key = k0 + 8 * u + g;
        if (c == 0 && key < nk) sc[key] = dot * scale;
      }
      if (more) {
#pragma unroll
        for (int u = 0; u < U; ++u) kv[u] = kn[u];
      }
    }
  }
  // the first V trip does not depend on the probabilities: its loads fly during the softmax
  s16x8 vv[U], vn[U];
  if (wave * (8 * U) < nk) load_trip(vv, rv, wave * (8 * U));
  __syncthreads();
  // word-timestamp alignment (WhisperTiming.swift:605-640): keep the pre-softmax scores of the alignment heads, row = decoder position
  if (qk_out && head_slot[h] >= 0) {
    float* dst = qk_out + (((int64_t)b * n_slots + head_slot[h]) * qk_ctx + pos_arr[b]) * nk;
    for (int i = tid; i < nk; i += 256) dst[i] = sc[i];
  }
  // ---- softmax over sc[0..nk)
  float m = -INFINITY;
  for (int i = tid; i < nk; i += 256) m = fmaxf(m, sc[i]);
  m = wave_max(m);
  if (lane == 0) red2[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red2[0], red2[1]), fmaxf(red2[2], red2[3]));
  float sum = 0.f;
  for (int i = tid; i < nk; i += 256) { const float p = __expf(sc[i] - m); sc[i] = p; sum += p; }
  sum = wave_sum(sum);
  if (lane == 0) red2[4 + wave] = sum;
  __syncthreads();
  sum = (red2[4] + red2[5]) + (red2[6] + red2[7]);
  // ---- out = P V
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int k0 = wave * (8 * U); k0 < nk; k0 += TRIP) {
    const bool more = k0 + TRIP < nk;
    if (more) load_trip(vn, rv, k0 + TRIP);
    float pw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = k0 + 8 * u + g;
      pw[u] = key < nk ? sc[key] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += pw[u] * T::to_f32((uint16_t)vv[u][j]);
    if (more) {
#pragma unroll
      for (int u = 0; u < U; ++u) vv[u] = vn[u];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    acc[j] += dpp_xor8(acc[j]);
    acc[j] += __shfl_xor(acc[j], 16, 64);
    acc[j] += __shfl_xor(acc[j], 32, 64);
  }
  if (g == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wave][c * 8 + j] = acc[j];
  }
  __syncthreads();
  if (tid < 64) {
    const float o = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) / sum;
    out[afrag_index(b, h * 64 + tid, D)] = T::from_f32(o);   // fragment order: the A operand of the output projection
  }
}

// ------------------------------------------------------------------------------------------------
// Decode head: logit rules + argmax + log-prob bookkeeping (WhisperDecoding.swift:158-169,186-358), all reductions in fp32; each
// clip advances its own position.  The rules exist once (head_rule, head_masked, head_reduce, head_decide, head_commit) and are
// shared by the one-workgroup head (dec_head: sampling, and the test reference of the split form) and the split greedy head
// (dec_head_partial + dec_head_final).
// ------------------------------------------------------------------------------------------------
struct HeadBufs {
  const float* logits;          // [B][V]
  int32_t* tokens;              // [B][n_ctx]
  int32_t* n_gen;               // [B]
  int32_t* finished;            // [B]
  int32_t* last_ts;             // [B] last generated token value > timestamp_begin (0 = none)
  float* sum_logprob;           // [B]
  int32_t* n_logprob;           // [B]
  float* no_speech;             // [B]
  const uint32_t* suppress;     // [2][nw]
  const float* uniforms;        // [B][n_ctx] explicit RNG for temperature > 0 (one value per generated token)
  DecClip clip;
};

constexpr int HEAD_NPT = 52;   // logits per thread held in registers: V <= 1024 * 52
struct ArgMax { float v; int i; };
__device__ __forceinline__ ArgMax amax(ArgMax a, ArgMax b) {   // larger value wins, lowest index wins ties (MLX argMax)
  return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ ArgMax wave_amax(ArgMax a) {
  // rows of 16 on DPP, then the four row winners as scalars (amax is associative and commutative: any order gives the same pair)
#define AMAX_STEP(CTRL) { const ArgMax b{dpp_f32<CTRL>(a.v), dpp_i32<CTRL>(a.i)}; a = amax(a, b); }
  AMAX_STEP(0xB1) AMAX_STEP(0x4E) AMAX_STEP(0x141) AMAX_STEP(0x140)
#undef AMAX_STEP
  ArgMax r = ArgMax{lane_f32(a.v, 0), __builtin_amdgcn_readlane(a.i, 0)};
  r = amax(r, ArgMax{lane_f32(a.v, 16), __builtin_amdgcn_readlane(a.i, 16)});
  r = amax(r, ArgMax{lane_f32(a.v, 32), __builtin_amdgcn_readlane(a.i, 32)});
  r = amax(r, ArgMax{lane_f32(a.v, 48), __builtin_amdgcn_readlane(a.i, 48)});
  return r;
}

// ---- rule state of clip b at this step (WhisperDecoding.swift:221-292)
struct HeadRule {
  bool active;                  // false: a finished clip (idles at its last position) or a forced token that wants no probe (just advances)
  bool decide;                  // past the forced prefix: a token is chosen
  bool heuristic, sup_ts_all, sup_text_below_eot, sup_below_tsb;
  int ts_floor;                 // suppress tsb <= idx < ts_floor
  int max_first;                // suppress idx > max_first (first token only)
  int num_gen, cur_len;         // num_gen == loop iteration of the reference
};
__device__ __forceinline__ HeadRule head_rule(const HeadBufs& hb, const DecodeParams& p, int b) {
  HeadRule r{};
  const int pos = hb.clip.pos[b], n_initial = hb.clip.n_init[b], sot_index = hb.clip.sot_idx[b];
  r.cur_len = pos + 1;
  const bool generating = r.cur_len >= n_initial;
  r.active = !(generating && hb.finished[b]) && (generating || pos == sot_index);
  r.decide = generating;
  r.num_gen = r.cur_len - n_initial;
  r.max_first = p.V;
  if (r.active && r.decide && p.timestamps) {
    const int32_t* toks = hb.tokens + (int64_t)b * p.n_ctx;
    const int tsb = p.timestamp_begin;
    const int last = toks[r.cur_len - 1];
    const bool last_was_ts = r.num_gen >= 1 && last >= tsb;
    const bool penult_was_ts = r.num_gen < 2 || toks[r.cur_len - 2] >= tsb;
    if (last_was_ts) { if (penult_was_ts) r.sup_ts_all = true; else r.sup_text_below_eot = true; }
    const int lt = hb.last_ts[b];
    if (lt > 0) r.ts_floor = penult_was_ts ? lt + 1 : lt;
    if (r.num_gen == 0) {
      r.sup_below_tsb = true;
      const int last_allowed = tsb + p.max_initial_ts;
      if (last_allowed < p.V) r.max_first = last_allowed;
    }
    r.heuristic = r.num_gen > 0;
  }
  return r;
}

// is vocabulary index i suppressed under the rules alone (hypothesis A)?  bits = the suppress bitmap of this step
__device__ __forceinline__ bool head_masked(const HeadRule& r, const DecodeParams& p, const uint32_t* bits, int i) {
  const int tsb = p.timestamp_begin;
  if ((bits[i >> 5] >> (i & 31)) & 1u) return true;
  if (p.timestamps) {
    if (i == p.no_timestamps) return true;
    if (r.sup_ts_all && i >= tsb) return true;
    if (r.sup_text_below_eot && i < p.eot) return true;
    if (i >= tsb && i < r.ts_floor) return true;
    if (r.sup_below_tsb && i < tsb) return true;
    if (i > r.max_first) return true;
  }
  return false;
}

// what a slice of the vocabulary reduces to: maxima, the argmax candidates A = rules only and B = rules + "text suppressed", and the
// exp-sums, each taken relative to this slice's own maximum of its kind
struct HeadPart { float mx_text, mx_ts, s_all, s_ts, bAv, bBv, fA, fB; int bAi, bBi; };
constexpr int HEAD_NONE = 0x7fffffff;          // argmax index of an empty candidate set
template <int NPT> using HeadKept = std::conditional_t<(NPT > 32), unsigned long long, unsigned>;

// the slice's logits, read ONCE into registers with all loads in flight together: thread tid holds indices base + tid + NTH u
template <int NTH, int NPT>
__device__ __forceinline__ void head_load(float (&x)[NPT], const float* lg, int base, int V) {
#pragma unroll
  for (int u = 0; u < NPT; ++u) { const int i = base + (int)threadIdx.x + NTH * u; x[u] = i < V ? lg[i] : -INFINITY; }
}

// A workgroup of NTH threads reduces the NTH * NPT logits from `base` on: pass 1 = every max / argmax, pass 2 = every exp-sum.
// Sums are fixed-order: per thread in u order, wave_sum, then the waves added in wave order from LDS.  okA: bit u = element u is kept
// under the rules (hypothesis A).  Every thread returns the whole record.
template <int NTH, int NPT>
__device__ __forceinline__ HeadPart head_reduce(const float (&x)[NPT], int base, const HeadRule& r, const HeadBufs& hb, const DecodeParams& p,
                                                HeadKept<NPT>& okA) {
  constexpr int NWV = NTH / 64;
  __shared__ float shf[NWV][4];
  __shared__ float sha[NWV][2];
  __shared__ int shai[NWV][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = p.V, tsb = p.timestamp_begin;
  const uint32_t* bits = hb.suppress + (r.num_gen == 0 ? (V + 31) / 32 : 0);
  // ---- pass 1: maxima
  float mx_text = -INFINITY, mx_ts = -INFINITY;
  ArgMax bA{-INFINITY, HEAD_NONE}, bB{-INFINITY, HEAD_NONE};
  okA = 0;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int i = base + tid + NTH * u;
    if (i >= V) continue;
    if (i >= tsb) mx_ts = fmaxf(mx_ts, x[u]); else mx_text = fmaxf(mx_text, x[u]);
    if (r.decide && !head_masked(r, p, bits, i)) {
      okA |= (HeadKept<NPT>)1 << u;
      bA = amax(bA, ArgMax{x[u], i});
      if (i >= tsb) bB = amax(bB, ArgMax{x[u], i});
    }
  }
  mx_text = wave_max(mx_text); mx_ts = wave_max(mx_ts);
  bA = wave_amax(bA); bB = wave_amax(bB);
  if (lane == 0) { shf[wave][0] = mx_text; shf[wave][1] = mx_ts; sha[wave][0] = bA.v; shai[wave][0] = bA.i; sha[wave][1] = bB.v; shai[wave][1] = bB.i; }
  __syncthreads();
  mx_text = shf[0][0]; mx_ts = shf[0][1]; bA = ArgMax{sha[0][0], shai[0][0]}; bB = ArgMax{sha[0][1], shai[0][1]};
  for (int w2 = 1; w2 < NWV; ++w2) {
    mx_text = fmaxf(mx_text, shf[w2][0]); mx_ts = fmaxf(mx_ts, shf[w2][1]);
    bA = amax(bA, ArgMax{sha[w2][0], shai[w2][0]}); bB = amax(bB, ArgMax{sha[w2][1], shai[w2][1]});
  }
  const float mx_all = fmaxf(mx_text, mx_ts);
  __syncthreads();
  // ---- pass 2: exp-sums (registers)
  float s_all = 0.f, s_ts = 0.f, fA = 0.f, fB = 0.f;
#pragma unroll
  for (int u = 0; u < NPT; ++u) {
    const int i = base + tid + NTH * u;
    if (i >= V) continue;
    s_all += __expf(x[u] - mx_all);
    if (r.heuristic && i >= tsb) s_ts += __expf(x[u] - mx_ts);
    if ((okA >> u) & 1) {
      fA += __expf(x[u] - bA.v);
      if (r.heuristic && i >= tsb) fB += __expf(x[u] - bB.v);
    }
  }
  s_all = wave_sum(s_all); s_ts = wave_sum(s_ts); fA = wave_sum(fA); fB = wave_sum(fB);
  if (lane == 0) { shf[wave][0] = s_all; shf[wave][1] = s_ts; shf[wave][2] = fA; shf[wave][3] = fB; }
  __syncthreads();
  s_all = s_ts = fA = fB = 0.f;
  for (int w2 = 0; w2 < NWV; ++w2) { s_all += shf[w2][0]; s_ts += shf[w2][1]; fA += shf[w2][2]; fB += shf[w2][3]; }
  return HeadPart{mx_text, mx_ts, s_all, s_ts, bA.v, bB.v, fA, fB, bA.i, bB.i};
}

// The timestamp heuristic (:299-322) decides between the two precomputed candidates of the clip's whole-vocabulary record:
// ts_lse = (max_ts - lse) + log(sum_ts exp(x - max_ts)) against the best text log-prob.
struct HeadPick { float lse; bool useB, all_masked; ArgMax best; float fsum; int next; };
__device__ __forceinline__ HeadPick head_decide(const HeadRule& r, const HeadPart& m) {
  HeadPick k;
  k.lse = fmaxf(m.mx_text, m.mx_ts) + __logf(m.s_all);
  k.useB = false;
  if (r.heuristic) {
    const float ts_lse = (m.mx_ts - k.lse) + __logf(m.s_ts);
    const float max_text = m.mx_text - k.lse;
    k.useB = ts_lse > max_text;                       // force a timestamp: text tokens suppressed too
  }
  k.best = k.useB ? ArgMax{m.bBv, m.bBi} : ArgMax{m.bAv, m.bAi};
  k.fsum = k.useB ? m.fB : m.fA;
  // Everything masked: reachable in the reference when the raw-logit timestamp heuristic fires right after a
  // timestamp pair rule; MLX argMax of an all -inf vector is index 0 and log(softmax) is NaN.  Mirror that.
  k.all_masked = k.best.i == HEAD_NONE;
  k.next = k.all_masked ? 0 : k.best.i;
  return k;
}

// One thread per clip, when the token consumed is <|startoftranscript|>: softmax(logits[sot])[no_speech] (:158-169)
__device__ __forceinline__ void head_probe(const HeadBufs& hb, const DecodeParams& p, int b, const HeadRule& r, float lse) {
  if (r.active && r.cur_len - 1 == hb.clip.sot_idx[b]) hb.no_speech[b] = __expf(hb.logits[(int64_t)b * p.V + p.no_speech] - lse);
}

// One thread per clip: the chosen token `next` (k.next, or what sampling drew in its place) goes into the clip's state.  Returns the
// clip's new position, or -1 if it does not advance (finished).
__device__ __forceinline__ int head_commit(const HeadBufs& hb, const DecodeParams& p, int b, const HeadRule& r, const HeadPick& k, int next) {
  const int pos = r.cur_len - 1, n_initial = r.cur_len - r.num_gen;
  int newpos = -1;
  if (!r.decide) newpos = pos + 1;                    // forced token (probed or not): just advance
  else if (r.active) {                                // (a finished clip idles at its last position)
    if (next != p.eot) {                              // EOT excluded from avg_logprob (:345-350)
      hb.sum_logprob[b] += k.all_masked ? __int_as_float(0x7fc00000) : (hb.logits[(int64_t)b * p.V + next] - k.best.v) - __logf(k.fsum);
      hb.n_logprob[b] += 1;
    }
    hb.tokens[(int64_t)b * p.n_ctx + r.cur_len] = next;
    hb.n_gen[b] = r.num_gen + 1;
    if (next > p.timestamp_begin) hb.last_ts[b] = next;               // strict '>' (:254-256)
    int cap = p.max_tokens - n_initial;
    if (p.max_new_tokens > 0 && p.max_new_tokens < cap) cap = p.max_new_tokens;
    if (next == p.eot || r.num_gen + 1 >= cap) hb.finished[b] = 1;
    else newpos = pos + 1;
  }
  if (newpos >= 0) hb.clip.pos[b] = newpos;
  return newpos;
}

// One workgroup per clip.  The clip's logits are read once into registers (52 per thread, V <= 53248) and reduced by head_reduce.
// temperature > 0: inverse-CDF sampling of softmax(filtered / T) with the caller's uniform (sampleFromDistribution, :395-410: first
// index whose cumsum >= r).
__global__ __launch_bounds__(1024) void dec_head(HeadBufs hb, DecodeParams p) {
  __shared__ float seg[HEAD_NPT * 16];
  __shared__ int s_pick[2];
  __shared__ float s_val[2];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const HeadRule r = head_rule(hb, p, b);
  if (!r.active) {
    if (tid == 0) head_commit(hb, p, b, r, HeadPick{}, 0);
    return;
  }
  const int tsb = p.timestamp_begin;
  float x[HEAD_NPT];
  head_load<1024, HEAD_NPT>(x, hb.logits + (int64_t)b * p.V, 0, p.V);
  HeadKept<HEAD_NPT> okA;
  const HeadPart m = head_reduce<1024, HEAD_NPT>(x, 0, r, hb, p, okA);
  const HeadPick k = head_decide(r, m);
  if (tid == 0) head_probe(hb, p, b, r, k.lse);
  int next = k.next;
  const float temperature = hb.clip.temp[b];
  if (r.decide && temperature > 0.0f && !k.all_masked) {
    // ---- sampling: p_i ~ exp((x_i - max) / T) over the kept set, first index whose cumulative sum >= r * total
    const float inv_t = 1.0f / temperature;
    auto weight = [&](int u) -> float {
      const int i = tid + 1024 * u;
      const bool kept = ((okA >> u) & 1ull) && (!k.useB || i >= tsb);
      return kept ? __expf((x[u] - k.best.v) * inv_t) : 0.f;
    };
#pragma unroll
    for (int u = 0; u < HEAD_NPT; ++u) {
      const float ssum = wave_sum(weight(u));         // segment (u, wave) covers indices [1024u + 64*wave, +64): index-ordered
      if (lane == 0) seg[u * 16 + wave] = ssum;
    }
    __syncthreads();
    if (tid == 0) {
      float total = 0.f;
      for (int j = 0; j < HEAD_NPT * 16; ++j) total += seg[j];
      const float rnd = hb.uniforms[(int64_t)b * p.n_ctx + r.num_gen];
      const float goal = rnd * total;
      float cum = 0.f; int sel = -1;
      for (int j = 0; j < HEAD_NPT * 16; ++j) {
        if (seg[j] > 0.f && cum + seg[j] >= goal) { sel = j; break; }
        cum += seg[j];
      }
      if (sel < 0) { for (int j = HEAD_NPT * 16 - 1; j >= 0; --j) if (seg[j] > 0.f) { sel = j; break; } cum -= 0.f; }
      s_pick[0] = sel; s_val[0] = cum; s_val[1] = goal;
    }
    __syncthreads();
    const int sel = s_pick[0];
    if (sel >= 0 && wave == (sel & 15)) {
      const int u_sel = sel >> 4;
      float mine = 0.f;
#pragma unroll
      for (int u = 0; u < HEAD_NPT; ++u) if (u == u_sel) mine = weight(u);
      float incl = mine;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
      const unsigned long long hit = __ballot(mine > 0.f && s_val[0] + incl >= s_val[1]);
      const unsigned long long any = __ballot(mine > 0.f);
      int ln = hit ? __ffsll((long long)hit) - 1 : 63 - __clzll((long long)any);   // rounding corner: last kept lane of the segment
      if (lane == 0) s_pick[1] = 1024 * u_sel + 64 * wave + ln;
    }
    __syncthreads();
    if (sel >= 0) next = s_pick[1];
  }
  if (tid == 0) head_commit(hb, p, b, r, k, next);
}

// ------------------------------------------------------------------------------------------------
// Greedy (temperature 0) head split over HEAD_SPLIT workgroups per clip: one workgroup per clip left 224 of the 256 CUs idle while
// 32 of them chewed 52 k logits each (46 us per step).  Phase 1 reduces a 1/HEAD_SPLIT slice of the vocabulary to a HeadPart record;
// phase 2 rescales and merges the records in slice order and applies the decision logic of dec_head (head_decide, head_commit).
// Sampling (temperature > 0) keeps the single-workgroup kernel.
// ------------------------------------------------------------------------------------------------
constexpr int HEAD_SPLIT = 32;   // <= 64: dec_head_final merges one record per lane
constexpr int HEAD_NPT2 = 7;       // logits per thread: 256 threads * 7 * 32 slices >= V

__global__ __launch_bounds__(256) void dec_head_partial(HeadBufs hb, DecodeParams p, HeadPart* __restrict__ parts) {
  const int k = blockIdx.x, b = blockIdx.y;
  // the slice's logits do not depend on the clip's rule state: their loads go out first, so the rule's chain of small dependent
  // loads (position -> generated count -> last tokens) runs in their shadow instead of ahead of them
  const int base = k * (256 * HEAD_NPT2);
  float x[HEAD_NPT2];
  head_load<256, HEAD_NPT2>(x, hb.logits + (int64_t)b * p.V, base, p.V);
  const HeadRule r = head_rule(hb, p, b);
  if (!r.active) return;
  HeadKept<HEAD_NPT2> okA;
  const HeadPart part = head_reduce<256, HEAD_NPT2>(x, base, r, hb, p, okA);
  if (threadIdx.x == 0) parts[b * HEAD_SPLIT + k] = part;
}

// merge the slice records in slice order (deterministic), decide, update the clip's state (same tail as dec_head); then, if the clip
// advanced, embed the token of the NEW position and apply the first LayerNorm of the next step (replaces that step's dec_embed_ln launch)
struct NextEmbed { const uint16_t* emb; const float* pos_emb; const float* gamma; const float* beta; float* x; uint16_t* h; int D; };

template <typename T>
__global__ __launch_bounds__(256) void dec_head_final(HeadBufs hb, DecodeParams p, const HeadPart* __restrict__ parts, NextEmbed ne) {
  __shared__ int s_newpos;
  __shared__ float sh[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  // wave 0 merges the clip's slice records, one per lane: maxima by butterfly, then the exp-sums rescaled to the merged maxima
  // (fixed butterfly order: deterministic)
  float mx_text = -INFINITY, mx_ts = -INFINITY, s_all = 0.f, s_ts = 0.f, fA = 0.f, fB = 0.f;
  ArgMax bA{-INFINITY, HEAD_NONE}, bB{-INFINITY, HEAD_NONE};
  const HeadRule r = head_rule(hb, p, b);
  if (tid < 64 && r.active) {
    HeadPart me{-INFINITY, -INFINITY, 0.f, 0.f, -INFINITY, -INFINITY, 0.f, 0.f, HEAD_NONE, HEAD_NONE};
    if (tid < HEAD_SPLIT) me = parts[b * HEAD_SPLIT + tid];
    mx_text = wave_max(me.mx_text); mx_ts = wave_max(me.mx_ts);
    bA = wave_amax(ArgMax{me.bAv, me.bAi}); bB = wave_amax(ArgMax{me.bBv, me.bBi});
    const float mx_all = fmaxf(mx_text, mx_ts);
    const float ml = fmaxf(me.mx_text, me.mx_ts);
    s_all = wave_sum(ml > -INFINITY ? me.s_all * __expf(ml - mx_all) : 0.f);
    s_ts = wave_sum(me.mx_ts > -INFINITY ? me.s_ts * __expf(me.mx_ts - mx_ts) : 0.f);
    fA = wave_sum(me.bAv > -INFINITY ? me.fA * __expf(me.bAv - bA.v) : 0.f);
    fB = wave_sum(me.bBv > -INFINITY ? me.fB * __expf(me.bBv - bB.v) : 0.f);
  }
  if (tid == 0) {
    const HeadPick k = head_decide(r, HeadPart{mx_text, mx_ts, s_all, s_ts, bA.v, bB.v, fA, fB, bA.i, bB.i});
    head_probe(hb, p, b, r, k.lse);
    s_newpos = head_commit(hb, p, b, r, k, k.next);
  }
  __syncthreads();
  const int np_ = s_newpos;
  if (np_ < 0 || np_ >= p.n_ctx) return;
  // ---- x[b] = E[token[b][np]] + P[np];  h[b] = LN(x[b])   (the next step's TextDecoder.swift:67 + first attn_ln)
  const int D = ne.D, nv = D >> 2;
  const int tok = hb.tokens[(int64_t)b * p.n_ctx + np_];
  const uint16_t* e = ne.emb + (int64_t)tok * D;
  const float* pe = ne.pos_emb + (int64_t)np_ * D;
  float* xr = ne.x + (int64_t)b * D;
  f32x4 v[ROW_NV];
#pragma unroll
  for (int i = 0; i < ROW_NV; ++i) {
    const int c = tid + 256 * i;
    if (c < nv) {
      const s16x4 ev = *reinterpret_cast<const s16x4*>(e + 4 * c);
      const f32x4 pv = *reinterpret_cast<const f32x4*>(pe + 4 * c);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[i][j] = T::to_f32((uint16_t)ev[j]) + pv[j];
      *reinterpret_cast<f32x4*>(xr + 4 * c) = v[i];
    } else v[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  row_layernorm_store<T>(v, nv, D, ne.gamma, ne.beta, ne.h, b, sh);
}

// compact outputs: generated tokens with EOT (and anything after) stripped; avg_logprob
__global__ void dec_finalize(const int32_t* __restrict__ tokens, const int32_t* __restrict__ n_gen,
                             const float* __restrict__ sum_lp, const int32_t* __restrict__ n_lp, int32_t* __restrict__ out_tokens,
                             int32_t* __restrict__ out_n, float* __restrict__ out_avg, const int32_t* __restrict__ n_init, DecodeParams p) {
  const int b = blockIdx.x;
  const int32_t* t = tokens + (int64_t)b * p.n_ctx + n_init[b];
  __shared__ int n_keep;
  if (threadIdx.x == 0) {
    int n = n_gen[b];
    for (int i = 0; i < n; ++i) if (t[i] == p.eot) { n = i; break; }
    n_keep = n;
    out_n[b] = n;
    out_avg[b] = n_lp[b] > 0 ? sum_lp[b] / (float)n_lp[b] : 0.0f;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < p.max_tokens; i += blockDim.x) out_tokens[(int64_t)b * p.max_tokens + i] = i < n_keep ? t[i] : 0;
}

// ------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------
int dec_launch_embed_ln(mia_whisper* w, const LNW& ln, hipStream_t s) {
  const int D = w->dims.n_text_state;
  if (w->dtype == MIA_F16)
    hipLaunchKernelGGL(dec_embed_ln<F16>, dim3(w->cur_B), dim3(256), 0, s, w->tokens, (const uint16_t*)w->tok_emb, w->dec_pos, ln.g, ln.b, w->dx, (uint16_t*)w->dh, w->clip.pos, D, w->dims.n_text_ctx);
  else
    hipLaunchKernelGGL(dec_embed_ln<BF16>, dim3(w->cur_B), dim3(256), 0, s, w->tokens, (const uint16_t*)w->tok_emb, w->dec_pos, ln.g, ln.b, w->dx, (uint16_t*)w->dh, w->clip.pos, D, w->dims.n_text_ctx);
  return 0;
}

int dec_launch_reduce_ln(mia_whisper* w, int S, const float* bias, const LNW& ln, hipStream_t s) {
  const int D = w->dims.n_text_state;
  if (w->dtype == MIA_F16)
    hipLaunchKernelGGL(dec_reduce_ln<F16>, dim3(w->cur_B), dim3(256), 0, s, w->partial, S, w->cur_B, bias, ln.g, ln.b, w->dx, (uint16_t*)w->dh, D);
  else
    hipLaunchKernelGGL(dec_reduce_ln<BF16>, dim3(w->cur_B), dim3(256), 0, s, w->partial, S, w->cur_B, bias, ln.g, ln.b, w->dx, (uint16_t*)w->dh, D);
  return 0;
}

int dec_launch_attention(mia_whisper* w, const void* q, const void* kc, const void* vc, void* out, int fixed_keys, int cap_keys,
                         hipStream_t s, float* qk_out, const int32_t* head_slot, int n_slots, int qk_ctx, bool self_nt) {
  if (cap_keys > DEC_MAX_KEYS) return -1;
  dim3 grid(w->dims.n_text_head, w->cur_B), block(256);
#define ATT(T_, U_, NTL_)                                                                                                            \
  hipLaunchKernelGGL((dec_attention<T_, U_, NTL_>), grid, block, 0, s, (const uint16_t*)q, (const uint16_t*)kc, (const uint16_t*)vc,   \
                     (uint16_t*)out, w->clip.pos, fixed_keys, cap_keys, w->dims.n_text_head, 0.125f, qk_out, head_slot, n_slots, qk_ctx)
  // cross attention (fixed_keys = the 1500 encoder positions): bandwidth-bound streaming of 2 x 192 KB per (clip, head), non-temporal;
  // self attention: at most n_text_ctx cached keys, latency-bound.  (U = 8 was measured: 10 us per step SLOWER than U = 4.)
  // (self K/V: each cached byte is read once per step, 0.66 MB x position; non-temporal when the step keeps its layer weights resident,
  //  whisper_decode.hip: dec_cache_policy)
  const bool nt = fixed_keys > 0 || self_nt;
  if (w->dtype == MIA_F16) { if (nt) ATT(F16, 4, true); else ATT(F16, 4, false); }
  else { if (nt) ATT(BF16, 4, true); else ATT(BF16, 4, false); }
#undef ATT
  return 0;
}

// true when the greedy head runs as partial + final kernels; the final kernel then also embeds the next position, so the step graph
// carries no dec_embed_ln of its own (the caller launches it once before the first step)
bool dec_head_is_split(const DecodeParams& p) {
  return p.greedy && !p.head_single && p.V <= 256 * HEAD_NPT2 * HEAD_SPLIT;
}

// test hook (mia_whisper_trace_logits): the raw logits the head is about to read, for the traced clips, filed under the position of
// the token this step consumed.  Runs inside the captured step graph, so what is traced is what the graph computed.
__global__ __launch_bounds__(256) void dec_trace_logits(const float* __restrict__ logits, const int32_t* __restrict__ pos, const int32_t* __restrict__ clips,
                                                        float* __restrict__ trace, int V, int n_ctx) {
  const int slot = blockIdx.y, b = clips[slot];
  const int p = pos[b];
  if (p < 0 || p >= n_ctx) return;
  const float* src = logits + (int64_t)b * V;
  float* dst = trace + ((int64_t)slot * n_ctx + p) * V;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < V; i += gridDim.x * 256) dst[i] = src[i];
}

int dec_launch_trace(mia_whisper* w, hipStream_t s) {
  if (!w->trace || w->trace_n <= 0) return -1;
  hipLaunchKernelGGL(dec_trace_logits, dim3(32, w->trace_n), dim3(256), 0, s, w->logits, w->clip.pos, w->trace_clips, w->trace, w->dims.n_vocab, w->dims.n_text_ctx);
  return 0;
}

int dec_launch_head(mia_whisper* w, int32_t* last_ts, const DecodeParams& p, hipStream_t s) {
  if (p.V > 1024 * HEAD_NPT) return -1;
  HeadBufs hb{w->logits, w->tokens, w->n_gen, w->finished, last_ts, w->sum_logprob, w->n_logprob, w->no_speech, w->suppress_bits, w->uniforms, w->clip};
  if (dec_head_is_split(p)) {
    // argmax path: the vocabulary is reduced by HEAD_SPLIT workgroups per clip, then merged (w->partial is free at this point of the step)
    HeadPart* parts = reinterpret_cast<HeadPart*>(w->partial);
    hipLaunchKernelGGL(dec_head_partial, dim3(HEAD_SPLIT, w->cur_B), dim3(256), 0, s, hb, p, parts);
    const LNW& ln0 = w->dec[0].attn_ln;
    NextEmbed ne{(const uint16_t*)w->tok_emb, w->dec_pos, ln0.g, ln0.b, w->dx, (uint16_t*)w->dh, w->dims.n_text_state};
    if (w->dtype == MIA_F16) hipLaunchKernelGGL(dec_head_final<F16>, dim3(w->cur_B), dim3(256), 0, s, hb, p, (const HeadPart*)parts, ne);
    else hipLaunchKernelGGL(dec_head_final<BF16>, dim3(w->cur_B), dim3(256), 0, s, hb, p, (const HeadPart*)parts, ne);
    return 0;
  }
  hipLaunchKernelGGL(dec_head, dim3(w->cur_B), dim3(1024), 0, s, hb, p);
  return 0;
}

int dec_launch_finalize(mia_whisper* w, int32_t* out_n, const DecodeParams& p, hipStream_t s) {
  hipLaunchKernelGGL(dec_finalize, dim3(w->cur_B), dim3(256), 0, s, w->tokens, w->n_gen, w->sum_logprob, w->n_logprob, w->out_tokens, out_n, w->out_avg, w->clip.n_init, p);
  return 0;
}
