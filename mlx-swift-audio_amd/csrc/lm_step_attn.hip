// lm_step_attn.hip -- the LM decode step's attention on the 16-bit KV cache, split over the keys and shared across a KV group: head dim
// 64 / 128, bf16 / f16, Q K^T and P V on v_mfma_f32_16x16x32, fp32 softmax, gfx950.  Serves lm_launch_attention (lm.hip) when
// mia_lm_set_step_attention(lm, 1) is set; it replaces lm_attention<.., FUSED = true>, which runs one workgroup per (query head,
// sequence), each walking its head's whole cache on the vector pipe with max_ctx scores in LDS.
//
// lm_step_attn_split: grid (Hkv, nb, ceil(max_ctx / 256)), 256 threads.  A workgroup owns SLICE `s` = keys [256 s, 256 s + 256) of one KV
// head of one sequence and attends for all G = Hq / Hkv <= 16 query heads of the group at once.  It reads st[seq].pos on the device and
// returns, writing nothing, when the sequence is frozen or the slice starts beyond pos; the slices are anchored at key 0, so what a
// workgroup computes depends on (sequence state, KV head, slice) only -- not on the batch, the capacity or graph versus direct launch.
//   * preamble (every live workgroup): the step's q rows of the G heads from the q|k|v GEMM's split-K slices -- sum of S <= 4 partials,
//     bias, optional per-head RMSNorm, RoPE, one 16-bit rounding: lm_attention's fused preamble, operation for operation -- into LDS as
//     the 16-bit rows [16][DH] (rows >= G zero).  The workgroup whose slice holds pos also finishes the new K / V row, is its only
//     writer to the cache, and uses the row from LDS; every other live workgroup reads cached keys only.
//   * the four waves own 64 keys each, as four 16-key MFMA tiles.  S = K Q^T: the K tile [16 keys][32 of dh] is the row-major A operand,
//     loaded cache -> registers (16 B per lane), the q rows are the B operand (lane & 15 = head).  Tile t feeds MFMA row m with key
//     32 (t >> 1) + 8 (m >> 2) + 4 (t & 1) + (m & 3) of the wave, so that the accumulators of tiles (2 u, 2 u + 1) are, register for
//     register, keys 8 (lane >> 4) + 0..7 of k-step u: the B operand P^T of O^T += V^T P^T in natural key order, no shuffle.
//   * softmax over the wave's 64 keys per head in fp32 (in-lane over 16 scores, xor 16 / 32 across the lane groups), keys > pos at -inf;
//     P is rounded to the 16-bit type (as in lm_prefill_attn.hip) and the rounding's remainder is carried: p = P0 + P1 + P2, each the
//     16-bit rounding of what the terms before it left, three MFMAs on the same V^T fragment (gemm_tap's three-way split).  A step's
//     attention row then differs from lm_attention's (fp32 P on the vector pipe) by fp32 rounding, so a 16-bit element of it flips about
//     once in 4 000 instead of every second time -- which is what keeps the two modes' logits inside the 0.02 sigma the prompt pass is
//     held to (measured: P0 alone 0.027 sigma, P0 + P1 0.022).  The sum l is of the unrounded p.
//   * V^T [DH][32 keys] per wave and k-step is staged cache -> registers -> LDS, transposed in the write (a lane packs a key pair into
//     one dword); 64-B rows, 16-B chunk index XOR ((d >> 2) ^ (d >> 4)) & 3: the 16 rows of one ds_read_b128 quarter-wave land in 16
//     distinct bank groups and the four dh chunks of one ds_write_b32 in four.  Rows past pos are staged as zeros.
//   * the waves' (m, l, acc) are merged through LDS in wave order (the staging buffer is reused) and the workgroup writes one fp32
//     partial (m, l, acc[DH]) per head to ws [seq][head][slice][DH + 2]; m is in the base-2 domain (raw maximum x dh^-0.5 log2 e).
// LDS: 16 x DH x 2 (q) + 2 x DH x 2 (new row) + 4 x DH x 64 (V^T / merge) + 512 bytes -- 37 888 at DH 128, 19 200 at DH 64, independent of the context.
//
// lm_step_attn_combine: grid (Hq, nb), DH threads.  Reads the (pos >> 8) + 1 live partials of its head in ascending slice order, rescales
// each by exp2(m_s - m), sums, divides and writes the 16-bit attention row.  No atomics, no workgroup waits on another, the order is
// fixed: a repeat returns the same bits.
#include "lm.h"
#include "mia_device.h"

namespace {

constexpr int SLICE = LM_STEP_SLICE;
constexpr int WAVE_KEYS = 64;

template <typename T, int DH, bool QKN>
__global__ __launch_bounds__(256) void lm_step_attn_split(LmStepAttn a, float scale_log2) {
  constexpr int half = DH / 2;
  constexpr int KS = DH / 32;                     // k-steps of S = K Q^T
  constexpr int DB = DH / 16;                     // 16-channel blocks of O^T
  constexpr int CH = DH / 8;                      // 16-B chunks per cache row
  constexpr int VT_BYTES = DH * 64;               // one wave's V^T [DH][32 keys]; later its merge rows [16 heads][DH] fp32 -- the same size
  __shared__ __attribute__((aligned(16))) uint16_t q16[16 * DH];
  __shared__ __attribute__((aligned(16))) uint16_t kn16[DH];
  __shared__ __attribute__((aligned(16))) uint16_t vn16[DH];
  __shared__ __attribute__((aligned(16))) char stage[4 * VT_BYTES];
  __shared__ float ml[4][16][2];

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
  const int64_t head_off = ((int64_t)seq * a.Hkv + kvh) * a.max_ctx * DH;
  uint16_t* Kg = a.kc + head_off;
  uint16_t* Vg = a.vc + head_off;

  // ---- preamble: lm_attention's, for the G query heads of the group (and, in the writer, the new K / V row)
  auto val = [&](int n) {                         // S <= 4 slices [S][nb][N], loads issued together
    float pv[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) pv[k] = a.part[((int64_t)(k < a.S ? k : a.S - 1) * a.nb + seq) * N + n];
    float r = a.bias ? a.bias[n] : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < a.S) r += pv[k];
    return r;
  };
  // one rotation pair (i, i + half) of the row that starts at `base`; on: the lane has a pair (every lane of the wave runs the shuffles)
  auto rope_pair = [&](int base, int i, bool on, const float* w, uint16_t& r0, uint16_t& r1) {
    float x0 = on ? val(base + i) : 0.f, x1 = on ? val(base + i + half) : 0.f;
    if constexpr (QKN) {
      float ss = x0 * x0 + x1 * x1;
#pragma unroll
      for (int o = 1; o < half; o <<= 1) ss += __shfl_xor(ss, o, 64);
      const float rstd = rsqrtf(ss / (float)DH + a.qk_eps);
      x0 = x0 * rstd * w[i]; x1 = x1 * rstd * w[i + half];
    }
    float sn, cs;
    sincosf((float)pos * a.inv_freq[i], &sn, &cs);
    r0 = T::from_f32(x0 * cs - x1 * sn); r1 = T::from_f32(x1 * cs + x0 * sn);
  };
  const int n_qpairs = G * half;                  // a multiple of half: a head's pairs are `half` consecutive, aligned lanes
  for (int e0 = 0; e0 < n_qpairs; e0 += 256) {
    const int e = e0 + tid, hl = e / half, i = e - hl * half;
    const bool on = e < n_qpairs;
    uint16_t r0, r1;
    rope_pair((kvh * G + hl) * DH, i, on, a.qkn, r0, r1);
    if (on) { q16[hl * DH + i] = r0; q16[hl * DH + i + half] = r1; }
  }
  for (int e = G * DH + tid; e < 16 * DH; e += 256) q16[e] = 0;
  if (writer) {
    if (wave == 0) {                              // the k pairs: lanes 0 .. half - 1
      const bool on = lane < half;
      const int i = on ? lane : lane - half;
      uint16_t r0, r1;
      rope_pair(Nq + kvh * DH, i, on, QKN ? a.qkn + DH : nullptr, r0, r1);
      if (on) {
        kn16[i] = r0; kn16[i + half] = r1;
        uint16_t* k = Kg + (int64_t)pos * DH;
        k[i] = r0; k[i + half] = r1;
      }
    } else if (tid - 64 < DH) {
      const int d = tid - 64;
      const uint16_t r = T::from_f32(val(Nq + Nk + kvh * DH + d));
      vn16[d] = r;
      Vg[(int64_t)pos * DH + d] = r;
    }
  }
  __syncthreads();

  const int g = lane >> 4, lr = lane & 15;
  const int k0w = k0s + WAVE_KEYS * wave;
  const bool live = k0w <= pos;                   // wave-uniform; the live waves are 0 .. n_live - 1
  const int last_cached = pos > 0 ? pos - 1 : 0;  // loads are clamped to it: nothing at or past pos (and so past max_ctx) is read from the cache

  f32x4 sacc[4];
  f32x4 oacc[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) oacc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  s16x8 pf[2][3];                                 // P^T of the two k-steps: the rounded p and the two roundings of what it left
  float m2 = -INFINITY, lsum = 0.f;

  // V rows of k-step u: lane -> key pair p = lane & 15 and chunks c = (lane >> 4) + 4 i
  u32x4 rv[CH / 4][2];
  auto load_v = [&](int u) {
#pragma unroll
    for (int i = 0; i < CH / 4; ++i)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = k0w + 32 * u + 2 * lr + e, c = g + 4 * i;
        u32x4 v = *reinterpret_cast<const u32x4*>(Vg + (int64_t)min(key, last_cached) * DH + 8 * c);
        if (key == pos) v = *reinterpret_cast<const u32x4*>(vn16 + 8 * c);
        if (key > pos) v = (u32x4){0u, 0u, 0u, 0u};
        rv[i][e] = v;
      }
  };
  char* vt = stage + wave * VT_BYTES;
  auto vswz = [](int d) { return ((d >> 2) ^ (d >> 4)) & 3; };
  auto stage_v = [&]() {
#pragma unroll
    for (int i = 0; i < CH / 4; ++i)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int d = 8 * (g + 4 * i) + j;
        const uint32_t lo = rv[i][0][j >> 1], hi = rv[i][1][j >> 1];
        const uint32_t w = (j & 1) ? (lo >> 16) | (hi & 0xffff0000u) : (lo & 0xffffu) | (hi << 16);
        *reinterpret_cast<uint32_t*>(vt + d * 64 + (((lr >> 2) ^ vswz(d)) << 4) + (lr & 3) * 4) = w;
      }
  };
  auto pv_step = [&](int u) {
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const int d = 16 * db + lr;
      const s16x8 vf = *reinterpret_cast<const s16x8*>(vt + d * 64 + ((g ^ vswz(d)) << 4));
#pragma unroll
      for (int term = 2; term >= 0; --term) oacc[db] = T::mfma16(vf, pf[u][term], oacc[db]);      // small terms first
    }
  };

  if (live) {
    // ---- S = K Q^T: MFMA row lr of tile t is key k0w + krow(t), accumulator register r of lane group g is key k0w + 32 (t >> 1) + 8 g + 4 (t & 1) + r
    s16x8 kf[4][KS];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = k0w + 32 * (t >> 1) + 8 * (lr >> 2) + 4 * (t & 1) + (lr & 3);
      const uint16_t* kp = Kg + (int64_t)min(key, last_cached) * DH + 8 * g;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        kf[t][kk] = *reinterpret_cast<const s16x8*>(kp + 32 * kk);
        if (key == pos) kf[t][kk] = *reinterpret_cast<const s16x8*>(kn16 + 32 * kk + 8 * g);
      }
    }
    load_v(0);
    s16x8 qf[KS];
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) qf[kk] = *reinterpret_cast<const s16x8*>(q16 + lr * DH + 32 * kk + 8 * g);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      sacc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) sacc[t] = T::mfma16(kf[t][kk], qf[kk], sacc[t]);
    }
    // ---- softmax of head lr over the wave's 64 keys (raw scores; p = exp2((s - m) c), c = dh^-0.5 log2 e)
    float mraw = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (k0w + 32 * (t >> 1) + 8 * g + 4 * (t & 1) + r > pos) sacc[t][r] = -INFINITY;
        mraw = fmaxf(mraw, sacc[t][r]);
      }
    mraw = fmaxf(mraw, __shfl_xor(mraw, 16, 64));
    mraw = fmaxf(mraw, __shfl_xor(mraw, 32, 64));    // finite: key k0w <= pos is in every head's row
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      float p[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        p[j] = __builtin_amdgcn_exp2f((sacc[2 * u + (j >> 2)][j & 3] - mraw) * scale_log2);
        lsum += p[j];
      }
#pragma unroll
      for (int term = 0; term < 3; ++term) {
        u32x4 w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          w[j] = pack2<T>(p[2 * j], p[2 * j + 1]);
          p[2 * j] -= T::to_f32((uint16_t)(w[j] & 0xffffu)); p[2 * j + 1] -= T::to_f32((uint16_t)(w[j] >> 16));      // exact: the remainder
        }
        pf[u][term] = __builtin_bit_cast(s16x8, w);
      }
    }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
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
    if (g == 0) { ml[wave][lr][0] = m2; ml[wave][lr][1] = lsum; }
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
      o += reinterpret_cast<const float*>(stage + w * VT_BYTES)[hl * DH + d] * f;
    }
    float* dst = a.ws + (((int64_t)seq * a.Hq + kvh * G + hl) * n_slices + slice) * (DH + 2);
    if (d == 0) { dst[0] = m; dst[1] = l; }
    dst[2 + d] = o;
  }
}

template <typename T, int DH>
__global__ __launch_bounds__(DH) void lm_step_attn_combine(LmStepAttn a) {
  const int seq = blockIdx.y, h = blockIdx.x, d = threadIdx.x;
  const LmState* st = a.st + seq;
  if (st->frozen) return;
  const int pos = st->pos;
  if (pos < 0 || pos >= a.max_ctx) return;
  const int n_live = (pos >> 8) + 1, n_slices = (a.max_ctx + SLICE - 1) / SLICE;
  const float* src = a.ws + ((int64_t)seq * a.Hq + h) * n_slices * (DH + 2);
  float m = src[0];
  for (int s = 1; s < n_live; ++s) m = fmaxf(m, src[(int64_t)s * (DH + 2)]);
  float l = 0.f, o = 0.f;
#pragma unroll 4
  for (int s = 0; s < n_live; ++s) {
    const float* p = src + (int64_t)s * (DH + 2);
    const float f = __builtin_amdgcn_exp2f(p[0] - m);
    l += p[1] * f;
    o += p[2 + d] * f;
  }
  a.out[((int64_t)seq * a.Hq + h) * DH + d] = T::from_f32(o / l);
}

}  // namespace

const char* lm_step_attn_check(int Hq, int Hkv, int dh) {
  if (dh != 64 && dh != 128) return "head_dim must be 64 or 128";
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv) return "n_heads must be a positive multiple of n_kv_heads";
  if (Hq / Hkv > LM_STEP_MAX_GROUP) return "at most 16 query heads per KV head (the columns of one 16x16x32 MFMA)";
  return nullptr;
}

// the second launch alone, for lm_step_attn_kvq.hip: its split kernel writes the same partials
int lm_step_attn_combine_launch(const LmStepAttn& a, hipStream_t s) {
  if (lm_step_attn_check(a.Hq, a.Hkv, a.dh) || !a.out || !a.ws || !a.st || a.nb <= 0 || a.max_ctx <= 0) return -1;
  const dim3 cgrid(a.Hq, a.nb);
#define SA_C(TT) do { if (a.dh == 128) hipLaunchKernelGGL((lm_step_attn_combine<TT, 128>), cgrid, dim3(128), 0, s, a); \
                      else hipLaunchKernelGGL((lm_step_attn_combine<TT, 64>), cgrid, dim3(64), 0, s, a); } while (0)
  if (a.dtype == MIA_F16) SA_C(F16); else SA_C(BF16);
#undef SA_C
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int lm_step_attn_launch(const LmStepAttn& a, hipStream_t s) {
  if (lm_step_attn_check(a.Hq, a.Hkv, a.dh) || !a.kc || !a.vc || !a.out || !a.ws || !a.st || !a.part || !a.inv_freq || a.S < 1 || a.S > 4 || a.nb <= 0 || a.max_ctx <= 0)
    return -1;
  const dim3 grid(a.Hkv, a.nb, lm_step_attn_slices(a.max_ctx)), cgrid(a.Hq, a.nb);
  const float scale_log2 = 1.4426950408889634f / sqrtf((float)a.dh);
#define SA_GO(TT, DD, NN) do { hipLaunchKernelGGL((lm_step_attn_split<TT, DD, NN>), grid, dim3(256), 0, s, a, scale_log2); \
                               hipLaunchKernelGGL((lm_step_attn_combine<TT, DD>), cgrid, dim3(DD), 0, s, a); } while (0)
#define SA_N(TT, DD) do { if (a.qkn) SA_GO(TT, DD, true); else SA_GO(TT, DD, false); } while (0)
  if (a.dtype == MIA_F16) { if (a.dh == 128) SA_N(F16, 128); else SA_N(F16, 64); }
  else                    { if (a.dh == 128) SA_N(BF16, 128); else SA_N(BF16, 64); }
#undef SA_N
#undef SA_GO
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
