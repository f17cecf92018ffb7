// skinny_device.h -- device-side pieces shared by the skinny GEMM sources (skinny_rowmajor.hip, skinny_quant.hip, skinny_frag.hip):
// cross-wave reduction, the rstd prologue, the prefetched vector epilogue and the buffer-resource loads.
#pragma once
#include <type_traits>

#include "gemm.h"
#include "mia_device.h"
#include "skinny.h"

// fixed-order cross-wave sum of the NW waves' K-slices: waves 1.. park their fragments in LDS, wave 0 adds them in wave order and
// is the only one to return true (it owns the epilogue)
template <int NT, int NW>
__device__ __forceinline__ bool skinny_wave_reduce(f32x4 (&acc)[NT][2], int wave, int lane) {
  if (NW == 1) return true;
  __shared__ f32x4 red[(NW > 1 ? NW - 1 : 1) * NT * 2 * 64];
  if (wave > 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) red[(((wave - 1) * NT + t) * 2 + mt) * 64 + lane] = acc[t][mt];
  }
  __syncthreads();
  if (wave > 0) return false;
#pragma unroll
  for (int w2 = 1; w2 < NW; ++w2)
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const f32x4 o = red[(((w2 - 1) * NT + t) * 2 + mt) * 64 + lane];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][mt][j] += o[j];
      }
  return true;
}

// rstd of the (up to 32) rows of this workgroup from the producer's per-tile partial sums of squares (SkinnyArgs::ss_in): computed by
// wave 0 at the START of the kernel -- its loads ride under the weight stream -- into LDS; the epilogue (wave 0 again, behind the
// reduction barrier when the workgroup has one) reads rs[row].  Lanes take tiles t = lane, lane + 64, ...; fixed-order sums.
__device__ __forceinline__ void skinny_rstd_prepare(const SkinnyArgs& a, float* rs, int m0, int wave, int lane) {
  if (!a.ss_in || wave != 0) return;
  // (the LM step uses this form with at most 4 rows -- lm.hip:lm_enqueue_step keeps the unfused chain for wider batches -- so a row at a time is fine:
  // all of a row's loads are issued together, one wave reduction per row)
  const int rows = a.M - m0 < 32 ? a.M - m0 : 32;
  for (int j = 0; j < rows; ++j) {
    float p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { const int t = lane + 64 * u; p[u] = t < a.ss_tiles ? a.ss_in[(int64_t)t * a.M + m0 + j] : 0.f; }   // tiles <= 512
    float v = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
    v = wave_sum(v);
    if (lane == 0) rs[j] = rsqrtf(v / (float)a.ss_dim + a.eps) * a.rs_scale;
  }
}

// The epilogue's small dependent loads (the lane's 4 bias values per tile, the cache position of its two rows) are issued by
// skinny_prefetch at the START of the kernel, next to the operand loads: fetched in the epilogue they added an L2 round trip to every
// biased GEMM of the chain, after the reduction barrier where nothing hides it.
template <int NT>
struct SkinnyPre { float bs[NT][4]; int pos[2]; float c1[NT][4], c2[NT][4]; };

template <int MODE, int NT>
__device__ __forceinline__ SkinnyPre<NT> skinny_prefetch(const SkinnyArgs& a, int n0, int m0, int lane) {
  SkinnyPre<NT> p;
  const int r = lane & 15, c = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + 4 * c;
#pragma unroll
    for (int j = 0; j < 4; ++j) p.bs[t][j] = (MODE != SK_PARTIAL && a.bias && n + j < a.N) ? a.bias[n + j] : 0.f;
    // LayerNorm fold constants of a consumer (SkinnyArgs::c1 / c2): one 16-byte load each (n is a multiple of 4, the arrays hipMalloc'ed)
    if (a.c1 && n + 3 < a.N) {
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(a.c1 + n), v2 = *reinterpret_cast<const f32x4*>(a.c2 + n);
#pragma unroll
      for (int j = 0; j < 4; ++j) { p.c1[t][j] = v1[j]; p.c2[t][j] = v2[j]; }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = a.c1 && n + j < a.N;
        p.c1[t][j] = in ? a.c1[n + j] : 0.f;
        p.c2[t][j] = in ? a.c2[n + j] : 0.f;
      }
    }
  }
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) {
    const int m = m0 + mt * 16 + r;
    p.pos[mt] = (MODE == SK_QKV && m < a.M) ? a.pos[m] : 0;
  }
  return p;
}

template <typename T, int MODE, int NT>
__device__ __forceinline__ void skinny_epilogue_v(const SkinnyArgs& a, const f32x4 (&acc)[NT][2], const SkinnyPre<NT>& pre, int n0, int m0, int split,
                                                  int lane, const float* st = nullptr) {
  static_assert(MODE != SK_SWIGLU, "SK_SWIGLU is stored by skinny_store");
  const int r = lane & 15, c = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int n = n0 + 16 * t + 4 * c;
    if (n >= a.N) continue;
    const bool full = n + 3 < a.N;
    const float (&bs)[4] = pre.bs[t];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int m = m0 + mt * 16 + r;
      if (m >= a.M) continue;
      f32x4 v = acc[t][mt];
      if (a.c1 && st) {      // the activation was x * gamma (SK_RESID producer): LN(x) W^T = rstd (acc - mean c1) + c2
        const float mean = st[2 * (mt * 16 + r)], rstd = st[2 * (mt * 16 + r) + 1];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = rstd * (v[j] - mean * pre.c1[t][j]) + pre.c2[t][j];
      }
      if (MODE == SK_PARTIAL) {
        float* dst = reinterpret_cast<float*>(a.out) + ((int64_t)split * a.M + m) * a.N + n;
        if (full && (a.N & 3) == 0) *reinterpret_cast<f32x4*>(dst) = v;
        else { for (int j = 0; j < 4; ++j) if (n + j < a.N) dst[j] = v[j]; }
        continue;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] += bs[j]; if (a.act == MIA_ACT_GELU) v[j] = gelu_erf(v[j]); }
      if (MODE == SK_OUTF32) {
        float* dst = reinterpret_cast<float*>(a.out) + (int64_t)m * a.ldo + n;
        if (full && (a.ldo & 1) == 0) {
          *reinterpret_cast<f32x2*>(dst) = (f32x2){v[0], v[1]};
          *reinterpret_cast<f32x2*>(dst + 2) = (f32x2){v[2], v[3]};
        } else { for (int j = 0; j < 4; ++j) if (n + j < a.N) dst[j] = v[j]; }
        continue;
      }
      const u32x2 pk = (u32x2){pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3])};
      uint16_t* o16 = reinterpret_cast<uint16_t*>(a.out);
      if (MODE == SK_OUT16) {
        if (a.out_frag) { *reinterpret_cast<u32x2*>(o16 + afrag_index(m, n, a.N)) = pk; continue; }   // host-checked: N % 16 == 0
        uint16_t* dst = o16 + (int64_t)m * a.ldo + n;
        if (full && (a.ldo & 3) == 0) *reinterpret_cast<u32x2*>(dst) = pk;
        else { for (int j = 0; j < 4; ++j) if (n + j < a.N) dst[j] = T::from_f32(v[j]); }
        continue;
      }
      // SK_QKV (host-checked: D % 64 == 0, N == 3 D): [0,D) -> q row-major, [D,2D) -> self K cache, [2D,3D) -> self V cache at pos[m]
      if (n < a.D) { *reinterpret_cast<u32x2*>(o16 + (int64_t)m * a.ldo + n) = pk; continue; }
      const int hd = (n - a.D) % a.D, h = hd >> 6, d = hd & 63;
      uint16_t* cache = n < 2 * a.D ? a.cache_k : a.cache_v;
      *reinterpret_cast<u32x2*>(cache + (((int64_t)m * a.H + h) * a.n_ctx + pre.pos[mt]) * 64 + d) = pk;
    }
  }
}

// Row-major-activation kernels (the LM step): the same vector stores.  SK_SWIGLU: a lane's 4 consecutive columns are (gate, up, gate, up)
// -> two outputs, one 4-byte store.
template <typename T, int MODE, int NT>
__device__ __forceinline__ void skinny_store(const SkinnyArgs& a, f32x4 (&acc)[NT][2], int n0, int m0, int split, int lane, const float* rs = nullptr) {
  const int r = lane & 15, c = lane >> 4;
  if (a.ss_in && rs) {       // the activation was stored un-normalised (SK_RESID producer): scale every row by its rstd first
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      const int mr = mt * 16 + r;
      const float sc = m0 + mr < a.M ? rs[mr] : 0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][mt][j] *= sc;
    }
  }
  if constexpr (MODE == SK_RESID) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = n0 + 16 * t + 4 * c;                 // host-checked: N % 16 == 0
      const f32x4 wv = *reinterpret_cast<const f32x4*>(a.nw + n);
      f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (a.bias) bv = *reinterpret_cast<const f32x4*>(a.bias + n);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + mt * 16 + r;
        float q = 0.f;
        if (m < a.M) {
          float* xp = a.xres + (int64_t)m * a.N + n;
          f32x4 x = *reinterpret_cast<const f32x4*>(xp);
#pragma unroll
          for (int j = 0; j < 4; ++j) { x[j] += acc[t][mt][j] + bv[j]; q += x[j] * x[j]; }
          *reinterpret_cast<f32x4*>(xp) = x;
          *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(a.out) + (int64_t)m * a.ldo + n) = (u32x2){pack2<T>(x[0] * wv[0], x[1] * wv[1]), pack2<T>(x[2] * wv[2], x[3] * wv[3])};
        }
        // the tile's 16 columns live in the 4 lanes r, r + 16, r + 32, r + 48: fixed-order sum (c = 0, 1, 2, 3)
        const float q1 = __shfl(q, r + 16, 64), q2 = __shfl(q, r + 32, 64), q3 = __shfl(q, r + 48, 64);
        if (c == 0 && m < a.M) a.ss_out[(int64_t)((n0 >> 4) + t) * a.M + m] = ((q + q1) + q2) + q3;
      }
    }
  } else if constexpr (MODE == SK_SWIGLU) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int n = n0 + 16 * t + 4 * c;
      if (n >= a.N) continue;
      float bs[4] = {0.f, 0.f, 0.f, 0.f};
      if (a.bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (n + j < a.N) bs[j] = a.bias[n + j];
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) {
        const int m = m0 + mt * 16 + r;
        if (m >= a.M) continue;
        float o[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float v = acc[t][mt][2 * q] + bs[2 * q], u = acc[t][mt][2 * q + 1] + bs[2 * q + 1];
          o[q] = (v / (1.0f + __expf(-v))) * u;
        }
        uint16_t* dst = reinterpret_cast<uint16_t*>(a.out) + (int64_t)m * a.ldo + (n >> 1);
        if (n + 3 < a.N && (a.ldo & 1) == 0) *reinterpret_cast<uint32_t*>(dst) = pack2<T>(o[0], o[1]);
        else { dst[0] = T::from_f32(o[0]); if (n + 2 < a.N) dst[1] = T::from_f32(o[1]); }
      }
    }
  } else {
    skinny_epilogue_v<T, MODE, NT>(a, acc, skinny_prefetch<MODE, NT>(a, n0, m0, lane), n0, m0, split, lane);
  }
}

// The fragment-order weight matrix of a Whisper-step GEMM as a buffer resource: 16-byte loads at 32-bit byte offsets whose cache policy
// is the instruction's immediate `aux` operand (0 = default, 2 = non-temporal).
struct WFragBuf {
  typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
  __amdgpu_buffer_rsrc_t rs;
  const uint16_t* base;
  __device__ __forceinline__ explicit WFragBuf(const SkinnyArgs& a) : base(a.W) {
    const unsigned bytes = (unsigned)(((a.N + 15) >> 4) << 4) * (unsigned)a.K * 2u;          // wave-uniform
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.W), (short)0, (int)bytes, 0x00020000);
  }
  // the activation fragments of the same GEMM ([ceil(M / 32)][K / 32][2][64 lanes][8])
  __device__ __forceinline__ WFragBuf(const SkinnyArgs& a, int) : base(a.A) {
    const unsigned bytes = (unsigned)(((a.M + 31) >> 5) << 5) * (unsigned)a.K * 2u;
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.A), (short)0, (int)bytes, 0x00020000);
  }
  // the LM step's weight matrix: row-major [N][K] or fragment order (rows padded to 16)
  __device__ __forceinline__ WFragBuf(const SkinnyArgs& a, bool frag) : base(a.W) {
    const unsigned rows = frag ? (unsigned)(((a.N + 15) >> 4) << 4) : (unsigned)a.N;
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.W), (short)0, (int)(rows * (unsigned)a.K * 2u), 0x00020000);
  }
  // the LM step's row-major activations [M][lda]
  struct RowMajorA {};
  __device__ __forceinline__ WFragBuf(const SkinnyArgs& a, RowMajorA) : base(a.A) {
    rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(a.A), (short)0, (int)((unsigned)a.M * (unsigned)a.lda * 2u), 0x00020000);
  }
  __device__ __forceinline__ uint32_t offset(const uint16_t* p) const { return (uint32_t)((const char*)p - (const char*)base); }
  template <int AUX>
  __device__ __forceinline__ s16x8 load(uint32_t byte_off) const {
    return __builtin_bit_cast(s16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, AUX));
  }
};
