// lm_sample.hip -- the LM decode step's samplers on gfx950: the Orpheus top-p sampler (OrpheusTTS.swift:375-470: repetition penalty ->
// temperature -> top-p -> categorical), also standalone as mia_sample_top_p, the RAS sampler of CosyVoice2 (Qwen2LM.swift:295-321,
// 433-488), the greedy argmax of Fun-ASR's decoder (FunASRModel.swift:160-163) and its top-k / top-p sampler for temperature > 0
// (:165-198), also standalone as mia_sample_top_k_top_p.  Stochastic stages: every categorical draw takes an
// explicit uniform (inverse CDF over the kept tokens); the reference draws from MLX's unseeded RNG, so parity is on the kept set /
// distribution, not on the stream.  The rest of the LM code sees the four launchers, the top-p workspace size and the RAS vocabulary
// bound (lm.h).
#include <cmath>

#include "lm.h"
#include "mia_device.h"

namespace {

// workgroup reductions of the 1024-thread RAS kernel
__device__ __forceinline__ float blk1024_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
  for (int i = 0; i < 16; ++i) r += sh[i];
  return r;
}
__device__ __forceinline__ float blk1024_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
  for (int i = 1; i < 16; ++i) r = fmaxf(r, sh[i]);
  return r;
}

template <typename V>
__device__ __forceinline__ V wave_incl_scan(V v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const V t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
  return v;
}

// ---- the top-p sampler, split over the vocabulary: SMX_G workgroups per sequence, one kernel per dependent phase ----
// One workgroup walking V = 156 940 logits six times took 82-91 us per token (46 GB/s: what one CU streams), 4-7 % of an Orpheus-3B
// step.  Here each of 32 workgroups owns one contiguous slice of the vocabulary (4 905 tokens at that V), holds it in registers
// (24 loads in flight per thread: one memory round trip per kernel) and the phases that need a vocabulary-wide result are separate
// kernels of the step graph (a kernel boundary inside a hipGraph costs 1.5 us, a grid barrier 4-5):
//   smx_max   repetition penalty on the slice's tokens; slice maximum of z / T
//   smx_exp   p = exp(z / T - max) written in place; slice sum; radix level 0 (sign | exponent) histogram of the slice
//   smx_level<1..3>  walk the previous level's merged histogram down to the bin where the descending cumulative sum crosses
//             top_p * total, then histogram the next 8 / 8 / 7 mantissa bits of the slice's members of that bin (level 3 also sums the
//             slice's probabilities ABOVE the bin: they are kept whatever the last 7 bits turn out to be)
//   smx_draw  one workgroup: walks the last level -> the exact bit pattern of the smallest kept probability + how many of its ties are
//             kept; every slice's kept sum and tie count from its level-3 slab; inverse-CDF draw in index order with the caller's
//             uniform (slice, then chunk, then token) + the sequence's bookkeeping
// Histograms: a bin is ONE u64, (count << 44) | sum of the bits below the level's digit -- every p of a bin shares the bits above, so
// the bin's sum is exactly count * base + ulp * sum(low): integer LDS atomics (tools/micro/lds_atomic_rate.hip: ds_add_f32 0.8
// lane-ops/ns, ds_add_u64 25), order-independent and exact, so the slices' histograms add up to the same u64 in any order.  A slice
// writes its 256-bin slab to global memory, the next kernel's workgroups each add the 32 slabs (every workgroup repeats the same walk
// and reaches the same bin; workgroup 0 records the level's result for the kernels after it -- in a slot of its own, since the other
// workgroups of the same launch are still reading the previous level's).  Ties at the threshold are kept lowest index first.
constexpr int SMX_G = 32;                              // vocabulary slices = workgroups per sequence
constexpr int SMX_NT = 256;                            // threads per workgroup (4 waves); also the widest level's bin count
constexpr int SMX_NW = SMX_NT / 64;
constexpr int SMX_U = 24;                              // loads in flight per thread: one batch covers a slice of 6 144 tokens (V <= 196 608)
constexpr int SMX_LV = 4;
constexpr int SMX_W[SMX_LV] = {9, 8, 8, 7};            // digit widths, top down: sign|exponent, then 23 mantissa bits
constexpr int SMX_SH[SMX_LV] = {23, 15, 7, 0};
constexpr int SMX_NB[SMX_LV] = {128, 256, 256, 128};   // (0 <= p <= 1: the top digit is <= 127)
constexpr int SMX_CP = 8, SMX_STRIDE = 257;            // LDS copies per lane group (a wave whose lanes all hit one bin must not serialise)
constexpr int SMX_CNT_SHIFT = 44;                      // V < 2^20 tokens, <= 23-bit `low`: 43 bits of sum

struct SmxLevel { double cum_above; double target; unsigned prefix, mask; };
struct SmxWs {                                         // per sequence
  float pmax[SMX_G], psum[SMX_G], pabove[SMX_G];
  SmxLevel lv[SMX_LV];                                 // lv[l]: the state after walking level l (l = 0 .. 2)
  unsigned long long slab[SMX_LV][SMX_G][SMX_NT];
};

struct SmxArgs { float* logits; int V; int32_t* tokens; int32_t* hist; const float* uniforms; LmState* st; SmxWs* ws; mia_lm_sampler sp; int n_prompt; int max_ctx; };
struct SmxCtx { float* P; int32_t* tokens; int32_t* hist; const float* uniforms; LmState* st; SmxWs* ws; int lo, hi, sl; };

// this workgroup's sequence (blockIdx.y) and slice (blockIdx.x): pointers and bounds only, no memory access
__device__ __forceinline__ SmxCtx smx_ctx(const SmxArgs& a) {
  SmxCtx c;
  const int b = blockIdx.y;
  c.st = a.st + b; c.P = a.logits + (int64_t)b * a.V; c.tokens = a.tokens + (int64_t)b * a.max_ctx; c.hist = a.hist + b * 64; c.uniforms = a.uniforms + (int64_t)b * a.max_ctx; c.ws = a.ws + b;
  c.sl = (a.V + SMX_G - 1) / SMX_G;
  c.lo = min(a.V, (int)blockIdx.x * c.sl); c.hi = min(a.V, c.lo + c.sl);
  return c;
}
// false while the prompt is still being consumed (or the sequence is done): nothing to draw.  (The step graph passes n_prompt = -1 and
// the state holds it: one graph serves every prompt length.)
__device__ __forceinline__ bool smx_drawing(const SmxArgs& a, const LmState& s) { return !(s.pos + 1 < (a.n_prompt < 0 ? s.n_prompt : a.n_prompt) || s.finished); }
__device__ __forceinline__ bool smx_use_top_p(const mia_lm_sampler& sp, int V) { return sp.top_p > 0.0f && sp.top_p < 1.0f && V > 1; }

// one batch of the slice, element u of thread t = token base + t + 256 u; the loads are unconditional (index clamped) so that they are
// all in flight before anything waits
__device__ __forceinline__ void smx_load(const float* __restrict__ P, int base, int hi, float (&v)[SMX_U]) {
  const int last = max(hi - 1, 0);
#pragma unroll
  for (int u = 0; u < SMX_U; ++u) v[u] = P[min(base + (int)threadIdx.x + SMX_NT * u, last)];
}
template <typename F>
__device__ __forceinline__ void smx_apply(const float (&v)[SMX_U], int base, int hi, F f) {
#pragma unroll
  for (int u = 0; u < SMX_U; ++u) { const int i = base + (int)threadIdx.x + SMX_NT * u; if (i < hi) f(i, v[u], u); }
}
// f over the whole slice; v0 = its first batch, already loaded
template <typename F>
__device__ __forceinline__ void smx_each(const float* __restrict__ P, int lo, int hi, const float (&v0)[SMX_U], F f) {
  smx_apply(v0, lo, hi, f);
  for (int base = lo + SMX_NT * SMX_U; base < hi; base += SMX_NT * SMX_U) { float v[SMX_U]; smx_load(P, base, hi, v); smx_apply(v, base, hi, f); }
}

template <typename V, int NW>
__device__ __forceinline__ V blk_excl_scan(V v, V* sh) {   // exclusive prefix over the workgroup in thread order; sh: NW words of scratch
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const V incl = wave_incl_scan(v, lane);
  V excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = (V)0;
  __syncthreads();
  if (lane == 63) sh[wave] = incl;
  __syncthreads();
  V base = (V)0;
#pragma unroll
  for (int i = 0; i < NW; ++i) if (i < wave) base += sh[i];
  return base + excl;
}
template <int NW>
__device__ __forceinline__ float blk_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) r += sh[i];
  return r;
}

// value of a bin record: count * (smallest member) + ulp * sum(low bits), exact in double
__device__ __forceinline__ double smx_bin_value(unsigned long long h, unsigned bits) {
  constexpr unsigned long long ONE = 1ull << SMX_CNT_SHIFT;
  const int e = max((int)((bits >> 23) & 0xffu), 1);
  const double ulp = __longlong_as_double((long long)(e - 150 + 1023) << 52);       // 2^(e - 150)
  return (double)(h >> SMX_CNT_SHIFT) * (double)__uint_as_float(bits) + (double)(h & (ONE - 1ull)) * ulp;
}

__device__ __forceinline__ void smx_hist_clear(unsigned long long* hb) {
  for (int i = threadIdx.x; i < SMX_CP * SMX_STRIDE; i += SMX_NT) hb[i] = 0ull;
}
template <int LVL>
__device__ __forceinline__ void smx_hist_put(unsigned long long* hb, float p, unsigned prefix, unsigned mask) {
  constexpr unsigned long long ONE = 1ull << SMX_CNT_SHIFT;
  constexpr int shf = SMX_SH[LVL], nb = SMX_NB[LVL];
  constexpr unsigned dmask = (1u << SMX_W[LVL]) - 1u, lmask = (1u << shf) - 1u;
  const unsigned b = __float_as_uint(p);
  if ((b & mask) != prefix) return;
  const int bin = min((int)((b >> shf) & dmask), nb - 1);
  atomicAdd(&hb[(threadIdx.x & (SMX_CP - 1)) * SMX_STRIDE + bin], ONE | (unsigned long long)(b & lmask));
}
// the slice's 256-bin slab to global memory (every bin written: no zeroing pass)
template <int LVL>
__device__ __forceinline__ void smx_hist_store(const SmxCtx& c, const unsigned long long* hb) {
  unsigned long long h = 0ull;
  if ((int)threadIdx.x < SMX_NB[LVL]) {
#pragma unroll
    for (int r = 0; r < SMX_CP; ++r) h += hb[r * SMX_STRIDE + threadIdx.x];
  }
  c.ws->slab[LVL][blockIdx.x][threadIdx.x] = h;
}

// Walk level LVL's merged histogram from the largest bin down until the cumulative sum crosses the target, as a workgroup-wide prefix
// sum: thread t owns descending position t (bin nb-1-t) and has the merged record h of its bin.  Returns the state after the level
// (identical in every thread of every workgroup of the launch); sel_bin = the bin it settled on.
template <int LVL>
__device__ __forceinline__ SmxLevel smx_walk(unsigned long long h, SmxLevel in, double* shd, int* s_i, double* s_d, int* sel_bin = nullptr) {
  constexpr int shf = SMX_SH[LVL], nb = SMX_NB[LVL];
  constexpr unsigned dmask = (1u << SMX_W[LVL]) - 1u;
  const int tid = threadIdx.x;
  if (tid == 0) { s_i[0] = 0x7fffffff; s_i[1] = -1; }
  const int bin = nb - 1 - tid;
  const bool occ = bin >= 0 && (h >> SMX_CNT_SHIFT) != 0ull;
  const double a = occ ? smx_bin_value(h, in.prefix | ((unsigned)bin << shf)) : 0.0;
  const double before = in.cum_above + blk_excl_scan<double, SMX_NW>(a, shd);      // (its barriers publish s_i's reset)
  if (occ && before + a > in.target) atomicMin(&s_i[0], tid);
  if (occ) atomicMax(&s_i[1], tid);
  __syncthreads();
  // never crossed (rounding corner): settle on the lowest occupied bin
  const int sel_r = s_i[0] != 0x7fffffff ? s_i[0] : max(s_i[1], 0);
  if (tid == sel_r) s_d[0] = before;
  __syncthreads();
  SmxLevel out = in;
  out.cum_above = s_d[0];
  out.prefix = in.prefix | (((unsigned)(nb - 1 - sel_r)) << shf);
  out.mask = in.mask | (dmask << shf);
  if (sel_bin) *sel_bin = nb - 1 - sel_r;
  __syncthreads();
  return out;
}
// thread t's merged record of bin nb-1-t: the 32 slices' slabs added up (all loads in flight at once)
template <int LVL>
__device__ __forceinline__ unsigned long long smx_merged(const SmxWs* ws) {
  const int bin = SMX_NB[LVL] - 1 - (int)threadIdx.x;
  const unsigned long long* sl = &ws->slab[LVL][0][max(bin, 0)];
  unsigned long long r[SMX_G];
#pragma unroll
  for (int g = 0; g < SMX_G; ++g) r[g] = sl[(size_t)g * SMX_NT];
  unsigned long long h = 0ull;
#pragma unroll
  for (int g = 0; g < SMX_G; ++g) h += r[g];
  return h;
}

__global__ __launch_bounds__(SMX_NT) void smx_max(SmxArgs a) {
  const SmxCtx c = smx_ctx(a);
  __shared__ float sh[SMX_NW];
  __shared__ int pen_tok[64];
  __shared__ float pen_val[64];
  __shared__ int n_pen;
  const int tid = threadIdx.x;
  float v0[SMX_U];
  smx_load(c.P, c.lo, c.hi, v0);
  const LmState s = *c.st;
  const int htok = tid < 64 ? c.hist[tid] : -1;
  if (tid == 0) n_pen = 0;
  if (!smx_drawing(a, s)) return;
  // 1. repetition penalty over the last `rep_window` generated tokens (gather all, then scatter: duplicates penalised once); a token
  //    lies in exactly one slice.  The slice is already in registers: the penalised values are patched in through a short LDS list
  __syncthreads();
  if (a.sp.rep_penalty != 1.0f && tid < s.n_hist && htok >= c.lo && htok < c.hi) {
    const float gth = c.P[htok];
    const float upd = gth < 0.f ? gth * a.sp.rep_penalty : gth / a.sp.rep_penalty;
    const int k = atomicAdd(&n_pen, 1);
    pen_tok[k] = htok; pen_val[k] = upd;
  }
  __syncthreads();
  const int np = n_pen;
  if (tid < np) c.P[pen_tok[tid]] = pen_val[tid];        // (duplicates write the same value)
  float mx = -INFINITY;
  smx_each(c.P, c.lo, c.hi, v0, [&](int i, float z, int) {
    for (int k = 0; k < np; ++k) z = pen_tok[k] == i ? pen_val[k] : z;
    mx = fmaxf(mx, z);
  });
  mx = wave_max(mx);
  if ((tid & 63) == 0) sh[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    float r = sh[0];
    for (int i = 1; i < SMX_NW; ++i) r = fmaxf(r, sh[i]);
    c.ws->pmax[blockIdx.x] = r * (1.0f / fmaxf(a.sp.temperature, 1e-6f));      // (T > 0: the maximum commutes with the scaling)
  }
}

__global__ __launch_bounds__(SMX_NT) void smx_exp(SmxArgs a) {
  const SmxCtx c = smx_ctx(a);
  __shared__ unsigned long long hb[SMX_CP * SMX_STRIDE];
  __shared__ float sh[SMX_NW];
  const int tid = threadIdx.x;
  float v0[SMX_U];
  smx_load(c.P, c.lo, c.hi, v0);
  float mx = c.ws->pmax[tid & (SMX_G - 1)];
  const LmState s = *c.st;
  if (!smx_drawing(a, s)) return;
  const bool use_top_p = smx_use_top_p(a.sp, a.V);
  smx_hist_clear(hb);
#pragma unroll
  for (int o = 1; o < SMX_G; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float inv_t = 1.0f / fmaxf(a.sp.temperature, 1e-6f);
  __syncthreads();
  // 2. the unnormalised probabilities p = exp(z / T - max) REPLACE the logits (the buffer is rewritten by the next step's head GEMM),
  //    so every later kernel reads the same p without another exp
  float tot = 0.f;
  smx_each(c.P, c.lo, c.hi, v0, [&](int i, float z, int) {
    const float p = __expf(z * inv_t - mx);
    c.P[i] = p; tot += p;
    if (use_top_p) smx_hist_put<0>(hb, p, 0u, 0u);
  });
  tot = blk_sum<SMX_NW>(tot, sh);                        // (its barriers also complete the histogram)
  if (tid == 0) c.ws->psum[blockIdx.x] = tot;
  if (use_top_p) smx_hist_store<0>(c, hb);
}

template <int LVL>      // 1 .. 3: walk level LVL-1, histogram level LVL
__global__ __launch_bounds__(SMX_NT) void smx_level(SmxArgs a) {
  const SmxCtx c = smx_ctx(a);
  if (!smx_use_top_p(a.sp, a.V)) return;
  __shared__ unsigned long long hb[SMX_CP * SMX_STRIDE];
  __shared__ double shd[SMX_NW];
  __shared__ double s_d[1];
  __shared__ int s_i[2];
  __shared__ float sh[SMX_NW];
  const int tid = threadIdx.x;
  float v0[SMX_U];
  smx_load(c.P, c.lo, c.hi, v0);
  const unsigned long long h = smx_merged<LVL - 1>(c.ws);
  SmxLevel in;
  if constexpr (LVL == 1) {
    float ps = c.ws->psum[tid & (SMX_G - 1)];
    float tot = 0.f;
#pragma unroll
    for (int g = 0; g < SMX_G; ++g) tot += __shfl(ps, g, 64);               // slice order: the same total in every workgroup
    in.cum_above = 0.0; in.target = (double)(a.sp.top_p * tot);             // the descending cumulative sum must EXCEED this
    in.prefix = 0u; in.mask = 0u;
  } else in = c.ws->lv[LVL - 2];
  const LmState s = *c.st;
  if (!smx_drawing(a, s)) return;
  smx_hist_clear(hb);
  const SmxLevel out = smx_walk<LVL - 1>(h, in, shd, s_i, s_d);           // (its barriers publish the cleared histogram)
  if (blockIdx.x == 0 && tid == 0) c.ws->lv[LVL - 1] = out;
  float above = 0.f;
  smx_each(c.P, c.lo, c.hi, v0, [&](int, float p, int) {
    smx_hist_put<LVL>(hb, p, out.prefix, out.mask);
    if (LVL == SMX_LV - 1 && (__float_as_uint(p) & out.mask) > out.prefix) above += p;
  });
  if (LVL == SMX_LV - 1) { above = blk_sum<SMX_NW>(above, sh); if (tid == 0) c.ws->pabove[blockIdx.x] = above; }
  else __syncthreads();
  smx_hist_store<LVL>(c, hb);
}

// 4. the last level's walk, then the inverse-CDF draw over the kept tokens in index order with the caller's uniform: serial over the 32
//    slices, then the whole workgroup resolves the selected slice (thread t owns CH contiguous tokens, a prefix sum finds the first
//    chunk that crosses the goal and its thread walks it in index order)
__global__ __launch_bounds__(SMX_NT) void smx_draw(SmxArgs a) {
  const SmxCtx c = smx_ctx(a);                            // gridDim.x = 1: lo / hi are not used here
  LmState* st = c.st;
  const int tid = threadIdx.x, lane = tid & 63;
  constexpr int L3 = SMX_LV - 1, NB3 = SMX_NB[L3];
  __shared__ double shd[SMX_NW];
  __shared__ double s_d[1];
  __shared__ float sh[SMX_NW];
  __shared__ int shi[SMX_NW];
  __shared__ float s_f[3];
  __shared__ int s_i[5];
  __shared__ unsigned long long part[SMX_NT];
  __shared__ float pkeep[SMX_G];
  __shared__ int ptie[SMX_G];
  __shared__ float slice[SMX_NT * SMX_U];
  const bool use_top_p = smx_use_top_p(a.sp, a.V);
  // level-3 records: thread t holds bin (t & 127) of the slices 16 (t >> 7) .. + 15 -- for the merged walk AND for the per-slice sums
  const int my_bin = tid & (NB3 - 1), g0 = (tid >> 7) * (SMX_G / 2);
  unsigned long long rec[SMX_G / 2];
#pragma unroll
  for (int g = 0; g < SMX_G / 2; ++g) rec[g] = use_top_p ? c.ws->slab[L3][g0 + g][my_bin] : 0ull;
  const float ps = c.ws->psum[tid & (SMX_G - 1)], pa = c.ws->pabove[tid & (SMX_G - 1)];
  SmxLevel in = c.ws->lv[L3 - 1];
  const LmState s = *st;
  const int pos = s.pos, cur_len = pos + 1;
  if (!smx_drawing(a, s)) {                               // still consuming the prompt (or done): nothing to draw
    if (tid == 0) st->pos = pos + 1;
    return;
  }
  const float u01 = c.uniforms[s.n_gen];
  unsigned thr_bits = 0u;        // keep p > thr, plus `keep_ties` of the p == thr (lowest index first)
  int keep_ties = 0x7fffffff;
  if (use_top_p) {
    unsigned long long hsum = 0ull;
#pragma unroll
    for (int g = 0; g < SMX_G / 2; ++g) hsum += rec[g];
    part[tid] = hsum;
    __syncthreads();
    const int wb = NB3 - 1 - tid;                         // the walk wants bin nb-1-t in thread t
    const unsigned long long h = wb >= 0 ? part[wb] + part[wb + NB3] : 0ull;
    int sel_bin = 0;
    const SmxLevel out = smx_walk<L3>(h, in, shd, s_i, s_d, &sel_bin);
    thr_bits = out.prefix;
    const float thr = __uint_as_float(thr_bits);
    // ties: keep the smallest k >= 1 with cum_above + k*thr > target
    int k = 1;
    if (thr > 0.f) { const double need = (out.target - out.cum_above) / (double)thr; k = need >= 2.0e9 ? 0x7fffffff : (int)floor(need) + 1; if (k < 1) k = 1; }
    keep_ties = k;
    // every slice's kept sum = what lies above the level-3 bin range + its bins above the selected one; its ties = the selected bin's count
    // (thread (g, j) adds bins 16 j .. 16 j + 15 of slice g from LDS)
    __shared__ unsigned long long recs[SMX_G][NB3 + 1];
#pragma unroll
    for (int g = 0; g < SMX_G / 2; ++g) recs[g0 + g][my_bin] = rec[g];
    __syncthreads();
    const int g = tid >> 3, j = tid & 7;
    const float pag = __shfl(pa, g & 31, 64);             // pabove[g] (lane l holds slice l & 31; every lane takes part in the shuffle)
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < NB3 / 8; ++q) {
      const int bin = j * (NB3 / 8) + q;
      const unsigned long long r = recs[g][bin];
      if (bin > sel_bin && (r >> SMX_CNT_SHIFT) != 0ull) acc += smx_bin_value(r, in.prefix | (unsigned)bin);
    }
    acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64); acc += __shfl_xor(acc, 4, 64);
    if (j == 0) { pkeep[g] = pag + (float)acc; ptie[g] = (int)(recs[g][sel_bin] >> SMX_CNT_SHIFT); }
  } else if (tid < SMX_G) { pkeep[tid] = ps; ptie[tid] = 0; }
  __syncthreads();
  const float thr = __uint_as_float(thr_bits);
  const float* __restrict__ P = c.P;
  if (tid < 64) {
    // the kept total, then the slice holding the goal (ties count lowest index first, up to keep_ties): prefix sums over the 32 slices
    // in lanes 0 .. 31 of the first wave (fixed order: deterministic)
    const bool on = lane < SMX_G;
    const int my_tie = on ? ptie[lane] : 0;
    const float my_keep = on ? pkeep[lane] : 0.f;
    const int tie_incl = wave_incl_scan(my_tie, lane);
    const int nt = __shfl(tie_incl, 63, 64);
    const int kt = use_top_p ? min(keep_ties, nt) : 0;
    const int used = min(kt, tie_incl - my_tie);          // ties already used by the slices before this one
    const int tk = min(my_tie, kt - used);
    const float add = my_keep + (float)tk * thr;
    const float add_incl = wave_incl_scan(add, lane);
    const float goal = u01 * __shfl(add_incl, 63, 64);
    const float cum = add_incl - add;
    const unsigned long long crosses = __ballot(on && cum + add > goal), holds = __ballot(on && add > 0.f);
    // goal >= kept total (rounding): the last slice that holds anything
    const int sel = crosses ? __ffsll((long long)crosses) - 1 : (holds ? 63 - __clzll((long long)holds) : 0);
    if (lane == sel) { s_f[1] = cum; s_f[2] = goal; s_i[1] = sel; s_i[2] = used; s_i[3] = kt; s_i[0] = 0x7fffffff; s_i[4] = -1; }
  }
  __syncthreads();
  const int sel = s_i[1], kt = s_i[3], ties0 = s_i[2];
  const float cum0 = s_f[1], goal = s_f[2];
  const int r_lo = min(a.V, sel * c.sl), r_hi = min(a.V, r_lo + c.sl);
  // the selected slice through LDS (coalesced, all loads in flight), then thread t reads its own contiguous chunk
  const bool staged = c.sl <= SMX_NT * SMX_U;
  if (staged) {
    float v[SMX_U];
    smx_load(P, r_lo, r_hi, v);
#pragma unroll
    for (int u = 0; u < SMX_U; ++u) slice[tid + SMX_NT * u] = v[u];
  }
  __syncthreads();
  auto at = [&](int i) { return staged ? slice[i - r_lo] : P[i]; };
  const int CH = (c.sl + SMX_NT - 1) / SMX_NT;
  const int t_lo = min(r_hi, r_lo + tid * CH), t_hi = min(r_hi, t_lo + CH);
  float tsum = 0.f; int tt = 0; bool any_kept = false;
  for (int i = t_lo; i < t_hi; ++i) {
    const float p = at(i); const unsigned b = __float_as_uint(p);
    if (!use_top_p || b > thr_bits) { tsum += p; any_kept = any_kept || p > 0.f; } else if (b == thr_bits) ++tt;
  }
  const float ex_sum = blk_excl_scan<float, SMX_NW>(tsum, sh);
  const int ex_tie = blk_excl_scan<int, SMX_NW>(tt, shi);
  const int used_before = min(kt, ties0 + ex_tie), used_after = min(kt, ties0 + ex_tie + tt);
  const float before = cum0 + ex_sum + (float)(used_before - ties0) * thr;
  const float after = cum0 + (ex_sum + tsum) + (float)(used_after - ties0) * thr;
  any_kept = any_kept || (used_after > used_before && thr > 0.f);
  if (any_kept) { atomicMax(&s_i[4], tid); if (after > goal) atomicMin(&s_i[0], tid); }
  __syncthreads();
  const int win = s_i[0] != 0x7fffffff ? s_i[0] : s_i[4];      // no chunk crosses (rounding): the last chunk that holds a kept token
  if (tid == (win < 0 ? 0 : win)) {
    int found = -1, last_kept = -1;
    float cum = before; int used = used_before;
    for (int i = t_lo; i < t_hi && found < 0; ++i) {
      const float p = at(i); const unsigned b = __float_as_uint(p);
      float kv = 0.f;
      if (!use_top_p || b > thr_bits) kv = p;
      else if (b == thr_bits && used < kt) { kv = thr; ++used; }
      if (kv > 0.f) { last_kept = i; if (cum + kv > goal) found = i; cum += kv; }
    }
    if (found < 0) found = last_kept >= 0 ? last_kept : min(r_lo, a.V - 1);
    const int next = found;
    const int ng = s.n_gen;
    if (cur_len < a.max_ctx) c.tokens[cur_len] = next;
    st->n_gen = ng + 1;
    bool stop = false;
    for (int k = 0; k < a.sp.n_stop; ++k) stop = stop || next == a.sp.stop_ids[k];
    if (!stop && a.sp.rep_window > 0) {                  // history is updated only for non-stop tokens (OrpheusTTS.swift:304-326)
      int nh = s.n_hist;
      if (nh < a.sp.rep_window) { c.hist[nh] = next; st->n_hist = nh + 1; }
      else { for (int k = 1; k < nh; ++k) c.hist[k - 1] = c.hist[k]; c.hist[nh - 1] = next; }
    }
    if (stop || ng + 1 >= a.sp.max_new_tokens || cur_len + 1 >= a.max_ctx) st->finished = 1;
    st->pos = pos + 1;
  }
  (void)lane;
}

// ---- RAS sampler of CosyVoice2 (Qwen2LM.swift:295-321, 433-488): nucleus (top-p 0.8 capped at top-k 25, renormalised, drawn in
// descending-probability order); if the pick already occurs >= win*tau times among the last `win` emitted tokens, redraw from the
// full softmax; while i < min_len an EOS pick is rejected and the whole trial repeated (<= 100 times).  Every categorical draw is
// an inverse CDF with the next caller-provided uniform (u_cursor walks the stream).

constexpr int RAS_NPT = 8;      // logits a thread keeps in registers: V <= 8192 (CosyVoice2: 6561 speech tokens + 3)
__global__ __launch_bounds__(1024) void lm_sample_ras(const float* __restrict__ logits, int V, int32_t* __restrict__ tokens, int32_t* __restrict__ out_tokens,
                                                      const float* __restrict__ uniforms, LmState* __restrict__ st, RasParams rp, int max_ctx) {
  __shared__ float sh[16];
  __shared__ float shv[2][16];
  __shared__ int shi[2][16];
  __shared__ float topv[32];
  __shared__ int topi[32];
  __shared__ int s_tok[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // one workgroup per sequence; the text-length-dependent bounds of the loop live in the sequence's state
  st += blockIdx.x; logits += (int64_t)blockIdx.x * V; tokens += (int64_t)blockIdx.x * max_ctx; out_tokens += (int64_t)blockIdx.x * max_ctx;
  uniforms += (int64_t)blockIdx.x * max_ctx;
  const int pos = st->pos, n_prompt = st->n_embeds;
  const int cur_len = pos + 1;
  if (cur_len < n_prompt || st->finished) { __syncthreads(); if (tid == 0 && !st->finished) st->pos = pos + 1; return; }
  const int step_i = cur_len - n_prompt;                 // loop index i of inferenceLoop
  // the whole row lives in registers (thread t holds ids t, t + 1024, ...): one read of the logits for the statistics and
  // all top-k rounds (re-reading them per round with a `taken` list cost 300 us per token at V = 6564)
  float x[RAS_NPT];
#pragma unroll
  for (int u = 0; u < RAS_NPT; ++u) { const int i = tid + 1024 * u; x[u] = i < V ? logits[i] : -INFINITY; }
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < RAS_NPT; ++u) mx = fmaxf(mx, x[u]);
  mx = blk1024_max(mx, sh);
  float tot = 0.f;
#pragma unroll
  for (int u = 0; u < RAS_NPT; ++u) if (tid + 1024 * u < V) tot += __expf(x[u] - mx);
  tot = blk1024_sum(tot, sh);
  // top-k (k <= 32), ordered by (value desc, index asc).  Fast path: a 3-level radix select (11 | 11 | 10 bits of the order-preserving
  // key, integer LDS atomics, one wave walks the bins) finds the k-th largest key, the <= 32 survivors are gathered and rank-sorted:
  // 8 barriers instead of one per rank (the iterated argmax below measured 2.1 us per round, 52 of the kernel's 60 us).  It is kept as
  // the fallback for the one case the select cannot order by itself: more logits equal to the threshold than slots left for them.
  const int K = rp.top_k < 32 ? rp.top_k : 32;
  __shared__ unsigned rh[3][2048];
  __shared__ int r_sel[4];                               // bin, count above it, count in it, gather cursor
  __shared__ float candv[32];
  __shared__ int candi[32];
  for (int i = tid; i < 3 * 2048; i += 1024) (&rh[0][0])[i] = 0u;
  if (tid == 0) r_sel[3] = 0;
  unsigned key[RAS_NPT];
#pragma unroll
  for (int u = 0; u < RAS_NPT; ++u) {
    const unsigned bits = __float_as_uint(x[u]);
    key[u] = tid + 1024 * u < V ? ((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u)) : 0u;    // 0 sorts below every float
  }
  __syncthreads();
  bool fast = true;
  {
    unsigned prefix = 0u, mask = 0u;
    int need = K, c_thr = 0;
    const int shifts[3] = {21, 10, 0}, widths[3] = {11, 11, 10};
#pragma unroll
    for (int lvl = 0; lvl < 3; ++lvl) {
      const int shf = shifts[lvl], nb = 1 << widths[lvl];
#pragma unroll
      for (int u = 0; u < RAS_NPT; ++u)
        if (key[u] != 0u && (key[u] & mask) == prefix) atomicAdd(&rh[lvl][(key[u] >> shf) & (unsigned)(nb - 1)], 1u);
      if (tid == 0) r_sel[0] = -1;
      __syncthreads();
      if (wave == 0) {                                   // lane l owns the bins nb-1 - per*l ... nb-per*(l+1), walked downwards
        const int per = nb >> 6;
        int mine = 0;
        for (int j = 0; j < per; ++j) mine += (int)rh[lvl][nb - 1 - (per * lane + j)];
        const int incl = wave_incl_scan(mine, lane), excl = incl - mine;
        if (excl < need && incl >= need) {
          int cum = excl;
          for (int j = 0; j < per; ++j) {
            const int bin = nb - 1 - (per * lane + j), cnt = (int)rh[lvl][bin];
            if (cum + cnt >= need) { r_sel[0] = bin; r_sel[1] = cum; r_sel[2] = cnt; break; }
            cum += cnt;
          }
        }
      }
      __syncthreads();
      if (r_sel[0] < 0) { fast = false; break; }        // fewer than k candidates (cannot happen for k <= V finite logits)
      prefix |= (unsigned)r_sel[0] << shf;
      mask |= (unsigned)(nb - 1) << shf;
      need -= r_sel[1];
      c_thr = r_sel[2];
      __syncthreads();
    }
    if (fast && c_thr > need) fast = false;              // ties at the threshold would have to be split by index: ordered path
    if (fast) {
#pragma unroll
      for (int u = 0; u < RAS_NPT; ++u)
        if (key[u] != 0u && key[u] >= prefix) { const int slot = atomicAdd(&r_sel[3], 1); if (slot < 32) { candv[slot] = x[u]; candi[slot] = tid + 1024 * u; } }
      __syncthreads();
      if (tid < K) {
        const float v = candv[tid]; const int ix = candi[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += (candv[j] > v || (candv[j] == v && candi[j] < ix)) ? 1 : 0;
        topv[rank] = __expf(v - mx) / tot; topi[rank] = ix;
      }
      __syncthreads();
    }
  }
  if (!fast) {
  for (int r = 0; r < K; ++r) {
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int u = 0; u < RAS_NPT; ++u) { const int i = tid + 1024 * u; if (i < V && x[u] > bv) { bv = x[u]; bi = i; } }   // ascending i: first maximum wins
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64); const int oi = __shfl_xor(bi, o, 64);
      if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    const int buf = r & 1;
    if (lane == 0) { shv[buf][wave] = bv; shi[buf][wave] = bi; }
    __syncthreads();
    float v = shv[buf][0]; int ix = shi[buf][0];
#pragma unroll
    for (int w2 = 1; w2 < 16; ++w2) { const float ov = shv[buf][w2]; const int oi = shi[buf][w2]; if (ov > v || (ov == v && oi < ix)) { v = ov; ix = oi; } }
    if (tid == 0) { topv[r] = __expf(v - mx) / tot; topi[r] = ix; }
    if (ix != 0x7fffffff && (ix & 1023) == tid) {
#pragma unroll
      for (int u = 0; u < RAS_NPT; ++u) if ((ix >> 10) == u) x[u] = -INFINITY;
    }
  }
  __syncthreads();
  }
  // per-wave partial sums of the full softmax in index order (for the fallback draw)
  const int per_wave = (V + 15) / 16;
  const int w_lo = wave * per_wave, w_hi = min(V, w_lo + per_wave);
  float wsum = 0.f;
  for (int i = w_lo + lane; i < w_hi; i += 64) wsum += __expf(logits[i] - mx);
  wsum = wave_sum(wsum);
  __shared__ float wtot[16];
  if (lane == 0) wtot[wave] = wsum;
  __syncthreads();
  __shared__ int s_need_full; __shared__ float s_goal; __shared__ int s_sel; __shared__ float s_cum;
  int trials = 0;
  int pick = -1;
  while (true) {                                         // trial loop (uniform across the block through shared state)
    if (tid == 0) {
      int cur = st->u_cursor;
      // nucleus: n = min(count(cumsum < top_p) + 1, top_k)
      float cum = 0.f; int below = 0;
      for (int r = 0; r < K; ++r) { cum += topv[r]; if (cum < rp.top_p) ++below; }
      int n = below + 1; if (n > K) n = K;
      float ns = 0.f;
      for (int r = 0; r < n; ++r) ns += topv[r];
      const float u = uniforms[cur < rp.n_uniforms ? cur : rp.n_uniforms - 1]; ++cur;
      float c2 = 0.f; int sel = n - 1;
      for (int r = 0; r < n; ++r) { c2 += topv[r]; if (c2 > u * ns) { sel = r; break; } }
      int tok = topi[sel];
      // repetition-aware fallback (rasSampling :463-488): over the last `win` EMITTED tokens
      int rep = 0; const int no = st->n_out;
      for (int q = max(0, no - rp.win); q < no; ++q) rep += out_tokens[q] == tok;
      int need_full = 0;
      if (no > 0 && (float)rep >= (float)rp.win * rp.tau) {
        need_full = 1;
        const float u2 = uniforms[cur < rp.n_uniforms ? cur : rp.n_uniforms - 1]; ++cur;
        const float goal = u2 * tot;
        float c3 = 0.f; int ws = 15;
        for (int w2 = 0; w2 < 16; ++w2) { if (c3 + wtot[w2] > goal) { ws = w2; break; } c3 += wtot[w2]; }
        s_goal = goal; s_sel = ws; s_cum = c3;
      }
      st->u_cursor = cur;
      s_need_full = need_full; s_tok[0] = tok;
    }
    __syncthreads();
    if (s_need_full) {
      if (wave == s_sel) {                               // ordered scan of the selected index range
        float cum = s_cum; int found = -1;
        for (int base = w_lo; base < w_hi && found < 0; base += 64) {
          const int i = base + lane;
          const float p = i < w_hi ? __expf(logits[i] - mx) : 0.f;
          float incl = p;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
          const unsigned long long hit = __ballot(p > 0.f && cum + incl > s_goal);
          if (hit) found = base + (__ffsll((long long)hit) - 1);
          cum += __shfl(incl, 63, 64);
        }
        if (found < 0) found = w_hi - 1;
        if (lane == 0) s_tok[0] = found;
      }
      __syncthreads();
    }
    pick = s_tok[0];
    ++trials;
    const bool ignore_eos = step_i < st->min_len;
    if (!(ignore_eos && pick == rp.eos) || trials > 100) break;   // the Swift throws after 100 rejected trials; we keep the EOS
    __syncthreads();
  }
  if (tid == 0) {
    const int ng = st->n_gen;
    st->n_gen = ng + 1;
    if (pick == rp.eos) st->finished = 1;
    else {
      if (cur_len < max_ctx) tokens[cur_len] = pick;     // embedding input of the next step (speech_embedding[pick])
      if (pick < rp.eos) { out_tokens[st->n_out] = pick; st->n_out += 1; }   // ids above EOS (fill tokens) are fed back, not emitted
      if (step_i + 1 >= st->max_len || cur_len + 1 >= max_ctx) st->finished = 1;
      st->pos = pos + 1;
    }
  }
}

// ---- greedy (Fun-ASR: FunASRConfig.temperature 0 -> sampleNextToken takes MLX.argMax, STT/FunASR/FunASRModel.swift:160-163) ----
// argmax over the whole vocabulary, lowest index on exact ties: GRD_G workgroups per sequence each reduce one contiguous slice (one
// workgroup walking 151 936 logits is what one CU streams; see the top-p sampler above), then one wave per sequence picks among the slice
// winners and does the loop's bookkeeping (FunASRSTT.swift:132-156): a stop id ends the sequence and is neither emitted nor counted.
constexpr int GRD_G = 32;
struct GreedyWs { float v[GRD_G]; int i[GRD_G]; };      // per sequence, at the head of its top-p workspace
static_assert(sizeof(GreedyWs) <= sizeof(SmxWs), "the greedy sampler borrows the top-p sampler's per-sequence workspace");

// (value, index) order: higher value first, then lower index; an index past the vocabulary marks "nothing yet" (all NaN / -inf slices)
__device__ __forceinline__ void grd_take(float& v, int& i, float v2, int i2) { if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; } }
__device__ __forceinline__ void grd_wave(float& v, int& i) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const float v2 = __shfl_xor(v, o, 64); const int i2 = __shfl_xor(i, o, 64); grd_take(v, i, v2, i2); }
}
__device__ __forceinline__ bool grd_drawing(const LmState& s) { return !(s.pos + 1 < s.n_embeds || s.finished); }

__global__ __launch_bounds__(256) void lm_greedy_part(const float* __restrict__ logits, int V, const LmState* __restrict__ st, char* __restrict__ ws, size_t ws_stride) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (!grd_drawing(st[b])) return;                       // still consuming the prompt, or done (uniform over the workgroup)
  logits += (int64_t)b * V;
  const int sl = (V + GRD_G - 1) / GRD_G, lo = min(V, (int)blockIdx.x * sl), hi = min(V, lo + sl);
  float v = -INFINITY; int i = 0x7fffffff;
  for (int k = lo + tid; k < hi; k += 256) grd_take(v, i, logits[k], k);
  grd_wave(v, i);
  if ((tid & 63) == 0) { shv[tid >> 6] = v; shi[tid >> 6] = i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) grd_take(v, i, shv[w], shi[w]);
    GreedyWs* g = (GreedyWs*)(ws + (size_t)b * ws_stride);
    g->v[blockIdx.x] = v; g->i[blockIdx.x] = i;
  }
}

__global__ __launch_bounds__(64) void lm_greedy_pick(int V, int32_t* __restrict__ tokens, int32_t* __restrict__ out_tokens, LmState* __restrict__ st,
                                                     const char* __restrict__ ws, size_t ws_stride, mia_lm_sampler sp, int max_ctx) {
  const int b = blockIdx.x, lane = threadIdx.x;
  st += b; tokens += (int64_t)b * max_ctx; out_tokens += (int64_t)b * max_ctx;
  const int pos = st->pos, n_prompt = st->n_embeds, cur_len = pos + 1;
  if (!grd_drawing(*st)) { if (lane == 0 && !st->finished) st->pos = pos + 1; return; }
  const GreedyWs* g = (const GreedyWs*)(ws + (size_t)b * ws_stride);
  float v = lane < GRD_G ? g->v[lane] : -INFINITY;
  int i = lane < GRD_G ? g->i[lane] : 0x7fffffff;
  grd_wave(v, i);
  if (lane != 0) return;
  const int pick = i < V ? i : 0;                        // a row without one ordered value (all NaN) must still give an id inside the table
  bool stop = false;
  for (int k = 0; k < sp.n_stop; ++k) stop = stop || pick == sp.stop_ids[k];
  st->n_gen += 1;
  if (stop) { st->finished = 1; return; }
  const int step_i = cur_len - n_prompt;
  if (cur_len < max_ctx) tokens[cur_len] = pick;         // embedding input of the next step (model.embed_tokens[pick])
  out_tokens[st->n_out] = pick; st->n_out += 1;
  if (step_i + 1 >= st->max_len || cur_len + 1 >= max_ctx) st->finished = 1;
  st->pos = pos + 1;
}

// ---- top-k, top-p inside the top-k set, categorical (Fun-ASR with temperature > 0: sampleNextToken's second branch,
// STT/FunASR/FunASRModel.swift:165-198; the rule as built is stated at mia_lm_generate_topk in mia.h) ----
// The kept set is the first k entries of the row under grd_take's order (higher value first, then lower index), k <= 1024 of V = 151 936
// for Qwen3: an exact radix select on an order-preserving 32-bit key of the logit, split over the vocabulary slices like the top-p sampler
// above (same slices, same register-resident slice, same slab-per-slice histograms merged by every workgroup of the next kernel):
//   tk_hist0       histogram of the key's top 8 bits over the slice
//   tk_level<1..3> walk the previous level's merged histogram from the top bin down to the bin holding the k-th largest key, then
//                  histogram the next 8 bits of the slice's members of that bin
//   tk_gather      the last walk gives the k-th largest key T exactly, how many keys lie above it and how many equal it.  Every slice
//                  appends its keys > T to the sequence's candidate list, and its share of the keys == T: ties are granted slice by
//                  slice in index order (each slice's tie count is the selected bin of its level-3 slab), and the one slice whose grant
//                  is smaller than its tie count walks its members in index order.  List positions come from an integer cursor: the
//                  SET is fixed by the rule, its order in the list is not, and tk_finish sorts it
//   tk_finish      one workgroup per sequence: rank sort of the <= 1024 (key, index) pairs in LDS, the nucleus cut, the inverse-CDF
//                  draw with the caller's uniform, the greedy loop's bookkeeping.  Sums are workgroup prefix sums in kept order: fixed
//                  order, no float atomics
// The logits are only read.  Histogram bins are u32 counts (integer LDS atomics, TK_CP copies per bin: the top digit of a row of logits
// is one or two values, so whole waves hit one bin -- the case SMX_CP exists for).
constexpr int TK_LV = 4;                                // 8-bit digits of the key, top down
constexpr int TK_CP = SMX_CP, TK_STRIDE = SMX_STRIDE;
// finishing workgroup: thread j owns kept entry j, so it is sized to k (64, 256 or 1024 threads: the default k = 50 is one wave, whose
// barriers cost nothing).  The scans add waves of 64 in order whatever the size, so the three instances give the same bits for the same row
constexpr int TK_FIN_MAX = 1024;

struct TkLevel { unsigned prefix, mask; int above; };   // the key's digits fixed so far; keys above that bin
// per sequence, inside the top-p workspace: 128 KB of slabs + 8 KB of candidates + the level records = 139 320 B of SmxWs's 262 624 B,
// so lm_sample_ws_bytes() stays sizeof(SmxWs)
struct TkWs {
  TkLevel lv[TK_LV];                                    // lv[l]: the state after walking level l (l = 0 .. 2)
  int cursor;                                           // candidates appended so far (zeroed by tk_hist0)
  unsigned slab[TK_LV][SMX_G][SMX_NT];
  unsigned long long cand[LM_TOPK_MAX_K];               // (key << 32) | ~index: descending = higher value first, then lower index
};
static_assert(sizeof(TkWs) == 139320 && sizeof(SmxWs) == 262624, "the sizes stated above");
static_assert(sizeof(TkWs) <= sizeof(SmxWs), "the top-k sampler borrows the top-p sampler's per-sequence workspace");

struct TkArgs { const float* logits; int V; int32_t* tokens; int32_t* out_tokens; const float* uniforms; LmState* st; SmxWs* ws; mia_lm_sampler sp; int k; int max_ctx;
                int32_t* kept_ids; int32_t* n_kept; };

// order-preserving key: a > b as floats <=> key(a) > key(b); -0 is +0 (equal as values: a tie, split by index); NaN = 0, below -inf
__device__ __forceinline__ unsigned tk_key(float x) {
  unsigned b = __float_as_uint(x);
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0u;
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float tk_value(unsigned key) {
  if (key == 0u) return __uint_as_float(0x7fc00000u);
  return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

__device__ __forceinline__ void tk_hist_clear(unsigned* hb) {
  for (int i = threadIdx.x; i < TK_CP * TK_STRIDE; i += SMX_NT) hb[i] = 0u;
}
template <int LVL>
__device__ __forceinline__ void tk_hist_put(unsigned* hb, unsigned key, unsigned prefix, unsigned mask) {
  if ((key & mask) != prefix) return;
  atomicAdd(&hb[(threadIdx.x & (TK_CP - 1)) * TK_STRIDE + ((key >> (24 - 8 * LVL)) & 0xffu)], 1u);
}
// the slice's 256-bin slab to global memory (every bin written: no zeroing pass)
template <int LVL>
__device__ __forceinline__ void tk_hist_store(TkWs* ws, const unsigned* hb) {
  unsigned h = 0u;
#pragma unroll
  for (int r = 0; r < TK_CP; ++r) h += hb[r * TK_STRIDE + threadIdx.x];
  ws->slab[LVL][blockIdx.x][threadIdx.x] = h;
}
// thread t's merged count of bin 255 - t: the 32 slices' slabs added up (all loads in flight at once)
template <int LVL>
__device__ __forceinline__ unsigned tk_merged(const TkWs* ws) {
  const unsigned* sl = &ws->slab[LVL][0][SMX_NT - 1 - (int)threadIdx.x];
  unsigned r[SMX_G];
#pragma unroll
  for (int g = 0; g < SMX_G; ++g) r[g] = sl[(size_t)g * SMX_NT];
  unsigned h = 0u;
#pragma unroll
  for (int g = 0; g < SMX_G; ++g) h += r[g];
  return h;
}
// Walk level LVL's merged histogram from the largest bin down to the bin that holds the k-th largest key: thread t owns descending
// position t (bin 255 - t) and its merged count.  Returns the state after the level (identical in every thread of every workgroup of
// the launch); *sel_cnt = the selected bin's count.  k <= V, and every entry of the row is counted (NaN in bin 0), so a bin always crosses.
template <int LVL>
__device__ __forceinline__ TkLevel tk_walk(unsigned cnt, TkLevel in, int k, int* shi, int* s_i, int* sel_cnt = nullptr) {
  const int tid = threadIdx.x;
  if (tid == 0) { s_i[0] = SMX_NT - 1; s_i[1] = in.above; s_i[2] = 0; }
  const int before = in.above + blk_excl_scan<int, SMX_NW>((int)cnt, shi);      // (its barriers publish s_i's reset)
  if (before < k && before + (int)cnt >= k) { s_i[0] = tid; s_i[1] = before; s_i[2] = (int)cnt; }
  __syncthreads();
  TkLevel out;
  out.prefix = in.prefix | ((unsigned)(SMX_NT - 1 - s_i[0]) << (24 - 8 * LVL));
  out.mask = in.mask | (0xffu << (24 - 8 * LVL));
  out.above = s_i[1];
  if (sel_cnt) *sel_cnt = s_i[2];
  __syncthreads();
  return out;
}

__device__ __forceinline__ TkWs* tk_ws(const TkArgs& a) { return (TkWs*)(a.ws + blockIdx.y); }
__device__ __forceinline__ void tk_slice(const TkArgs& a, int& lo, int& hi) {
  const int sl = (a.V + SMX_G - 1) / SMX_G;
  lo = min(a.V, (int)blockIdx.x * sl); hi = min(a.V, lo + sl);
}

__global__ __launch_bounds__(SMX_NT) void tk_hist0(TkArgs a) {
  __shared__ unsigned hb[TK_CP * TK_STRIDE];
  const float* __restrict__ P = a.logits + (int64_t)blockIdx.y * a.V;
  TkWs* ws = tk_ws(a);
  int lo, hi; tk_slice(a, lo, hi);
  float v0[SMX_U];
  smx_load(P, lo, hi, v0);
  if (!grd_drawing(a.st[blockIdx.y])) return;           // still consuming the prompt, or done (uniform over the workgroup)
  tk_hist_clear(hb);
  if (blockIdx.x == 0 && threadIdx.x == 0) ws->cursor = 0;
  __syncthreads();
  smx_each(P, lo, hi, v0, [&](int, float z, int) { tk_hist_put<0>(hb, tk_key(z), 0u, 0u); });
  __syncthreads();
  tk_hist_store<0>(ws, hb);
}

template <int LVL>      // 1 .. 3: walk level LVL-1, histogram level LVL
__global__ __launch_bounds__(SMX_NT) void tk_level(TkArgs a) {
  __shared__ unsigned hb[TK_CP * TK_STRIDE];
  __shared__ int shi[SMX_NW];
  __shared__ int s_i[3];
  const float* __restrict__ P = a.logits + (int64_t)blockIdx.y * a.V;
  TkWs* ws = tk_ws(a);
  int lo, hi; tk_slice(a, lo, hi);
  float v0[SMX_U];
  smx_load(P, lo, hi, v0);
  if (!grd_drawing(a.st[blockIdx.y])) return;
  const unsigned cnt = tk_merged<LVL - 1>(ws);
  TkLevel in{0u, 0u, 0};
  if constexpr (LVL > 1) in = ws->lv[LVL - 2];
  tk_hist_clear(hb);
  const TkLevel out = tk_walk<LVL - 1>(cnt, in, a.k, shi, s_i);          // (its barriers publish the cleared histogram)
  if (blockIdx.x == 0 && threadIdx.x == 0) ws->lv[LVL - 1] = out;       // (a slot of its own: the launch's other workgroups still read lv[LVL-2])
  smx_each(P, lo, hi, v0, [&](int, float z, int) { tk_hist_put<LVL>(hb, tk_key(z), out.prefix, out.mask); });
  __syncthreads();
  tk_hist_store<LVL>(ws, hb);
}

__global__ __launch_bounds__(SMX_NT) void tk_gather(TkArgs a) {
  __shared__ int shi[SMX_NW];
  __shared__ int s_i[3];
  __shared__ int s_n, s_base;
  __shared__ unsigned long long list[LM_TOPK_MAX_K];    // this slice's kept entries (at most k of them by construction; bounded anyway)
  const float* __restrict__ P = a.logits + (int64_t)blockIdx.y * a.V;
  TkWs* ws = tk_ws(a);
  int lo, hi; tk_slice(a, lo, hi);
  const int tid = threadIdx.x, lane = tid & 63;
  float v0[SMX_U];
  smx_load(P, lo, hi, v0);
  if (!grd_drawing(a.st[blockIdx.y])) return;
  constexpr int L3 = TK_LV - 1;
  const unsigned cnt = tk_merged<L3>(ws);
  const TkLevel in = ws->lv[L3 - 1];
  if (tid == 0) s_n = 0;
  int n_tie = 0;
  const TkLevel out = tk_walk<L3>(cnt, in, a.k, shi, s_i, &n_tie);       // (its barriers publish s_n)
  const unsigned T = out.prefix;                         // the k-th largest key
  const int sel_bin = (int)(T & 0xffu);
  // ties granted to this slice: what the slices before it leave of k - above, at most its own count
  const int need = min(a.k - out.above, n_tie);
  const int tg = lane < SMX_G ? (int)ws->slab[L3][lane][sel_bin] : 0;
  const int tg_incl = wave_incl_scan(tg, lane);
  const int my_tie = __shfl(tg, (int)blockIdx.x, 64), tie_before = __shfl(tg_incl, (int)blockIdx.x, 64) - my_tie;
  const int grant = max(0, min(my_tie, need - tie_before));
  auto put = [&](unsigned key, int i) {
    const int slot = atomicAdd(&s_n, 1);
    if (slot < LM_TOPK_MAX_K) list[slot] = ((unsigned long long)key << 32) | (unsigned)~i;
  };
  const bool all_ties = grant == my_tie;
  smx_each(P, lo, hi, v0, [&](int i, float z, int) {
    const unsigned key = tk_key(z);
    if (key > T || (all_ties && key == T)) put(key, i);
  });
  if (!all_ties && grant > 0 && tid < 64) {
    // the cut falls inside this slice: the first wave walks it in index order, 256 entries a round, until the grant is used up
    int used = 0;
    for (int base = lo; base < hi && used < grant; base += 256) {
      float z[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) z[q] = P[min(base + 64 * q + lane, hi - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int i = base + 64 * q + lane;
        const bool tie = i < hi && tk_key(z[q]) == T;
        const unsigned long long m = __ballot(tie);
        const int rank = used + __popcll(m & ((1ull << lane) - 1ull));
        if (tie && rank < grant) put(T, i);
        used += __popcll(m);
      }
    }
  }
  __syncthreads();
  const int n = min(s_n, LM_TOPK_MAX_K);
  if (tid == 0) s_base = n > 0 ? atomicAdd(&ws->cursor, n) : 0;
  __syncthreads();
  const int base = s_base;
  for (int j = tid; j < n; j += SMX_NT) if (base + j < LM_TOPK_MAX_K) ws->cand[base + j] = list[j];
}

// LDS at 1024 threads: the pairs (8 KB), the sorted values and ids (4 + 4 KB), scan scratch: 16.2 KB static
template <int NT>
__global__ __launch_bounds__(NT) void tk_finish(TkArgs a) {
  constexpr int NW = NT / 64;
  __shared__ unsigned long long comp[NT];
  __shared__ float sv[NT];
  __shared__ int si[NT];
  __shared__ float shf[NW];
  __shared__ int shn[NW];
  __shared__ float s_tot;
  __shared__ int s_pick;
  const int b = blockIdx.x, tid = threadIdx.x;
  LmState* st = a.st + b;
  const TkWs* ws = (const TkWs*)(a.ws + b);
  int32_t* tokens = a.tokens + (int64_t)b * a.max_ctx;
  int32_t* out_tokens = a.out_tokens + (int64_t)b * a.max_ctx;
  const LmState s = *st;
  const int pos = s.pos, cur_len = pos + 1;
  __syncthreads();                                       // every wave holds the state before thread 0 advances it
  if (!grd_drawing(s)) { if (tid == 0 && !s.finished) st->pos = pos + 1; return; }
  const int n = min(min(ws->cursor, a.k), NT);                             // = k
  const float u01 = a.uniforms[(int64_t)b * a.max_ctx + min(s.u_cursor, a.max_ctx - 1)];
  const unsigned long long mine = tid < n ? ws->cand[tid] : 0ull;
  comp[tid] = mine;
  __syncthreads();
  // 3. kept order: rank = how many pairs come first (the pairs are distinct: the index is part of them)
  if (tid < n) {
    int rank = 0;
    for (int j = 0; j < n; ++j) rank += comp[j] > mine ? 1 : 0;
    sv[rank] = tk_value((unsigned)(mine >> 32)); si[rank] = (int)~(unsigned)mine;
  }
  __syncthreads();
  // block-wide inclusive prefix sum in kept order; the total of all threads in *tot
  auto incl_scan = [&](float v, float* tot) {
    const float ex = blk_excl_scan<float, NW>(v, shf);
    if (tid == NT - 1) s_tot = ex + v;
    __syncthreads();
    *tot = s_tot;
    __syncthreads();
    return ex + v;
  };
  const float x = tid < n ? sv[tid] : 0.f, x_max = n > 0 ? sv[0] : 0.f;
  int pick = 0, nk = n;
  if (n > 0 && !isnan(x_max)) {                          // (a row without one ordered value: id 0, as the greedy sampler)
    // 4. e_j = exp((x_j - x_max) / T); an entry equal to the maximum is 1 whatever its value (+-inf included), a kept NaN is 0
    float e = 0.f;
    if (tid < n && !isnan(x)) e = x == x_max ? 1.f : __expf((x - x_max) / a.sp.temperature);
    if (a.sp.top_p < 1.0f) {
      float tot, one;
      (void)incl_scan(e, &tot);
      const float cum = incl_scan(e / tot, &one);
      const int below = blk_excl_scan<int, NW>(tid < n && cum < a.sp.top_p ? 1 : 0, shn);
      if (tid == NT - 1) s_pick = below + (tid < n && cum < a.sp.top_p ? 1 : 0);
      __syncthreads();
      nk = max(1, min(s_pick + 1, n));
      __syncthreads();
    }
    // 5. q over the first nk kept entries, w = q + 1e-10, first j with cumsum(w)_j > u * sum(w)
    float tot, wtot;
    (void)incl_scan(tid < nk ? e : 0.f, &tot);
    const float w = tid < nk ? e / tot + 1e-10f : 0.f;
    const float cw = incl_scan(w, &wtot);
    if (tid == 0) s_pick = nk - 1;
    __syncthreads();
    if (tid < nk && cw > u01 * wtot) atomicMin(&s_pick, tid);
    __syncthreads();
    pick = si[s_pick];
  }
  if (a.kept_ids && tid < nk) a.kept_ids[tid] = si[tid];
  if (tid != 0) return;
  if (a.n_kept) *a.n_kept = nk;
  if (pick < 0 || pick >= a.V) pick = 0;
  // 6. the greedy loop's bookkeeping (lm_greedy_pick), plus the uniform just used
  bool stop = false;
  for (int q = 0; q < a.sp.n_stop; ++q) stop = stop || pick == a.sp.stop_ids[q];
  st->n_gen = s.n_gen + 1;
  st->u_cursor = s.u_cursor + 1;
  if (stop) { st->finished = 1; return; }
  const int step_i = cur_len - s.n_embeds;
  if (cur_len < a.max_ctx) tokens[cur_len] = pick;       // embedding input of the next step (model.embed_tokens[pick])
  out_tokens[s.n_out] = pick; st->n_out = s.n_out + 1;
  if (step_i + 1 >= s.max_len || cur_len + 1 >= a.max_ctx) st->finished = 1;
  st->pos = pos + 1;
}

}  // namespace

static_assert(LM_TOPK_MAX_K == TK_FIN_MAX, "lm.h states the largest k the finishing workgroup holds");
static_assert(LM_RAS_MAX_VOCAB == 1024 * RAS_NPT, "lm.h states the RAS kernel's register-resident vocabulary");

size_t lm_sample_ws_bytes() { return sizeof(SmxWs); }

void lm_sample_launch(hipStream_t s, float* logits, int V, int32_t* tokens, int32_t* hist, const float* uniforms, LmState* st, void* ws, const mia_lm_sampler& sp,
                      int n_prompt, int max_ctx, int B) {
  const dim3 g(SMX_G, B), one(1, B), blk(SMX_NT);
  const SmxArgs a{logits, V, tokens, hist, uniforms, st, (SmxWs*)ws, sp, n_prompt, max_ctx};
  hipLaunchKernelGGL(smx_max, g, blk, 0, s, a);
  hipLaunchKernelGGL(smx_exp, g, blk, 0, s, a);
  hipLaunchKernelGGL(smx_level<1>, g, blk, 0, s, a);
  hipLaunchKernelGGL(smx_level<2>, g, blk, 0, s, a);
  hipLaunchKernelGGL(smx_level<3>, g, blk, 0, s, a);
  hipLaunchKernelGGL(smx_draw, one, blk, 0, s, a);
}

void lm_sample_ras_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, const float* uniforms, LmState* st, const RasParams& rp,
                          int max_ctx, int B) {
  hipLaunchKernelGGL(lm_sample_ras, dim3(B), dim3(1024), 0, s, logits, V, tokens, out_tokens, uniforms, st, rp, max_ctx);
}

void lm_sample_greedy_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, LmState* st, void* ws, const mia_lm_sampler& sp,
                             int max_ctx, int B) {
  hipLaunchKernelGGL(lm_greedy_part, dim3(GRD_G, B), dim3(256), 0, s, logits, V, (const LmState*)st, (char*)ws, sizeof(SmxWs));
  hipLaunchKernelGGL(lm_greedy_pick, dim3(B), dim3(64), 0, s, V, tokens, out_tokens, st, (const char*)ws, sizeof(SmxWs), sp, max_ctx);
}

void lm_sample_topk_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, const float* uniforms, LmState* st, void* ws,
                           const mia_lm_sampler& sp, int k, int max_ctx, int B, int32_t* kept_ids, int32_t* n_kept) {
  const dim3 g(SMX_G, B), blk(SMX_NT);
  const TkArgs a{logits, V, tokens, out_tokens, uniforms, st, (SmxWs*)ws, sp, k, max_ctx, kept_ids, n_kept};
  hipLaunchKernelGGL(tk_hist0, g, blk, 0, s, a);
  hipLaunchKernelGGL(tk_level<1>, g, blk, 0, s, a);
  hipLaunchKernelGGL(tk_level<2>, g, blk, 0, s, a);
  hipLaunchKernelGGL(tk_level<3>, g, blk, 0, s, a);
  hipLaunchKernelGGL(tk_gather, g, blk, 0, s, a);
  if (k <= 64) hipLaunchKernelGGL(tk_finish<64>, dim3(B), dim3(64), 0, s, a);
  else if (k <= 256) hipLaunchKernelGGL(tk_finish<256>, dim3(B), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(tk_finish<TK_FIN_MAX>, dim3(B), dim3(TK_FIN_MAX), 0, s, a);
}

// standalone top-k / top-p sampler on caller-provided logits (FunASRModel.sampleNextToken with temperature > 0, FunASRModel.swift:165-198)
extern "C" int mia_sample_top_k_top_p(mia_ctx* ctx, const float* logits, int V, float temperature, int top_k, float top_p, float uniform, int32_t* out,
                                      int32_t* kept_ids, int32_t* n_kept) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, logits && out && V > 0, "sample_top_k_top_p: logits, out and V > 0 required");
  MIA_CHECK_ARG(ctx, std::isfinite(temperature) && temperature > 0.f, "sample_top_k_top_p: temperature must be finite and positive");
  MIA_CHECK_ARG(ctx, std::isfinite(top_p) && top_p > 0.f, "sample_top_k_top_p: top_p must be finite and positive");
  MIA_CHECK_ARG(ctx, top_k >= 0, "sample_top_k_top_p: top_k must not be negative (0 = the reference's 50)");
  const int k = std::min(top_k > 0 ? top_k : 50, V);
  if (k > LM_TOPK_MAX_K) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "sample_top_k_top_p: k %d exceeds %d", k, LM_TOPK_MAX_K);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const size_t row = align_up((size_t)V * 4, 256), tail_bytes = 1024 + (size_t)LM_TOPK_MAX_K * 4;
  char* ws = (char*)mia_workspace(ctx, row + tail_bytes + sizeof(SmxWs));
  if (!ws) return MIA_ERR_OUT_OF_MEMORY;
  float* d_logits = (float*)ws;
  char* tail = ws + row;
  int32_t* d_tok = (int32_t*)tail;             // [2]
  int32_t* d_out = (int32_t*)(tail + 64);      // [2]: the pick at [0]
  float* d_u = (float*)(tail + 128);           // [2]
  LmState* d_st = (LmState*)(tail + 192);
  int32_t* d_nk = (int32_t*)(tail + 512);
  int32_t* d_kept = (int32_t*)(tail + 1024);   // [LM_TOPK_MAX_K]
  void* d_smx = tail + tail_bytes;
  LmState st{}; st.n_embeds = 1; st.max_len = 1;
  hipStream_t s = ctx->stream;
  MIA_HIP(ctx, hipMemcpyAsync(d_logits, logits, (size_t)V * 4, hipMemcpyHostToDevice, s));
  MIA_HIP(ctx, hipMemsetAsync(tail, 0, 1024, s));
  MIA_HIP(ctx, hipMemcpyAsync(d_u, &uniform, 4, hipMemcpyHostToDevice, s));
  MIA_HIP(ctx, hipMemcpyAsync(d_st, &st, sizeof(st), hipMemcpyHostToDevice, s));
  mia_lm_sampler sp{}; sp.temperature = temperature; sp.top_p = top_p;
  lm_sample_topk_launch(s, d_logits, V, d_tok, d_out, d_u, d_st, d_smx, sp, k, 2, 1, d_kept, d_nk);
  MIA_HIP(ctx, hipGetLastError());
  int32_t nk = 0;
  MIA_HIP(ctx, hipMemcpyAsync(out, d_out, 4, hipMemcpyDeviceToHost, s));
  MIA_HIP(ctx, hipMemcpyAsync(&nk, d_nk, 4, hipMemcpyDeviceToHost, s));
  MIA_HIP(ctx, hipStreamSynchronize(s));
  if (n_kept) *n_kept = nk;
  if (kept_ids && nk > 0) MIA_HIP(ctx, hipMemcpy(kept_ids, d_kept, (size_t)std::min(nk, k) * 4, hipMemcpyDeviceToHost));
  return MIA_OK;
}

// standalone sampler on caller-provided logits (OrpheusTTS.sampleNextToken, OrpheusTTS.swift:375-470)
extern "C" int mia_sample_top_p(mia_ctx* ctx, const float* logits, int V, const int32_t* history, int n_hist, float rep_penalty, float temperature,
                                float top_p, float uniform, int32_t* out) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, logits && out && V > 0 && n_hist >= 0 && n_hist <= 64, "sample_top_p: bad arguments");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const size_t need = align_up((size_t)V * 4, 256) + 1024 + sizeof(SmxWs);
  char* ws = (char*)mia_workspace(ctx, need);
  if (!ws) return MIA_ERR_OUT_OF_MEMORY;
  float* d_logits = (float*)ws;
  char* tail = ws + align_up((size_t)V * 4, 256);
  int32_t* d_tok = (int32_t*)tail;            // [2]: tokens[0..1]
  int32_t* d_hist = (int32_t*)(tail + 64);    // [64]
  float* d_u = (float*)(tail + 64 + 256);
  LmState* d_st = (LmState*)(tail + 64 + 256 + 64);
  SmxWs* d_smx = (SmxWs*)(tail + 1024);
  LmState st{0, n_hist, 0, 0};
  hipStream_t s = ctx->stream;
  MIA_HIP(ctx, hipMemcpyAsync(d_logits, logits, (size_t)V * 4, hipMemcpyHostToDevice, s));
  if (n_hist) MIA_HIP(ctx, hipMemcpyAsync(d_hist, history, (size_t)n_hist * 4, hipMemcpyHostToDevice, s));
  MIA_HIP(ctx, hipMemcpyAsync(d_u, &uniform, 4, hipMemcpyHostToDevice, s));
  MIA_HIP(ctx, hipMemcpyAsync(d_st, &st, sizeof(st), hipMemcpyHostToDevice, s));
  mia_lm_sampler sp{}; sp.temperature = temperature; sp.top_p = top_p; sp.rep_penalty = rep_penalty; sp.rep_window = 0; sp.max_new_tokens = 1;
  lm_sample_launch(s, d_logits, V, d_tok, d_hist, d_u, d_st, d_smx, sp, 1, 2, 1);
  MIA_HIP(ctx, hipGetLastError());
  MIA_HIP(ctx, hipMemcpyAsync(out, d_tok + 1, 4, hipMemcpyDeviceToHost, s));
  MIA_HIP(ctx, hipStreamSynchronize(s));
  return MIA_OK;
}
