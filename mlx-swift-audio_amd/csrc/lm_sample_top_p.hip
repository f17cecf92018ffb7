// lm_sample_top_p.hip -- the Orpheus top-p sampler of the LM decode step on gfx950 (OrpheusTTS.swift:375-470: repetition penalty ->
// temperature -> top-p -> categorical), also standalone as mia_sample_top_p.  The categorical draw takes an explicit uniform (inverse
// CDF over the kept tokens); the reference draws from MLX's unseeded RNG, so parity is on the kept set / distribution, not on the
// stream.  The rest of the LM code sees the launcher and the workspace size (lm.h); what the samplers share is lm_sample_device.h.
#include "host_io.h"
#include "lm_sample_device.h"

namespace {

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
constexpr int SMX_LV = 4;
constexpr int SMX_W[SMX_LV] = {9, 8, 8, 7};            // digit widths, top down: sign|exponent, then 23 mantissa bits
constexpr int SMX_SH[SMX_LV] = {23, 15, 7, 0};
constexpr int SMX_NB[SMX_LV] = {128, 256, 256, 128};   // (0 <= p <= 1: the top digit is <= 127)
constexpr int SMX_CNT_SHIFT = 44;                      // V < 2^20 tokens, <= 23-bit `low`: 43 bits of sum

struct SmxLevel { double cum_above; double target; unsigned prefix, mask; };
struct SmxWs {                                         // per sequence
  float pmax[SMX_G], psum[SMX_G], pabove[SMX_G];
  SmxLevel lv[SMX_LV];                                 // lv[l]: the state after walking level l (l = 0 .. 2)
  unsigned long long slab[SMX_LV][SMX_G][SMX_NT];
};
static_assert(sizeof(SmxWs) == LM_SAMPLE_WS_BYTES, "the per-sequence workspace the greedy and top-k samplers borrow");

struct SmxArgs { float* logits; int V; int32_t* tokens; int32_t* hist; const float* uniforms; LmState* st; SmxWs* ws; mia_lm_sampler sp; int n_prompt; int max_ctx; };
struct SmxCtx { float* P; int32_t* tokens; int32_t* hist; const float* uniforms; LmState* st; SmxWs* ws; int lo, hi, sl; };

// this workgroup's sequence (blockIdx.y) and slice (blockIdx.x): pointers and bounds only, no memory access
__device__ __forceinline__ SmxCtx smx_ctx(const SmxArgs& a) {
  SmxCtx c;
  const int b = blockIdx.y;
  c.st = a.st + b; c.P = a.logits + (int64_t)b * a.V; c.tokens = a.tokens + (int64_t)b * a.max_ctx; c.hist = a.hist + b * 64; c.uniforms = a.uniforms + (int64_t)b * a.max_ctx; c.ws = a.ws + b;
  const LmSlice sl = lm_slice(a.V);
  c.sl = sl.sl; c.lo = sl.lo; c.hi = sl.hi;
  return c;
}
// the prompt is tokens; the step graph passes n_prompt = -1 and the state holds it: one graph serves every prompt length
__device__ __forceinline__ bool smx_drawing(const SmxArgs& a, const LmState& s) { return lm_drawing(s, a.n_prompt < 0 ? s.n_prompt : a.n_prompt); }
__device__ __forceinline__ bool smx_use_top_p(const mia_lm_sampler& sp, int V) { return sp.top_p > 0.0f && sp.top_p < 1.0f && V > 1; }

// value of a bin record: count * (smallest member) + ulp * sum(low bits), exact in double
__device__ __forceinline__ double smx_bin_value(unsigned long long h, unsigned bits) {
  constexpr unsigned long long ONE = 1ull << SMX_CNT_SHIFT;
  const int e = max((int)((bits >> 23) & 0xffu), 1);
  const double ulp = __longlong_as_double((long long)(e - 150 + 1023) << 52);       // 2^(e - 150)
  return (double)(h >> SMX_CNT_SHIFT) * (double)__uint_as_float(bits) + (double)(h & (ONE - 1ull)) * ulp;
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
  const double before = in.cum_above + block_excl_scan<double, SMX_NW>(a, shd);     // (its barriers publish s_i's reset)
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

__global__ __launch_bounds__(SMX_NT) void smx_max(SmxArgs a) {
  const SmxCtx c = smx_ctx(a);
  __shared__ float sh[SMX_NW];
  __shared__ int pen_tok[64];
  __shared__ float pen_val[64];
  __shared__ int n_pen;
  const int tid = threadIdx.x;
  float v0[SMX_U];
  slice_load(c.P, c.lo, c.hi, v0);
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
  slice_each(c.P, c.lo, c.hi, v0, [&](int i, float z, int) {
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
  slice_load(c.P, c.lo, c.hi, v0);
  float mx = c.ws->pmax[tid & (SMX_G - 1)];
  const LmState s = *c.st;
  if (!smx_drawing(a, s)) return;
  const bool use_top_p = smx_use_top_p(a.sp, a.V);
  slab_clear(hb);
#pragma unroll
  for (int o = 1; o < SMX_G; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float inv_t = 1.0f / fmaxf(a.sp.temperature, 1e-6f);
  __syncthreads();
  // 2. the unnormalised probabilities p = exp(z / T - max) REPLACE the logits (the buffer is rewritten by the next step's head GEMM),
  //    so every later kernel reads the same p without another exp
  float tot = 0.f;
  slice_each(c.P, c.lo, c.hi, v0, [&](int i, float z, int) {
    const float p = __expf(z * inv_t - mx);
    c.P[i] = p; tot += p;
    if (use_top_p) smx_hist_put<0>(hb, p, 0u, 0u);
  });
  tot = block_sum<SMX_NW>(tot, sh);                        // (its barriers also complete the histogram)
  if (tid == 0) c.ws->psum[blockIdx.x] = tot;
  if (use_top_p) slab_store<unsigned long long, SMX_NB[0]>(c.ws->slab[0], hb);
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
  slice_load(c.P, c.lo, c.hi, v0);
  const unsigned long long h = slab_merged<unsigned long long, SMX_NB[LVL - 1]>(c.ws->slab[LVL - 1]);
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
  slab_clear(hb);
  const SmxLevel out = smx_walk<LVL - 1>(h, in, shd, s_i, s_d);           // (its barriers publish the cleared histogram)
  if (blockIdx.x == 0 && tid == 0) c.ws->lv[LVL - 1] = out;
  float above = 0.f;
  slice_each(c.P, c.lo, c.hi, v0, [&](int, float p, int) {
    smx_hist_put<LVL>(hb, p, out.prefix, out.mask);
    if (LVL == SMX_LV - 1 && (__float_as_uint(p) & out.mask) > out.prefix) above += p;
  });
  if (LVL == SMX_LV - 1) { above = block_sum<SMX_NW>(above, sh); if (tid == 0) c.ws->pabove[blockIdx.x] = above; }
  else __syncthreads();
  slab_store<unsigned long long, SMX_NB[LVL]>(c.ws->slab[LVL], hb);
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
    if (tid == 0) st->pos = pos + 1;                      // a finished sequence advances too; the RAS, greedy and top-k finishers leave it in place.  Kept as it is
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
    slice_load(P, r_lo, r_hi, v);
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
  const float ex_sum = block_excl_scan<float, SMX_NW>(tsum, sh);
  const int ex_tie = block_excl_scan<int, SMX_NW>(tt, shi);
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

}  // namespace

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

// standalone sampler on caller-provided logits (OrpheusTTS.sampleNextToken, OrpheusTTS.swift:375-470)
extern "C" int mia_sample_top_p(mia_ctx* ctx, const float* logits, int V, const int32_t* history, int n_hist, float rep_penalty, float temperature,
                                float top_p, float uniform, int32_t* out) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, logits && out && V > 0 && n_hist >= 0 && n_hist <= 64, "sample_top_p: bad arguments");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  Carve cv;      // tokens [2]; history [64] (the kernels read all of it, use n_hist)
  const size_t o_logits = cv.add((size_t)V * 4), o_tok = cv.add(8), o_hist = cv.add(64 * 4), o_u = cv.add(4), o_st = cv.add(sizeof(LmState)), o_smx = cv.add(sizeof(SmxWs));
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  HostIo io = HostIo::host(ctx);
  const LmState st{0, n_hist, 0, 0};
  float* d_logits = (float*)io.in(logits, ws + o_logits, (size_t)V * 4);      // rewritten in place by the sampler
  int32_t* d_tok = (int32_t*)(ws + o_tok);
  const int32_t* d_hist = io.table(history, ws + o_hist, (size_t)n_hist * 4);
  const float* d_u = io.table(&uniform, ws + o_u, 4);
  LmState* d_st = (LmState*)io.table(&st, ws + o_st, sizeof(st));
  mia_lm_sampler sp{}; sp.temperature = temperature; sp.top_p = top_p; sp.rep_penalty = rep_penalty; sp.rep_window = 0; sp.max_new_tokens = 1;
  lm_sample_launch(ctx->stream, d_logits, V, d_tok, (int32_t*)d_hist, d_u, d_st, ws + o_smx, sp, 1, 2, 1);
  MIA_HIP(ctx, hipGetLastError());
  io.fetch(out, d_tok + 1, 4);
  return io.finish();
}
