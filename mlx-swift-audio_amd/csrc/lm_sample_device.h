// lm_sample_device.h -- device-side pieces shared by the sampler sources (lm_sample_top_p.hip, lm_sample_ras.hip, lm_sample_topk.hip and
// the frame sampler of marvis_kernels.hip): workgroup scans and reductions, the vocabulary slices and their register-resident loader,
// the histogram slabs of the two radix selects, the (value, index) order and the bookkeeping of the greedy loop.
#pragma once
#include "lm.h"
#include "mia_device.h"

// ---- scans and reductions: `sh` is NW words of LDS scratch; each opens with a barrier, so the scratch may be reused back to back ----
template <typename V>
__device__ __forceinline__ V wave_incl_scan(V v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const V t = __shfl_up(v, o, 64); if (lane >= o) v += t; }
  return v;
}
// Exclusive prefix over the workgroup in thread order, and (if asked for) the total of all threads.  A wave's total is its lane 63's
// inclusive value; the wave totals are added serially in wave order, from zero, for the prefix and for the total alike.  The samplers'
// exact-equality tests pin this order: a tree over the waves, or a total taken from the last thread's prefix, gives other bits.
template <typename V, int NW>
__device__ __forceinline__ V block_excl_scan(V v, V* sh, V* total = nullptr) {
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
  if (total) {
    V tot = (V)0;
#pragma unroll
    for (int i = 0; i < NW; ++i) tot += sh[i];
    *total = tot;
  }
  return base + excl;
}
// all-reduce over the workgroup: the waves' results combined serially in wave order
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) r += sh[i];
  return r;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) r = fmaxf(r, sh[i]);
  return r;
}

// ---- the vocabulary split over SMX_G workgroups per sequence (blockIdx.x = slice): top-p, greedy and top-k share the geometry ----
constexpr int SMX_G = 32;                              // vocabulary slices = workgroups per sequence
constexpr int SMX_NT = 256;                            // threads per workgroup (4 waves); also the widest level's bin count
constexpr int SMX_NW = SMX_NT / 64;
constexpr int SMX_U = 24;                              // loads in flight per thread: one batch covers a slice of 6 144 tokens (V <= 196 608)
// per-sequence sampler workspace (lm_sample_ws_bytes()): the top-p sampler's SmxWs; the greedy and top-k samplers borrow it
constexpr size_t LM_SAMPLE_WS_BYTES = 262624;

struct LmSlice { int sl, lo, hi; };                    // tokens per slice; this workgroup's [lo, hi)
__device__ __forceinline__ LmSlice lm_slice(int V) {
  LmSlice c;
  c.sl = (V + SMX_G - 1) / SMX_G;
  c.lo = min(V, (int)blockIdx.x * c.sl); c.hi = min(V, c.lo + c.sl);
  return c;
}
// one batch of the slice, element u of thread t = token base + t + 256 u; the loads are unconditional (index clamped) so that they are
// all in flight before anything waits
__device__ __forceinline__ void slice_load(const float* __restrict__ P, int base, int hi, float (&v)[SMX_U]) {
  const int last = max(hi - 1, 0);
#pragma unroll
  for (int u = 0; u < SMX_U; ++u) v[u] = P[min(base + (int)threadIdx.x + SMX_NT * u, last)];
}
template <typename F>
__device__ __forceinline__ void slice_apply(const float (&v)[SMX_U], int base, int hi, F f) {
#pragma unroll
  for (int u = 0; u < SMX_U; ++u) { const int i = base + (int)threadIdx.x + SMX_NT * u; if (i < hi) f(i, v[u], u); }
}
// f over the whole slice; v0 = its first batch, already loaded
template <typename F>
__device__ __forceinline__ void slice_each(const float* __restrict__ P, int lo, int hi, const float (&v0)[SMX_U], F f) {
  slice_apply(v0, lo, hi, f);
  for (int base = lo + SMX_NT * SMX_U; base < hi; base += SMX_NT * SMX_U) { float v[SMX_U]; slice_load(P, base, hi, v); slice_apply(v, base, hi, f); }
}

// false while the prompt (n_prompt positions, by the caller's loop: tokens or embedding rows) is still being consumed, or the sequence is
// done: nothing to draw
__device__ __forceinline__ bool lm_drawing(const LmState& s, int n_prompt) { return !(s.pos + 1 < n_prompt || s.finished); }

// ---- histogram slabs of the radix selects.  R: the bin record (u64 count | sum for top-p, u32 count for top-k); NB: bins of the level.
// A workgroup histograms into SMX_CP copies in LDS (a wave whose lanes all hit one bin must not serialise), folds them into its slice's
// slab in global memory, and every workgroup of the next kernel adds the SMX_G slabs up.  What goes into a bin and how a level is walked
// differ per sampler (an exact sum toward a floating target; a count toward the k-th entry) and stay with it.
constexpr int SMX_CP = 8, SMX_STRIDE = 257;
template <typename R>
__device__ __forceinline__ void slab_clear(R* hb) {
  for (int i = threadIdx.x; i < SMX_CP * SMX_STRIDE; i += SMX_NT) hb[i] = (R)0;
}
// this slice's slab of the level's [SMX_G][SMX_NT] to global memory (every word written, zero past the level's bins: no zeroing pass)
template <typename R, int NB>
__device__ __forceinline__ void slab_store(R (*level)[SMX_NT], const R* hb) {
  R h = (R)0;
  if (NB >= SMX_NT || (int)threadIdx.x < NB) {
#pragma unroll
    for (int r = 0; r < SMX_CP; ++r) h += hb[r * SMX_STRIDE + threadIdx.x];
  }
  level[blockIdx.x][threadIdx.x] = h;
}
// thread t's merged record of bin NB-1-t: the level's slabs added up (all loads in flight at once)
template <typename R, int NB>
__device__ __forceinline__ R slab_merged(const R (*level)[SMX_NT]) {
  const int bin = NB - 1 - (int)threadIdx.x;
  const R* sl = &level[0][NB >= SMX_NT ? bin : max(bin, 0)];
  R r[SMX_G];
#pragma unroll
  for (int g = 0; g < SMX_G; ++g) r[g] = sl[(size_t)g * SMX_NT];
  R h = (R)0;
#pragma unroll
  for (int g = 0; g < SMX_G; ++g) h += r[g];
  return h;
}

// ---- (value, index) order: higher value first, then lower index; an index past the vocabulary marks "nothing yet" (all NaN / -inf) ----
__device__ __forceinline__ void vi_take(float& v, int& i, float v2, int i2) { if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; } }
__device__ __forceinline__ void vi_wave(float& v, int& i) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const float v2 = __shfl_xor(v, o, 64); const int i2 = __shfl_xor(i, o, 64); vi_take(v, i, v2, i2); }
}

// The greedy loop's bookkeeping for one drawn id (FunASRSTT.swift:132-156), by one thread; s: the state as read before the draw.  A stop
// id ends the sequence and is neither emitted nor counted; otherwise the id feeds the next step, is emitted, and the budget
// (LmState::max_len steps past the embedding-row prompt) or the context may end the sequence.
__device__ __forceinline__ void lm_emit_greedy(LmState* st, const LmState& s, int pick, const mia_lm_sampler& sp, int32_t* tokens, int32_t* out_tokens, int max_ctx) {
  const int cur_len = s.pos + 1;
  bool stop = false;
  for (int k = 0; k < sp.n_stop; ++k) stop = stop || pick == sp.stop_ids[k];
  st->n_gen = s.n_gen + 1;
  if (stop) { st->finished = 1; return; }
  const int step_i = cur_len - s.n_embeds;
  if (cur_len < max_ctx) tokens[cur_len] = pick;         // embedding input of the next step (model.embed_tokens[pick])
  out_tokens[s.n_out] = pick; st->n_out = s.n_out + 1;
  if (step_i + 1 >= s.max_len || cur_len + 1 >= max_ctx) st->finished = 1;
  st->pos = s.pos + 1;
}
