// lm_sample_topk.hip -- the samplers of Fun-ASR's decoder on gfx950: the greedy argmax (FunASRModel.swift:160-163) and the top-k / top-p
// sampler for temperature > 0 (:165-198), also standalone as mia_sample_top_k_top_p.  The categorical draw takes an explicit uniform
// (inverse CDF over the kept tokens); the reference draws from MLX's unseeded RNG, so parity is on the kept set / distribution, not on
// the stream.  Both borrow the top-p sampler's per-sequence workspace.  The rest of the LM code sees the two launchers and the largest k
// (lm.h); what the samplers share is lm_sample_device.h.
#include <cmath>

#include "host_io.h"
#include "lm_sample_device.h"

namespace {

// every sequence in these loops has an embedding-row prompt
__device__ __forceinline__ bool grd_drawing(const LmState& s) { return lm_drawing(s, s.n_embeds); }

// ---- greedy (Fun-ASR: FunASRConfig.temperature 0 -> sampleNextToken takes MLX.argMax, STT/FunASR/FunASRModel.swift:160-163) ----
// argmax over the whole vocabulary, lowest index on exact ties: SMX_G workgroups per sequence each reduce one contiguous slice (one
// workgroup walking 151 936 logits is what one CU streams; see lm_sample_top_p.hip), then one wave per sequence picks among the slice
// winners and does the loop's bookkeeping (lm_emit_greedy).
struct GreedyWs { float v[SMX_G]; int i[SMX_G]; };      // per sequence, at the head of its workspace
static_assert(sizeof(GreedyWs) <= LM_SAMPLE_WS_BYTES, "the greedy sampler borrows the top-p sampler's per-sequence workspace");

__global__ __launch_bounds__(256) void lm_greedy_part(const float* __restrict__ logits, int V, const LmState* __restrict__ st, char* __restrict__ ws, size_t ws_stride) {
  __shared__ float shv[4];
  __shared__ int shi[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (!grd_drawing(st[b])) return;                       // still consuming the prompt, or done (uniform over the workgroup)
  logits += (int64_t)b * V;
  const LmSlice c = lm_slice(V);
  float v = -INFINITY; int i = 0x7fffffff;
  for (int k = c.lo + tid; k < c.hi; k += 256) vi_take(v, i, logits[k], k);
  vi_wave(v, i);
  if ((tid & 63) == 0) { shv[tid >> 6] = v; shi[tid >> 6] = i; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 4; ++w) vi_take(v, i, shv[w], shi[w]);
    GreedyWs* g = (GreedyWs*)(ws + (size_t)b * ws_stride);
    g->v[blockIdx.x] = v; g->i[blockIdx.x] = i;
  }
}

__global__ __launch_bounds__(64) void lm_greedy_pick(int V, int32_t* __restrict__ tokens, int32_t* __restrict__ out_tokens, LmState* __restrict__ st,
                                                     const char* __restrict__ ws, size_t ws_stride, mia_lm_sampler sp, int max_ctx) {
  const int b = blockIdx.x, lane = threadIdx.x;
  st += b; tokens += (int64_t)b * max_ctx; out_tokens += (int64_t)b * max_ctx;
  const LmState s = *st;
  if (!grd_drawing(s)) { if (lane == 0 && !s.finished) st->pos = s.pos + 1; return; }
  const GreedyWs* g = (const GreedyWs*)(ws + (size_t)b * ws_stride);
  float v = lane < SMX_G ? g->v[lane] : -INFINITY;
  int i = lane < SMX_G ? g->i[lane] : 0x7fffffff;
  vi_wave(v, i);
  if (lane != 0) return;
  const int pick = i < V ? i : 0;                        // a row without one ordered value (all NaN) must still give an id inside the table
  lm_emit_greedy(st, s, pick, sp, tokens, out_tokens, max_ctx);
}

// ---- top-k, top-p inside the top-k set, categorical (Fun-ASR with temperature > 0: sampleNextToken's second branch,
// STT/FunASR/FunASRModel.swift:165-198; the rule as built is stated at mia_lm_generate_topk in mia.h) ----
// The kept set is the first k entries of the row under the (value, index) order (higher value first, then lower index), k <= 1024 of
// V = 151 936 for Qwen3: an exact radix select on an order-preserving 32-bit key of the logit, split over the vocabulary slices like the
// top-p sampler (same slices, same register-resident slice, same slab-per-slice histograms merged by every workgroup of the next kernel):
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
// The logits are only read.  Histogram bins are u32 counts (integer LDS atomics, SMX_CP copies per bin: the top digit of a row of logits
// is one or two values, so whole waves hit one bin -- the case SMX_CP exists for).
constexpr int TK_LV = 4;                                // 8-bit digits of the key, top down: every level has SMX_NT bins
// finishing workgroup: thread j owns kept entry j, so it is sized to k (64, 256 or 1024 threads: the default k = 50 is one wave, whose
// barriers cost nothing).  The scans add waves of 64 in order whatever the size, so the three instances give the same bits for the same row
constexpr int TK_FIN_MAX = 1024;

struct TkLevel { unsigned prefix, mask; int above; };   // the key's digits fixed so far; keys above that bin
// per sequence, inside the top-p workspace: 128 KB of slabs + 8 KB of candidates + the level records = 139 320 B of its 262 624 B,
// so lm_sample_ws_bytes() stays the top-p sampler's size
struct TkWs {
  TkLevel lv[TK_LV];                                    // lv[l]: the state after walking level l (l = 0 .. 2)
  int cursor;                                           // candidates appended so far (zeroed by tk_hist0)
  unsigned slab[TK_LV][SMX_G][SMX_NT];
  unsigned long long cand[LM_TOPK_MAX_K];               // (key << 32) | ~index: descending = higher value first, then lower index
};
static_assert(sizeof(TkWs) == 139320 && LM_SAMPLE_WS_BYTES == 262624, "the sizes stated above");
static_assert(sizeof(TkWs) <= LM_SAMPLE_WS_BYTES, "the top-k sampler borrows the top-p sampler's per-sequence workspace");

struct TkArgs { const float* logits; int V; int32_t* tokens; int32_t* out_tokens; const float* uniforms; LmState* st; char* ws; mia_lm_sampler sp; int k; int max_ctx;
                int32_t* kept_ids; int32_t* n_kept; };

// order-preserving key: a > b as floats <=> key(a) > key(b); -0 is +0 (equal as values: a tie, split by index); NaN = 0, below -inf
// (not the RAS kernel's key, which has neither case: the two order NaN and -0 differently)
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

template <int LVL>
__device__ __forceinline__ void tk_hist_put(unsigned* hb, unsigned key, unsigned prefix, unsigned mask) {
  if ((key & mask) != prefix) return;
  atomicAdd(&hb[(threadIdx.x & (SMX_CP - 1)) * SMX_STRIDE +((key >> (24 - 8 * LVL)) & 0xffu)], 1u);
}
// Walk level LVL's merged histogram from the largest bin down to the bin that holds the k-th largest key: thread t owns descending
// position t (bin 255 - t) and its merged count.  Returns the state after the level (identical in every thread of every workgroup of
// the launch); *sel_cnt = the selected bin's count.  k <= V, and every entry of the row is counted (NaN in bin 0), so a bin always crosses.
template <int LVL>
__device__ __forceinline__ TkLevel tk_walk(unsigned cnt, TkLevel in, int k, int* shi, int* s_i, int* sel_cnt = nullptr) {
  const int tid = threadIdx.x;
  if (tid == 0) { s_i[0] = SMX_NT - 1; s_i[1] = in.above; s_i[2] = 0; }
  const int before = in.above + block_excl_scan<int, SMX_NW>((int)cnt, shi);      // (its barriers publish s_i's reset)
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

__device__ __forceinline__ TkWs* tk_ws(const TkArgs& a, int64_t b) { return (TkWs*)(a.ws + b * (int64_t)LM_SAMPLE_WS_BYTES); }
// the slice's slab of level LVL to global memory / thread t's merged count of bin 255 - t
template <int LVL>
__device__ __forceinline__ void tk_hist_store(TkWs* ws, const unsigned* hb) { slab_store<unsigned, SMX_NT>(ws->slab[LVL], hb); }
template <int LVL>
__device__ __forceinline__ unsigned tk_merged(const TkWs* ws) { return slab_merged<unsigned, SMX_NT>(ws->slab[LVL]); }

__global__ __launch_bounds__(SMX_NT) void tk_hist0(TkArgs a) {
  __shared__ unsigned hb[SMX_CP * SMX_STRIDE];
  const float* __restrict__ P = a.logits + (int64_t)blockIdx.y * a.V;
  TkWs* ws = tk_ws(a, blockIdx.y);
  const LmSlice sl = lm_slice(a.V);
  const int lo = sl.lo, hi = sl.hi;
  float v0[SMX_U];
  slice_load(P, lo, hi, v0);
  if (!grd_drawing(a.st[blockIdx.y])) return;           // still consuming the prompt, or done (uniform over the workgroup)
  slab_clear(hb);
  if (blockIdx.x == 0 && threadIdx.x == 0) ws->cursor = 0;
  __syncthreads();
  slice_each(P, lo, hi, v0, [&](int, float z, int) { tk_hist_put<0>(hb, tk_key(z), 0u, 0u); });
  __syncthreads();
  tk_hist_store<0>(ws, hb);
}

template <int LVL>      // 1 .. 3: walk level LVL-1, histogram level LVL
__global__ __launch_bounds__(SMX_NT) void tk_level(TkArgs a) {
  __shared__ unsigned hb[SMX_CP * SMX_STRIDE];
  __shared__ int shi[SMX_NW];
  __shared__ int s_i[3];
  const float* __restrict__ P = a.logits + (int64_t)blockIdx.y * a.V;
  TkWs* ws = tk_ws(a, blockIdx.y);
  const LmSlice sl = lm_slice(a.V);
  const int lo = sl.lo, hi = sl.hi;
  float v0[SMX_U];
  slice_load(P, lo, hi, v0);
  if (!grd_drawing(a.st[blockIdx.y])) return;
  const unsigned cnt = tk_merged<LVL - 1>(ws);
  TkLevel in{0u, 0u, 0};
  if constexpr (LVL > 1) in = ws->lv[LVL - 2];
  slab_clear(hb);
  const TkLevel out = tk_walk<LVL - 1>(cnt, in, a.k, shi, s_i);          // (its barriers publish the cleared histogram)
  if (blockIdx.x == 0 && threadIdx.x == 0) ws->lv[LVL - 1] = out;       // (a slot of its own: the launch's other workgroups still read lv[LVL-2])
  slice_each(P, lo, hi, v0, [&](int, float z, int) { tk_hist_put<LVL>(hb, tk_key(z), out.prefix, out.mask); });
  __syncthreads();
  tk_hist_store<LVL>(ws, hb);
}

__global__ __launch_bounds__(SMX_NT) void tk_gather(TkArgs a) {
  __shared__ int shi[SMX_NW];
  __shared__ int s_i[3];
  __shared__ int s_n, s_base;
  __shared__ unsigned long long list[LM_TOPK_MAX_K];    // this slice's kept entries (at most k of them by construction; bounded anyway)
  const float* __restrict__ P = a.logits + (int64_t)blockIdx.y * a.V;
  TkWs* ws = tk_ws(a, blockIdx.y);
  const LmSlice sl = lm_slice(a.V);
  const int lo = sl.lo, hi = sl.hi;
  const int tid = threadIdx.x, lane = tid & 63;
  float v0[SMX_U];
  slice_load(P, lo, hi, v0);
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
  slice_each(P, lo, hi, v0, [&](int i, float z, int) {
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
  const TkWs* ws = tk_ws(a, b);
  int32_t* tokens = a.tokens + (int64_t)b * a.max_ctx;
  int32_t* out_tokens = a.out_tokens + (int64_t)b * a.max_ctx;
  const LmState s = *st;
  __syncthreads();                                      // every wave holds the state before thread 0 advances it
  if (!grd_drawing(s)) { if (tid == 0 && !s.finished) st->pos = s.pos + 1; return; }
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
  // block-wide inclusive prefix sum in kept order; the total of all threads in *tot.  The total is the LAST THREAD's inclusive value,
  // (prefix + v): in floating point that is not block_excl_scan's total (the wave totals added up), whose last bits can differ, and
  // the nucleus cut and the draw compare against it -- so the exchange through s_tot stays
  auto incl_scan = [&](float v, float* tot) {
    const float ex = block_excl_scan<float, NW>(v, shf);
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
      const int below = block_excl_scan<int, NW>(tid < n && cum < a.sp.top_p ? 1 : 0, shn);
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
  // 6. the uniform just used, then the greedy loop's bookkeeping
  st->u_cursor = s.u_cursor + 1;
  lm_emit_greedy(st, s, pick, a.sp, tokens, out_tokens, a.max_ctx);
}

}  // namespace

static_assert(LM_TOPK_MAX_K == TK_FIN_MAX, "lm.h states the largest k the finishing workgroup holds");

void lm_sample_greedy_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, LmState* st, void* ws, const mia_lm_sampler& sp,
                             int max_ctx, int B) {
  hipLaunchKernelGGL(lm_greedy_part, dim3(SMX_G, B), dim3(256), 0, s, logits, V, (const LmState*)st, (char*)ws, LM_SAMPLE_WS_BYTES);
  hipLaunchKernelGGL(lm_greedy_pick, dim3(B), dim3(64), 0, s, V, tokens, out_tokens, st, (const char*)ws, LM_SAMPLE_WS_BYTES, sp, max_ctx);
}

void lm_sample_topk_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, const float* uniforms, LmState* st, void* ws,
                           const mia_lm_sampler& sp, int k, int max_ctx, int B, int32_t* kept_ids, int32_t* n_kept) {
  const dim3 g(SMX_G, B), blk(SMX_NT);
  const TkArgs a{logits, V, tokens, out_tokens, uniforms, st, (char*)ws, sp, k, max_ctx, kept_ids, n_kept};
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
  Carve cv;      // tokens [2]; out: emitted tokens [2] (the pick at [0]), then n_kept
  const size_t o_logits = cv.add((size_t)V * 4), o_tok = cv.add(8), o_out = cv.add(12), o_u = cv.add(4), o_st = cv.add(sizeof(LmState)),
               o_kept = cv.add((size_t)LM_TOPK_MAX_K * 4), o_smx = cv.add(LM_SAMPLE_WS_BYTES);
  char* ws = nullptr;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  HostIo io = HostIo::host(ctx);
  LmState st{}; st.n_embeds = 1; st.max_len = 1;         // one step past a one-row prompt: the draw always happens and writes the pick and n_kept
  const float* d_logits = io.in(logits, ws + o_logits, (size_t)V * 4);
  const float* d_u = io.table(&uniform, ws + o_u, 4);
  LmState* d_st = (LmState*)io.table(&st, ws + o_st, sizeof(st));
  int32_t* d_out = (int32_t*)(ws + o_out);
  int32_t* d_kept = (int32_t*)(ws + o_kept);
  mia_lm_sampler sp{}; sp.temperature = temperature; sp.top_p = top_p;
  lm_sample_topk_launch(ctx->stream, d_logits, V, (int32_t*)(ws + o_tok), d_out, d_u, d_st, ws + o_smx, sp, k, 2, 1, d_kept, d_out + 2);
  MIA_HIP(ctx, hipGetLastError());
  int32_t res[3] = {0, 0, 0};
  io.fetch(res, d_out, 12);
  if (const int rc = io.finish()) return rc;
  *out = res[0];
  if (n_kept) *n_kept = res[2];
  if (kept_ids && res[2] > 0) { io.fetch(kept_ids, d_kept, (size_t)std::min(res[2], k) * 4); return io.finish(); }
  return MIA_OK;
}
