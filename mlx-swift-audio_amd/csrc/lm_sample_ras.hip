// lm_sample_ras.hip -- the RAS sampler of CosyVoice2 on gfx950 (Qwen2LM.swift:295-321, 433-488): nucleus (top-p 0.8 capped at top-k 25,
// renormalised, drawn in descending-probability order); if the pick already occurs >= win*tau times among the last `win` emitted tokens,
// redraw from the full softmax; while i < min_len an EOS pick is rejected and the whole trial repeated (<= 100 times).  Every categorical
// draw is an inverse CDF with the next caller-provided uniform (u_cursor walks the stream); the reference draws from MLX's unseeded RNG,
// so parity is on the kept set / distribution, not on the stream.  The rest of the LM code sees the launcher and the vocabulary bound
// (lm.h); what the samplers share is lm_sample_device.h.
#include "lm_sample_device.h"

namespace {

constexpr int RAS_NW = 16;      // one workgroup of 1024 threads per sequence
constexpr int RAS_NPT = 8;     // logits a thread keeps in registers: V <= 8192 (CosyVoice2: 6561 speech tokens + 3)
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
  if (!lm_drawing(*st, n_prompt)) { __syncthreads(); if (tid == 0 && !st->finished) st->pos = pos + 1; return; }
  const int step_i = cur_len - n_prompt;                 // loop index i of inferenceLoop
  // the whole row lives in registers (thread t holds ids t, t + 1024, ...): one read of the logits for the statistics and
  // all top-k rounds (re-reading them per round with a `taken` list cost 300 us per token at V = 6564)
  float x[RAS_NPT];
#pragma unroll
  for (int u = 0; u < RAS_NPT; ++u) { const int i = tid + 1024 * u; x[u] = i < V ? logits[i] : -INFINITY; }
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < RAS_NPT; ++u) mx = fmaxf(mx, x[u]);
  mx = block_max<RAS_NW>(mx, sh);
  float tot = 0.f;
#pragma unroll
  for (int u = 0; u < RAS_NPT; ++u) if (tid + 1024 * u < V) tot += __expf(x[u] - mx);
  tot = block_sum<RAS_NW>(tot, sh);
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
  }    // (not the top-k sampler's tk_key: no NaN case and no -0 case here, so the two order NaN and -0 differently)
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
    vi_wave(bv, bi);
    const int buf = r & 1;
    if (lane == 0) { shv[buf][wave] = bv; shi[buf][wave] = bi; }
    __syncthreads();
    float v = shv[buf][0]; int ix = shi[buf][0];
#pragma unroll
    for (int w2 = 1; w2 < RAS_NW; ++w2) vi_take(v, ix, shv[buf][w2], shi[buf][w2]);
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
          const float incl = wave_incl_scan(p, lane);
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

}  // namespace

static_assert(LM_RAS_MAX_VOCAB == 1024 * RAS_NPT, "lm.h states the RAS kernel's register-resident vocabulary");

void lm_sample_ras_launch(hipStream_t s, const float* logits, int V, int32_t* tokens, int32_t* out_tokens, const float* uniforms, LmState* st, const RasParams& rp,
                          int max_ctx, int B) {
  hipLaunchKernelGGL(lm_sample_ras, dim3(B), dim3(1024), 0, s, logits, V, tokens, out_tokens, uniforms, st, rp, max_ctx);
}
