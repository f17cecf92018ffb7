// marvis_kernels.hip -- the kernels a Marvis frame adds to the LM step chain (marvis.hip): the masked multi-table embedding sum
// (MarvisModel._embedTokens + the mask + sum of generateFrame, MarvisModel.swift:474-476,553-577), the ascending top-p sampler of
// every head (the rule is stated at mia_sample_top_p_ascending in mia.h) and the frame's bookkeeping (MarvisTTS.decodePrompt,
// MarvisTTS.swift:483-503).  Workgroup b of the sampler and of the bookkeeping is sequence b.
#include "lm_sample_device.h"
#include "marvis.h"

namespace {

// acc[0..3] += the four 16-bit values at p
template <typename T>
__device__ __forceinline__ void add4(f32x4& acc, const uint16_t* __restrict__ p) {
  const s16x4 v = *reinterpret_cast<const s16x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] += T::to_f32((uint16_t)v[j]);
}

__device__ __forceinline__ int clamp_id(int id, int rows) { return id < 0 ? 0 : (id < rows ? id : rows - 1); }   // never a wild address

// one workgroup per row; columns are added in index order (audio 0 .. K-1, then text), so a row's sum does not depend on its neighbours
template <typename T>
__global__ __launch_bounds__(256) void mv_embed_rows(const int32_t* __restrict__ ids, const int32_t* __restrict__ mask, const int2* __restrict__ rowmap, int K, int V,
                                                     int text_vocab, const uint16_t* __restrict__ audio_emb, const uint16_t* __restrict__ text_emb,
                                                     float* __restrict__ out, int max_ctx, int D, LmState* __restrict__ bb_state) {
  const int r = blockIdx.x, W = K + 1;
  const int seq = rowmap[r].x, pos = rowmap[r].y;
  if (pos < 0 || pos >= max_ctx) return;
  ids += (int64_t)r * W; mask += (int64_t)r * W;
  float* o = out + ((int64_t)seq * max_ctx + pos) * D;
  for (int e = threadIdx.x * 4; e < D; e += 1024) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < K; ++c)
      if (mask[c]) add4<T>(acc, audio_emb + ((int64_t)c * V + clamp_id(ids[c], V)) * D + e);
    if (mask[K]) add4<T>(acc, text_emb + (int64_t)clamp_id(ids[K], text_vocab) * D + e);
    *reinterpret_cast<f32x4*>(o + e) = acc;
  }
  if (threadIdx.x == 0) atomicMax(&bb_state[seq].n_embeds, pos + 1);     // the backbone reads these positions as embedding rows
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------
// (the workgroup scan and reductions are lm_sample_device.h's: their order is a function of the thread index alone)
constexpr int SMP_NT = 1024, SMP_NW = SMP_NT / 64, SMP_NPT = MV_MAX_VOCAB / SMP_NT;

__device__ __forceinline__ float key_p(unsigned long long k) { const uint32_t hi = (uint32_t)(k >> 32); return hi ? __uint_as_float(hi - 1u) : 0.f; }

// NP: the power of two >= V the sort runs on (dynamic LDS: NP keys of 8 bytes)
__global__ __launch_bounds__(SMP_NT) void mv_sample(MvSampleArgs a, int NP) {
  extern __shared__ unsigned long long keys[];
  __shared__ float wred[SMP_NW];
  __shared__ int sh_j0, sh_pick, sh_id;
  const int b = blockIdx.x;
  if (a.st) a.st += b;
  if (a.st && a.st->finished) return;    // the same for every thread
  a.logits += b * a.ld_logits; a.uniforms += b * a.ld_uniforms; a.out += (int64_t)b * a.ld_ids;
  if (a.forced) a.forced += (int64_t)b * a.ld_ids;
  if (a.emb_out) a.emb_out += (int64_t)b * a.D;
  const int tid = threadIdx.x, V = a.V;
  int ucur = a.st ? a.st->u_cursor : 0;
  ucur = ucur < 0 ? 0 : (ucur < a.n_uniforms ? ucur : a.n_uniforms - 1);      // never past the buffer
  const float u = a.uniforms[ucur];
  // 1. p = softmax(x / T) with the maximum subtracted; a NaN has p = 0
  float z[SMP_NPT];
  float m = -INFINITY;
#pragma unroll
  for (int i = 0; i < SMP_NPT; ++i) {
    const int j = tid + SMP_NT * i;
    z[i] = j < V ? a.logits[j] / a.temperature : NAN;
    m = fmaxf(m, z[i]);                  // fmaxf drops a NaN operand
  }
  m = block_max<SMP_NW>(m, wred);
  float e[SMP_NPT], s = 0.f;
#pragma unroll
  for (int i = 0; i < SMP_NPT; ++i) {
    float v = z[i] == z[i] ? expf(z[i] - m) : 0.f;
    v = v == v ? v : 0.f;
    e[i] = v; s += v;
  }
  const float S = block_sum<SMP_NW>(s, wred);
  if (tid == 0) { sh_j0 = V - 1; sh_pick = V - 1; sh_id = 0; }
  int n_kept = 0;
  if (S > 0.f && S < INFINITY) {
    // 2. ascending by p, lower index first on equal p, a NaN below every number: one 64-bit key per entry
#pragma unroll
    for (int i = 0; i < SMP_NPT; ++i) {
      const int j = tid + SMP_NT * i;
      if (j < NP) {
        unsigned long long k = ~0ull;    // padding sorts behind every entry
        if (j < V) k = ((unsigned long long)(z[i] == z[i] ? __float_as_uint(e[i] / S) + 1u : 0u) << 32) | (uint32_t)j;
        keys[j] = k;
      }
    }
    __syncthreads();
    for (int k = 2; k <= NP; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < NP; i += SMP_NT) {
          const int x = i ^ j;
          if (x > i) {
            const unsigned long long ka = keys[i], kb = keys[x];
            if ((ka > kb) == ((i & k) == 0)) { keys[i] = kb; keys[x] = ka; }
          }
        }
        __syncthreads();
      }
    // 3. inclusive cumulative sum in that order: each thread owns C consecutive entries (re-read from LDS in every pass: runtime loops
    //    instead of register arrays)
    const int C = NP >= SMP_NT ? NP / SMP_NT : 1, base = tid * C;
    const int end = base + C < V ? base + C : V;
    float run = 0.f;
    for (int pos = base; pos < end; ++pos) run += key_p(keys[pos]);
    float total;
    float pre = block_excl_scan<float, SMP_NW>(run, wred, &total);
    // 4. kept: from the first entry whose cumulative sum exceeds 1 - top_p (none: the largest alone)
    const float thr = 1.0f - a.top_p;
    {
      float c = pre; int first = V;
      for (int pos = base; pos < end; ++pos) { c += key_p(keys[pos]); if (c > thr && first == V) first = pos; }
      if (first < V) atomicMin(&sh_j0, first);
    }
    __syncthreads();
    const int j0 = sh_j0;
    n_kept = V - j0;
    // 5. inverse CDF over the kept entries, ascending
    const int kbeg = base > j0 ? base : j0;
    run = 0.f;
    for (int pos = kbeg; pos < end; ++pos) run += key_p(keys[pos]);
    pre = block_excl_scan<float, SMP_NW>(run, wred, &total);
    const float target = u * total;
    {
      float c = pre; int first = V;
      for (int pos = kbeg; pos < end; ++pos) { c += key_p(keys[pos]); if (c > target && first == V) first = pos; }
      if (first < V) atomicMin(&sh_pick, first);
    }
    __syncthreads();
    if (tid == 0) sh_id = (int)(uint32_t)keys[sh_pick];
    if (a.kept_ids) for (int pos = j0 + tid; pos < V; pos += SMP_NT) a.kept_ids[pos - j0] = (int)(uint32_t)keys[pos];
  }
  __syncthreads();
  if (tid == 0) {
    if (a.forced) sh_id = clamp_id(*a.forced, V);
    *a.out = sh_id;
    if (a.n_kept) *a.n_kept = n_kept;
    if (a.st) a.st->u_cursor = ucur + 1;
  }
  __syncthreads();
  if (a.emb) {                           // the picked id's embedding row, the next decoder row's projection input
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.emb + (int64_t)sh_id * a.D);
    uint32_t* dst = reinterpret_cast<uint32_t*>(a.emb_out);
    for (int i = tid; i < a.D / 2; i += SMP_NT) dst[i] = src[i];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void mv_frame_end(MvFrameEndArgs a) {
  __shared__ int sh_fin, sh_pos;
  const int b = blockIdx.x;
  a.st += b; a.bb_state += b; a.dec_state += b; a.frame += (int64_t)b * a.ld_ids; a.frames_out += (int64_t)b * a.frames_cap * a.ld_ids;
  a.embeds += (int64_t)b * a.max_ctx * a.D;
  if (threadIdx.x == 0) {
    a.dec_state->pos = 0;                // every frame starts the decoder on an empty cache
    int fin = a.st->finished;
    if (!fin) {
      int any = 0;
      for (int i = 0; i < a.cb; ++i) any |= a.frame[i];
      if (!any) { a.st->finished = 1; fin = 1; a.bb_state->frozen = 1; a.dec_state->frozen = 1; }       // the all-zero frame ends the sentence and is not emitted; further steps of the sequence are no-ops
      else {
        const int n = a.st->n_frames;
        if (n < a.frames_cap) { for (int i = 0; i < a.cb; ++i) a.frames_out[(int64_t)n * a.ld_ids + i] = a.frame[i]; a.st->n_frames = n + 1; }
      }
    }
    sh_fin = fin; sh_pos = a.bb_state->pos;
  }
  __syncthreads();
  const int pos = sh_pos;
  if (sh_fin || pos < 0 || pos >= a.max_ctx) return;
  // the fed-back row [frame | 0] with mask [1 .. 1 | 0]
  const uint16_t* emb = (const uint16_t*)a.audio_emb;
  float* o = a.embeds + (int64_t)pos * a.D;
  for (int e = threadIdx.x * 4; e < a.D; e += 1024) {
    f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < a.cb; ++c) add4<T>(acc, emb + ((int64_t)c * a.V + clamp_id(a.frame[c], a.V)) * a.D + e);
    *reinterpret_cast<f32x4*>(o + e) = acc;
  }
  if (threadIdx.x == 0) a.bb_state->n_embeds = pos + 1;
}

}  // namespace

void mv_launch_embed_rows(hipStream_t s, int dtype, const int32_t* ids, const int32_t* mask, const int2* rowmap, int T, int K, int V, int text_vocab,
                          const void* audio_emb, const void* text_emb, float* out, int max_ctx, int D, LmState* bb_state) {
  const bool f16 = dtype == MIA_F16;
  LAUNCH_T(mv_embed_rows, dim3(T), dim3(256), 0, ids, mask, rowmap, K, V, text_vocab, (const uint16_t*)audio_emb, (const uint16_t*)text_emb, out, max_ctx, D, bb_state);
}

void mv_launch_sample(hipStream_t s, const MvSampleArgs& a, int B) {
  int NP = 2;
  while (NP < a.V) NP <<= 1;
  hipLaunchKernelGGL(mv_sample, dim3(B), dim3(SMP_NT), (size_t)NP * 8, s, a, NP);
}

// the widest row's keys are 64 KB of dynamic LDS next to the kernel's static words: above the default limit, so it is raised once
int mv_sampler_init() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(mv_sample), hipFuncAttributeMaxDynamicSharedMemorySize, MV_MAX_VOCAB * 8) == hipSuccess ? 0 : -1;
}

void mv_launch_frame_end(hipStream_t s, int dtype, const MvFrameEndArgs& a, int B) {
  const bool f16 = dtype == MIA_F16;
  LAUNCH_T(mv_frame_end, dim3(B), dim3(256), 0, a);
}
