// mimi_encode_kernels.hip -- the Mimi encoder's own fp32 kernels on gfx950.  The SEANet encoder's convolutions, the transformer's
// linears, the latent downsample and the quantiser's two input projections run on conv_gemm_f32, the attention on attn_f32 and the
// Cin = 1 input convolution on conv_in1 (codec_kernels.hip).
//
//  * mimi_edge_rows    ConvDownsample1d pads with padMode .edge (Conv.swift:341-355): the transformer's P rows are staged behind
//                      `front` copies of row 0 and in front of `back` copies of row P - 1, so the tap GEMM runs the k = 4, stride 2
//                      convolution over materialised rows (it has no edge mode, and gets none).
//  * mimi_rvq_stage    one stage of the split residual quantiser's encode chain (Quantization.swift:50-56, 110-120): per frame
//                      idx = argmin_j (c2[j] - r . e[j]), lowest index on equal distances, then r <- r - e[idx].  Frames are
//                      independent, stages are serial per frame, and one stage of a 32-frame tile against 2048 x 256 entries is
//                      33.5 MFLOP: a tile kept in one workgroup through all stages would leave a 10 s clip (125 frames) on 4 CUs.
//                      So a stage is one launch and the ENTRIES are split across workgroups: workgroup (tile of 32 frames, slice of
//                      128 entries) holds the tile's residual in LDS, forms the 32 x 128 dot products on v_mfma_f32_32x32x2_f32 (one
//                      32-entry block per wave: A = entries, B = frames, so a lane owns one frame's column and 16 entries of it),
//                      keeps a per-frame (distance, index) minimum and writes one partial per (frame, slice).  The argmin over
//                      slices needs every slice, so it is the NEXT stage's prologue: each workgroup reduces the previous stage's
//                      partials of its tile (lexicographic on (distance, index): the lowest index wins a tie whatever the slice
//                      count), forms r - e[idx] in LDS, and the slice-0 workgroup stores the code and the new residual (a ping-pong
//                      buffer the stage after reads).  No grid-wide synchronisation, no atomics.  rvq_first's single stage rides in
//                      the first launch as extra grid slices on its own projected vector; mimi_rvq_finish reduces the last stage.
//                      The k order of a dot product is a fixed permutation of 0 .. dq - 1 (a lane's float4 feeds four MFMA steps), the
//                      same in every workgroup, so a distance has one value wherever it is computed.
//  * mimi_rvq_finish   the (distance, index) reduction of a chain's last stage.
#include "mia_device.h"
#include "mimi.h"

namespace {

__device__ __forceinline__ bool lex_less(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

__global__ __launch_bounds__(256) void mimi_edge_rows(const float* __restrict__ x, float* __restrict__ y, int64_t P, int D, int front, int64_t rows) {
  const int d4 = D >> 2;
  const int64_t total = rows * d4;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t row = e / d4;
    const int c = (int)(e - row * d4) * 4;
    int64_t src = row - front;
    src = src < 0 ? 0 : (src >= P ? P - 1 : src);
    *reinterpret_cast<f32x4*>(y + row * D + c) = *reinterpret_cast<const f32x4*>(x + src * D + c);
  }
}

struct RvqStageArgs { MimiRvqChain a, b; int64_t T, Tpad; int bins, dq, slices; };

__global__ __launch_bounds__(256) void mimi_rvq_stage(RvqStageArgs g) {
  extern __shared__ float sm[];          // the tile's residual, [32][dq + 4]
  __shared__ float s_d[4][MIMI_RVQ_TILE];
  __shared__ int s_i[4][MIMI_RVQ_TILE];
  __shared__ int s_code[MIMI_RVQ_TILE];
  const bool second = (int)blockIdx.y >= g.slices;
  const MimiRvqChain c = second ? g.b : g.a;
  const int slice = second ? (int)blockIdx.y - g.slices : (int)blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t f0 = (int64_t)blockIdx.x * MIMI_RVQ_TILE;
  const int dq = g.dq, RS = dq + 4, q4 = dq >> 2;

  // ---- prologue: finish the previous stage for this tile
  if (c.prev_pd) {
    if (tid < MIMI_RVQ_TILE) {
      const int64_t f = f0 + tid;
      float bd = c.prev_pd[f];
      int bi = c.prev_pi[f];
      for (int u = 1; u < g.slices; ++u) {
        const float d = c.prev_pd[(int64_t)u * g.Tpad + f];
        const int i = c.prev_pi[(int64_t)u * g.Tpad + f];
        if (lex_less(d, i, bd, bi)) { bd = d; bi = i; }
      }
      s_code[tid] = bi;
      if (slice == 0 && f < g.T) c.prev_codes[f] = bi;
    }
    __syncthreads();
  }
  for (int e = tid; e < MIMI_RVQ_TILE * q4; e += 256) {
    const int fr = e / q4, k = (e - fr * q4) * 4;
    const int64_t f = f0 + fr;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (f < g.T) {
      v = *reinterpret_cast<const f32x4*>(c.r_in + f * c.ld_in + k);
      if (c.prev_pd) {
        v = v - *reinterpret_cast<const f32x4*>(c.e_prev + (int64_t)s_code[fr] * dq + k);
        if (slice == 0) *reinterpret_cast<f32x4*>(c.r_out + f * dq + k) = v;
      }
    }
    *reinterpret_cast<f32x4*>(sm + fr * RS + k) = v;
  }
  __syncthreads();

  // ---- this stage over the slice: wave w takes the 32-entry blocks w, w + 4, ... of it, in ascending order
  const int h = lane >> 5, col = lane & 31;
  const int j_end = min((slice + 1) * MIMI_RVQ_SLICE, g.bins);
  float best = INFINITY;
  int bi = g.bins - 1;                    // a valid entry whatever happens (no distance below +inf: overflow or NaN in the input)
  for (int jb = slice * MIMI_RVQ_SLICE + wave * 32; jb < j_end; jb += 128) {
    const int ja = min(jb + col, g.bins - 1);             // rows past the codebook read its last row and are masked below
    const float* er = c.e + (int64_t)ja * dq + 4 * h;
    const float* rr = sm + col * RS + 4 * h;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // step 4 (q / 8) + u of half h multiplies k = q + 4 h + u.  32 k per trip: the entries' four float4 of the next trip are in
    // flight under this trip's 16 MFMAs (one load per four MFMAs, issued just before them, left the wave waiting on each)
    auto load4 = [&](f32x4* d, int q) {
#pragma unroll
      for (int t = 0; t < 4; ++t) d[t] = *reinterpret_cast<const f32x4*>(er + q + 8 * t);
    };
    const int q_full = dq & ~31;
    f32x4 cur[4], nxt[4];
    if (q_full) load4(cur, 0);
    for (int q = 0; q < q_full; q += 32) {
      if (q + 32 < q_full) load4(nxt, q + 32);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(rr + q + 8 * t);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(cur[t][u], bv[u], acc, 0, 0, 0);
      }
      if (q + 32 < q_full) {
#pragma unroll
        for (int t = 0; t < 4; ++t) cur[t] = nxt[t];
      }
    }
    for (int q = q_full; q < dq; q += 8) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(er + q);
      const f32x4 bv = *reinterpret_cast<const f32x4*>(rr + q);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
    }
    // the lane holds frame `col` against entries jb + (r & 3) + 8 (r >> 2) + 4 h, ascending in r: `<` keeps the lowest index
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = jb + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (j < g.bins) {
        const float d = c.c2[j] - acc[r];
        if (d < best) { best = d; bi = j; }
      }
    }
  }
  {
    const float od = __shfl_xor(best, 32, 64);
    const int oi = __shfl_xor(bi, 32, 64);
    if (lex_less(od, oi, best, bi)) { best = od; bi = oi; }
  }
  if (lane < 32) { s_d[wave][col] = best; s_i[wave][col] = bi; }
  __syncthreads();
  if (tid < MIMI_RVQ_TILE) {
    float bd = s_d[0][tid];
    int bj = s_i[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) if (lex_less(s_d[w][tid], s_i[w][tid], bd, bj)) { bd = s_d[w][tid]; bj = s_i[w][tid]; }
    c.pd[(int64_t)slice * g.Tpad + f0 + tid] = bd;
    c.pi[(int64_t)slice * g.Tpad + f0 + tid] = bj;
  }
}

__global__ __launch_bounds__(256) void mimi_rvq_finish(const float* __restrict__ pd_a, const int32_t* __restrict__ pi_a, int32_t* __restrict__ codes_a,
                                                       const float* __restrict__ pd_b, const int32_t* __restrict__ pi_b, int32_t* __restrict__ codes_b,
                                                       int64_t T, int64_t Tpad, int slices) {
  const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= T) return;
  const float* pd = blockIdx.y ? pd_b : pd_a;
  const int32_t* pi = blockIdx.y ? pi_b : pi_a;
  float bd = pd[f];
  int bi = pi[f];
  for (int u = 1; u < slices; ++u) {
    const float d = pd[(int64_t)u * Tpad + f];
    const int i = pi[(int64_t)u * Tpad + f];
    if (lex_less(d, i, bd, bi)) { bd = d; bi = i; }
  }
  (blockIdx.y ? codes_b : codes_a)[f] = bi;
}

inline int ok() { return hipGetLastError() == hipSuccess ? 0 : -1; }

}  // namespace

int mimi_edge_rows_launch(const float* x, float* y, int64_t P, int D, int front, int back, hipStream_t s) {
  if (P <= 0 || D <= 0 || D % 4 || front < 0 || back < 0) return -1;
  const int64_t rows = front + P + back, total = rows * (D / 4);
  hipLaunchKernelGGL(mimi_edge_rows, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, s, x, y, P, D, front, rows);
  return ok();
}

int mimi_rvq_stage_launch(const MimiRvqChain& a, const MimiRvqChain& b, int64_t T, int bins, int dq, hipStream_t s) {
  // the residual tile [32][dq + 4] must fit the 64 KB a launch gets without asking for more
  if (T <= 0 || bins <= 0 || dq <= 0 || dq % 8 || dq > 504 || !a.r_in || !a.e || !a.c2 || !a.pd || !a.pi || a.ld_in % 4) return -1;
  if (a.prev_pd && !(a.prev_pi && a.e_prev && a.prev_codes && a.r_out)) return -1;
  if (b.e && (!b.r_in || !b.c2 || !b.pd || !b.pi || b.ld_in % 4 || b.prev_pd)) return -1;
  const int64_t tiles = (T + MIMI_RVQ_TILE - 1) / MIMI_RVQ_TILE;
  const int slices = mimi_rvq_slices(bins);
  if (tiles > 0x7fffffff || slices * 2 > 65535) return -1;
  RvqStageArgs g{a, b, T, tiles * MIMI_RVQ_TILE, bins, dq, slices};
  hipLaunchKernelGGL(mimi_rvq_stage, dim3((unsigned)tiles, (unsigned)(b.e ? 2 * slices : slices)), dim3(256), (size_t)MIMI_RVQ_TILE * (dq + 4) * 4, s, g);
  return ok();
}

int mimi_rvq_finish_launch(const float* pd_a, const int32_t* pi_a, int32_t* codes_a, const float* pd_b, const int32_t* pi_b, int32_t* codes_b,
                           int64_t T, int bins, hipStream_t s) {
  if (T <= 0 || bins <= 0 || !pd_a || !pi_a || !codes_a || (pd_b && !(pi_b && codes_b))) return -1;
  const int64_t Tpad = (T + MIMI_RVQ_TILE - 1) / MIMI_RVQ_TILE * MIMI_RVQ_TILE;
  hipLaunchKernelGGL(mimi_rvq_finish, dim3((unsigned)((T + 255) / 256), pd_b ? 2 : 1), dim3(256), 0, s, pd_a, pi_a, codes_a, pd_b, pi_b, codes_b, T, Tpad,
                     mimi_rvq_slices(bins));
  return ok();
}
