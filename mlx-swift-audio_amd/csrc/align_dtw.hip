// align_dtw.hip -- dynamic time warping and its backtrace for the word-timestamp alignment (WhisperTiming.swift:46-130), on the device,
// with the host form it replaces kept beside it (dtw_host: mode 0 of mia_op_dtw and of mia_whisper_set_align_dtw).
//
// The recurrence: acc[i][j] = cost[i-1][j-1] + min-by-rule(acc[i-1][j-1], acc[i-1][j], acc[i][j-1]) in fp32, one add per cell, with the
// host's literal comparisons deciding the move (c0 < c1 && c0 < c2 -> 0, c1 < c0 && c1 < c2 -> 1, else 2).  A cell depends on its three
// predecessors only, so every traversal order gives the host's bits; what is left to design is the order.
//
// Work split (dtw_wave<R>): ONE WAVE PER CLIP, one workgroup of 64 lanes, no atomics, no workgroup waits on another, fixed order.
//   * Lane l owns the R consecutive token rows l*R .. l*R + R - 1 (R = 1 | 2 | 4 | 7 by the batch's largest row count: 64 | 128 | 256 |
//     448 rows) and keeps acc of its rows at the previous column in R registers.
//   * Skewed time: at step t lane l works on column j = t - l.  The two values it needs from the row above its block -- acc at columns j
//     and j - 1 of lane l - 1's bottom row -- are that lane's results of the last two steps: ONE one-lane DPP shift (wave_shr:1, a VALU
//     modifier, no LDS crossbar) per step brings the first, the second is the value the previous step brought.  No barrier in the loop.
//     Columns outside [0, M) need no predicate: with cost 0 there a lane that has not started keeps +inf (0 + inf), which is exactly the
//     border column, and a lane that has finished is read by nobody.  A clip takes M + ceil(N / R) - 1 steps of R cells.
//   * Cost loads do not depend on acc: each lane fetches its R rows four columns at a time (one 16-byte load per row where the four lie
//     inside the row), one group of four steps ahead of their use.
//   * Moves are 2 bits per cell.  A lane packs 16 STEPS of a row into one register, so all lanes flush together every 16 steps, as
//     whole dwords, coalesced: trace[step / 16][r][lane].  The cell (i, j) lives at step j + i / R, which the backtrace recomputes.
//   * Backtrace, same wave: the path is monotone in both indices, so its step index never grows.  The trace comes back through LDS in
//     chunks of 256 steps (16 dwords x R x 64 lanes, contiguous in memory, <= 28 KB), newest first; lane 0 walks inside a chunk on LDS
//     (re-reading a dword only when the row or the 16-step group changes), files the path backwards in LDS, and the wave writes it out
//     forwards, coalesced.  A path longer than path_cap is not written; its length is, and the host call fails on it.
// Bound: latency.  One wave per clip keeps one SIMD per clip busy with a dependent chain of about 12 VALU operations per cell; the
// memory traffic (cost once, 2 bits per cell out and back) is negligible beside it.
#include <algorithm>
#include <cmath>

#include "align_dtw.h"

void dtw_host(const float* cost, int N, int M, int64_t ld, std::vector<int32_t>& ti, std::vector<int32_t>& tj) {
  const int R = N + 1, Cc = M + 1;
  std::vector<float> acc((size_t)R * Cc, INFINITY);
  std::vector<int8_t> tr((size_t)R * Cc, -1);
  acc[0] = 0.f;
  for (int j = 1; j <= M; ++j)
    for (int i = 1; i <= N; ++i) {
      const float c0 = acc[(size_t)(i - 1) * Cc + j - 1], c1 = acc[(size_t)(i - 1) * Cc + j], c2 = acc[(size_t)i * Cc + j - 1];
      float c; int8_t t;
      if (c0 < c1 && c0 < c2) { c = c0; t = 0; } else if (c1 < c0 && c1 < c2) { c = c1; t = 1; } else { c = c2; t = 2; }
      acc[(size_t)i * Cc + j] = cost[(int64_t)(i - 1) * ld + (j - 1)] + c;
      tr[(size_t)i * Cc + j] = t;
    }
  for (int j = 0; j < Cc; ++j) tr[j] = 2;
  for (int i = 0; i < R; ++i) tr[(size_t)i * Cc] = 1;
  int i = N, j = M;
  ti.clear(); tj.clear();
  while (i > 0 || j > 0) {
    ti.push_back(i - 1); tj.push_back(j - 1);
    const int8_t t = tr[(size_t)i * Cc + j];
    if (t == 0) { --i; --j; } else if (t == 1) --i; else if (t == 2) --j; else { if (i > 0) --i; if (j > 0) --j; }
  }
  std::reverse(ti.begin(), ti.end()); std::reverse(tj.begin(), tj.end());
}

namespace {

constexpr int DTW_CHUNK_WORDS = 16;      // trace dwords (16 steps each) per LDS chunk: 256 steps

struct __attribute__((packed, aligned(4))) DtwCost4 { float v[4]; };      // four columns of a row: 4-byte aligned, whatever ld is

// bottom-row value of the lane above (lane 0: the border row, +inf)
__device__ __forceinline__ float dtw_from_above(float bottom, int lane) {
  const int inf = __builtin_bit_cast(int, INFINITY);
  const int v = __builtin_amdgcn_update_dpp(inf, __builtin_bit_cast(int, bottom), 0x138, 0xf, 0xf, false);     // wave_shr:1
  return lane == 0 ? INFINITY : __builtin_bit_cast(float, v);
}

template <int R>
__global__ __launch_bounds__(64) void dtw_wave(DtwArgs a, int64_t trace_stride) {
  __shared__ uint32_t chunk[DTW_CHUNK_WORDS * R * 64];
  __shared__ uint32_t pbuf[DTW_MAX_ROWS + DTW_MAX_COLS];      // the path backwards: i | j << 16 (1-based cell indices)
  __shared__ int s_len;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int N = a.n_rows[b] - a.row_sub, M = a.n_cols[b];
  if (N < 1 || N > R * 64 || N > a.max_rows || M < 1 || M > a.max_cols) {      // the host refuses these; never index by them
    if (lane == 0) a.path_len[b] = 0;
    return;
  }
  const float* cost = a.cost + (int64_t)b * a.clip_stride;
  uint32_t* tr = a.trace + (int64_t)b * trace_stride;
  const int64_t ld = a.ld;
  const int n_lanes = (N + R - 1) / R, steps = M + n_lanes - 1, TW = (steps + 15) >> 4;
  const int row0 = lane * R;

  // four columns, starting at step t0, of this lane's R rows.  Rows past N - 1 and columns past M - 1 are read by nobody and take the
  // last row's / column's values; columns before 0 must be finite (0) so that +inf stays +inf there.  Offsets fit 32 bits (dtw_check).
  int roff[R];
#pragma unroll
  for (int r = 0; r < R; ++r) roff[r] = min(row0 + r, N - 1) * (int)ld;
  auto load4 = [&](float (&dst)[R][4], int t0) {
    const int j = t0 - lane;
    if (t0 >= 63 && t0 + 3 < M) {              // wave-uniform: every lane's four columns lie inside the row
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const DtwCost4 v = *reinterpret_cast<const DtwCost4*>(cost + roff[r] + j);
#pragma unroll
        for (int s = 0; s < 4; ++s) dst[r][s] = v.v[s];
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float v = cost[roff[r] + min(max(j + s, 0), M - 1)];
          dst[r][s] = j + s >= 0 ? v : 0.f;
        }
    }
  };

  float left[R];                               // acc[row][j - 1] of this lane's rows; +inf: the border column
#pragma unroll
  for (int r = 0; r < R; ++r) left[r] = INFINITY;
  float bottom = INFINITY;                     // left[R - 1] as the lane below reads it
  float diag = lane == 0 ? 0.f : INFINITY;     // acc[row0 - 1][j - 1]: acc[0][0] = 0 for the very first cell, +inf on every other border
  float cur[R][4], nxt[R][4];
  load4(cur, 0);
  for (int tw = 0; tw < TW; ++tw) {
    uint32_t bits[R];
#pragma unroll
    for (int r = 0; r < R; ++r) bits[r] = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      load4(nxt, tw * 16 + q * 4 + 4);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const float up = dtw_from_above(bottom, lane);      // acc[row0 - 1][j]
        float c0 = diag, c1 = up;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float c2 = left[r];
          const bool m0 = c0 < c1 && c0 < c2, m1 = c1 < c0 && c1 < c2;
          const float c = m0 ? c0 : (m1 ? c1 : c2);
          bits[r] |= m0 ? 0u : (m1 ? 1u << (2 * (q * 4 + s)) : 2u << (2 * (q * 4 + s)));
          const float v = cur[r][s] + c;
          c0 = c2; c1 = v; left[r] = v;
        }
        bottom = c1; diag = up;
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int s = 0; s < 4; ++s) cur[r][s] = nxt[r][s];
    }
#pragma unroll
    for (int r = 0; r < R; ++r) tr[((int64_t)tw * R + r) * 64 + lane] = bits[r];
  }

  // ---- backtrace: chunks of the trace through LDS, newest first; lane 0 walks
  __threadfence_block();
  int i = N, j = M, len = 0;                   // lane 0's walk (cell indices, 1-based; 0 = border)
  int have = -1; uint32_t word = 0u;           // the trace dword lane 0 holds: key = step group * 512 + row
  for (int c = (TW - 1) / DTW_CHUNK_WORDS; c >= 0; --c) {
    __syncthreads();                           // the trace stores / the walk on the previous chunk are done
    const int n_words = min(DTW_CHUNK_WORDS, TW - c * DTW_CHUNK_WORDS) * R * 64;
    const uint32_t* src = tr + (int64_t)c * DTW_CHUNK_WORDS * R * 64;
    for (int k = lane; k < n_words; k += 64) chunk[k] = src[k];
    __syncthreads();
    if (lane == 0) {
      while (i > 0 || j > 0) {
        int mv;
        if (i == 0) mv = 2;                    // trace row 0
        else if (j == 0) mv = 1;               // trace column 0
        else {
          const int owner = (i - 1) / R, r = (i - 1) - owner * R, t = (j - 1) + owner;
          if (t < c * DTW_CHUNK_WORDS * 16) break;      // in an older chunk
          const int key = (t >> 4) * 512 + i;
          if (key != have) { word = chunk[(((t >> 4) - c * DTW_CHUNK_WORDS) * R + r) * 64 + owner]; have = key; }
          mv = (word >> (2 * (t & 15))) & 3u;
        }
        pbuf[len++] = (uint32_t)i | ((uint32_t)j << 16);      // at most N + M entries: every move lowers i + j
        if (mv == 0) { --i; --j; } else if (mv == 1) --i; else --j;
      }
    }
  }
  if (lane == 0) { s_len = len; a.path_len[b] = len; }
  __syncthreads();
  const int L = s_len;
  if (L > a.path_cap) return;                  // reported through path_len; nothing is written
  int32_t* ti = a.text_idx + (int64_t)b * a.path_cap;
  int32_t* tj = a.time_idx + (int64_t)b * a.path_cap;
  for (int k = lane; k < L; k += 64) {
    const uint32_t v = pbuf[L - 1 - k];
    ti[k] = (int32_t)(v & 0xffffu) - 1;
    tj[k] = (int32_t)(v >> 16) - 1;
  }
}

int dtw_rows_per_lane(int max_rows) { return max_rows <= 64 ? 1 : max_rows <= 128 ? 2 : max_rows <= 256 ? 4 : 7; }
int64_t dtw_trace_stride(int max_rows, int max_cols) {      // dwords per clip: every step group x R x 64 lanes
  return (int64_t)((max_cols + 63 + 15) / 16) * dtw_rows_per_lane(max_rows) * 64;
}

}  // namespace

size_t dtw_trace_bytes(int B, int max_rows, int max_cols) { return (size_t)B * dtw_trace_stride(max_rows, max_cols) * 4; }

const char* dtw_check(const DtwArgs& a) {
  if (!a.cost || !a.n_rows || !a.n_cols || !a.trace || !a.text_idx || !a.time_idx || !a.path_len) return "dtw: null pointer";
  if (a.B <= 0 || a.path_cap <= 0 || a.row_sub < 0 || a.clip_stride < 0) return "dtw: bad argument";
  if (a.max_rows < 1 || a.max_rows > DTW_MAX_ROWS || a.max_cols < 1 || a.max_cols > DTW_MAX_COLS) return "dtw: at most 448 rows and 1500 columns";
  if (a.ld < a.max_cols || a.max_rows * a.ld >= (1ll << 31)) return "dtw: ld must cover the row, a clip stay below 2^31 elements";
  return nullptr;
}

int dtw_launch(const DtwArgs& a, hipStream_t s) {
  if (dtw_check(a)) return -1;
  const int64_t stride = dtw_trace_stride(a.max_rows, a.max_cols);
  switch (dtw_rows_per_lane(a.max_rows)) {
    case 1: hipLaunchKernelGGL(dtw_wave<1>, dim3(a.B), dim3(64), 0, s, a, stride); break;
    case 2: hipLaunchKernelGGL(dtw_wave<2>, dim3(a.B), dim3(64), 0, s, a, stride); break;
    case 4: hipLaunchKernelGGL(dtw_wave<4>, dim3(a.B), dim3(64), 0, s, a, stride); break;
    default: hipLaunchKernelGGL(dtw_wave<7>, dim3(a.B), dim3(64), 0, s, a, stride); break;
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// DTW of B cost matrices without a model around them.  mode 0: dtw_host; mode 1: upload + dtw_wave.  Host pointers.
extern "C" int mia_op_dtw(mia_ctx* ctx, const float* cost, int B, int rows, int64_t ld, const int32_t* n_rows, const int32_t* n_cols, int mode,
                          int32_t* text_idx, int32_t* time_idx, int32_t* path_len, int path_cap) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, cost && n_rows && n_cols && text_idx && time_idx && path_len, "op_dtw: null pointer");
  MIA_CHECK_ARG(ctx, B > 0 && rows > 0 && ld > 0 && path_cap > 0 && (int64_t)B * rows * ld < (1ll << 31), "op_dtw: bad shape");
  MIA_CHECK_ARG(ctx, mode == 0 || mode == 1, "op_dtw: mode must be 0 (host) or 1 (device), got %d", mode);
  int max_rows = 0, max_cols = 0;
  for (int b = 0; b < B; ++b) {
    MIA_CHECK_ARG(ctx, n_rows[b] >= 1 && n_rows[b] <= rows && n_cols[b] >= 1 && n_cols[b] <= ld, "op_dtw: clip %d: %d x %d outside [1, %d] x [1, %lld]",
                  b, n_rows[b], n_cols[b], rows, (long long)ld);
    max_rows = std::max(max_rows, n_rows[b]); max_cols = std::max(max_cols, n_cols[b]);
  }
  if (mode == 0) {
    std::vector<int32_t> ti, tj;
    for (int b = 0; b < B; ++b) {
      dtw_host(cost + (size_t)b * rows * ld, n_rows[b], n_cols[b], ld, ti, tj);
      if ((int)ti.size() > path_cap) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_dtw: path_cap %d too small (need %zu)", path_cap, ti.size());
      path_len[b] = (int32_t)ti.size();
      std::copy(ti.begin(), ti.end(), text_idx + (size_t)b * path_cap);
      std::copy(tj.begin(), tj.end(), time_idx + (size_t)b * path_cap);
    }
    return MIA_OK;
  }
  if (max_rows > DTW_MAX_ROWS || max_cols > DTW_MAX_COLS)
    return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "op_dtw: the device DTW takes at most %d x %d (got %d x %d)", DTW_MAX_ROWS, DTW_MAX_COLS, max_rows, max_cols);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const int cap = std::min(path_cap, max_rows + max_cols);      // no path is longer: a shorter device buffer loses nothing
  std::vector<int32_t> got((size_t)(2 * cap + 1) * B);          // [text | time][B][cap], lengths [B]; before io: it must outlive it
  HostIo io = HostIo::host(ctx);
  const size_t cb = (size_t)B * rows * ld * 4;
  Carve cv;
  const size_t o_cost = cv.add(cb), o_nr = cv.add((size_t)B * 4), o_nc = cv.add((size_t)B * 4), o_out = cv.add(got.size() * 4),
               o_tr = cv.add(dtw_trace_bytes(B, max_rows, max_cols));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  DtwArgs a;
  a.cost = io.in(cost, ws + o_cost, cb); a.clip_stride = (int64_t)rows * ld; a.ld = ld;
  a.n_rows = io.in(n_rows, ws + o_nr, (size_t)B * 4); a.n_cols = io.in(n_cols, ws + o_nc, (size_t)B * 4);
  a.B = B; a.max_rows = max_rows; a.max_cols = max_cols; a.trace = (uint32_t*)(ws + o_tr);
  a.text_idx = (int32_t*)(ws + o_out); a.time_idx = a.text_idx + (size_t)B * cap; a.path_len = a.time_idx + (size_t)B * cap; a.path_cap = cap;
  if (const char* e = dtw_check(a)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_%s", e);
  if (dtw_launch(a, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_dtw: launch failed");
  io.fetch(got.data(), a.text_idx, got.size() * 4);
  if (int rc = io.finish()) return rc;
  const int32_t* len = got.data() + (size_t)2 * B * cap;
  for (int b = 0; b < B; ++b) {
    if (len[b] > path_cap) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "op_dtw: path_cap %d too small (need %zu)", path_cap, (size_t)len[b]);
    path_len[b] = len[b];
    std::copy(got.data() + (size_t)b * cap, got.data() + (size_t)b * cap + len[b], text_idx + (size_t)b * path_cap);
    std::copy(got.data() + (size_t)(B + b) * cap, got.data() + (size_t)(B + b) * cap + len[b], time_idx + (size_t)b * path_cap);
  }
  return MIA_OK;
}
