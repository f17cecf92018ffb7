// kokoro_lstm.hip -- Kokoro's bidirectional LSTM (TTS/Kokoro/BuildingBlocks/LSTM.swift), fp32, gfx950, B = 1.
//
// The input projection of both directions is one launch of the fp32 tap GEMM: xproj [T][8 H] = x W_ih^T + (b_ih + b_hh).  The
// recurrence is ONE LAUNCH PER TIME STEP carrying both directions: the stream orders the steps, so no workgroup ever waits on another
// (no flag, no grid barrier, no cooperative launch -- DESIGN.md, "Kokoro text half", decision 2).
//
// Step kernel: grid (H / 16, 2 directions), 256 threads.  A workgroup owns 16 hidden units, i.e. the 64 rows of W_hh that feed their
// i, f, g, o gates; the repack at load makes those 64 rows one contiguous slice (64 KB at H = 256, resident in L2 across the steps).
// A wave owns 4 units; its four 16-lane groups each own one unit and walk its four gate rows, lane l reading the 16-byte pieces
// l, l + 16, ... of the row (256 contiguous bytes per group and load).  The previous h comes straight from the output buffer (row
// t - 1, columns [0, H) forward; row t + 1, columns [H, 2 H) reverse) into registers, once per lane for all four rows.  A row's dot
// product is the lane's fma chain in column order, then the xor tree 8, 4, 2, 1 inside the group: a fixed order, no atomics.  Lane 0
// of a group then holds all four gate sums of its unit and applies them (expf / tanhf, not the fast intrinsics), updates c in
// the [2][H] state buffer and writes h into out[t][dir H + j].  The first step of a direction reads no state at all.
#include "../../include/mia.h"
#include "codec.h"
#include "kokoro_text.h"

namespace {

// every element of the packed block from the raw tensors: one thread per destination element
__global__ __launch_bounds__(256) void kokoro_lstm_pack(KokoroLstmRaw raw, int In, int H, float* __restrict__ dst) {
  const int64_t n_ih = (int64_t)8 * H * In, n_b = 8 * H, n_hh = (int64_t)8 * H * H;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_ih + n_b + n_hh) return;
  float v;
  if (i < n_ih) {
    const int64_t r = i / In; const int d = (int)(r / (4 * H));
    v = raw.w_ih[d][i - (int64_t)d * 4 * H * In];
  } else if (i < n_ih + n_b) {
    const int r = (int)(i - n_ih), d = r / (4 * H), q = r - d * 4 * H;
    v = raw.b_ih[d][q] + raw.b_hh[d][q];
  } else {
    int64_t k = i - n_ih - n_b;                                   // [d][blk][gate][u][col]
    const int col = (int)(k % H); k /= H;
    const int u = (int)(k % KOKORO_LSTM_U); k /= KOKORO_LSTM_U;
    const int gate = (int)(k % 4); k /= 4;
    const int nblk = H / KOKORO_LSTM_U, blk = (int)(k % nblk), d = (int)(k / nblk);
    v = raw.w_hh[d][((int64_t)gate * H + blk * KOKORO_LSTM_U + u) * H + col];
  }
  dst[i] = v;
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// step s of T: the forward direction is at row s, the reverse one at row T - 1 - s
__global__ __launch_bounds__(256) void kokoro_lstm_step(const float* __restrict__ xproj, const float* __restrict__ whh, float* out, int64_t ldo,
                                                        float* __restrict__ c, int s, int T, int H) {
  const int dir = blockIdx.y, blk = blockIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> 4, l16 = lane & 15;
  const int u = wave * 4 + grp, j = blk * KOKORO_LSTM_U + u;
  const int64_t row = dir ? T - 1 - s : s;
  const int H4 = H >> 2;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (s > 0) {
    const float4* hp = reinterpret_cast<const float4*>(out + (dir ? row + 1 : row - 1) * ldo + dir * H);
    float4 hv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k4 = l16 + 16 * i; hv[i] = k4 < H4 ? hp[k4] : make_float4(0.f, 0.f, 0.f, 0.f); }
    const float4* wp = reinterpret_cast<const float4*>(whh + ((int64_t)(dir * gridDim.x + blk) * 4 * KOKORO_LSTM_U) * H);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4* wr = wp + (int64_t)(q * KOKORO_LSTM_U + u) * H4;
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int k4 = l16 + 16 * i;
        if (k4 < H4) {
          const float4 w = wr[k4];
          a = fmaf(w.x, hv[i].x, a); a = fmaf(w.y, hv[i].y, a); a = fmaf(w.z, hv[i].z, a); a = fmaf(w.w, hv[i].w, a);
        }
      }
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o);
      acc[q] = a;
    }
  }
  if (l16 == 0) {
    const float* xp = xproj + row * (8 * (int64_t)H) + dir * 4 * H + j;
    const float gi = sigmoidf(xp[0] + acc[0]), gf = sigmoidf(xp[H] + acc[1]);
    const float gg = tanhf(xp[2 * H] + acc[2]), go = sigmoidf(xp[3 * H] + acc[3]);
    const float cp = s > 0 ? c[dir * H + j] : 0.f;
    const float cn = gf * cp + gi * gg;
    c[dir * H + j] = cn;
    out[row * ldo + dir * H + j] = go * tanhf(cn);
  }
}

}  // namespace

int kokoro_lstm_pack_launch(const KokoroLstmRaw& raw, int In, int H, float* block, KokoroLstm& w, hipStream_t st) {
  if (!kokoro_lstm_shape_ok(In, H) || ((uintptr_t)block & 15)) return 1;
  const size_t n = kokoro_lstm_floats(In, H);
  hipLaunchKernelGGL(kokoro_lstm_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, raw, In, H, block);
  w.wih = block; w.bias = block + (size_t)8 * H * In; w.whh = w.bias + 8 * H; w.In = In; w.H = H;
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

int kokoro_lstm_run(mia_ctx* ctx, const KokoroLstm& w, const float* x, int64_t ldx, int64_t T, float* scratch, float* out, int64_t ldo) {
  const int H = w.H;
  if (!kokoro_lstm_shape_ok(w.In, H)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "bilstm: H must be a multiple of 16 up to 256 and In a multiple of 32 up to 1024 (got H %d, In %d)", H, w.In);
  if (T < 1 || T > KOKORO_MAX_ROWS) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "bilstm: the row count must be in [1, %d] (got %lld)", KOKORO_MAX_ROWS, (long long)T);
  if (!x || !out || ldx < w.In || ldo < 2 * H || ldx % 4 || ldo % 4 || ((uintptr_t)x & 15) || ((uintptr_t)out & 15) || ((uintptr_t)scratch & 15))
    return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "bilstm: rows must be 16-byte aligned and as wide as In / 2 H");
  float* xproj = scratch; float* c = scratch + (size_t)T * 8 * H;
  ConvGemmArgs g;
  g.X = x; g.ldx = ldx; g.T_in = (int)T; g.W = w.wih; g.bias = w.bias;
  g.Y = xproj; g.ldy = 8 * H; g.T_out = (int)T; g.M = (int)T; g.N = 8 * H; g.Cin = w.In;
  if (int rc = codec_conv_gemm_run(ctx, g, 1, "bilstm")) return rc;
  const dim3 grid((unsigned)(H / KOKORO_LSTM_U), 2);
  for (int s = 0; s < (int)T; ++s)
    hipLaunchKernelGGL(kokoro_lstm_step, grid, dim3(256), 0, ctx->stream, xproj, w.whh, out, ldo, c, s, (int)T, H);
  if (hipGetLastError() != hipSuccess) return mia_fail(ctx, MIA_ERR_DEVICE, "bilstm: kernel launch failed");
  return MIA_OK;
}

extern "C" int mia_op_bilstm(mia_ctx* ctx, const float* x, int64_t ldx, int64_t T, int In, int H, const float* w_ih, const float* w_hh,
                             const float* b_ih, const float* b_hh, const float* w_ih_r, const float* w_hh_r, const float* b_ih_r,
                             const float* b_hh_r, float* out, int64_t ldo) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, w_ih && w_hh && b_ih && b_hh && w_ih_r && w_hh_r && b_ih_r && b_hh_r, "op_bilstm: null weight");
  MIA_CHECK_ARG(ctx, kokoro_lstm_shape_ok(In, H), "op_bilstm: H must be a multiple of 16 up to 256 and In a multiple of 32 up to 1024 (got H %d, In %d)", H, In);
  MIA_CHECK_ARG(ctx, T >= 1 && T <= KOKORO_MAX_ROWS, "op_bilstm: the row count must be in [1, %d] (got %lld)", KOKORO_MAX_ROWS, (long long)T);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const size_t packed = align_up(kokoro_lstm_floats(In, H), 64);
  float* ws = (float*)mia_workspace(ctx, (packed + kokoro_lstm_scratch(T, H)) * 4);
  if (!ws) return MIA_ERR_OUT_OF_MEMORY;
  const KokoroLstmRaw raw = {{w_ih, w_ih_r}, {w_hh, w_hh_r}, {b_ih, b_ih_r}, {b_hh, b_hh_r}};
  KokoroLstm w;
  if (kokoro_lstm_pack_launch(raw, In, H, ws, w, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "op_bilstm: repack launch failed");
  return kokoro_lstm_run(ctx, w, x, ldx, T, ws + packed, out, ldo);
}
