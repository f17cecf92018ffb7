// conv_gemm_w16.hip -- the tap-structured GEMM of codec_kernels.hip on bf16 WEIGHTS and fp32 activations, on the bf16 matrix cores
// (v_mfma_f32_32x32x16_bf16), exact: nothing is rounded on the way to the accumulator.
//
//   Y[row(m)][n] = epi( sum_{tap,c} pre(X[m*x_row_mul + tap*dil - pad][c]) * W[z*w_phase_stride + n*ldw + tap*Cin + c] + bias[n] )
//   row(m) = m*y_row_mul + y_row_off + z*y_phase_step, dropped outside [0, T_out); X rows outside [0, T_in) read as zero
//   pre = identity | leaky-ReLU(lrelu_slope);  epi = (+R) ; (*out_scale when != 0) ; (+R2)   -- conv_gemm_f32's order
//
// The split.  An fp32 value is the exact sum of three bf16 values, hi = rn(v), mid = rn(v - hi), lo = v - hi - mid (8 + 8 + 8
// significand bits; both differences are exact in fp32, and lo needs no rounding), and a bf16 x bf16 product is exact in fp32.  So
// x * w = hi * w + mid * w + lo * w with every product exact, and the GEMM is three bf16 MFMAs per k16 step into ONE fp32 accumulator:
// the result differs from conv_gemm_f32's on the same (bf16-valued) weights by accumulation rounding and order only.
// |v| below about 2^-110 loses low bits of lo to bf16's exponent floor (2^-133): an absolute error below 2^-126 per term, accepted.
// A non-finite activation gives NaN (inf - inf in the split) where the fp32 kernel would give inf.
//
// The work.  256 threads = 2 x 2 waves, block tile (64 WM) x (64 WN): <2,2> = 128 x 128, <2,1> = 128 x 64, <1,1> = 64 x 64, chosen by
// codec_conv_gemm_launch's fill rule.  A stage is 64 k = two 32-channel chunks; a chunk never straddles a tap (Cin % 32 == 0), so a
// stage holds two taps at Cin = 32 and may end mid-tap at Cin = 96; chunks past K are zero.
//   * X: fp32, unconditional clamped 16-byte loads and a mask (a predicated load drains vmcnt, codec_kernels.hip), 8 consecutive k per
//     thread.  When the registers go to LDS the leaky-ReLU and the out-of-range zeroing are applied, THEN the value is split, once per
//     element, and each term goes to its own LDS plane with one ds_write_b128 (splitting after the LDS read would repeat the vector
//     work in the two waves that share every A fragment).
//   * W: bf16, global -> registers -> LDS with no conversion.
//   * LDS rows are 64 k + 8 bf16 of padding = 144 bytes: the MFMA's fragment order (lane l: row l & 31, the 8 consecutive k at
//     8 (l >> 5)) is one ds_read_b128 per operand, and 16 consecutive rows at one k offset cover all 64 banks once.
//   * per k16 step and 32 x 32 tile: 4 ds_read_b128 (three A planes, one B fragment that feeds all three) and 3 MFMAs, added in the
//     fixed order hi, mid, lo.  Stages, k16 steps and terms are visited in an order that depends on (taps, Cin) alone -- never on M,
//     on the tile or on the grid -- so a row's bits do not depend on what it is stacked with (DESIGN.md "Mimi" decision 4).
//   * one LDS buffer (72 KB for 128 x 128, 54 KB for 128 x 64, 36 KB for 64 x 64): the next stage's global loads fly under this
//     stage's MFMAs in registers, and two workgroups per CU (144 KB of the 160) hide each other's barriers.  DESIGN.md section 3 has
//     the reasoning and the registers per instantiation.
#include <algorithm>

#include "codec.h"
#include "mia_device.h"

namespace {

constexpr int W16_RS = 72;       // bf16 elements per LDS row

// v[0..7] -> the three bf16 planes, two values per dword (v_cvt_pk_bf16_f32: round to nearest even)
__device__ __forceinline__ void split3(const float (&v)[8], u32x4& hi, u32x4& mid, u32x4& lo) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = v[2 * j], b = v[2 * j + 1];
    const uint32_t ph = pack2<BF16>(a, b);
    const float a1 = a - __uint_as_float(ph << 16), b1 = b - __uint_as_float(ph & 0xffff0000u);        // exact
    const uint32_t pm = pack2<BF16>(a1, b1);
    const float a2 = a1 - __uint_as_float(pm << 16), b2 = b1 - __uint_as_float(pm & 0xffff0000u);      // exact, 8 bits
    hi[j] = ph; mid[j] = pm; lo[j] = pack2<BF16>(a2, b2);
  }
}

template <int WM, int WN>
__global__ __launch_bounds__(256) void conv_gemm_w16(ConvGemmArgs g, const uint16_t* __restrict__ Wg) {
  constexpr int GBM = 64 * WM, GBN = 64 * WN, GBK = 64;
  constexpr int PLANE = GBM * W16_RS;
  __shared__ __attribute__((aligned(16))) uint16_t As[3 * PLANE];       // hi | mid | lo
  __shared__ __attribute__((aligned(16))) uint16_t Bs[GBN * W16_RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int m0 = blockIdx.x * GBM, n0 = blockIdx.y * GBN;
  const int z = blockIdx.z;
  const uint16_t* __restrict__ W = Wg + (int64_t)z * g.w_phase_stride;
  const float* __restrict__ X = g.X;
  const int Ktot = g.taps * g.Cin;
  const int64_t ldw = g.ldw > 0 ? g.ldw : Ktot;

  // staging: per chunk a thread owns 8 consecutive k (two float4 of X, one 16-byte load of W) of WM rows of A and WN rows of B
  const int s_row = tid >> 2, s_k = (tid & 3) * 8;
  float4 ra[2][WM][2];
  u32x4 rb[2][WN];
  uint32_t amask = 0, bmask = 0;            // bit (ch * 2 + i): element is inside the tensor
  int xr0[WM], xo0[WM];
  int64_t wb[WN];
  uint32_t mok = 0, nok = 0;
  const int ldx_i = (int)g.ldx, xo_max = (g.T_in - 1) * ldx_i;       // host-checked: every row offset fits 31 bits
#pragma unroll
  for (int i = 0; i < WM; ++i) {
    const int m = m0 + s_row + 64 * i;
    xr0[i] = m * g.x_row_mul - g.pad;
    xo0[i] = xr0[i] * ldx_i;
    mok |= (m < g.M ? 1u : 0u) << i;
  }
#pragma unroll
  for (int i = 0; i < WN; ++i) {
    const int n = n0 + s_row + 64 * i;
    wb[i] = (int64_t)(n < g.N ? n : g.N - 1) * ldw + s_k;
    nok |= (n < g.N ? 1u : 0u) << i;
  }
  int tap_b = 0, cb = 0;                    // the stage's first chunk starts at k = tap_b * Cin + cb (stages are visited in order)
  auto load_tiles = [&](int kbase) {
    if (kbase > 0) {                        // advance by one stage (wave-uniform scalar work)
      cb += GBK;
      while (cb >= g.Cin) { cb -= g.Cin; ++tap_b; }
    }
    amask = 0; bmask = 0;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      int tap = tap_b, cc = cb + 32 * ch;
      if (cc >= g.Cin) { cc -= g.Cin; ++tap; }          // cb < Cin and Cin >= 32: at most one wrap
      const bool kin = tap < g.taps;        // == (kbase + 32 ch < Ktot)
      if (!kin) { tap = g.taps - 1; cc = g.Cin - 32; }
      const int k0 = tap * g.Cin + cc;
      const int tapd = tap * g.dil, tapo = tapd * ldx_i;
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const int xr = xr0[i] + tapd;
        const bool ok = kin && ((mok >> i) & 1u) && xr >= 0 && xr < g.T_in;
        const int xo = min(max(xo0[i] + tapo, 0), xo_max);
        const float4* p = reinterpret_cast<const float4*>(X + xo + cc + s_k);
        ra[ch][i][0] = p[0];
        ra[ch][i][1] = p[1];
        amask |= (ok ? 1u : 0u) << (ch * 2 + i);
      }
#pragma unroll
      for (int i = 0; i < WN; ++i) {
        rb[ch][i] = *reinterpret_cast<const u32x4*>(W + wb[i] + k0);
        bmask |= ((kin && ((nok >> i) & 1u)) ? 1u : 0u) << (ch * 2 + i);
      }
    }
  };
  auto store_tiles = [&]() {
    const float slope = g.lrelu_slope;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
#pragma unroll
      for (int i = 0; i < WM; ++i) {
        const float4 q0 = ra[ch][i][0], q1 = ra[ch][i][1];
        float v[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        const bool ok = (amask >> (ch * 2 + i)) & 1u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (slope > 0.f) v[j] = v[j] > 0.f ? v[j] : v[j] * slope;
          if (!ok) v[j] = 0.f;
        }
        u32x4 hi, mid, lo;
        split3(v, hi, mid, lo);
        uint16_t* d = As + (s_row + 64 * i) * W16_RS + 32 * ch + s_k;
        *reinterpret_cast<u32x4*>(d) = hi;
        *reinterpret_cast<u32x4*>(d + PLANE) = mid;
        *reinterpret_cast<u32x4*>(d + 2 * PLANE) = lo;
      }
#pragma unroll
      for (int i = 0; i < WN; ++i) {
        u32x4 w = rb[ch][i];
        if (!((bmask >> (ch * 2 + i)) & 1u)) w = (u32x4){0u, 0u, 0u, 0u};
        *reinterpret_cast<u32x4*>(Bs + (s_row + 64 * i) * W16_RS + 32 * ch + s_k) = w;
      }
    }
  };

  f32x16 acc[WM][WN];
#pragma unroll
  for (int i = 0; i < WM; ++i)
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int a_off = (wr * 32 * WM + (lane & 31)) * W16_RS + 8 * (lane >> 5);
  const int b_off = (wc * 32 * WN + (lane & 31)) * W16_RS + 8 * (lane >> 5);
  const int nk = (Ktot + GBK - 1) / GBK;
  load_tiles(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                       // previous stage fully consumed
    store_tiles();
    __syncthreads();
    if (kt + 1 < nk) load_tiles((kt + 1) * GBK);   // global loads fly under the MFMAs below
    // the fragments of k16 step s + 1 are read before the MFMAs of step s issue (codec_kernels.hip: left to the compiler every MFMA
    // waits on the ds_read in front of it)
    s16x8 fa[2][3][WM], fb[2][WN];
    auto lds_step = [&](int buf, int s) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int i = 0; i < WM; ++i) fa[buf][p][i] = *reinterpret_cast<const s16x8*>(As + p * PLANE + a_off + i * 32 * W16_RS + 16 * s);
#pragma unroll
      for (int j = 0; j < WN; ++j) fb[buf][j] = *reinterpret_cast<const s16x8*>(Bs + b_off + j * 32 * W16_RS + 16 * s);
    };
    lds_step(0, 0);
#pragma unroll
    for (int s = 0; s < GBK / 16; ++s) {
      const int cur = s & 1;
      if (s + 1 < GBK / 16) lds_step(cur ^ 1, s + 1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int p = 0; p < 3; ++p)          // hi, mid, lo: each accumulator takes them in this order; neighbours in issue order are independent
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int j = 0; j < WN; ++j) acc[i][j] = BF16::mfma32(fa[cur][p][i], fb[cur][j], acc[i][j]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // epilogue: lane owns column n = ..+(lane&31), rows (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
  for (int j = 0; j < WN; ++j) {
    const int n = n0 + wc * 32 * WN + j * 32 + (lane & 31);
    if (n >= g.N) continue;
    const float bias = g.bias ? g.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wr * 32 * WM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= g.M) continue;
        const int64_t yr = (int64_t)m * g.y_row_mul + g.y_row_off + (int64_t)z * g.y_phase_step;
        if (yr < 0 || yr >= g.T_out) continue;
        float v = acc[i][j][r] + bias;
        if (g.R) v += g.R[yr * g.ldr + n];
        if (g.out_scale != 0.f) v *= g.out_scale;
        if (g.R2) v += g.R2[yr * g.ldr + n];
        g.Y[yr * g.ldy + n] = v;
      }
  }
}

// fp32 -> bf16, round to nearest even (the copies mia_kokoro_use_w16 forms of the folded weights)
__global__ __launch_bounds__(256) void w16_round(const float* __restrict__ src, uint16_t* __restrict__ dst, int64_t n) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) dst[e] = BF16::from_f32(src[e]);
}

}  // namespace

const char* conv_gemm_w16_check(const ConvGemmArgs& g, const uint16_t* w, bool* unsupported) {
  const char* field = g.W ? "conv_gemm_w16: W must be null (the weights are the bf16 argument)"
                      : g.alpha || g.ralpha ? "conv_gemm_w16: alpha (snake prologue) is not served"
                      : g.elu_pre ? "conv_gemm_w16: elu_pre is not served"
                      : g.noise || g.noise_seq_off ? "conv_gemm_w16: noise is not served"
                      : g.tanh_out ? "conv_gemm_w16: tanh_out is not served"
                      : g.gelu ? "conv_gemm_w16: act is not served"
                      : g.phase_len || g.x_phase_step ? "conv_gemm_w16: phase_len / x_phase_step are not served"
                      : g.n_seq != 1 || g.seq_len ? "conv_gemm_w16: n_seq > 1 / seq_len are not served"
                      : nullptr;
  if (unsupported) *unsupported = field != nullptr;
  if (field) return field;
  if (!w || ((uintptr_t)w & 15)) return "conv_gemm_w16: the bf16 weights must be 16-byte aligned";
  if (const char* e = codec_conv_gemm_check(g)) return e;
  if (g.ldw % 8 || g.w_phase_stride % 8) return "conv_gemm_w16: ldw and w_phase_stride must be multiples of 8 (16-byte rows of bf16)";
  return nullptr;
}

int conv_gemm_w16_launch(const ConvGemmArgs& g, const uint16_t* w, int phases, hipStream_t s, int tile) {
  // codec_conv_gemm_launch's rule: 128-row tiles only when they still give every CU work; otherwise 64 x 64 tiles (4x the workgroups)
  const int64_t big_blocks = (int64_t)((g.M + 127) / 128) * ((g.N + 127) / 128) * phases;
  if (tile == 0) tile = big_blocks < 384 ? 1 : g.N > 64 ? 3 : 2;
  if (tile == 1) hipLaunchKernelGGL((conv_gemm_w16<1, 1>), dim3((g.M + 63) / 64, (g.N + 63) / 64, phases), dim3(256), 0, s, g, w);
  else if (tile == 2) hipLaunchKernelGGL((conv_gemm_w16<2, 1>), dim3((g.M + 127) / 128, (g.N + 63) / 64, phases), dim3(256), 0, s, g, w);
  else if (tile == 3) hipLaunchKernelGGL((conv_gemm_w16<2, 2>), dim3((g.M + 127) / 128, (g.N + 127) / 128, phases), dim3(256), 0, s, g, w);
  else return -1;
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int conv_w16_round_launch(const float* src, uint16_t* dst, int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(w16_round, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, src, dst, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
