// kokoro_kernels.hip -- the kernels Kokoro's decoder and F0 / N predictor need beside the fp32 tap GEMM (codec_kernels.hip), gfx950:
// style rows, instance-norm statistics, AdaIN + activation, the depthwise transposed "pool", the harmonic source, STFT 20 / 5 and
// its inverse.  Launch interface: kokoro.h; layer programs: kokoro.hip.
#include <algorithm>

#include "kokoro.h"

namespace {

constexpr float KOKORO_EPS = 1e-5f;                 // InstanceNorm1d.swift (eps of the normalisation)
constexpr int INORM_CH = 64, INORM_LANES = 4;       // a workgroup: 64 channels (one 256-byte row segment per wave) x 4 row lanes

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// one wave per output row
__global__ __launch_bounds__(256) void kokoro_style_rows(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ s,
                                                         float* __restrict__ out, int rows, int sd) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  float acc = 0.f;
  for (int k = lane; k < sd; k += 64) acc = fmaf(W[(int64_t)r * sd + k], s[k], acc);
  acc = wave_sum(acc);
  if (lane == 0) out[r] = acc + b[r];
}

// slice partials: grid (channel groups of 64, slices of `rows` rows).  Every thread of a channel sums x - K and (x - K)^2 with the SAME
// shift K = the channel's first row, so the partials of the four row lanes (through LDS, in lane order) and of the slices (in the final
// kernel, in slice order) combine by plain addition.  A channel whose mean dwarfs its spread loses nothing: x - K is exact there, and
// the cancellation left in Q - S^2 / n is that of data whose mean lies about one spread from zero.  (Chan's rule on fp32 slice means
// was tried first: a mean near 100 is rounded to 4e-6 at every combine, which is 4e-4 of a spread of 0.01.)
__global__ __launch_bounds__(256) void kokoro_inorm_partial(const float* __restrict__ x, int64_t ld, int64_t T, int C, int rows,
                                                            float* __restrict__ part) {
  __shared__ float sh[2][INORM_LANES][INORM_CH];
  const int tx = threadIdx.x & (INORM_CH - 1), ty = threadIdx.x >> 6;
  const int c = blockIdx.x * INORM_CH + tx;
  const int64_t r0 = (int64_t)blockIdx.y * rows, r1 = min(T, r0 + rows);
  float s = 0.f, q = 0.f;
  if (c < C) {
    const float K = x[c];
    for (int64_t r = r0 + ty; r < r1; r += INORM_LANES) {
      const float d = x[r * ld + c] - K;
      s += d; q += d * d;
    }
  }
  sh[0][ty][tx] = s; sh[1][ty][tx] = q;
  __syncthreads();
  if (ty == 0 && c < C) {
    for (int l = 1; l < INORM_LANES; ++l) { s += sh[0][l][tx]; q += sh[1][l][tx]; }
    const int64_t S = gridDim.y;
    part[((int64_t)0 * S + blockIdx.y) * C + c] = s;
    part[((int64_t)1 * S + blockIdx.y) * C + c] = q;
  }
}

// one thread per channel: the slices in order, population variance (MLX.variance), then what the caller asked for (kokoro.h)
__global__ __launch_bounds__(256) void kokoro_inorm_final(const float* __restrict__ x, const float* __restrict__ part, int S, int C, float n,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int C_style,
                                                          float* __restrict__ out0, float* __restrict__ out1, float* __restrict__ out2) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f, q = 0.f;
  for (int i = 0; i < S; ++i) { s += part[((int64_t)0 * S + i) * C + c]; q += part[((int64_t)1 * S + i) * C + c]; }
  const float m = x[c] + s / n;
  const float var = __fdiv_rn(fmaxf(q - s * (s / n), 0.f), n);
  const float rstd = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(var, KOKORO_EPS)));
  if (!gamma) { out0[c] = m; out1[c] = rstd; return; }
  const bool live = c < C_style;
  out0[c] = live ? m : 0.f;
  out1[c] = live ? (1.0f + gamma[c]) * rstd : 0.f;
  out2[c] = live ? beta[c] : 0.f;
}

template <bool SNAKE>
__global__ __launch_bounds__(256) void kokoro_adain_act(const float* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy, int64_t T,
                                                        int C4, const float4* __restrict__ mean, const float4* __restrict__ a,
                                                        const float4* __restrict__ beta, const float4* __restrict__ alpha,
                                                        const float4* __restrict__ ralpha, float slope) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= T * C4) return;
  const int64_t t = i / C4; const int c4 = (int)(i - t * C4);
  const float4 v = *reinterpret_cast<const float4*>(x + t * ldx + 4 * c4);
  const float4 mu = mean[c4], sc = a[c4], be = beta[c4];
  float r[4] = {sc.x * (v.x - mu.x) + be.x, sc.y * (v.y - mu.y) + be.y, sc.z * (v.z - mu.z) + be.z, sc.w * (v.w - mu.w) + be.w};
  if (SNAKE) {
    const float4 al = alpha[c4], ra = ralpha[c4];
    const float av[4] = {al.x, al.y, al.z, al.w}, rv[4] = {ra.x, ra.y, ra.z, ra.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float sn = sinf(av[k] * r[k]); r[k] = r[k] + rv[k] * (sn * sn); }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = r[k] > 0.f ? r[k] : slope * r[k];
  }
  *reinterpret_cast<float4*>(y + t * ldy + 4 * c4) = make_float4(r[0], r[1], r[2], r[3]);
}

// ConvTransposed1d k 3 / stride 2 / pad 1 per channel, y'[2 i - 1 + k] += x[i] w[k], then one zero row in front:
//   y[0] = 0 (no bias: it is padding), y[2 j + 1] = x[j] w[1] + b, y[2 j + 2] = x[j] w[2] + x[j + 1] w[0] + b   (j + 1 < T)
__global__ __launch_bounds__(256) void kokoro_pool(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ w,
                                                   const float* __restrict__ bias, int64_t T, int C) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * T * C) return;
  const int64_t r = i / C; const int c = (int)(i - r * C);
  float v = 0.f;
  if (r > 0) {
    const int64_t o = r - 1, j = o >> 1;
    if (o & 1) v = x[j * C + c] * w[c * 3 + 2] + x[(j + 1) * C + c] * w[c * 3 + 0] + bias[c];      // o = 2 j + 1 <= 2 T - 3: j + 1 < T
    else v = x[j * C + c] * w[c * 3 + 1] + bias[c];
  }
  y[i] = v;
}

__global__ __launch_bounds__(256) void kokoro_pack(const float* __restrict__ in, float* __restrict__ out, int64_t ld, int col0, int C, int64_t T) {
  __shared__ float tile[32][33];
  const int64_t t0 = (int64_t)blockIdx.x * 32; const int c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i; const int64_t t = t0 + tx;
    tile[i][tx] = (c < C && t < T) ? in[(int64_t)c * T + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int64_t t = t0 + i; const int c = c0 + tx;
    if (t < T && c < C) out[t * ld + col0 + c] = tile[tx][i];
  }
}

__global__ __launch_bounds__(256) void kokoro_curve_cols(const float* __restrict__ f0, const float* __restrict__ nn, const float* __restrict__ wf,
                                                         const float* __restrict__ wn, float* __restrict__ o1, int64_t ld1, int col1,
                                                         float* __restrict__ o2, int64_t ld2, int col2, int64_t T) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= T) return;
  float a = 0.f, b = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int64_t q = 2 * t + k - 1;
    if (q >= 0 && q < 2 * T) { a += wf[k] * f0[q]; b += wn[k] * nn[q]; }
  }
  a += wf[3]; b += wn[3];
  o1[t * ld1 + col1] = a; o1[t * ld1 + col1 + 1] = b;
  if (o2) { o2[t * ld2 + col2] = a; o2[t * ld2 + col2 + 1] = b; }
}

// P[i][h] = ((cumsum_i(rad_h) 2) pi) up, rad_h[i] = ((f0[i] (h + 1)) / sr) mod 1 with the sign of the divisor (KokoroSineGen.swift:43-58;
// the 1 / up down-interpolation of the piecewise-constant full-rate track returns the frame's own value: 0.5 x + 0.5 x)
__global__ __launch_bounds__(256) void kokoro_phase_scan(const float* __restrict__ f0, float* __restrict__ P, int64_t L, int H, float sr, float up) {
  __shared__ float sf[1024];
  float c = 0.f;
  const int h = threadIdx.x;
  for (int64_t base = 0; base < L; base += 1024) {
    const int n = (int)min((int64_t)1024, L - base);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) sf[i] = f0[base + i];
    __syncthreads();
    if (h < H) {
      const float hm = (float)(h + 1);
      for (int i = 0; i < n; ++i) {
        float rad = fmodf(__fdiv_rn(__fmul_rn(sf[i], hm), sr), 1.0f);
        if (rad < 0.f) rad = __fadd_rn(rad, 1.0f);
        c = __fadd_rn(c, rad);
        P[(base + i) * H + h] = __fmul_rn(__fmul_rn(__fmul_rn(c, 2.0f), 3.14159274101257324f), up);
      }
    }
  }
}

// one thread per sample j: x = (j scale + 0.5 scale) - 0.5, lo = floor(x) (-1 for the first up / 2 samples: that row is the LAST one,
// as a negative index of the reference's gather counts from the end), hi = min(lo + 1, L - 1)   (Interpolate.swift:80-111)
__global__ __launch_bounds__(256) void kokoro_source(const float* __restrict__ f0, const float* __restrict__ P, const float* __restrict__ noise,
                                                     const float* __restrict__ lw, float lb, float* __restrict__ src, int64_t L, int up, int H,
                                                     float scale, float thr) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= L * up) return;
  const float xf = __fsub_rn(__fadd_rn(__fmul_rn((float)j, scale), __fmul_rn(0.5f, scale)), 0.5f);
  const float lo = floorf(xf);
  int64_t ilo = (int64_t)lo;
  const int64_t ihi = min(ilo + 1, L - 1);
  const float wh = __fsub_rn(xf, lo), wl = __fsub_rn(1.0f, wh);
  if (ilo < 0) ilo += L;
  if (ilo > L - 1) ilo = L - 1;                     // never taken for L <= 20000 (checked on the host side of the restatement); keeps the read in bounds
  const float f = f0[j / up];
  const float uv = f > thr ? 1.f : 0.f;
  const float namp = __fadd_rn(__fmul_rn(uv, 0.003f), __fdiv_rn(__fmul_rn(__fsub_rn(1.f, uv), 0.1f), 3.0f));
  float acc = lb;
  for (int h = 0; h < H; ++h) {
    const float ph = L == 1 ? P[h] : __fadd_rn(__fmul_rn(P[ilo * H + h], wl), __fmul_rn(P[ihi * H + h], wh));
    float v = __fmul_rn(__fmul_rn(sinf(ph), 0.1f), uv);
    if (noise) v = __fadd_rn(v, __fmul_rn(namp, noise[j * H + h]));
    acc = fmaf(lw[h], v, acc);
  }
  src[j] = tanhf(acc);
}

// cos / sin of 2 pi k / 20 and hanning(21)[0..<20] = 0.5 - 0.5 cos(2 pi n / 20)   (MLXSTFT.swift:12-20)
__constant__ float c_cos20[20] = {1.f, 0.95105651629515357f, 0.80901699437494742f, 0.58778525229247313f, 0.30901699437494742f, 0.f,
                                  -0.30901699437494742f, -0.58778525229247313f, -0.80901699437494742f, -0.95105651629515357f, -1.f,
                                  -0.95105651629515357f, -0.80901699437494742f, -0.58778525229247313f, -0.30901699437494742f, 0.f,
                                  0.30901699437494742f, 0.58778525229247313f, 0.80901699437494742f, 0.95105651629515357f};
__constant__ float c_sin20[20] = {0.f, 0.30901699437494742f, 0.58778525229247313f, 0.80901699437494742f, 0.95105651629515357f, 1.f,
                                  0.95105651629515357f, 0.80901699437494742f, 0.58778525229247313f, 0.30901699437494742f, 0.f,
                                  -0.30901699437494742f, -0.58778525229247313f, -0.80901699437494742f, -0.95105651629515357f, -1.f,
                                  -0.95105651629515357f, -0.80901699437494742f, -0.58778525229247313f, -0.30901699437494742f};
__device__ __forceinline__ float hann20(int n) { return 0.5f - 0.5f * c_cos20[n]; }

// one thread per (frame, bin).  Bins 0 and 10 of a real transform have no imaginary part: it is set to +0, so their phase is 0 or +pi.
// The same holds for every bin of frame 0: centred on sample 0 of the reflect-padded signal, under a window symmetric about that point,
// the frame is even about its centre and its transform is real (and one of its bins always has a negative real part: DESIGN.md).
__global__ __launch_bounds__(256) void kokoro_stft(const float* __restrict__ s, float* __restrict__ out, int64_t n, int64_t F) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= F * 16) return;
  const int64_t f = i >> 4; const int k = (int)(i & 15);
  float* o = out + f * 32;
  if (k >= KOKORO_BINS) { o[11 + k] = 0.f; o[16 + k] = 0.f; return; }      // k = 11..15: the padding columns 22..26 and 27..31
  float re = 0.f, im = 0.f;
#pragma unroll
  for (int m = 0; m < KOKORO_NFFT; ++m) {
    int64_t q = KOKORO_HOP * f + m - KOKORO_NFFT / 2;
    q = q < 0 ? -q : (q >= n ? 2 * (n - 1) - q : q);
    const float v = s[q] * hann20(m);
    const int tw = (k * m) % KOKORO_NFFT;
    re = fmaf(v, c_cos20[tw], re);
    im = fmaf(v, -c_sin20[tw], im);
  }
  if (k == 0 || k == KOKORO_BINS - 1 || f == 0) im = 0.f;
  o[k] = sqrtf(re * re + im * im);
  o[KOKORO_BINS + k] = atan2f(im, re);
}

// spec = exp(.) (no clamp), phase = sin(.); the unwrap of the reference is the identity on phases in [-1, 1]; inverse real transform
// (the imaginary parts of bins 0 and 10 do not enter), 1 / 20, x window   (Generator.swift:182-188, MLXSTFT.swift:115-143)
__global__ __launch_bounds__(256) void kokoro_istft_frames(const float* __restrict__ hp, int64_t ld, float* __restrict__ fr, int64_t F) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= F * KOKORO_NFFT) return;
  const int64_t f = i / KOKORO_NFFT; const int m = (int)(i - f * KOKORO_NFFT);
  const float* h = hp + f * ld;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < KOKORO_BINS; ++k) {
    const float mag = expf(h[k]), ph = sinf(h[KOKORO_BINS + k]);
    const float re = mag * cosf(ph), im = mag * sinf(ph);
    const int tw = (k * m) % KOKORO_NFFT;
    if (k == 0 || k == KOKORO_BINS - 1) acc += re * c_cos20[tw];
    else acc += 2.0f * (re * c_cos20[tw] - im * c_sin20[tw]);
  }
  fr[i] = acc * 0.05f * hann20(m);
}

// gather overlap-add, divided by the window SUM where it is not zero, trimmed by 10 at both ends   (MLXSTFT.swift:145-160)
__global__ __launch_bounds__(256) void kokoro_overlap_add(const float* __restrict__ fr, float* __restrict__ pcm, int64_t F, int64_t n) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int64_t j = t + KOKORO_NFFT / 2;
  const int64_t f_hi = min(j / KOKORO_HOP, F - 1);
  const int64_t f_lo = j >= KOKORO_NFFT - 1 ? (j - (KOKORO_NFFT - 1) + KOKORO_HOP - 1) / KOKORO_HOP : 0;
  float acc = 0.f, ws = 0.f;
  for (int64_t f = f_lo; f <= f_hi; ++f) {
    const int m = (int)(j - KOKORO_HOP * f);
    acc += fr[f * KOKORO_NFFT + m];
    ws += hann20(m);
  }
  pcm[t] = ws != 0.f ? acc / ws : acc;
}

unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }
int launched() { return hipGetLastError() == hipSuccess ? 0 : 1; }

// rows per slice: enough slices to put about 2048 workgroups on the 256 CUs whatever the shape (4800 x 128: 2 channel groups x 1024
// slices of 5 rows; 40 x 1090: 18 groups x 10 slices), never fewer than 4 rows (one per row lane)
int inorm_rows(int64_t T, int C) {
  const int64_t groups = (C + INORM_CH - 1) / INORM_CH;
  const int64_t want = std::max<int64_t>(1, 2048 / groups);
  return (int)std::max<int64_t>(INORM_LANES, (T + want - 1) / want);
}
int64_t inorm_slices(int64_t T, int C) { const int r = inorm_rows(T, C); return (T + r - 1) / r; }

}  // namespace

int kokoro_style_launch(const float* W, const float* b, const float* s, float* out, int rows, int sd, hipStream_t st) {
  hipLaunchKernelGGL(kokoro_style_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, W, b, s, out, rows, sd);
  return launched();
}

size_t kokoro_inorm_scratch(int64_t T, int C) { return (size_t)(3 * inorm_slices(T, C) * C); }

int kokoro_inorm_launch(const float* x, int64_t ld, int64_t T, int C, float* part, const float* gamma, const float* beta, int C_style,
                        float* out0, float* out1, float* out2, hipStream_t st) {
  const int rows = inorm_rows(T, C);
  const int64_t S = inorm_slices(T, C);
  if (S > 65535) return 1;
  hipLaunchKernelGGL(kokoro_inorm_partial, dim3((unsigned)((C + INORM_CH - 1) / INORM_CH), (unsigned)S), dim3(256), 0, st, x, ld, T, C, rows, part);
  hipLaunchKernelGGL(kokoro_inorm_final, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, x, part, (int)S, C, (float)T, gamma, beta, C_style, out0, out1, out2);
  return launched();
}

int kokoro_adain_act_launch(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t T, int C, const float* mean, const float* a,
                            const float* beta, const float* alpha, const float* ralpha, float slope, hipStream_t st) {
  if (C % 4 || ldx % 4 || ldy % 4) return 1;
  const int C4 = C / 4;
  const float4 *m4 = (const float4*)mean, *a4 = (const float4*)a, *b4 = (const float4*)beta;
  if (alpha) hipLaunchKernelGGL(kokoro_adain_act<true>, dim3(blocks(T * C4)), dim3(256), 0, st, x, ldx, y, ldy, T, C4, m4, a4, b4, (const float4*)alpha, (const float4*)ralpha, slope);
  else hipLaunchKernelGGL(kokoro_adain_act<false>, dim3(blocks(T * C4)), dim3(256), 0, st, x, ldx, y, ldy, T, C4, m4, a4, b4, (const float4*)nullptr, (const float4*)nullptr, slope);
  return launched();
}

int kokoro_pool_launch(const float* x, float* y, const float* w, const float* bias, int64_t T, int C, hipStream_t st) {
  hipLaunchKernelGGL(kokoro_pool, dim3(blocks(2 * T * C)), dim3(256), 0, st, x, y, w, bias, T, C);
  return launched();
}

int kokoro_pack_launch(const float* in, float* out, int64_t ld, int col0, int C, int64_t T, hipStream_t st) {
  hipLaunchKernelGGL(kokoro_pack, dim3((unsigned)((T + 31) / 32), (unsigned)((C + 31) / 32)), dim3(256), 0, st, in, out, ld, col0, C, T);
  return launched();
}

int kokoro_curve_cols_launch(const float* f0, const float* n, const float* wf, const float* wn, float* o1, int64_t ld1, int col1, float* o2,
                             int64_t ld2, int col2, int64_t T, hipStream_t st) {
  hipLaunchKernelGGL(kokoro_curve_cols, dim3(blocks(T)), dim3(256), 0, st, f0, n, wf, wn, o1, ld1, col1, o2, ld2, col2, T);
  return launched();
}

int kokoro_source_launch(const float* f0, float* P, const float* noise, const float* lw, float lb, float* src, int64_t L, int up, int H,
                         float sr, float thr, hipStream_t st) {
  hipLaunchKernelGGL(kokoro_phase_scan, dim3(1), dim3(256), 0, st, f0, P, L, H, sr, (float)up);
  const float scale = (float)L / (float)(L * up);
  hipLaunchKernelGGL(kokoro_source, dim3(blocks(L * up)), dim3(256), 0, st, f0, P, noise, lw, lb, src, L, up, H, scale, thr);
  return launched();
}

int kokoro_stft_launch(const float* src, float* har, int64_t n, hipStream_t st) {
  const int64_t F = n / KOKORO_HOP + 1;
  hipLaunchKernelGGL(kokoro_stft, dim3(blocks(F * 16)), dim3(256), 0, st, src, har, n, F);
  return launched();
}

int kokoro_istft_launch(const float* post, int64_t ld, float* fr, float* pcm, int64_t F, hipStream_t st) {
  hipLaunchKernelGGL(kokoro_istft_frames, dim3(blocks(F * KOKORO_NFFT)), dim3(256), 0, st, post, ld, fr, F);
  const int64_t n = KOKORO_HOP * (F - 1);
  hipLaunchKernelGGL(kokoro_overlap_add, dim3(blocks(n)), dim3(256), 0, st, fr, pcm, F, n);
  return launched();
}
