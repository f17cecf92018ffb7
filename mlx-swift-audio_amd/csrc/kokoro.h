// kokoro.h -- launch interface of Kokoro's own kernels (kokoro_kernels.hip; loader, layer programs and C ABI in kokoro.hip).
// Every activation is time-major fp32 [T][ld], ld = the channel count rounded up to 32 with the padding columns held at zero.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int KOKORO_NFFT = 20, KOKORO_HOP = 5, KOKORO_BINS = 11;      // the only STFT the kernels are written for
constexpr int KOKORO_MAX_HARM = 16;

// out[r] = W[r][:] . s + b[r]: every AdaIN's fc of a handle in one launch (W: the concatenated fc weights [rows][sd])
int kokoro_style_launch(const float* W, const float* b, const float* s, float* out, int rows, int sd, hipStream_t st);

// Instance-norm statistics of x [T][ld] over the T rows, per channel c < C: slice partials of sum(x - K) and sum((x - K)^2), K = the
// channel's first row, added in a fixed order (deterministic, no atomics).  part: kokoro_inorm_scratch(T, C) floats.
//   gamma == null: out0[c] = mean, out1[c] = 1 / sqrt(var + eps)                                     (the operator-level hook)
//   gamma != null: out0[c] = mean, out1[c] = (1 + gamma[c]) / sqrt(var + eps), out2[c] = beta[c] for c < C_style, and 0 for
//                  C_style <= c < C (the padding columns of a buffer stay zero through the AdaIN that follows)
size_t kokoro_inorm_scratch(int64_t T, int C);
int kokoro_inorm_launch(const float* x, int64_t ld, int64_t T, int C, float* part, const float* gamma, const float* beta, int C_style,
                        float* out0, float* out1, float* out2, hipStream_t st);

// y[t][c] = act(a[c] (x[t][c] - mean[c]) + beta[c]), c < C (C % 4 == 0); act: alpha == null ? leaky-ReLU(slope) : snake
// v + ralpha sin^2(alpha v)
int kokoro_adain_act_launch(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t T, int C, const float* mean, const float* a,
                            const float* beta, const float* alpha, const float* ralpha, float slope, hipStream_t st);

// depthwise ConvTransposed1d (k 3, stride 2, pad 1) with one zero row in front: x [T][C] -> y [2 T][C]; w [C][3], bias [C]
int kokoro_pool_launch(const float* x, float* y, const float* w, const float* bias, int64_t T, int C, hipStream_t st);

// in [C][T] (channel-major, as the reference holds it) -> out[t * ld + col0 + c]
int kokoro_pack_launch(const float* in, float* out, int64_t ld, int col0, int C, int64_t T, hipStream_t st);

// F0_conv / N_conv (1 -> 1, k 3, stride 2, pad 1) of the two 2 T-sample curves into column col0 (F0) and col0 + 1 (N) of up to two
// buffers.  wf / wn: folded weights [3] followed by the bias [1]
int kokoro_curve_cols_launch(const float* f0, const float* n, const float* wf, const float* wn, float* o1, int64_t ld1, int col1,
                             float* o2, int64_t ld2, int col2, int64_t T, hipStream_t st);

// harmonic source: P [L][H] phase track, then one thread per full-rate sample (up = 300 for the production shape)
int kokoro_source_launch(const float* f0, float* P, const float* noise, const float* lw, float lb, float* src, int64_t L, int up, int H,
                         float sr, float thr, hipStream_t st);
// STFT 20 / 5 with reflect padding: src [n] -> har [F][32], F = n / 5 + 1: 11 magnitudes, 11 phases, 10 zeros
int kokoro_stft_launch(const float* src, float* har, int64_t n, hipStream_t st);
// conv_post rows [F][ld] (11 log-magnitudes, 11 phase arguments) -> frames fr [F][20] -> pcm [5 (F - 1)]
int kokoro_istft_launch(const float* post, int64_t ld, float* fr, float* pcm, int64_t F, hipStream_t st);
