// mel_s3gen.hip -- 80-bin 24 kHz log-mel of the S3Gen / CosyVoice2 prompt features (SURVEY.md row 16 "mel", K1/K2 variant).
//
// Replaces s3genMelSpectrogram (Codec/S3Gen/Mel/S3GenMel.swift:43-102): reflect pad (n_fft - hop)/2 = 720, frames of 1920 at
// hop 480 (center: false), periodic Hann (hanningWindow(1921)[0..<1920]), |rfft|, slaney mel filterbank 0..8000 Hz
// (S3TokenizerUtils.swift:301-375), log(max(., 1e-5)).  Output [80][frames], channel-major like the reference.
//
// The 1920-point transform is ONE overlapping-window GEMM on the exact-fp32 matrix cores: the padded signal is viewed as rows of 32
// samples, frame f starts at row 15 f (x_row_mul = 15) and spans 60 taps, and the weight matrix is the Hann-windowed DFT basis for
// the bins the filterbank touches (k <= 640: 8 kHz), cosine rows then sine rows.  A small kernel takes magnitudes, applies the
// sparse filterbank rows and the log.  This runs once per prompt (CosyVoice2TTS.swift:370-430), not per utterance.
#include <cmath>
#include <vector>

#include "codec.h"
#include "frontend_tables.h"
#include "mia_device.h"
#include "mia_internal.h"

namespace {

constexpr int NFFT = 1920, HOP = 480, PAD = (NFFT - HOP) / 2, NMEL = 80, SR = 24000;
constexpr int NBIN = NFFT / 2 + 1;

struct S3GenMelTables { float* dft; float* fb_w; int* fb_meta; int nbp; int nnz; };

__global__ __launch_bounds__(256) void mel24_reflect_pad(const float* __restrict__ x, float* __restrict__ xp, int64_t T, int64_t Tp_alloc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= Tp_alloc) return;
  int64_t q = i - PAD;
  const int64_t Tp = T + 2 * PAD;
  float v = 0.f;
  if (i < Tp) {
    q = q < 0 ? -q : (q >= T ? 2 * (T - 1) - q : q);
    v = (q >= 0 && q < T) ? x[q] : 0.f;
  }
  xp[i] = v;
}

// spec [F][2 nbp] (cos part | sin part) -> out[m][f] = log(max(sum_k |X_k| w[m][k], 1e-5))
__global__ __launch_bounds__(256) void mel24_finish(const float* __restrict__ spec, const float* __restrict__ fb_w, const int* __restrict__ fb_meta,
                                                    float* __restrict__ out, int F, int nbp) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)F * NMEL) return;
  const int f = (int)(e / NMEL), m = (int)(e % NMEL);
  const int lo = fb_meta[m * 3], cnt = fb_meta[m * 3 + 1], off = fb_meta[m * 3 + 2];
  const float* re = spec + (int64_t)f * 2 * nbp + lo;
  const float* im = re + nbp;
  float acc = 0.f;
  for (int c = 0; c < cnt; ++c) acc = fmaf(sqrtf(re[c] * re[c] + im[c] * im[c]), fb_w[off + c], acc);
  out[(int64_t)m * F + f] = logf(fmaxf(acc, 1e-5f));
}

int get_tables(mia_ctx* ctx, S3GenMelTables& out) {
  const mia_table_key key{MIA_TAB_S3GEN_MEL, 0, 0};
  const mia_tables* t = mia_tables_find(ctx, key);
  if (!t) {
    std::vector<float> win, dense, w, dft;
    std::vector<int> meta;
    fe::slaney_filters(NMEL, NBIN, (float)SR, NFFT, 8000.0f, dense);      // fMin 0, fMax 8000
    fe::compact_filters(dense, NMEL, NBIN, w, meta);
    const int kmax = fe::last_live_bin(meta), nbp = (kmax + 1 + 31) / 32 * 32;
    fe::hann_periodic(NFFT, win);                                          // hanningWindow(1921)[0..<1920]
    fe::dft_rows(NFFT, kmax + 1, nbp, NFFT, NFFT, win.data(), dft);
    if (int rc = mia_tables_build(ctx, key, {dft, w, meta}, {nbp, (int)w.size()}, &t)) return rc;
  }
  out = S3GenMelTables{(float*)t->dev[0], (float*)t->dev[1], (int*)t->dev[2], t->meta[0], t->meta[1]};
  return MIA_OK;
}

}  // namespace

extern "C" int64_t mia_mel_s3gen_frames(int64_t n_samples) {
  const int64_t Tp = n_samples + 2 * PAD;
  return Tp < NFFT ? 0 : 1 + (Tp - NFFT) / HOP;
}

extern "C" int mia_mel_s3gen(mia_ctx* ctx, const float* pcm, int64_t n_samples, float* mel, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, pcm && mel && HostIo::valid(mem), "mel_s3gen: bad argument");
  MIA_CHECK_ARG(ctx, n_samples > PAD && n_samples <= (int64_t)24000 * 600, "mel_s3gen: n_samples must be in (%d, 10 min]", PAD);
  const int64_t F = mia_mel_s3gen_frames(n_samples);
  MIA_CHECK_ARG(ctx, F > 0, "mel_s3gen: input too short for one frame");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  S3GenMelTables tb;
  if (int rc = get_tables(ctx, tb)) return rc;
  hipStream_t s = ctx->stream;
  const int64_t Tp = n_samples + 2 * PAD;
  const int64_t rows = (Tp + 31) / 32 + 1;
  HostIo io(ctx, mem);
  const size_t n_xp = (size_t)rows * 32, n_spec = (size_t)F * 2 * tb.nbp, n_out = (size_t)F * NMEL;
  Carve cv;
  const size_t o_in = cv.add(io.staged((size_t)n_samples * 4)), o_xp = cv.add(n_xp * 4), o_spec = cv.add(n_spec * 4), o_out = cv.add(io.staged(n_out * 4));
  char* ws = (char*)mia_workspace(ctx, cv.bytes);
  if (!ws) return MIA_ERR_OUT_OF_MEMORY;
  float* xp = (float*)(ws + o_xp); float* spec = (float*)(ws + o_spec);
  const float* x = io.in(pcm, ws + o_in, (size_t)n_samples * 4);
  hipLaunchKernelGGL(mel24_reflect_pad, dim3((unsigned)((n_xp + 255) / 256)), dim3(256), 0, s, x, xp, n_samples, (int64_t)n_xp);
  ConvGemmArgs g;
  g.X = xp; g.ldx = 32; g.T_in = (int)rows; g.W = tb.dft; g.Y = spec; g.ldy = 2 * tb.nbp; g.T_out = (int)F;
  g.M = (int)F; g.N = 2 * tb.nbp; g.Cin = 32; g.taps = NFFT / 32; g.x_row_mul = HOP / 32;
  if (const char* e = codec_conv_gemm_check(g)) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "mel_s3gen: %s", e);
  if (codec_conv_gemm_launch(g, 1, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "mel_s3gen: GEMM launch failed");
  float* dst = io.out(mel, ws + o_out, n_out * 4);
  hipLaunchKernelGGL(mel24_finish, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, spec, tb.fb_w, tb.fb_meta, dst, (int)F, tb.nbp);
  MIA_HIP(ctx, hipGetLastError());
  return io.finish();
}

// ---- linear-interpolation resampler of the CosyVoice2 prompt path ---------------------------------------------------------------------------
// Replaces resampleAudio -> linearInterpolate1d (TTS/CosyVoice2/CosyVoice2TTS.swift:733-744, TTS/CosyVoice2/HiFiGAN/CosyHiFTGenerator.swift:17-60):
// new_T = int(float(T) * scale) (at least 1); src = (i + 0.5) * (float(T) / float(new_T)) - 0.5 clipped to [0, T - 1.001];
// out = x[floor] * (1 - frac) + x[min(floor + 1, T - 1)] * frac -- every operation in float32 and unfused, like the reference.
namespace {
__global__ __launch_bounds__(256) void resample_linear_kernel(const float* __restrict__ x, float* __restrict__ out, int64_t T, int64_t newT, float ratio,
                                                              float clip_hi) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= newT) return;
  float idx = __fsub_rn(__fmul_rn(__fadd_rn((float)i, 0.5f), ratio), 0.5f);
  idx = fminf(fmaxf(idx, 0.f), clip_hi);
  const float lo = floorf(idx);
  const int64_t ilo = (int64_t)lo, ihi = ilo + 1 < T - 1 ? ilo + 1 : T - 1;
  const float wh = __fsub_rn(idx, lo), wl = __fsub_rn(1.0f, wh);
  out[i] = __fadd_rn(__fmul_rn(x[ilo], wl), __fmul_rn(x[ihi], wh));
}
}  // namespace

extern "C" int64_t mia_resample_linear_len(int64_t n_samples, float scale) {
  const int64_t n = (int64_t)((float)n_samples * scale);
  return n == 0 ? 1 : n;
}

extern "C" int mia_resample_linear(mia_ctx* ctx, const float* x, int64_t n_samples, float scale, float* out, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, x && out && n_samples > 0 && n_samples < ((int64_t)1 << 24) && scale > 0.f && HostIo::valid(mem),
                "resample_linear: bad argument (n_samples must stay below 2^24: the reference indexes in float32)");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const int64_t newT = mia_resample_linear_len(n_samples, scale);
  hipStream_t s = ctx->stream;
  HostIo io(ctx, mem);
  Carve cv;
  const size_t o_x = cv.add(io.staged((size_t)n_samples * 4)), o_o = cv.add(io.staged((size_t)newT * 4));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  const float* d_x = io.in(x, ws + o_x, (size_t)n_samples * 4);
  float* d_o = io.out(out, ws + o_o, (size_t)newT * 4);
  hipLaunchKernelGGL(resample_linear_kernel, dim3((unsigned)((newT + 255) / 256)), dim3(256), 0, s, d_x, d_o, n_samples, newT,
                     (float)n_samples / (float)newT, (float)n_samples - 1.001f);
  MIA_HIP(ctx, hipGetLastError());
  return io.finish();
}
