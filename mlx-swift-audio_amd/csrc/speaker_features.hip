// speaker_features.hip -- the sample arithmetic of OuteTTS speaker-profile creation on gfx950 (TTS/OuteTTS/OuteTTSAudioProcessor.swift):
// preprocessAudioForSpeaker (:289-336), extractAudioFeatures (:191-216), computeSpectralCentroid (:219-277), calculatePitch /
// extractSinglePitchValue (:15-161).  The word / code slicing of createSpeakerFromTranscription (:363-453) is integer arithmetic on the
// host (outetts.py).
//
// FFT.  The spectral centroid needs a real DFT of N = 2^ceil(log2 n) points for a segment of n samples, any N from 2 to 2^24.  The input
// is carried as complex with a zero imaginary part (DESIGN.md section 7 says why not the half-size trick).
//   N <= kFftBlock (2^14): one 1024-thread workgroup per segment, the whole transform in LDS as float2 [N] (128 KB at 2^14, opted in with
//     hipFuncSetAttribute).  Stockham autosort, decimation in frequency: radix-4 passes, one radix-2 pass at the end when log2 N is odd.
//     A pass reads all its operands into registers (at most 4 butterflies = 16 complex values per thread), barrier, writes, barrier: one
//     buffer instead of two, which is what lets 2^14 points fit.  Reads are unit-stride 8-byte accesses (conflict-free); the writes of
//     pass i have stride 4^(i+1) / 4 float2 between a butterfly's outputs, so the first pass writes at an 8-dword lane stride (4-way
//     conflicts on the 32-bank write path) and later passes are conflict-free.  Not tuned further: the transform is a few microseconds.
//   N > kFftBlock: four-step.  N = N1 N2 (N1 = 2^floor(e/2)), n = n1 + N1 n2, k = N2 k1 + k2:
//       X[N2 k1 + k2] = sum_n1 W_N1^(n1 k1) [ W_N^(n1 k2) sum_n2 x[n1 + N1 n2] W_N2^(n2 k2) ]
//     step 1: workgroup n1 transforms its stride-N1 column (length N2), multiplies by W_N^(n1 k2), stores transposed into Z[k2][n1];
//     step 2: workgroup k2 transforms the contiguous row Z[k2][.] (length N1) and runs the epilogue on bins N2 k1 + k2.
//   Twiddles are tables built on the host in double from exact integer arguments: T1[k] = exp(-2 pi i k / 2^14) serves every LDS pass
//   (sub-length m reads T1[p 2^14 / m], no product of twiddles), and the four-step factor W_N^M = exp(-2 pi i M' / 2^24), M' = M 2^(24-e),
//   is T1[M' >> 10] (1 + T2[M' & 1023]) with T2[b] = exp(-2 pi i b / 2^24) - 1 (|T2| < 4e-4, so W + W T2 is within one ulp of W_N^M).
//
// Reductions.  Every sum (sum x^2, sum m, sum f m, the mean over pitch frames) is accumulated in double in a fixed order that depends on
// the segment alone: a thread adds its own elements in index order, a wave reduces by shuffles, the 16 wave sums are added in order, and
// partial results of several workgroups are combined by one wave per segment in index order.  No float atomics.  A segment's result is
// therefore the same bits whatever else is in the call.
//
// Pitch.  The reference zero-pads each windowed 400-sample frame to 800, runs vDSP_fft_zrip forward and then inverse WITHOUT multiplying
// the spectrum by its conjugate, and reads the first 400 entries of the packed real part.  That round trip is the identity times a
// constant, so its "autocorrelation" is autocorr[j] = C (w x)[2j] for j < 200 and 0 for 200 <= j < 400 (tests/test_outetts_speaker_host.py
// proves it against a literal restatement of the packing).  This file computes that closed form: one wave per frame.
#include <algorithm>
#include <cmath>
#include <mutex>

#include "mia_internal.h"

struct mia_speaker_audio {
  mia_ctx* ctx = nullptr;
  int64_t n = 0;
  int sample_rate = 0;
  float* pcm = nullptr;      // the preprocessed clip, fp32 [n]
  int launches = 0;          // kernels launched by the last mia_speaker_audio_features call
};

namespace {

constexpr int kFftBlockLog2 = 14, kFftBlock = 1 << kFftBlockLog2;       // largest single-workgroup transform
constexpr int kFftMaxLog2 = 24;                                         // 2^24 samples = 11.6 min at 24 kHz
constexpr int kLoBits = kFftMaxLog2 - kFftBlockLog2;
constexpr int kThreads = 1024, kBf = kFftBlock / 4 / kThreads;          // radix-4 butterflies per thread at the largest size
constexpr int kStatChunk = 1 << 16;                                     // samples per statistics workgroup
constexpr int kFrame = 400, kHop = 160;                                 // calculatePitch's defaults
constexpr float kMinFreq = 75.0f, kMaxFreq = 600.0f, kVoicing = 0.3f;
// Apple's documented constants, none of them in the reference's tree -- verify on a Mac:
constexpr float kVdspForwardScale = 2.0f;            // vDSP_fft_zrip forward = 2 x the mathematical DFT (matters only against the 1e-10)
constexpr float kVdspRoundTrip = 2.0f * 800.0f;      // forward then inverse zrip of 800 points = 2N x the input (matters only against the 1e-8s)
constexpr double kHannNorm = 0.8165;                 // vDSP_HANN_NORM: w[n] = 0.8165 (1 - cos(2 pi n / N))

struct SegRec {            // one per segment, built on the host
  int64_t start, len;
  int64_t frame0;          // first pitch frame of the segment in the call's frame list
  int32_t n_frames;
  int32_t stat0, n_stat;   // statistics partials [stat0, stat0 + n_stat)
  int32_t part0, n_part;   // centroid partials
  int32_t pad;
};

struct SpeakerTables { float2* t1; float2* t2; float* hann; };

// one rounding less per component than the four-product form (the build has -ffp-contract=off, so the fused form is spelled out)
__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return float2{fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)}; }

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;            // lane 0 holds the sum
}

// ---- statistics: sum x^2 (double), max |x|, non-finite flag; workgroup c of segment s covers samples [c, c + 1) * kStatChunk ----------
__global__ __launch_bounds__(256) void seg_stats_kernel(const float* __restrict__ audio, const SegRec* __restrict__ recs, double* __restrict__ statp) {
  const SegRec r = recs[blockIdx.y];
  if ((int)blockIdx.x >= r.n_stat) return;
  const int64_t lo = (int64_t)blockIdx.x * kStatChunk, hi = r.len < lo + kStatChunk ? r.len : lo + kStatChunk;
  double sq = 0.0;
  float mx = 0.0f;
  int bad = 0;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float v = audio[r.start + i];
    sq += (double)v * (double)v;
    mx = fmaxf(mx, fabsf(v));
    bad |= !(fabsf(v) <= 3.402823466e38f);
  }
  __shared__ double s_sq[4];
  __shared__ float s_mx[4];
  __shared__ int s_bad[4];
  sq = wave_sum(sq);
  for (int off = 32; off > 0; off >>= 1) { mx = fmaxf(mx, __shfl_down(mx, off, 64)); bad |= __shfl_down(bad, off, 64); }
  if ((threadIdx.x & 63) == 0) { s_sq[threadIdx.x >> 6] = sq; s_mx[threadIdx.x >> 6] = mx; s_bad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = statp + (size_t)(r.stat0 + blockIdx.x) * 3;
    o[0] = ((s_sq[0] + s_sq[1]) + s_sq[2]) + s_sq[3];
    o[1] = (double)fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    o[2] = (double)(s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]);
  }
}

// the statistics of one segment from its partials, by one wave, in index order; every lane returns the same values
__device__ void stats_combine(const SegRec& r, const double* __restrict__ statp, double& sq, float& mx, int& bad) {
  const int lane = threadIdx.x & 63;
  double a = 0.0;
  float m = 0.0f;
  int b = 0;
  for (int i = lane; i < r.n_stat; i += 64) {
    const double* p = statp + (size_t)(r.stat0 + i) * 3;
    a += p[0]; m = fmaxf(m, (float)p[1]); b |= (int)p[2];
  }
  a = wave_sum(a);
  for (int off = 32; off > 0; off >>= 1) { m = fmaxf(m, __shfl_down(m, off, 64)); b |= __shfl_down(b, off, 64); }
  sq = __shfl(a, 0, 64); mx = __shfl(m, 0, 64); bad = __shfl(b, 0, 64);
}

// ---- preprocessAudioForSpeaker: gain to the target RMS and the peak limiter folded into ONE factor (the reference multiplies twice in
// fp32: one rounding apart).  n_eff = max(n, 0.4 s): the zero padding adds nothing to the sums, only to the count. ----------------------
__global__ __launch_bounds__(64) void speaker_gain_kernel(const SegRec* __restrict__ recs, const double* __restrict__ statp, int64_t n_eff,
                                                          float target_db, float peak_db, float* __restrict__ factor) {
  double sq; float mx; int bad;
  stats_combine(recs[0], statp, sq, mx, bad);
  if (threadIdx.x != 0) return;
  const double rms_db = 20.0 * log10(sqrt(sq / (double)n_eff) + 1e-10);
  const float gain = (float)pow(10.0, ((double)target_db - rms_db) / 20.0);
  const float thr = (float)pow(10.0, (double)peak_db / 20.0);
  const float peak = mx * gain;                       // max |x gain| = |max x| gain: rounding is monotone
  *factor = peak > thr ? (float)((double)gain * ((double)thr / (double)peak)) : gain;
}

__global__ __launch_bounds__(256) void speaker_scale_kernel(float* __restrict__ x, int64_t n, const float* __restrict__ factor) {
  const float f = *factor;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) x[i] *= f;
}

// ---- pitch: one wave per frame ---------------------------------------------------------------------------------------------------------
struct PitchArgs {
  const float* audio; const SegRec* recs; const float* hann; float* pitch;
  int64_t total_frames; int S, sample_rate, lo, hi;
};

__global__ __launch_bounds__(256) void pitch_frames_kernel(PitchArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= a.total_frames) return;
  int s = 0;                                            // the last segment whose first frame is <= g owns it (empty ones share a frame0)
  for (int lo = 0, hi = a.S - 1; lo <= hi;) {
    const int mid = (lo + hi) >> 1;
    if (a.recs[mid].frame0 <= g) { s = mid; lo = mid + 1; } else hi = mid - 1;
  }
  const SegRec r = a.recs[s];
  const int64_t f0 = (g - r.frame0) * kHop;             // frame offset inside the segment; samples past len are the zero padding
  const float* __restrict__ x = a.audio + r.start;
  auto ac = [&](int j) -> float {                        // autocorr[j] of the reference's round trip (closed form)
    if (j >= kFrame / 2) return 0.0f;
    const int64_t i = f0 + 2 * j;
    const float v = i < r.len ? x[i] : 0.0f;
    return kVdspRoundTrip * (a.hann[2 * j] * v);
  };
  float best = ac(a.lo + lane);
  int bj = a.lo + lane;                                  // lo + 63 < hi is checked on the host
  for (int j = a.lo + lane + 64; j < a.hi; j += 64) {
    const float v = ac(j);
    if (v > best) { best = v; bj = j; }
  }
  for (int off = 32; off > 0; off >>= 1) {               // vDSP_maxvi: the lowest index among equal maxima
    const float v = __shfl_xor(best, off, 64);
    const int j = __shfl_xor(bj, off, 64);
    if (v > best || (v == best && j < bj)) { best = v; bj = j; }
  }
  if (lane != 0) return;
  float pitch = 0.0f;
  const float ac0 = ac(0) + 1e-8f;
  if (best / ac0 > kVoicing && bj > 0) {
    float delta = 0.0f;
    if (bj < kFrame - 1) {
      const float alpha = ac(bj - 1), beta = best, gamma = ac(bj + 1);
      delta = 0.5f * (alpha - gamma) / (alpha - 2.0f * beta + gamma + 1e-8f);
    }
    const float period = ((float)bj + delta) / (float)a.sample_rate;
    const float p = period > 0.0f ? 1.0f / period : 0.0f;
    pitch = fminf(fmaxf(p, kMinFreq), kMaxFreq);
  }
  a.pitch[g] = pitch;
}

// ---- FFT ---------------------------------------------------------------------------------------------------------------------------------
enum { FFT_WHOLE = 0, FFT_STEP1 = 1, FFT_STEP2 = 2 };

struct FftArgs {
  const float* audio; const SegRec* recs; const int32_t* ids;      // workgroup row y handles segment ids[y]
  float2* z;               // four-step intermediate [rows][N]
  double* part;            // centroid partials, 2 doubles each
  float2* spec;            // operator hook: bins 0..N/2 of the one segment
  const float2* t1; const float2* t2;
  float step;              // sample_rate / N
  int log2n;               // length of this workgroup's transform
  int e, l1, l2;           // N = 2^e = N1 N2, N1 = 2^l1, N2 = 2^l2 (four-step)
};

template <int MODE, bool SPEC>
__global__ __launch_bounds__(kThreads) void fft_kernel(FftArgs a) {
  extern __shared__ __align__(16) float2 sh[];
  const int tid = threadIdx.x, y = blockIdx.y;
  const int n = 1 << a.log2n;
  const SegRec r = a.recs[a.ids[y]];
  for (int j = tid; j < n; j += kThreads) {
    float2 v = {0.0f, 0.0f};
    if (MODE == FFT_WHOLE) { if (j < r.len) v.x = a.audio[r.start + j]; }
    else if (MODE == FFT_STEP1) { const int64_t i = (int64_t)blockIdx.x + ((int64_t)j << a.l1); if (i < r.len) v.x = a.audio[r.start + i]; }
    else v = a.z[((int64_t)y << a.e) + ((int64_t)blockIdx.x << a.l1) + j];
    sh[j] = v;
  }
  __syncthreads();
  const int q4 = n >> 2;
  int log2m = a.log2n, log2s = 0;
  for (; log2m >= 2; log2m -= 2, log2s += 2) {
    float2 v[kBf][4];
#pragma unroll
    for (int i = 0; i < kBf; ++i) {
      const int b = tid + i * kThreads;
      if (b < q4) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[i][c] = sh[b + c * q4];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kBf; ++i) {
      const int b = tid + i * kThreads;
      if (b < q4) {
        const int p = b >> log2s, q = b & ((1 << log2s) - 1);
        const int t = p << (kFftBlockLog2 - log2m);
        const float2 A = v[i][0], B = v[i][1], Cc = v[i][2], D = v[i][3];
        const float2 apc = {A.x + Cc.x, A.y + Cc.y}, amc = {A.x - Cc.x, A.y - Cc.y};
        const float2 bpd = {B.x + D.x, B.y + D.y}, bmd = {B.x - D.x, B.y - D.y};
        const float2 jb = {-bmd.y, bmd.x};                                  // i (b - d)
        const int o = q + ((4 * p) << log2s), st = 1 << log2s;
        sh[o] = float2{apc.x + bpd.x, apc.y + bpd.y};
        sh[o + st] = cmul(a.t1[t], float2{amc.x - jb.x, amc.y - jb.y});
        sh[o + 2 * st] = cmul(a.t1[2 * t], float2{apc.x - bpd.x, apc.y - bpd.y});
        sh[o + 3 * st] = cmul(a.t1[3 * t], float2{amc.x + jb.x, amc.y + jb.y});
      }
    }
    __syncthreads();
  }
  if (log2m == 1) {                                      // the last radix-2 pass: twiddle 1, in place
    const int half = n >> 1;
    for (int b = tid; b < half; b += kThreads) {
      const float2 A = sh[b], B = sh[b + half];
      sh[b] = float2{A.x + B.x, A.y + B.y};
      sh[b + half] = float2{A.x - B.x, A.y - B.y};
    }
    __syncthreads();
  }
  if (MODE == FFT_STEP1) {                               // times W_N^(n1 k2), transposed store
    const int n1 = blockIdx.x;
    for (int k2 = tid; k2 < n; k2 += kThreads) {
      const uint32_t M = ((uint32_t)n1 * (uint32_t)k2) << (kFftMaxLog2 - a.e);      // n1 k2 < N <= 2^24
      const float2 w = a.t1[M >> kLoBits], d = a.t2[M & ((1u << kLoBits) - 1)];
      const float2 wd = cmul(w, d);
      a.z[((int64_t)y << a.e) + ((int64_t)k2 << a.l1) + n1] = cmul(sh[k2], float2{w.x + wd.x, w.y + wd.y});
    }
    return;
  }
  // bins of this workgroup: k = j (whole) or N2 j + k2 (step 2), j < n; the packed format keeps bins 0 .. N/2 - 1 and folds Nyquist into bin 0
  const int k2 = MODE == FFT_STEP2 ? (int)blockIdx.x : 0, shift = MODE == FFT_STEP2 ? a.l2 : 0;
  if (SPEC) {
    const int64_t halfN = (int64_t)1 << (a.e - 1);
    for (int j = tid; j < n; j += kThreads) {
      const int64_t k = ((int64_t)j << shift) + k2;
      if (k <= halfN) a.spec[k] = sh[j];
    }
    return;
  }
  double ws = 0.0, ms = 0.0;
  for (int j = tid; j < (n >> 1); j += kThreads) {
    const int64_t k = ((int64_t)j << shift) + k2;
    float re = kVdspForwardScale * sh[j].x, im = kVdspForwardScale * sh[j].y;
    if (k == 0) im = kVdspForwardScale * sh[n >> 1].x;   // realp[0] = DC, imagp[0] = Nyquist
    const float mag = sqrtf(re * re + im * im);
    ws += (double)((float)k * a.step) * (double)mag;
    ms += (double)mag;
  }
  __shared__ double red[2][kThreads / 64];
  ws = wave_sum(ws); ms = wave_sum(ms);
  if ((tid & 63) == 0) { red[0][tid >> 6] = ws; red[1][tid >> 6] = ms; }
  __syncthreads();
  if (tid == 0) {
    double w = 0.0, m = 0.0;
    for (int i = 0; i < kThreads / 64; ++i) { w += red[0][i]; m += red[1][i]; }
    double* o = a.part + (size_t)(r.part0 + (int)blockIdx.x) * 2;
    o[0] = w; o[1] = m;
  }
}

// ---- one wave per segment: combine the partials, apply extractAudioFeatures' normalisation and rounding ----------------------------------
__global__ __launch_bounds__(64) void seg_finish_kernel(const SegRec* __restrict__ recs, const double* __restrict__ statp, const double* __restrict__ part,
                                                        const float* __restrict__ pitch, int sample_rate, int32_t* __restrict__ feat, float* __restrict__ raw) {
  const int s = blockIdx.x, lane = threadIdx.x;
  const SegRec r = recs[s];
  double sq; float mx; int bad;
  stats_combine(r, statp, sq, mx, bad);
  double ws = 0.0, ms = 0.0, ps = 0.0;
  for (int i = lane; i < r.n_part; i += 64) { ws += part[(size_t)(r.part0 + i) * 2]; ms += part[(size_t)(r.part0 + i) * 2 + 1]; }
  for (int i = lane; i < r.n_frames; i += 64) ps += (double)fminf(fmaxf(pitch[r.frame0 + i], kMinFreq), kMaxFreq);   // unvoiced frames (0) become 75
  ws = wave_sum(ws); ms = wave_sum(ms); ps = wave_sum(ps);
  if (lane != 0) return;
  float rms = 0.0f, cen = 0.0f, pn = 0.0f;
  if (r.len > 0 && !bad) {                               // validateAudio: empty or non-finite -> default features
    rms = (float)sqrt(sq / (double)r.len);
    cen = (float)ms > 1e-10f ? (float)(ws / ms) : 0.0f;
    const float avg = r.n_frames > 0 ? (float)(ps / (double)r.n_frames) : 0.0f;
    pn = fminf(fmaxf((avg - kMinFreq) / (kMaxFreq - kMinFreq), 0.0f), 1.0f);
  }
  const float ne = fminf(rms, 1.0f), nc = fminf(cen / (float)(sample_rate / 2), 1.0f);
  feat[s * 3 + 0] = (int32_t)roundf(ne * 100.0f);      // Int(round(v * 100)): half away from zero
  feat[s * 3 + 1] = (int32_t)roundf(nc * 100.0f);
  feat[s * 3 + 2] = (int32_t)roundf(pn * 100.0f);
  if (raw) { raw[s * 3 + 0] = rms; raw[s * 3 + 1] = cen; raw[s * 3 + 2] = pn; }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
int speaker_tables(mia_ctx* ctx, SpeakerTables& out) {
  const mia_table_key key{MIA_TAB_SPEAKER, 0, 0};
  const mia_tables* t = mia_tables_find(ctx, key);
  if (!t) {
    std::vector<float2> t1(kFftBlock), t2((size_t)1 << kLoBits);
    std::vector<float> hann(kFrame);
    for (int k = 0; k < kFftBlock; ++k) {                  // k / 2^14 of a turn: the argument is exact
      const double ang = 2.0 * M_PI * (double)k / (double)kFftBlock;
      t1[k] = float2{(float)cos(ang), (float)-sin(ang)};
    }
    for (int b = 0; b < (1 << kLoBits); ++b) {             // exp(-i t) - 1 = -2 sin^2(t / 2) - i sin t
      const double ang = 2.0 * M_PI * (double)b / (double)(1 << kFftMaxLog2), h = sin(0.5 * ang);
      t2[b] = float2{(float)(-2.0 * h * h), (float)-sin(ang)};
    }
    for (int i = 0; i < kFrame; ++i) hann[i] = (float)(kHannNorm * (1.0 - cos(2.0 * M_PI * (double)i / (double)kFrame)));
    if (int rc = mia_tables_build(ctx, key, {t1, t2, hann}, {}, &t)) return rc;
  }
  out = SpeakerTables{(float2*)t->dev[0], (float2*)t->dev[1], (float*)t->dev[2]};
  return MIA_OK;
}

int ceil_log2(int64_t n) { int e = 0; while (((int64_t)1 << e) < n) ++e; return e; }

size_t fft_lds(int log2n) { return sizeof(float2) << log2n; }

template <int MODE, bool SPEC>
void fft_launch(hipStream_t s, unsigned gx, unsigned gy, const FftArgs& a, int& launches) {
  ++launches;
  static std::once_flag once;
  std::call_once(once, [] { (void)hipFuncSetAttribute((const void*)fft_kernel<MODE, SPEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds(kFftBlockLog2)); });
  hipLaunchKernelGGL((fft_kernel<MODE, SPEC>), dim3(gx, gy), dim3(kThreads), fft_lds(a.log2n), s, a);
}

// the transform of `rows` segments of size class e: one launch up to 2^14, two above
template <bool SPEC>
void fft_class(hipStream_t s, FftArgs a, int e, int rows, int sample_rate, int& launches) {
  a.e = e; a.step = (float)sample_rate / (float)((int64_t)1 << e);
  if (e <= kFftBlockLog2) {
    a.log2n = e; a.l1 = a.l2 = 0;
    fft_launch<FFT_WHOLE, SPEC>(s, 1, (unsigned)rows, a, launches);
    return;
  }
  a.l1 = e / 2; a.l2 = e - a.l1;
  a.log2n = a.l2;
  fft_launch<FFT_STEP1, SPEC>(s, 1u << a.l1, (unsigned)rows, a, launches);
  a.log2n = a.l1;
  fft_launch<FFT_STEP2, SPEC>(s, 1u << a.l2, (unsigned)rows, a, launches);
}

int centroid_parts(int e) { return e < 1 ? 0 : e <= kFftBlockLog2 ? 1 : 1 << (e - e / 2); }

int64_t pitch_frames(int64_t n) {                        // calculatePitch's framing; a segment of n <= 80 samples traps there, 0 frames here
  const int64_t total = n + (kFrame - n % kHop) % kHop;
  return total < kFrame ? 0 : (total - kFrame) / kHop + 1;
}

void launch_stats(hipStream_t s, const float* audio, const SegRec* d_recs, double* d_stat, int max_chunks, int S) {
  hipLaunchKernelGGL(seg_stats_kernel, dim3((unsigned)std::max(max_chunks, 1), (unsigned)S), dim3(256), 0, s, audio, d_recs, d_stat);
}

}  // namespace

extern "C" mia_speaker_audio* mia_speaker_audio_create(mia_ctx* ctx, const float* pcm, int64_t n, int sample_rate, float target_loudness_db,
                                                       float peak_limit_db) {
  if (!ctx) return nullptr;
  auto fail = [&](int code, const char* msg) -> mia_speaker_audio* { mia_fail(ctx, code, "speaker_audio_create: %s", msg); return nullptr; };
  if (!pcm || n <= 0 || sample_rate <= 0) return fail(MIA_ERR_INVALID_ARGUMENT, "null pcm, n <= 0 or sample_rate <= 0");
  if (n > ((int64_t)1 << kFftMaxLog2)) return fail(MIA_ERR_INVALID_ARGUMENT, "more than 2^24 samples");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(MIA_ERR_DEVICE, "hipSetDevice failed");
  hipStream_t s = ctx->stream;
  SegRec rec{};
  rec.len = n; rec.n_stat = (int32_t)((n + kStatChunk - 1) / kStatChunk);
  Carve cv;
  const size_t o_rec = cv.add(sizeof(SegRec)), o_stat = cv.add((size_t)rec.n_stat * 3 * sizeof(double)), o_fac = cv.add(sizeof(float));
  char* ws;
  if (!cv.workspace(ctx, ws)) return nullptr;
  mia_speaker_audio* a = new mia_speaker_audio();
  a->ctx = ctx; a->n = n; a->sample_rate = sample_rate;
  if (hipMalloc((void**)&a->pcm, (size_t)n * sizeof(float)) != hipSuccess) { delete a; return fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed for the clip"); }
  HostIo io = HostIo::device(ctx);
  io.table(pcm, a->pcm, (size_t)n * sizeof(float));
  const SegRec* d_rec = io.table(&rec, ws + o_rec, sizeof(SegRec));
  double* d_stat = (double*)(ws + o_stat);
  float* d_fac = (float*)(ws + o_fac);
  const int64_t n_eff = std::max<int64_t>(n, (int64_t)(0.4f * (float)sample_rate));      // minSamples = Int(0.4 * Float(sampleRate))
  if (!std::isnan(target_loudness_db)) {                 // NaN: the clip is kept as given (extractAudioFeatures of raw samples)
    launch_stats(s, a->pcm, d_rec, d_stat, rec.n_stat, 1);
    hipLaunchKernelGGL(speaker_gain_kernel, dim3(1), dim3(64), 0, s, d_rec, (const double*)d_stat, n_eff, target_loudness_db, peak_limit_db, d_fac);
    hipLaunchKernelGGL(speaker_scale_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, s, a->pcm, n, (const float*)d_fac);
  }
  io.check(hipGetLastError());
  if (io.finish() != MIA_OK) { (void)hipFree(a->pcm); delete a; return nullptr; }
  return a;
}

extern "C" void mia_speaker_audio_free(mia_speaker_audio* a) {
  if (!a) return;
  (void)hipSetDevice(a->ctx->device);
  (void)hipDeviceSynchronize();     // an encode on any stream of the device may still read the clip
  (void)hipFree(a->pcm);
  delete a;
}

extern "C" int64_t mia_speaker_audio_len(const mia_speaker_audio* a) { return a ? a->n : 0; }

extern "C" int mia_speaker_audio_launches(const mia_speaker_audio* a) { return a ? a->launches : 0; }

extern "C" const float* mia_speaker_audio_data(const mia_speaker_audio* a) { return a ? a->pcm : nullptr; }

extern "C" int mia_speaker_audio_read(mia_speaker_audio* a, int64_t first, int64_t n, float* out) {
  if (!a) return MIA_ERR_INVALID_ARGUMENT;
  mia_ctx* ctx = a->ctx;
  MIA_CHECK_ARG(ctx, out, "speaker_audio_read: null out");
  MIA_CHECK_ARG(ctx, first >= 0 && n >= 0 && first <= a->n && n <= a->n - first, "speaker_audio_read: samples [%lld, +%lld) outside [0, %lld]",
                (long long)first, (long long)n, (long long)a->n);
  if (n == 0) return MIA_OK;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io = HostIo::device(ctx);
  io.fetch(out, a->pcm + first, (size_t)n * sizeof(float));
  return io.finish();
}

extern "C" int mia_speaker_audio_features(mia_speaker_audio* a, const int64_t* start, const int64_t* len, int S, int32_t* feat, float* raw) {
  if (!a) return MIA_ERR_INVALID_ARGUMENT;
  mia_ctx* ctx = a->ctx;
  MIA_CHECK_ARG(ctx, start && len && feat, "speaker_audio_features: null argument");
  MIA_CHECK_ARG(ctx, S > 0 && S <= 65535, "speaker_audio_features: S must be in [1, 65535] (got %d)", S);
  for (int s = 0; s < S; ++s)
    MIA_CHECK_ARG(ctx, start[s] >= 0 && len[s] >= 0 && start[s] <= a->n && len[s] <= a->n - start[s],
                  "speaker_audio_features: segment %d = [%lld, +%lld) outside [0, %lld]", s, (long long)start[s], (long long)len[s], (long long)a->n);
  const int sr = a->sample_rate;
  const int lo = std::max(1, (int)((float)sr / kMaxFreq)), hi = std::min(kFrame, (int)((float)sr / kMinFreq));
  MIA_CHECK_ARG(ctx, lo + 64 <= hi, "speaker_audio_features: sample rate %d leaves no pitch search range", sr);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  SpeakerTables tb;
  int rc = speaker_tables(ctx, tb);
  if (rc != MIA_OK) return rc;
  // segment records, and the segments of every FFT size class side by side
  std::vector<SegRec> recs((size_t)S);
  std::vector<int32_t> ids;
  int cls_first[kFftMaxLog2 + 2] = {0}, cls_count[kFftMaxLog2 + 1] = {0};
  int64_t frames = 0, stats = 0, parts = 0;
  size_t z_floats2 = 0;
  int max_chunks = 0;
  std::vector<int> e_of((size_t)S);
  for (int s = 0; s < S; ++s) {
    SegRec& r = recs[s];
    r = SegRec{};
    r.start = start[s]; r.len = len[s];
    r.frame0 = frames; r.n_frames = (int32_t)pitch_frames(len[s]); frames += r.n_frames;
    r.stat0 = (int32_t)stats; r.n_stat = (int32_t)((len[s] + kStatChunk - 1) / kStatChunk); stats += r.n_stat;
    max_chunks = std::max(max_chunks, (int)r.n_stat);
    const int e = len[s] > 0 ? ceil_log2(len[s]) : 0;          // N = 2^ceil(log2 n); N = 1 has no packed bins
    e_of[s] = e;
    r.part0 = (int32_t)parts; r.n_part = centroid_parts(e); parts += r.n_part;
    if (e >= 1) ++cls_count[e];
  }
  for (int e = 1; e <= kFftMaxLog2; ++e) {
    cls_first[e + 1] = cls_first[e] + cls_count[e];
    if (e > kFftBlockLog2) z_floats2 = std::max(z_floats2, (size_t)cls_count[e] << e);
  }
  ids.resize((size_t)std::max(cls_first[kFftMaxLog2 + 1], 1));
  { int fill[kFftMaxLog2 + 1] = {0};
    for (int s = 0; s < S; ++s) if (e_of[s] >= 1) ids[(size_t)cls_first[e_of[s]] + fill[e_of[s]]++] = s; }
  Carve cv;
  const size_t o_rec = cv.add(recs.size() * sizeof(SegRec)), o_ids = cv.add(ids.size() * 4), o_stat = cv.add((size_t)std::max<int64_t>(stats, 1) * 3 * sizeof(double));
  const size_t o_part = cv.add((size_t)std::max<int64_t>(parts, 1) * 2 * sizeof(double)), o_pitch = cv.add((size_t)std::max<int64_t>(frames, 1) * 4);
  const size_t o_z = cv.add(z_floats2 * sizeof(float2)), o_feat = cv.add((size_t)S * 3 * 4), o_raw = cv.add((size_t)S * 3 * 4);
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  hipStream_t st = ctx->stream;
  HostIo io = HostIo::device(ctx);
  const SegRec* d_recs = io.table(recs.data(), ws + o_rec, recs.size() * sizeof(SegRec));
  const int32_t* d_ids = io.table(ids.data(), ws + o_ids, ids.size() * 4);
  double* d_stat = (double*)(ws + o_stat);
  double* d_part = (double*)(ws + o_part);
  float* d_pitch = (float*)(ws + o_pitch);
  int32_t* d_feat = (int32_t*)(ws + o_feat);
  float* d_raw = (float*)(ws + o_raw);
  int launches = 2;                                      // the statistics and the finish kernel
  launch_stats(st, a->pcm, d_recs, d_stat, max_chunks, S);
  if (frames > 0) {
    ++launches;
    PitchArgs p{a->pcm, d_recs, tb.hann, d_pitch, frames, S, sr, lo, hi};
    hipLaunchKernelGGL(pitch_frames_kernel, dim3((unsigned)((frames + 3) / 4)), dim3(256), 0, st, p);
  }
  FftArgs f{};
  f.audio = a->pcm; f.recs = d_recs; f.z = (float2*)(ws + o_z); f.part = d_part; f.t1 = tb.t1; f.t2 = tb.t2;
  for (int e = 1; e <= kFftMaxLog2; ++e) {
    if (!cls_count[e]) continue;
    f.ids = d_ids + cls_first[e];
    fft_class<false>(st, f, e, cls_count[e], sr, launches);
  }
  hipLaunchKernelGGL(seg_finish_kernel, dim3((unsigned)S), dim3(64), 0, st, d_recs, (const double*)d_stat, (const double*)d_part, (const float*)d_pitch, sr,
                     d_feat, d_raw);
  io.check(hipGetLastError());
  a->launches = launches;
  io.fetch(feat, d_feat, (size_t)S * 3 * 4);
  if (raw) io.fetch(raw, d_raw, (size_t)S * 3 * 4);
  return io.finish();
}

extern "C" int64_t mia_op_rfft_block(void) { return kFftBlock; }

extern "C" int mia_op_rfft_pow2(mia_ctx* ctx, const float* x, int64_t n, int64_t N, float* out) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, x && out, "op_rfft_pow2: null pointer");
  MIA_CHECK_ARG(ctx, N >= 2 && N <= ((int64_t)1 << kFftMaxLog2) && (N & (N - 1)) == 0, "op_rfft_pow2: N must be a power of two in [2, 2^24] (got %lld)", (long long)N);
  MIA_CHECK_ARG(ctx, n > 0 && n <= N, "op_rfft_pow2: n must be in [1, N] (got %lld)", (long long)n);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  SpeakerTables tb;
  int rc = speaker_tables(ctx, tb);
  if (rc != MIA_OK) return rc;
  const int e = ceil_log2(N);
  SegRec rec{};
  rec.len = n;
  const int32_t id0 = 0;
  const size_t spec_bytes = (size_t)(N / 2 + 1) * sizeof(float2);
  Carve cv;
  const size_t o_rec = cv.add(sizeof(SegRec)), o_id = cv.add(4), o_x = cv.add((size_t)n * 4), o_z = cv.add(e > kFftBlockLog2 ? (size_t)N * sizeof(float2) : 0);
  const size_t o_spec = cv.add(spec_bytes);
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  HostIo io = HostIo::device(ctx);
  FftArgs f{};
  f.recs = io.table(&rec, ws + o_rec, sizeof(SegRec));
  f.ids = io.table(&id0, ws + o_id, 4);
  f.audio = io.table(x, ws + o_x, (size_t)n * 4);
  f.z = (float2*)(ws + o_z); f.spec = (float2*)(ws + o_spec); f.t1 = tb.t1; f.t2 = tb.t2;
  int launches = 0;
  fft_class<true>(ctx->stream, f, e, 1, 1, launches);
  io.check(hipGetLastError());
  io.fetch(out, ws + o_spec, spec_bytes);
  return io.finish();
}
