// funasr_frontend.hip -- Fun-ASR's front end on gfx950: preprocessAudio (STT/FunASR/FunASRAudio.swift:197-216) =
// funASRLogMelSpectrogram (:57-94) -> applyLFR (:108-154) -> applyCMVN without precomputed statistics (:176-179).
//
// A sibling of logmel.hip rather than a third mode of it: the window (symmetric Hamming), the frame count (1 + L/160, last frame kept),
// the bins (0..199), the filterbank (HTK on the reference's 200-point grid), the log (natural, no clip-maximum clamp) and the output
// (fp32 rows of a ragged stack) all differ, and the two existing modes stay byte for byte what they were.  What is shared is the method:
//   fa_logmel     one workgroup per 32 frames of a clip; the reflect-padded, windowed frames go to LDS, the 400-point real DFT is a
//                 [32 x 400] x [400 x 2*224] contraction on v_mfma_f32_32x32x2_f32 (a k-ordered fp32 fma chain), |X|^2 is formed in-lane,
//                 the sparse filterbank is applied from LDS and ln(max(., 1e-10)) stored as fp32 [frames][80];
//   fa_lfr_stats  per (clip, column) mean and standard deviation of the LFR rows (row i = frames 6i-3 .. 6i+3, clamped at both ends --
//                 3 copies of frame 0 on the left, copies of the last frame on the right), two passes over the rows, four row groups per
//                 column combined in a fixed order;
//   fa_lfr_norm   gathers each LFR row again and writes (x - mean) / (std + 1e-6).
#include "funasr_host.h"
#include "mia_device.h"
#include "mia_internal.h"
#include "sensevoice.h"

#include <algorithm>
#include <mutex>

namespace {

using namespace funasr;
constexpr int NBP = 224;      // bins padded to 7 tiles of 32 (bins 200 .. 223 carry zero twiddles)
constexpr int FB = 32;        // frames per workgroup
constexpr int FSTR = 401;     // LDS row stride of the windowed frame matrix (odd: conflict-free columns)
constexpr int PSTR = 225;     // LDS row stride of the power matrix
constexpr int MAX_NNZ = 1024;
constexpr int FEAT = NMEL * LFR_M;   // 560

struct FaClip {
  int64_t off;        // first sample of the clip in pcm
  int64_t len;        // samples
  int64_t frame0;     // first row of the clip in the mel scratch
  int64_t row0;       // first row of the clip in the LFR output
  int32_t n_frames, t_lfr;
};

__device__ __forceinline__ float fa_sample(const float* __restrict__ x, int64_t L, int64_t v) {   // reflectPad1D (:280-310), L > 200
  if (v < 0) v = -v;
  if (v >= L) v = 2 * (L - 1) - v;
  return x[v];
}

__global__ __launch_bounds__(256) void fa_logmel(const float* __restrict__ pcm, const FaClip* __restrict__ clips, const float* __restrict__ window,
                                                 const float* __restrict__ twiddle, const float* __restrict__ fb_w, const int* __restrict__ fb_meta,
                                                 int fb_nnz, float* __restrict__ mel) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* F = reinterpret_cast<float*>(smem_raw);            // [FB][FSTR]
  float* P = F + FB * FSTR;                                 // [FB][PSTR]
  float* W = P + FB * PSTR;                                 // [MAX_NNZ]
  int* META = reinterpret_cast<int*>(W + MAX_NNZ);          // [NMEL][3]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const FaClip ci = clips[blockIdx.y];
  const int64_t f0 = (int64_t)blockIdx.x * FB;
  if (f0 >= ci.n_frames) return;                            // uniform per workgroup
  const float* x = pcm + ci.off;

  for (int i = tid; i < fb_nnz; i += 256) W[i] = fb_w[i];
  for (int i = tid; i < NMEL * 3; i += 256) META[i] = fb_meta[i];
  for (int idx = tid; idx < FB * NFFT; idx += 256) {
    const int i = idx / NFFT, k = idx - i * NFFT;
    const int64_t f = f0 + i < ci.n_frames ? f0 + i : ci.n_frames - 1;      // rows past the clip's last frame repeat it (never stored)
    F[i * FSTR + k] = fa_sample(x, ci.len, f * HOP + k - NFFT / 2) * window[k];
  }
  __syncthreads();

  // A[i][k] = F[i][k] (lane: i = lane & 31, k = k0 + (lane >> 5)); B[k][j] = twiddle[k][cos | sin][j]
  const int ai = (lane & 31) * FSTR + (lane >> 5);
  for (int t = wave; t < NBP / 32; t += 4) {
    f32x16 accC = {0}, accS = {0};
    const float* twc = twiddle + (size_t)(lane >> 5) * (2 * NBP) + 32 * t + (lane & 31);
#pragma unroll 8
    for (int k0 = 0; k0 < NFFT; k0 += 2) {
      const float a = F[ai + k0];
      const float bc = twc[(size_t)k0 * (2 * NBP)];
      const float bs = twc[(size_t)k0 * (2 * NBP) + NBP];
      accC = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bc, accC, 0, 0, 0);
      accS = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bs, accS, 0, 0, 0);
    }
    const int j = 32 * t + (lane & 31);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      P[i * PSTR + j] = accC[r] * accC[r] + accS[r] * accS[r];
    }
  }
  __syncthreads();

  for (int idx = tid; idx < FB * NMEL; idx += 256) {
    const int i = idx / NMEL, m = idx - i * NMEL;
    const int64_t f = f0 + i;
    if (f >= ci.n_frames) continue;
    const int lo = META[m * 3 + 0], cnt = META[m * 3 + 1], off = META[m * 3 + 2];
    const float* p = P + i * PSTR + lo;
    float acc = 0.0f;
    for (int c = 0; c < cnt; ++c) acc = fmaf(p[c], W[off + c], acc);
    mel[(ci.frame0 + f) * NMEL + m] = logf(fmaxf(acc, 1e-10f));
  }
}

// LFR element (row i, column j): mel frame clamp(6 i - 3 + j / 80, 0, n_frames - 1), channel j % 80
__device__ __forceinline__ float lfr_at(const float* __restrict__ mel, const FaClip& ci, int i, int j) {
  int f = LFR_N * i - (LFR_M - 1) / 2 + j / NMEL;
  f = f < 0 ? 0 : (f >= ci.n_frames ? ci.n_frames - 1 : f);
  return mel[(ci.frame0 + f) * NMEL + j % NMEL];
}

// grid (ceil(560 / 64), B), block 256 = 64 columns x 4 row groups; stats [B][560][2] = (mean, std + 1e-6)
__global__ __launch_bounds__(256) void fa_lfr_stats(const float* __restrict__ mel, const FaClip* __restrict__ clips, float* __restrict__ stats) {
  __shared__ double red[4][64];
  const FaClip ci = clips[blockIdx.y];
  const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + cl;
  const bool live = j < FEAT;
  double s = 0.0;
  if (live) for (int i = rg; i < ci.t_lfr; i += 4) s += (double)lfr_at(mel, ci, i, j);
  red[rg][cl] = s;
  __syncthreads();
  const double mean = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) / (double)ci.t_lfr;
  __syncthreads();
  double q = 0.0;
  if (live) for (int i = rg; i < ci.t_lfr; i += 4) { const double d = (double)lfr_at(mel, ci, i, j) - mean; q += d * d; }
  red[rg][cl] = q;
  __syncthreads();
  if (live && rg == 0) {
    const double var = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) / (double)ci.t_lfr;       // population variance
    stats[((size_t)blockIdx.y * FEAT + j) * 2 + 0] = (float)mean;
    stats[((size_t)blockIdx.y * FEAT + j) * 2 + 1] = (float)(sqrt(var) + 1e-6);
  }
}

__global__ __launch_bounds__(256) void fa_lfr_norm(const float* __restrict__ mel, const FaClip* __restrict__ clips, const float* __restrict__ stats,
                                                   float* __restrict__ out, int64_t stride) {
  const FaClip ci = clips[blockIdx.y];
  const int64_t total = (int64_t)ci.t_lfr * FEAT;
  const float* st = stats + (size_t)blockIdx.y * FEAT * 2;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / FEAT), j = (int)(e - (int64_t)i * FEAT);
    out[(ci.row0 + i) * stride + j] = (lfr_at(mel, ci, i, j) - st[2 * j]) / st[2 * j + 1];
  }
}

struct FaTables { float* window; float* twiddle; float* fb_w; int* fb_meta; int fb_nnz; };

int fa_tables(mia_ctx* ctx, FaTables& out) {
  const mia_table_key key{MIA_TAB_FUNASR, 0, 0};
  const mia_tables* t = mia_tables_find(ctx, key);
  if (!t) {
    std::vector<float> win, tw, dense, w;
    std::vector<int> meta;
    hamming_window(win);
    fe::twiddle_400(NFREQ, NBP, tw);
    mel_filters(dense);
    fe::compact_filters(dense, NMEL, NFREQ, w, meta);
    if ((int)w.size() > MAX_NNZ) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "funasr front end: filterbank has %zu non-zeros (> %d)", w.size(), MAX_NNZ);
    if (int rc = mia_tables_build(ctx, key, {win, tw, w, meta}, {(int)w.size()}, &t)) return rc;
  }
  out = FaTables{(float*)t->dev[0], (float*)t->dev[1], (float*)t->dev[2], (int*)t->dev[3], t->meta[0]};
  return MIA_OK;
}

constexpr size_t LOGMEL_LDS = (size_t)(FB * FSTR + FB * PSTR + MAX_NNZ) * 4 + NMEL * 3 * 4;

}  // namespace

int funasr_plan(mia_ctx* ctx, const int64_t* offs, int B, FunasrPlan& plan) {
  MIA_CHECK_ARG(ctx, offs && B > 0, "sensevoice_features: offs must be non-null and B > 0");
  plan.B = B; plan.frames = 0; plan.rows = 0; plan.max_frames = 0;
  plan.t_lfr.resize(B);
  for (int b = 0; b < B; ++b) {
    const int64_t len = offs[b + 1] - offs[b];
    if (offs[b] < 0 || len <= NFFT / 2)
      return mia_fail(ctx, MIA_ERR_INVALID_AUDIO, "sensevoice_features: clip %d has %lld samples: the reflect padding needs more than %d", b, (long long)len, NFFT / 2);
    if (n_frames(len) > (1ll << 30)) return mia_fail(ctx, MIA_ERR_INVALID_AUDIO, "sensevoice_features: clip %d is too long", b);
    plan.t_lfr[b] = (int32_t)t_lfr(len);
    plan.frames += n_frames(len);
    plan.rows += plan.t_lfr[b];
    if (n_frames(len) > plan.max_frames) plan.max_frames = n_frames(len);
  }
  return MIA_OK;
}

size_t funasr_scratch_bytes(const FunasrPlan& plan) {
  return align_up((size_t)plan.B * sizeof(FaClip), 256) + align_up((size_t)plan.B * FEAT * 2 * 4, 256) + align_up((size_t)plan.frames * NMEL * 4, 256);
}

// pcm_dev: the clips back to back (device); feats_dev fp32 [plan.rows][stride]; scratch: funasr_scratch_bytes(plan) bytes (device)
int funasr_features_device(mia_ctx* ctx, const float* pcm_dev, const int64_t* offs, const FunasrPlan& plan, float* feats_dev, int64_t stride, void* scratch) {
  MIA_CHECK_ARG(ctx, stride >= FEAT, "sensevoice_features: stride must be >= %d", FEAT);
  FaTables tb;
  int rc = fa_tables(ctx, tb);
  if (rc != MIA_OK) return rc;
  const int B = plan.B;
  std::vector<FaClip> clips(B);
  int64_t frame0 = 0, row0 = 0;
  int max_lfr = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t len = offs[b + 1] - offs[b];
    clips[b] = FaClip{offs[b], len, frame0, row0, (int32_t)n_frames(len), plan.t_lfr[b]};
    frame0 += n_frames(len); row0 += plan.t_lfr[b];
    if (plan.t_lfr[b] > max_lfr) max_lfr = plan.t_lfr[b];
  }
  char* s = (char*)scratch;
  FaClip* d_clips = (FaClip*)s; s += align_up((size_t)B * sizeof(FaClip), 256);
  float* d_stats = (float*)s; s += align_up((size_t)B * FEAT * 2 * 4, 256);
  float* d_mel = (float*)s;
  hipStream_t st = ctx->stream;
  HostIo io = HostIo::device(ctx);             // clips[] lives on this call's stack: no return before its upload has been read
  io.table(clips.data(), d_clips, (size_t)B * sizeof(FaClip));
  static std::once_flag lds_once;
  static hipError_t lds_rc = hipSuccess;
  std::call_once(lds_once, [] { lds_rc = hipFuncSetAttribute((const void*)fa_logmel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LOGMEL_LDS); });
  MIA_HIP(ctx, lds_rc);
  double bytes = (double)plan.rows * FEAT * 4.0;
  for (int b = 0; b < B; ++b) bytes += (double)clips[b].len * 4.0;
  const int rec = mia_prof_begin(ctx, MIA_PROF_LOGMEL, bytes);
  hipLaunchKernelGGL(fa_logmel, dim3((unsigned)((plan.max_frames + FB - 1) / FB), (unsigned)B), dim3(256), LOGMEL_LDS, st, pcm_dev, d_clips, tb.window,
                     tb.twiddle, tb.fb_w, tb.fb_meta, tb.fb_nnz, d_mel);
  hipLaunchKernelGGL(fa_lfr_stats, dim3((FEAT + 63) / 64, (unsigned)B), dim3(256), 0, st, d_mel, d_clips, d_stats);
  const unsigned gx = (unsigned)std::min<int64_t>(((int64_t)max_lfr * FEAT + 255) / 256, 1024);
  hipLaunchKernelGGL(fa_lfr_norm, dim3(gx, (unsigned)B), dim3(256), 0, st, d_mel, d_clips, d_stats, feats_dev, stride);
  mia_prof_end(ctx, rec);
  MIA_HIP(ctx, hipGetLastError());
  return io.finish();
}

extern "C" int64_t mia_sensevoice_feature_rows(const int64_t* offs, int B) {
  if (!offs || B <= 0) return -1;
  int64_t rows = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t len = offs[b + 1] - offs[b];
    if (len <= 0) return -1;
    rows += t_lfr(len);
  }
  return rows;
}

extern "C" int mia_sensevoice_features(mia_ctx* ctx, const float* pcm, const int64_t* offs, int B, float* feats_out, int32_t* t_lfr_out, int64_t stride, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, pcm && offs && feats_out && t_lfr_out && B > 0, "sensevoice_features: null pointer or B <= 0");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "sensevoice_features: bad mem");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  FunasrPlan plan;
  int rc = funasr_plan(ctx, offs, B, plan);
  if (rc != MIA_OK) return rc;
  const size_t sc = funasr_scratch_bytes(plan);
  const size_t pcm_bytes = (size_t)offs[B] * 4, out_bytes = (size_t)plan.rows * stride * 4;
  HostIo io(ctx, mem);
  Carve cv;
  cv.add(sc);
  const size_t o_pcm = cv.add(io.staged(pcm_bytes)), o_out = cv.add(io.staged(out_bytes));
  char* ws = (char*)mia_workspace(ctx, cv.bytes);
  if (!ws) return MIA_ERR_OUT_OF_MEMORY;
  const float* d_pcm = io.in(pcm, ws + o_pcm, pcm_bytes);
  float* d_out = io.out(feats_out, ws + o_out, out_bytes);
  if (io.host() && stride > FEAT) MIA_HIP(ctx, hipMemsetAsync(d_out, 0, out_bytes, ctx->stream));
  if ((rc = funasr_features_device(ctx, d_pcm, offs, plan, d_out, stride, ws)) != MIA_OK) return rc;
  if ((rc = io.finish()) != MIA_OK) return rc;
  for (int b = 0; b < B; ++b) t_lfr_out[b] = plan.t_lfr[b];
  return MIA_OK;
}

// The log-mel stage alone (funASRLogMelSpectrogram), the front end's test tap: mel_out float32 [sum (1 + L_b / 160)][80], the clips' frames
// back to back.  It runs the whole front end and hands out the fp32 log-mel the later stages read.
extern "C" int mia_op_funasr_logmel(mia_ctx* ctx, const float* pcm, const int64_t* offs, int B, float* mel_out, int mem) {
  if (!ctx) return MIA_ERR_INVALID_ARGUMENT;
  MIA_CHECK_ARG(ctx, pcm && offs && mel_out && B > 0, "op_funasr_logmel: null pointer or B <= 0");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "op_funasr_logmel: bad mem");
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  FunasrPlan plan;
  int rc = funasr_plan(ctx, offs, B, plan);
  if (rc != MIA_OK) return rc;
  const size_t sc = funasr_scratch_bytes(plan), pcm_bytes = (size_t)offs[B] * 4, feat_bytes = (size_t)plan.rows * FEAT * 4;
  HostIo io(ctx, mem);
  Carve cv;
  cv.add(sc);
  const size_t o_feat = cv.add(feat_bytes), o_pcm = cv.add(io.staged(pcm_bytes));
  char* ws = (char*)mia_workspace(ctx, cv.bytes);
  if (!ws) return MIA_ERR_OUT_OF_MEMORY;
  const float* d_pcm = io.in(pcm, ws + o_pcm, pcm_bytes);
  if ((rc = funasr_features_device(ctx, d_pcm, offs, plan, (float*)(ws + o_feat), FEAT, ws)) != MIA_OK) return rc;
  const char* d_mel = ws + align_up((size_t)B * sizeof(FaClip), 256) + align_up((size_t)B * FEAT * 2 * 4, 256);
  io.check(hipMemcpyAsync(mel_out, d_mel, (size_t)plan.frames * NMEL * 4, io.to_caller(), ctx->stream));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));      // a test tap: it returns with the mel in place in either mode
  return io.finish();
}
