// audio_trim.hip -- the sample arithmetic of Utils/AudioTrimmer.swift on gfx950: findSpeechBounds (:218-274), the frame energies and the
// two threshold scans that trimSilence (:142-207) shares with it.  The word logic of the same file (:285-567) is host integer and float
// code (trim.py).  Call sites: TTS/CosyVoice2/CosyVoice2Engine.swift:420-424, TTS/OuteTTS/OuteTTSEngine.swift:250-254.
//
// Frames.  numFrames = max(1, (n - frame) / hop + 1), the division truncating toward zero; frame i covers [i hop, min(i hop + frame, n)).
// Only the one frame of a clip shorter than `frame` is short, and samples behind the last whole frame are in no frame.
//
// Energies.  One wave per frame.  Element j of a frame goes to lane j % 64 whatever the frame's address, a lane adds its squares in
// index order in double (the square of an fp32 value is exact there), the 64 lane sums are combined by a fixed xor-shuffle tree, and one
// division gives the mean square.  A frame's energy is therefore the same bits wherever the frame sits and whatever else is in the
// clip.  No float atomics.
//
// Threshold.  The reference compares 20 log10(max(rms, 1e-10)) >= max_dB - top_db.  In real arithmetic that is
// max(ms, 1e-20) >= max(ms_max, 1e-20) ratio with ratio = 10^(-top_db / 10), computed once on the host in double: no transcendental on
// the device.  A frame with a non-finite energy fails the call (MIA_ERR_INVALID_AUDIO): the reference's max() over NaN depends on the
// order of its operands and is not worth copying.
//
// Launches.  Two per bounds call, whatever the clip length: the energy pass (a grid of at most kMaxBlocks workgroups striding over the
// frames, each leaving its maximum and its non-finite flag) and one finishing workgroup (maximum of the partials, the two scans, the
// conversion to samples).  Energies and partials live in the ctx workspace; three int64 come back.
#include <algorithm>
#include <cmath>

#include "mia_internal.h"

struct mia_clip {
  mia_ctx* ctx = nullptr;
  int64_t n = 0;
  int sample_rate = 0;
  float* pcm = nullptr;      // the clip as given, fp32 [n]
  int launches = 0;          // kernels launched by the last mia_clip_speech_bounds call
};

namespace {

constexpr int64_t kMaxSamples = (int64_t)1 << 26;       // 46.6 min at 24 kHz
constexpr int64_t kMaxFrame = (int64_t)1 << 20;
constexpr int64_t kMaxFrames = (int64_t)1 << 22;
constexpr int kWaves = 4, kThreads = 64 * kWaves;       // frames per workgroup pass
constexpr int kMaxBlocks = 2048;
constexpr int kFinishThreads = 1024;
constexpr double kFloor = 1e-20;                        // max(rms, 1e-10), squared
constexpr double kDblMax = 1.7976931348623157e308;

int64_t num_frames(int64_t n, int64_t frame, int64_t hop) {
  const int64_t f = (n - frame) / hop + 1;               // C++ truncates toward zero, as Swift does
  return f < 1 ? 1 : f;
}

// ---- energy pass: ms[g] = mean square of frame first + g, g < count; workgroup b also leaves max and non-finite flag of its frames ------
__global__ __launch_bounds__(kThreads) void frame_energy_kernel(const float* __restrict__ pcm, int64_t n, int64_t frame, int64_t hop, int64_t first,
                                                                int64_t count, double* __restrict__ ms, double* __restrict__ pmax, int* __restrict__ pbad) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double mx = 0.0;
  int bad = 0;
  for (int64_t g = (int64_t)blockIdx.x * kWaves + wave; g < count; g += (int64_t)gridDim.x * kWaves) {
    const int64_t lo = (first + g) * hop;                // < n: checked on the host
    const int64_t len = n - lo < frame ? n - lo : frame;
    const float* __restrict__ x = pcm + lo;
    double sq = 0.0;
    for (int64_t j = lane; j < len; j += 64) {
      const double v = (double)x[j];
      sq += v * v;
    }
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off, 64);       // every lane ends with the same bits
    const double m = sq / (double)len;
    if (lane == 0) ms[g] = m;
    bad |= !(m <= kDblMax);
    mx = m > mx ? m : mx;                                // a NaN never enters: the flag carries it
  }
  __shared__ double s_mx[kWaves];
  __shared__ int s_bad[kWaves];
  if (lane == 0) { s_mx[wave] = mx; s_bad[wave] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = s_mx[0];
    int b = s_bad[0];
    for (int w = 1; w < kWaves; ++w) { m = s_mx[w] > m ? s_mx[w] : m; b |= s_bad[w]; }
    pmax[blockIdx.x] = m;
    pbad[blockIdx.x] = b;
  }
}

// ---- finish: one workgroup.  res = {start sample, end sample, status}: status 1 found, 0 not found, -1 a non-finite energy ---------------
__global__ __launch_bounds__(kFinishThreads) void bounds_finish_kernel(const double* __restrict__ ms, int64_t nf, const double* __restrict__ pmax,
                                                                       const int* __restrict__ pbad, int nparts, double ratio, int64_t hop, int64_t n,
                                                                       int64_t* __restrict__ res) {
  __shared__ double s_mx[kFinishThreads / 64];
  __shared__ int s_bad[kFinishThreads / 64];
  __shared__ long long s_lo[kFinishThreads / 64], s_hi[kFinishThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double mx = 0.0;
  int bad = 0;
  for (int i = tid; i < nparts; i += kFinishThreads) { const double p = pmax[i]; mx = p > mx ? p : mx; bad |= pbad[i]; }
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(mx, off, 64);
    mx = o > mx ? o : mx;
    bad |= __shfl_xor(bad, off, 64);
  }
  if (lane == 0) { s_mx[wave] = mx; s_bad[wave] = bad; }
  __syncthreads();
  mx = s_mx[0]; bad = s_bad[0];
  for (int w = 1; w < kFinishThreads / 64; ++w) { mx = s_mx[w] > mx ? s_mx[w] : mx; bad |= s_bad[w]; }
  const double thr = (mx > kFloor ? mx : kFloor) * ratio;
  long long lo = nf, hi = -1;                            // first and last qualifying frame
  for (int64_t i = tid; i < nf; i += kFinishThreads) {
    const double m = ms[i];
    if ((m > kFloor ? m : kFloor) >= thr) { if (i < lo) lo = i; hi = i; }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const long long a = __shfl_xor(lo, off, 64), b = __shfl_xor(hi, off, 64);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  if (lane == 0) { s_lo[wave] = lo; s_hi[wave] = hi; }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < kFinishThreads / 64; ++w) { lo = s_lo[w] < lo ? s_lo[w] : lo; hi = s_hi[w] > hi ? s_hi[w] : hi; }
  int64_t start = 0, end = 0, status = 0;
  if (bad) status = -1;
  else if (hi >= 0) {
    start = lo * hop;                                    // lo < nf: lo hop <= n
    end = hi + 1 > n / hop ? n : (hi + 1) * hop;         // min((hi + 1) hop, n) without the product overflowing
    status = start < end ? 1 : 0;
  }
  res[0] = start; res[1] = end; res[2] = status;
}

int grid_for(int64_t count) { return (int)std::min<int64_t>((count + kWaves - 1) / kWaves, kMaxBlocks); }

}  // namespace

extern "C" int64_t mia_clip_num_frames(int64_t n, int64_t frame, int64_t hop) {
  if (n <= 0 || frame <= 0 || hop <= 0) return 0;
  return num_frames(n, frame, hop);
}

extern "C" mia_clip* mia_clip_create(mia_ctx* ctx, const float* pcm, int64_t n, int sample_rate) {
  if (!ctx) return nullptr;
  auto fail = [&](int code, const char* msg) -> mia_clip* { mia_fail(ctx, code, "clip_create: %s", msg); return nullptr; };
  if (!pcm || n <= 0 || sample_rate <= 0) return fail(MIA_ERR_INVALID_ARGUMENT, "null pcm, n <= 0 or sample_rate <= 0");
  if (n > kMaxSamples) return fail(MIA_ERR_INVALID_ARGUMENT, "more than 2^26 samples");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(MIA_ERR_DEVICE, "hipSetDevice failed");
  mia_clip* c = new mia_clip();
  c->ctx = ctx; c->n = n; c->sample_rate = sample_rate;
  if (hipMalloc((void**)&c->pcm, (size_t)n * sizeof(float)) != hipSuccess) { delete c; return fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed for the clip"); }
  HostIo io = HostIo::device(ctx);
  io.table(pcm, c->pcm, (size_t)n * sizeof(float));
  if (io.finish() != MIA_OK) { (void)hipFree(c->pcm); delete c; return nullptr; }
  return c;
}

extern "C" void mia_clip_free(mia_clip* c) {
  if (!c) return;
  (void)hipSetDevice(c->ctx->device);
  (void)hipDeviceSynchronize();     // a later stage on any stream of the device may still read the clip
  (void)hipFree(c->pcm);
  delete c;
}

extern "C" int64_t mia_clip_len(const mia_clip* c) { return c ? c->n : 0; }

extern "C" const float* mia_clip_data(const mia_clip* c) { return c ? c->pcm : nullptr; }

extern "C" int mia_clip_launches(const mia_clip* c) { return c ? c->launches : 0; }

extern "C" int mia_clip_read(mia_clip* c, int64_t first, int64_t n, float* out) {
  if (!c) return MIA_ERR_INVALID_ARGUMENT;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, out, "clip_read: null out");
  MIA_CHECK_ARG(ctx, first >= 0 && n >= 0 && first <= c->n && n <= c->n - first, "clip_read: samples [%lld, +%lld) outside [0, %lld]",
                (long long)first, (long long)n, (long long)c->n);
  if (n == 0) return MIA_OK;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  HostIo io = HostIo::device(ctx);
  io.fetch(out, c->pcm + first, (size_t)n * sizeof(float));
  return io.finish();
}

extern "C" int mia_clip_speech_bounds(mia_clip* c, int64_t frame, int64_t hop, float top_db, int64_t* start, int64_t* end, int* found) {
  if (!c) return MIA_ERR_INVALID_ARGUMENT;
  mia_ctx* ctx = c->ctx;
  c->launches = 0;
  MIA_CHECK_ARG(ctx, start && end && found, "clip_speech_bounds: null output");
  MIA_CHECK_ARG(ctx, frame > 0 && hop > 0, "clip_speech_bounds: frame and hop must be positive (got %lld, %lld)", (long long)frame, (long long)hop);
  MIA_CHECK_ARG(ctx, frame <= kMaxFrame, "clip_speech_bounds: frame above 2^20 samples (got %lld)", (long long)frame);
  MIA_CHECK_ARG(ctx, std::isfinite(top_db), "clip_speech_bounds: top_db is not finite");
  const int64_t nf = num_frames(c->n, frame, hop);
  if (nf > kMaxFrames) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "clip_speech_bounds: %lld frames, more than 2^22", (long long)nf);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  const int grid = grid_for(nf);
  Carve cv;
  const size_t o_ms = cv.add((size_t)nf * sizeof(double)), o_max = cv.add(kMaxBlocks * sizeof(double)), o_bad = cv.add(kMaxBlocks * sizeof(int));
  const size_t o_res = cv.add(3 * sizeof(int64_t));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  double* d_ms = (double*)(ws + o_ms);
  double* d_max = (double*)(ws + o_max);
  int* d_bad = (int*)(ws + o_bad);
  int64_t* d_res = (int64_t*)(ws + o_res);
  const double ratio = std::pow(10.0, -(double)top_db / 10.0);
  hipStream_t s = ctx->stream;
  HostIo io = HostIo::device(ctx);
  hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, (const float*)c->pcm, c->n, frame, hop, (int64_t)0, nf, d_ms, d_max, d_bad);
  hipLaunchKernelGGL(bounds_finish_kernel, dim3(1), dim3(kFinishThreads), 0, s, (const double*)d_ms, nf, (const double*)d_max, (const int*)d_bad, grid, ratio,
                     hop, c->n, d_res);
  io.check(hipGetLastError());
  c->launches = 2;
  int64_t res[3] = {0, 0, 0};
  io.fetch(res, d_res, sizeof(res));
  const int rc = io.finish();
  if (rc != MIA_OK) return rc;
  if (res[2] < 0) return mia_fail(ctx, MIA_ERR_INVALID_AUDIO, "clip_speech_bounds: a frame has a non-finite energy (NaN or Inf sample)");
  *start = res[0]; *end = res[1]; *found = (int)res[2];
  return MIA_OK;
}

extern "C" int mia_clip_frame_energy(mia_clip* c, int64_t frame, int64_t hop, int64_t first_frame, int64_t n_frames, double* ms_out) {
  if (!c) return MIA_ERR_INVALID_ARGUMENT;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, ms_out, "clip_frame_energy: null output");
  MIA_CHECK_ARG(ctx, frame > 0 && hop > 0, "clip_frame_energy: frame and hop must be positive (got %lld, %lld)", (long long)frame, (long long)hop);
  MIA_CHECK_ARG(ctx, frame <= kMaxFrame, "clip_frame_energy: frame above 2^20 samples (got %lld)", (long long)frame);
  const int64_t nf = num_frames(c->n, frame, hop);
  if (nf > kMaxFrames) return mia_fail(ctx, MIA_ERR_UNSUPPORTED, "clip_frame_energy: %lld frames, more than 2^22", (long long)nf);
  MIA_CHECK_ARG(ctx, first_frame >= 0 && n_frames > 0 && first_frame < nf && n_frames <= nf - first_frame,
                "clip_frame_energy: frames [%lld, +%lld) outside the clip's %lld", (long long)first_frame, (long long)n_frames, (long long)nf);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  Carve cv;
  const size_t o_ms = cv.add((size_t)n_frames * sizeof(double)), o_max = cv.add(kMaxBlocks * sizeof(double)), o_bad = cv.add(kMaxBlocks * sizeof(int));
  char* ws;
  if (!cv.workspace(ctx, ws)) return MIA_ERR_OUT_OF_MEMORY;
  HostIo io = HostIo::device(ctx);
  hipLaunchKernelGGL(frame_energy_kernel, dim3((unsigned)grid_for(n_frames)), dim3(kThreads), 0, ctx->stream, (const float*)c->pcm, c->n, frame, hop, first_frame,
                     n_frames, (double*)(ws + o_ms), (double*)(ws + o_max), (int*)(ws + o_bad));
  io.check(hipGetLastError());
  io.fetch(ms_out, ws + o_ms, (size_t)n_frames * sizeof(double));
  return io.finish();
}
