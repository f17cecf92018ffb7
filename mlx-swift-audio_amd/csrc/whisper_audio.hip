// whisper_audio.hip -- the device-resident log-mel of WhisperSTT.transcribe's seek loop on gfx950.
// Replaces, for a batch of clips, `let mel = whisperLogMelSpectrogram(audio:nMels:padding: nSamples)` (STT/Whisper/WhisperSTT.swift:140-145)
// and the per-window `padOrTrimMel(mel[seek ..< seek + segmentSize], nFrames).asType(.float16)` + model.encode (:171-182): the mel of every
// whole clip is computed once (one batched log-mel launch) and stays in HBM as fp32; each encode of the loop then names its windows by
// (clip, seek, n_valid) and ONE gather kernel slices, zero-pads, rounds and lays them out for conv1 -- no host copy of the mel, no numpy
// rounding, no per-window upload, no pad_mel_kernel.
//
// mel_gather_kernel is a pure stream: 4 B read + 2 B written per element (2.3 MB per 30 s window at 128 mels).  Because a window is a run
// of whole rows, source and destination of window b are both CONTIGUOUS (n_valid * n_mels floats -> 2T * n_mels 16-bit values behind the
// leading zero row), so the kernel walks 8-element chunks of a flat range: two 16-byte loads and one 16-byte store per lane, every address
// 16-byte aligned when n_mels % 8 == 0 (320 / 512 B source rows, 160 / 256 B destination rows, one-row destination offset).  Chunks past
// n_valid rows store zeros without loading: the buffer is reused by calls with other n_valid.
#include <algorithm>

#include "whisper.h"

struct mia_whisper_audio {
  mia_ctx* ctx = nullptr;       // the context the mel was computed on (its device holds it)
  int n_mels = 0, n_clips = 0;
  int64_t F = 0;                // frames per clip slot
  float* mel = nullptr;         // fp32 [n_clips][F][n_mels]
};

namespace {

struct MelWindow {   // 16 bytes: one per batch row, read by every workgroup of the row
  int64_t src;       // element offset of the window's first value in the resident mel
  int32_t n_valid;   // rows taken from the mel; the remaining 2T - n_valid rows are zeros
  int32_t pad;
};

template <typename T>
__global__ __launch_bounds__(256) void mel_gather_kernel(const float* __restrict__ mel, const MelWindow* __restrict__ win,
                                                         uint16_t* __restrict__ out, int n_mels, int rows) {
  const int b = blockIdx.y;
  const MelWindow wi = win[b];
  const float* __restrict__ src = mel + wi.src;
  uint16_t* __restrict__ dst = out + ((int64_t)b * (rows + 2) + 1) * n_mels;     // row 0 of every window stays zero (conv1's left pad)
  const int chunks = rows * n_mels / 8, valid = wi.n_valid * n_mels / 8;
  for (int c = blockIdx.x * 256 + threadIdx.x; c < chunks; c += gridDim.x * 256) {
    u32x4 o = {0u, 0u, 0u, 0u};
    if (c < valid) {
      const f32x4 lo = *reinterpret_cast<const f32x4*>(src + (int64_t)c * 8);
      const f32x4 hi = *reinterpret_cast<const f32x4*>(src + (int64_t)c * 8 + 4);
      o = u32x4{pack2<T>(lo[0], lo[1]), pack2<T>(lo[2], lo[3]), pack2<T>(hi[0], hi[1]), pack2<T>(hi[2], hi[3])};
    }
    *reinterpret_cast<u32x4*>(dst + (int64_t)c * 8) = o;
  }
}

// the window table of handle w holds at least B records (device + pinned staging); called outside the encode-stream scope
int reserve_windows(mia_whisper* w, int B) {
  mia_ctx* ctx = w->ctx;
  if (!w->ev_win) MIA_HIP(ctx, hipEventCreateWithFlags(&w->ev_win, hipEventDisableTiming));
  if (B <= w->win_cap) return MIA_OK;
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (w->enc_stream) MIA_HIP(ctx, hipStreamSynchronize(w->enc_stream));
  if (w->win_dev) { (void)hipFree(w->win_dev); w->win_dev = nullptr; }
  if (w->win_host) { (void)hipHostFree(w->win_host); w->win_host = nullptr; }
  w->win_cap = 0;
  const int cap = (int)align_up((size_t)B, 32);
  if (hipMalloc(&w->win_dev, (size_t)cap * sizeof(MelWindow)) != hipSuccess)
    return mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed for the window table (%d rows)", cap);
  if (hipHostMalloc(&w->win_host, (size_t)cap * sizeof(MelWindow)) != hipSuccess)
    return mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "hipHostMalloc failed for the window table (%d rows)", cap);
  w->win_cap = cap;
  return MIA_OK;
}

}  // namespace

extern "C" mia_whisper_audio* mia_whisper_audio_create(mia_whisper* w, const float* pcm, const int64_t* offs, int n_clips,
                                                       int64_t pad_right, int mem) {
  if (!w) return nullptr;
  mia_ctx* ctx = w->ctx;
  auto fail = [&](int code, const char* msg) -> mia_whisper_audio* { mia_fail(ctx, code, "whisper_audio_create: %s", msg); return nullptr; };
  if (!pcm || !offs || n_clips <= 0) return fail(MIA_ERR_INVALID_ARGUMENT, "null input or n_clips <= 0");
  if (pad_right < 0) return fail(MIA_ERR_INVALID_ARGUMENT, "pad_right must be >= 0");
  if (!HostIo::valid(mem)) return fail(MIA_ERR_INVALID_ARGUMENT, "bad mem");
  const int n_mels = w->dims.n_mels;
  if (n_mels % 8 != 0) return fail(MIA_ERR_UNSUPPORTED, "n_mels must be a multiple of 8 (16-byte rows)");
  int64_t F = 0;
  for (int b = 0; b < n_clips; ++b) {
    const int64_t len = offs[b + 1] - offs[b];
    if (len <= 0) return fail(MIA_ERR_INVALID_AUDIO, "empty clip");
    F = std::max<int64_t>(F, (len + pad_right) / 160);
  }
  if (F <= 0) return fail(MIA_ERR_INVALID_AUDIO, "Input is too short for STFT");
  if (hipSetDevice(ctx->device) != hipSuccess) return fail(MIA_ERR_DEVICE, "hipSetDevice failed");
  const size_t sc = mia_logmel_direct_scratch_bytes(n_clips, F);
  const size_t pcm_bytes = (size_t)offs[n_clips] * sizeof(float);
  HostIo io(ctx, mem);
  Carve cv;
  cv.add(sc);
  const size_t o_pcm = cv.add(io.staged(pcm_bytes));
  char* ws = (char*)mia_workspace(ctx, cv.bytes);
  if (!ws) return nullptr;
  mia_whisper_audio* a = new mia_whisper_audio();
  a->ctx = ctx; a->n_mels = n_mels; a->n_clips = n_clips; a->F = F;
  if (hipMalloc((void**)&a->mel, (size_t)n_clips * F * n_mels * sizeof(float)) != hipSuccess) {
    delete a;
    return fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed for the resident mel");
  }
  const float* d_pcm = io.in(pcm, ws + o_pcm, pcm_bytes);
  // fp32, dense time-major: the single-pass form of the front end; it returns with the stream drained, so any stream may read the mel
  int rc = mia_logmel_device(ctx, d_pcm, offs, n_clips, n_mels, 0, pad_right, F, a->mel, MIA_F32, false, F * n_mels, n_mels, 1, 0, ws);
  if (rc == MIA_OK) rc = io.finish();
  if (rc != MIA_OK) { (void)hipFree(a->mel); delete a; return nullptr; }
  return a;
}

extern "C" void mia_whisper_audio_free(mia_whisper_audio* a) {
  if (!a) return;
  (void)hipSetDevice(a->ctx->device);
  (void)hipDeviceSynchronize();     // an encode on any stream of the device may still read the mel
  (void)hipFree(a->mel);
  delete a;
}

extern "C" int64_t mia_whisper_audio_frames(const mia_whisper_audio* a) { return a ? a->F : 0; }

extern "C" int mia_whisper_audio_read(mia_whisper_audio* a, int clip, int64_t first_frame, int64_t n_frames, float* out) {
  if (!a) return MIA_ERR_INVALID_ARGUMENT;
  mia_ctx* ctx = a->ctx;
  MIA_CHECK_ARG(ctx, out, "whisper_audio_read: null out");
  MIA_CHECK_ARG(ctx, clip >= 0 && clip < a->n_clips, "whisper_audio_read: clip %d outside [0, %d)", clip, a->n_clips);
  MIA_CHECK_ARG(ctx, first_frame >= 0 && n_frames >= 0 && first_frame <= a->F && n_frames <= a->F - first_frame,
                "whisper_audio_read: frames [%lld, +%lld) outside [0, %lld]", (long long)first_frame, (long long)n_frames, (long long)a->F);
  if (n_frames == 0) return MIA_OK;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  MIA_HIP(ctx, hipMemcpyAsync(out, a->mel + ((int64_t)clip * a->F + first_frame) * a->n_mels, (size_t)n_frames * a->n_mels * sizeof(float),
                              hipMemcpyDeviceToHost, ctx->stream));
  MIA_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return MIA_OK;
}

extern "C" int mia_whisper_encode_audio_windows(mia_whisper* w, mia_whisper_audio* a, const int32_t* clip, const int64_t* seek,
                                                const int32_t* n_valid, int B) {
  if (!w) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = w->ctx;
  MIA_CHECK_ARG(ctx, a && clip && seek && n_valid, "encode_audio_windows: null argument");
  MIA_CHECK_ARG(ctx, B > 0, "encode_audio_windows: B must be > 0 (got %d)", B);
  const mia_whisper_dims& d = w->dims;
  const int rows = 2 * d.n_audio_ctx;
  MIA_CHECK_ARG(ctx, a->n_mels == d.n_mels, "encode_audio_windows: the audio holds %d mels, the model takes %d", a->n_mels, d.n_mels);
  MIA_CHECK_ARG(ctx, a->ctx->device == ctx->device, "encode_audio_windows: the audio lives on device %d, the model on %d", a->ctx->device,
                ctx->device);
  for (int b = 0; b < B; ++b) {
    MIA_CHECK_ARG(ctx, clip[b] >= 0 && clip[b] < a->n_clips, "encode_audio_windows: clip[%d] = %d outside [0, %d)", b, clip[b], a->n_clips);
    MIA_CHECK_ARG(ctx, seek[b] >= 0, "encode_audio_windows: seek[%d] = %lld is negative", b, (long long)seek[b]);
    MIA_CHECK_ARG(ctx, n_valid[b] >= 0 && n_valid[b] <= rows, "encode_audio_windows: n_valid[%d] = %d outside [0, %d]", b, n_valid[b], rows);
    MIA_CHECK_ARG(ctx, seek[b] <= a->F - n_valid[b], "encode_audio_windows: window %d = frames [%lld, +%d) ends past the %lld frames held", b,
                  (long long)seek[b], n_valid[b], (long long)a->F);
  }
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  // a larger batch re-allocates the batch buffers / the window table: that synchronises the CONTEXT's stream, so it happens before the scope
  int rc = whisper_reserve(w, B);
  if (rc != MIA_OK) return rc;
  if ((rc = reserve_windows(w, B)) != MIA_OK) return rc;
  EncStreamScope scope(w);
  MIA_HIP(ctx, hipEventSynchronize(w->ev_win));      // the previous call's copy has left the staging (no-op before the first record)
  MelWindow* hw = (MelWindow*)w->win_host;
  for (int b = 0; b < B; ++b) hw[b] = MelWindow{((int64_t)clip[b] * a->F + seek[b]) * a->n_mels, n_valid[b], 0};
  MIA_HIP(ctx, hipMemcpyAsync(w->win_dev, hw, (size_t)B * sizeof(MelWindow), hipMemcpyHostToDevice, ctx->stream));
  MIA_HIP(ctx, hipEventRecord(w->ev_win, ctx->stream));
  const int chunks = rows * d.n_mels / 8;
  // memory-bound: about 2048 workgroups over the whole batch, each lane striding over its row's chunks
  const unsigned gx = (unsigned)std::max(1, std::min((chunks + 255) / 256, std::max(1, 2048 / B)));
  const int rec = mia_prof_begin(ctx, MIA_PROF_MEL_GATHER, (double)B * rows * d.n_mels * 6.0);
  if (w->dtype == MIA_F16)
    hipLaunchKernelGGL(mel_gather_kernel<F16>, dim3(gx, (unsigned)B), dim3(256), 0, ctx->stream, a->mel, (const MelWindow*)w->win_dev,
                       (uint16_t*)w->mel_pad, d.n_mels, rows);
  else
    hipLaunchKernelGGL(mel_gather_kernel<BF16>, dim3(gx, (unsigned)B), dim3(256), 0, ctx->stream, a->mel, (const MelWindow*)w->win_dev,
                       (uint16_t*)w->mel_pad, d.n_mels, rows);
  mia_prof_end(ctx, rec);
  MIA_HIP(ctx, hipGetLastError());
  return whisper_encode_from_padded_mel(w, B);
}
