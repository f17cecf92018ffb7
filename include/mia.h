/* mia.h -- C ABI of the MI355X-native speech-inference hot path ("mia" = MI355X audio).
 *
 * This is the drop-in boundary described in SURVEY.md section 8(b).  The reference
 * (smdesai/mlx-swift-audio, 100 % Swift on MLX) has no FFI seam of its own; its model actors call
 * MLXArray ops directly.  Every entry point below replaces one such call site and cites it
 * (paths relative to /root/reference/package).  A Swift binding is shown in INTEGRATION.md.
 *
 * Conventions (mirroring the actor model of the reference, WhisperSTT.swift:11):
 *   - opaque handles; one mia_ctx == one device + one HIP stream; calls on a ctx are serialised by
 *     the caller (like the Swift actor); no globals; no exceptions cross the ABI.
 *   - every function returns mia_status (0 = ok, <0 = error mirroring STTError cases,
 *     Models/STTError.swift:6-46); mia_last_error(ctx) returns a human readable string.
 *   - caller owns all input/output buffers.  `mem` says where they live: MIA_MEM_HOST (plain host
 *     pointers, the library copies) or MIA_MEM_DEVICE (HBM pointers valid on the ctx device; no copy,
 *     no synchronisation -- work is merely enqueued on the ctx stream).  A MIA_MEM_HOST call returns, with
 *     success or with an error, only when no copy that touches the caller's buffers is still pending.
 *   - there is NO CPU fallback: without a gfx950 device every compute entry point fails with
 *     MIA_ERR_DEVICE.
 */
#ifndef MIA_H
#define MIA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mia_ctx mia_ctx;
typedef struct mia_whisper mia_whisper;
typedef struct mia_codec mia_codec;
typedef struct mia_lm mia_lm;
typedef struct mia_s3tok mia_s3tok;

typedef enum {
  MIA_OK = 0,
  MIA_ERR_INVALID_ARGUMENT = -1, /* STTError.invalidArgument */
  MIA_ERR_MODEL_NOT_LOADED = -2, /* STTError.modelNotLoaded */
  MIA_ERR_INVALID_AUDIO = -3,    /* STTError.invalidAudio */
  MIA_ERR_OUT_OF_MEMORY = -4,
  MIA_ERR_DEVICE = -5,           /* no usable gfx950 device / HIP failure */
  MIA_ERR_UNSUPPORTED = -6
} mia_status;

typedef enum { MIA_F32 = 0, MIA_F16 = 1, MIA_BF16 = 2, MIA_U32 = 3 /* packed quantisation codes */ } mia_dtype;
typedef enum { MIA_MEM_HOST = 0, MIA_MEM_DEVICE = 1 } mia_mem;

/* ---- context -------------------------------------------------------------------------------- */
/* Library version string (static storage). */
const char* mia_version(void);
/* Create a context on `device_ordinal` with a private non-blocking HIP stream. NULL on failure. */
mia_ctx* mia_create(int device_ordinal);
/* Same, but enqueue on a caller-provided hipStream_t (e.g. torch's current stream). */
mia_ctx* mia_create_on_stream(int device_ordinal, void* hip_stream);
void mia_destroy(mia_ctx* ctx);
const char* mia_last_error(const mia_ctx* ctx);
/* hipStream_t of the context (for events recorded by the caller). */
void* mia_stream(mia_ctx* ctx);
/* Block until everything enqueued on the ctx stream has finished. */
int mia_synchronize(mia_ctx* ctx);

/* ---- profiling ------------------------------------------------------------------------------ */
/* Optional HIP-event timing of kernel classes on the ctx stream (events bracket each launch of the class).
 * Classes: "logmel" (work = algorithmic bytes), "enc_gemm", "crosskv_gemm", "enc_attention" (work = FLOPs),
 * "enc_norm" (bytes), "decode" (work = decoder steps), "mel_gather" (bytes; mia_whisper_encode_audio_windows), "decode_kept"
 * (the same records as "decode", for the passes whose step kept the decoder layers' weights resident in the Infinity Cache; none when
 * the layer weights exceed the cache budget and are streamed).  Reading synchronises the stream. */
int mia_profile_enable(mia_ctx* ctx, int on);
int mia_profile_reset(mia_ctx* ctx);
int mia_profile_read(mia_ctx* ctx, const char* kernel_class, int64_t* launches, double* total_ms, double* total_work);
/* Algorithmic bytes of the fp32 codec / flow / vocoder launches (tap GEMMs, depthwise convs, embeds, noise blocks) issued by the CALLING
 * HOST THREAD since the last reset: per launch each distinct input row once + each output element once + the weights once + residual
 * inputs once (SURVEY.md 8(d)'s byte model for SNAC / DAC / HiFT).  reset != 0 clears the counter after reading. */
double mia_profile_codec_bytes(int reset);

/* ---- DSP front end -------------------------------------------------------------------------- */
/* Whisper log-mel.  Replaces whisperLogMelSpectrogram(audio:nMels:padding:)
 * (STT/Whisper/WhisperAudio.swift:78-137, called at STT/Whisper/WhisperSTT.swift:140-145) and the
 * shared stft/melFilters it uses (Codec/S3Tokenizer/S3TokenizerUtils.swift:224-375).
 *   pcm      float32 mono 16 kHz, clips concatenated; clip b = pcm[offs[b] .. offs[b+1])
 *   offs     int64[B+1], ALWAYS a host pointer
 *   n_mels   80 or 128
 *   pad_right zero samples appended to every clip before the STFT (reference passes 480000)
 *   n_frames_out frames emitted per clip; frame f >= (len_b+pad_right)/160 is written as 0.0
 *            (padOrTrimMel, WhisperSTT.swift:624-635).  The per-clip global max of the max-8 clamp
 *            always covers the whole padded utterance, as in the reference.
 *   mel      out, [B][n_frames_out][n_mels] time-major, dtype out_dtype
 */
int mia_logmel_whisper(mia_ctx* ctx, const float* pcm, const int64_t* offs, int B, int n_mels,
                       int64_t pad_right, int64_t n_frames_out, void* mel, int out_dtype, int mem);

/* S3Tokenizer log-mel (periodic Hann, channel-major output [B][n_mels][n_frames_out]).  Replaces
 * logMelSpectrogram / logMelSpectrogramChatterbox (Codec/S3Tokenizer/S3TokenizerUtils.swift:102-208,
 * called at TTS/CosyVoice2/CosyVoice2TTS.swift:386). */
int mia_logmel_s3(mia_ctx* ctx, const float* pcm, const int64_t* offs, int B, int n_mels,
                  int64_t pad_right, int64_t n_frames_out, void* mel, int out_dtype, int mem);

/* 80-bin 24 kHz log-mel of the CosyVoice2 / S3Gen prompt features.  Replaces s3genMelSpectrogram
 * (Codec/S3Gen/Mel/S3GenMel.swift:43-102, called from TTS/CosyVoice2/CosyVoice2TTS.swift:370-430): reflect pad 720,
 * n_fft 1920, hop 480, periodic Hann, |rfft|, slaney filterbank 0..8 kHz, natural log clamped at 1e-5.
 *   pcm float32 mono 24 kHz [n_samples]; mel out float32 [80][mia_mel_s3gen_frames(n_samples)] (channel-major). */
int64_t mia_mel_s3gen_frames(int64_t n_samples);
int mia_mel_s3gen(mia_ctx* ctx, const float* pcm, int64_t n_samples, float* mel, int mem);

/* Linear-interpolation resampler of the CosyVoice2 prompt path (resampleAudio -> linearInterpolate1d, TTS/CosyVoice2/CosyVoice2TTS.swift:733-744,
 * TTS/CosyVoice2/HiFiGAN/CosyHiFTGenerator.swift:17-60; align_corners = false index rule, float32 arithmetic as in the reference).
 * scale = to_rate / from_rate as float32; out holds mia_resample_linear_len(n_samples, scale) samples. */
int64_t mia_resample_linear_len(int64_t n_samples, float scale);
int mia_resample_linear(mia_ctx* ctx, const float* x, int64_t n_samples, float scale, float* out, int mem);
/* Anti-aliased sample-rate conversion of input audio (e.g. 44.1 / 48 kHz files -> 16 kHz for Whisper, -> 24 kHz for the codecs).  The
 * reference uses AVAudioConverter here (Audio/AudioResampler.swift:15-88), whose filter is not specified in its sources: this is a
 * documented polyphase windowed-sinc interpolator (Kaiser beta 8.6, 16 zero crossings per side, roll-off 0.945, unit DC gain per
 * phase; definition in csrc/resample.hip) -- a stated substitute, not a parity claim.  n_out = floor(n_samples * to / from)
 * (mia_resample_sinc_len).  mia_resample_sinc_table returns the phase filters (float32 [L][taps], L = to / gcd) for inspection. */
int64_t mia_resample_sinc_len(int64_t n_samples, int from_rate, int to_rate);
int mia_resample_sinc_table(int from_rate, int to_rate, float* table, int capacity, int* L_out, int* taps_out);
int mia_resample_sinc(mia_ctx* ctx, const float* x, int64_t n_samples, int from_rate, int to_rate, float* out, int64_t out_capacity,
                      int64_t* n_out, int mem);

/* ---- data-parallel exchange (SURVEY.md section 8b "multi-GPU", 8e) ------------------------------------------------- */
/* Clips shard across the GPUs of one node (one process and one mia_ctx per GPU, full weight replica per rank); the path's only
 * exchange is ONE all-gather of the int32 token rows per pass, over RCCL / xGMI, enqueued on the context's own stream.  The
 * reference has no multi-device path (one actor, one Metal device: STT/Whisper/WhisperSTT.swift:11); these entry points are what
 * a Swift host driving 8 processes would bind.
 *   shard rule: contiguous shards, the first n_items % world ranks hold one item more (mia_dp_shard_range, host arithmetic);
 *   mia_dp_available: 1 when RCCL can be bound in this process; mia_dp_init is a collective, so ranks vote on this first;
 *   mia_dp_unique_id: rank 0 makes the 128-byte RCCL id and hands it to the other ranks by its own means (pipe, file, env);
 *   mia_dp_init: collective over all ranks (ncclCommInitRank); one communicator per context; mia_dp_shutdown destroys it
 *     (mia_destroy does too);
 *   mia_dp_gather_tokens: DEVICE pointers; local_tokens [b_local][L] + local_counts [b_local] of this rank ->
 *     all_tokens [n_items][L] + all_counts [n_items] in global clip order on EVERY rank; stream-ordered, no host sync in steady state;
 *   mia_dp_unpack_host: the unpadding step of the gather on host buffers (gathered [world][cap][L], cap = mia_dp_shard_cap). */
int mia_dp_shard_range(int n_items, int rank, int world, int* lo, int* hi);
int mia_dp_shard_cap(int n_items, int world);
int mia_dp_unpack_host(const int32_t* gathered, int n_items, int world, int L, int32_t* dense);
int mia_dp_available(void);
int mia_dp_unique_id(mia_ctx* ctx, void* id128);
int mia_dp_init(mia_ctx* ctx, int rank, int world, const void* unique_id);
int mia_dp_shutdown(mia_ctx* ctx);
int mia_dp_gather_tokens(mia_ctx* ctx, const int32_t* local_tokens, const int32_t* local_counts, int b_local, int L, int n_items,
                         int32_t* all_tokens, int32_t* all_counts);

/* ---- operator level -------------------------------------------------------------------------- */
/* y = act(x W^T + b) + r : the dense contraction behind every MLXNN Linear on the path
 * (e.g. STT/Whisper/Layers/MultiHeadAttention.swift:40-58,134; ResidualAttentionBlock.swift:91).
 *   x [M][lda] and w [N][K] in `dtype` (MIA_BF16|MIA_F16), y [M][ldy] in `dtype` or fp32 (out_f32),
 *   bias fp32 [N] or NULL, r fp32 [M][ldr] or NULL, act 0 = none / 1 = exact-erf GELU / act 2 = ReLU (PositionwiseFeedForward,
 *   Codec/S3Gen/Transformer/PositionwiseFeedForward.swift; runs on the 128^2 tiles whatever the variant).  K % 64 == 0.
 *   variant 0 = register-staged tiles, 1 = LDS-DMA staged tiles (default elsewhere).  Buffers live in `mem`. */
int mia_op_linear(mia_ctx* ctx, const void* x, int64_t lda, const void* w, const float* bias, const float* r, int64_t ldr,
                  void* y, int64_t ldy, int M, int N, int K, int act, int dtype, int out_f32, int variant, int mem);

/* Test hook: mia_op_linear (no residual, no activation) with the two special store layouts of the Whisper encoder / decoder GEMMs.  Rows
 * are tokens of stacked clips, m = b*T + t with M = B*T, columns are head channels, n = h*64 + d.
 *   epi 1 (QKV_VT), N == 3*H*64 (q | k | v thirds), T % 4 == 0, Tpad % 4 == 0, Tpad >= T, ldy % 4 == 0, ldy >= 2*H*64:
 *     columns n < 2*H*64 (q | k) go to y[m][n], row stride ldy; the V third goes transposed per head to
 *     vt[((b*H + h)*64 + d)*Tpad + t] (vt [B][H][64][Tpad]).  Columns t >= T of vt and columns >= 2*H*64 of y are never written.
 *   epi 2 (HEADMAJOR), N == H*64: y[((b*H + h)*T + t)*64 + d] (y [B][H][T][64]; ldy and vt are unused).
 * out_f32 != 0 and batch != 1 exist to be refused (the special epilogues store 16 bit and take the flattened M = B*T form).
 * variant as mia_op_linear, plus 2 = 256^2 tiles, 4 = 256^2 8-phase tiles, 3 = auto.  y and vt 8-byte aligned.  Buffers live in `mem`;
 * with host pointers y and vt are uploaded before the launch, so the bytes the GEMM does not write come back as they were.  Anything
 * else is MIA_ERR_INVALID_ARGUMENT and launches nothing. */
int mia_op_linear_epi(mia_ctx* ctx, const void* x, int64_t lda, const void* w, const float* bias, void* y, int64_t ldy, void* vt, int M, int N,
                      int K, int epi, int T, int H, int Tpad, int batch, int dtype, int out_f32, int variant, int mem);

/* Test hook: the Whisper encoder's self-attention (head dim 64, full softmax((q k^T) / 8) v, fp32 softmax; qkvAttention,
 * STT/Whisper/Layers/MultiHeadAttention.swift:85-135) in the layout the fused QKV GEMM (epi 1 above) leaves behind:
 *   qk [B*T][ld_qk] in `dtype` (MIA_BF16 | MIA_F16), q of head h in columns h*64.., k in columns H*64 + h*64..; vt [B][H][64][Tpad], V
 *   transposed per head; out [B*T][ld_out] in `dtype`, columns >= H*64 of a row are left as they are.
 *   vt columns [T, align_up(T, 64)) are read and multiplied by a zero weight, so they must hold finite values (the model zeroes vt once
 *   and the GEMM never writes them); columns at or beyond align_up(T, 64) are never read.
 * Tpad % 64 == 0, Tpad >= T, ld_qk % 8 == 0, ld_qk >= 2*H*64, ld_out % 4 == 0, ld_out >= H*64, B*T < 2^31; qk and vt 16-byte aligned, out
 * 8-byte aligned.  Anything else is MIA_ERR_INVALID_ARGUMENT and launches nothing.  Deterministic.  Buffers live in `mem`; with host
 * pointers every operand is copied on its own and out is uploaded first. */
int mia_op_attention_h64(mia_ctx* ctx, const void* qk, int64_t ld_qk, const void* vt, void* out, int64_t ld_out, int B, int T, int H, int Tpad,
                         int dtype, int mem);
/* The same with the kernel form chosen by the caller (tests, measurements): variant 0 = 128 queries per workgroup, register-staged K / V^T;
 * 1 = 128 queries, LDS-DMA ring; 2 = 256 queries (64 per wave), LDS-DMA ring; -1 = what mia_op_attention_h64 launches at this shape (2 for
 * T >= 1024 when ceil(T / 256) * H * B >= 480, else 1).  Every form runs at every T and computes the same bits. */
int mia_op_attention_h64_variant(mia_ctx* ctx, const void* qk, int64_t ld_qk, const void* vt, void* out, int64_t ld_out, int B, int T, int H,
                                 int Tpad, int dtype, int variant, int mem);

/* fp32 Conv1d / Linear, the contraction behind every MLXNN Conv1d / Linear of the codec, flow and vocoder stages
 * (e.g. Codec/S3Gen/S3GenDecoder.swift:40-48, Codec/S3Gen/Matcha/MatchaTransformer.swift:36-56), time-major, DEVICE pointers:
 *   y[t][n] = act(b[n] + sum_{k,c} x[t*stride + k*dil - pad][c] * w[n][k][c]) (+ r[t][n]);  x [T_in][ldx], w [N][taps][Cin] (Cin % 32 == 0),
 *   act 0 none / 1 exact-erf GELU / 2 ELU / 3 abs / 4 SiLU / 5 leaky-ReLU(0.01) / 6 ReLU.  Rows outside [0, T_in) read as zero.
 *   ldx % 4 == 0, ldx >= Cin, ldy >= N, x and w 16-byte aligned; anything else is MIA_ERR_INVALID_ARGUMENT. */
int mia_op_conv1d_f32(mia_ctx* ctx, const float* x, int64_t ldx, int T_in, const float* w, const float* bias, const float* r, float* y,
                      int64_t ldy, int T_out, int N, int Cin, int taps, int stride, int dil, int pad, int act);

/* MLX affine de-quantisation of a checkpoint tensor at load time (the reference's default checkpoints are 4-bit, group 64:
 * STT/Whisper/WhisperModel.swift:189-196, TTS/Orpheus/TTSEngine/OrpheusWeightLoader.swift:28-60):
 *   out[r][c] = scales[r][c / group] * code[r][c] + biases[r][c / group],  code c of row r = bits [(c % (32/bits)) * bits, ...) of
 *   wq[r][c / (32/bits)] (uint32, little end first); at 6 bits a row is one little-endian bit stream, code c in bits [6 c, 6 c + 6) of
 *   the row's bytes (4 codes in 3 bytes, cols % 64 == 0).  bits 4 | 6 | 8; scales / biases in scale_dtype; out in out_dtype (MIA_F32 | F16 | BF16). */
int mia_dequant_affine(mia_ctx* ctx, const uint32_t* wq, const void* scales, const void* biases, int64_t rows, int64_t cols,
                       int group_size, int bits, int scale_dtype, void* out, int out_dtype, int mem);

/* fp32 scaled-dot-product attention, head dim 64, unmasked, DEVICE pointers (MLXFast.scaledDotProductAttention as called at
 * Codec/S3Gen/Matcha/MatchaTransformer.swift:58-66): q / k / v float32 [B*T][ld*] with head h in columns h*64 .. h*64+63. */
int mia_op_attention_f32(mia_ctx* ctx, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, float* out,
                         int64_t ldo, int B, int T, int H, float scale);

/* Test hook: the tap-structured fp32 GEMM behind mia_op_conv1d_f32 with every argument of its internal launch exposed, so each mode the
 * codec, flow and vocoder programs use (transposed convolutions as output phases, snake / leaky-ReLU prologues, noise and residual
 * epilogues, stacked sequences) can be compared with a reference on its own.  DEVICE pointers, enqueued on the context's stream.
 * For grid phase z in [0, phases) and stacked sequence u in [0, n_seq):
 *   Y[u*y_seq_step + row(m)][n] = epi( sum_{tap,c} pre(X[u*x_seq_step + z*x_phase_step + m*x_row_mul + tap*dil - pad][c])
 *                                                  * W[z*w_phase_stride + n*ldw + tap*Cin + c] + bias[n] ),   m in [0, M), n in [0, N)
 *   row(m) = m*y_row_mul + y_row_off + z*y_phase_step; rows outside [0, T_out) are dropped.  X rows (relative to the sequence / phase
 *   base) outside [0, T_valid) read as zero, T_valid = min(T_in, seq_len[u]) | min(T_in, phase_len[z]) | T_in.
 *   pre: alpha != NULL: snake x + ralpha[c] * sin^2(alpha[c] x), ralpha NULL -> 1 / (alpha[c] + 1e-9); else lrelu_slope > 0: leaky ReLU.
 *   epi(v): v = act(v) (codes of mia_op_conv1d_f32, 6 = ReLU); noise ? v = R + noise[row] * v : v += R; out_scale != 0: v *= out_scale;
 *   v += R2; tanh_out: v = tanh(v).  R / R2 have row stride ldr and Y's row mapping.  With n_seq > 1 and noise, sequence u's noise value
 *   for row r is noise[noise_seq_off[u] + r] and rows at or past seq_len[u] are not written.
 * Cin % 32 == 0, ldx % 4 == 0, ldx >= Cin, ldw == 0 (dense, taps*Cin) or a multiple of 4 >= taps*Cin; X and W 16-byte aligned. */
typedef struct {
  const float* X; int64_t ldx; int32_t T_in;
  const float* W; int64_t ldw; int64_t w_phase_stride;
  const float* bias;
  const float* alpha; const float* ralpha;
  float lrelu_slope;
  float* Y; int64_t ldy; int32_t T_out;
  int32_t y_row_mul, y_row_off, y_phase_step;
  const float* R; const float* R2; int64_t ldr;
  const float* noise;
  float out_scale;
  int32_t M, N, Cin, taps, dil, pad;
  int32_t x_row_mul;
  int32_t act;
  int32_t tanh_out;
  const int32_t* phase_len; int32_t x_phase_step;
  int32_t n_seq; int64_t x_seq_step, y_seq_step;
  const int32_t* seq_len; const int32_t* noise_seq_off;
} mia_conv_gemm_desc;
int mia_op_conv_gemm_f32(mia_ctx* ctx, const mia_conv_gemm_desc* d, int phases);

/* Test hook: mia_op_attention_f32 with the remaining modes of the fp32 attention kernel.  p [T][ldp] (nullable) = positional keys shared
 * by the batch, with bias_u / bias_v [H][64]: score(i, j) = ((q_i + u) . k_j + (q_i + v) . p_j) * scale (RelPositionMultiHeadedAttention,
 * Codec/S3Gen/Transformer/Attention.swift:143-195).  seq_len int32 [B] (nullable): keys at or beyond seq_len[b] are masked, and sequence
 * b's rows below it equal its own B = 1 call bit for bit.  chunk > 0: query i sees keys j < (i / chunk + 1) * chunk.  DEVICE pointers. */
int mia_op_attention_f32_ex(mia_ctx* ctx, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* p,
                            int64_t ldp, const float* bias_u, const float* bias_v, float* out, int64_t ldo, int B, int T, int H, float scale,
                            const int32_t* seq_len, int chunk);

/* 16-bit scaled-dot-product attention, head dim 128, full (non-causal) softmax in fp32 on the matrix cores: Fun-ASR's
 * MultiHeadAttentionSANM and FunASRMultiHeadAttention (STT/FunASR/Layers/MultiHeadAttentionSANM.swift:155-162, :245-251).
 *   q / k / v [B*T][ld*] in `dtype` (MIA_BF16 | MIA_F16) with head h in columns h*128 .. h*128+127, each with its own pointer and row
 *   stride (multiples of 8 elements, 16-byte aligned), so a fused [M][3 D] q|k|v buffer and three separate ones both fit; out [B*T][ldo]
 *   in `dtype`; scale = d_k^-0.5.  Any T >= 1.  seq_len (int32 [B], nullable, in `mem`): keys at or beyond seq_len[b] are masked, rows of
 *   `out` at or beyond it are left as they are, and sequence b's rows equal its own B = 1, T = seq_len[b] call bit for bit.
 *   Deterministic (fixed summation order).  Buffers live in `mem`. */
int mia_op_attention_h128(mia_ctx* ctx, const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, void* out,
                          int64_t ldo, int B, int T, int H, float scale, const int32_t* seq_len, int dtype, int mem);

/* The SANM memory (forwardFSMN, STT/FunASR/Layers/MultiHeadAttentionSANM.swift:90-116) added into an fp32 stream:
 *   x[t][c] += v[t][c] + sum_k w[k][c] * v[t + k - left][c], rows outside the sequence read as zero; left = (K - 1) / 2 + sanm_shift
 *   must lie in [0, K - 1].  x fp32 [B*T][ldx], v [B*T][ldv] in `dtype` (the v third of a q|k|v buffer), w fp32 [K][D], D % 4 == 0,
 *   seq_len int32 [B] or NULL (no tap crosses a sequence's end; rows at or beyond it are untouched).  Buffers live in `mem`. */
int mia_op_fsmn_add(mia_ctx* ctx, float* x, int64_t ldx, const void* v, int64_t ldv, const float* w, int B, int T, int D, int K, int left,
                    const int32_t* seq_len, int dtype, int mem);

/* The log-mel stage of Fun-ASR's front end alone (funASRLogMelSpectrogram, STT/FunASR/FunASRAudio.swift:57-94), the test tap of
 * mia_sensevoice_features: mel_out float32 [sum_b (1 + L_b / 160)][80], natural log, the clips' frames back to back.  offs HOST. */
int mia_op_funasr_logmel(mia_ctx* ctx, const float* pcm, const int64_t* offs, int B, float* mel_out, int mem);

/* The LM's single-token grouped-query attention over a KV cache it fills itself (the kernels behind attentionWithCacheUpdate,
 * TTS/Orpheus/BuildingBlocks/TransformerBlock.swift:91-99), without a model around it.  q [Hq][dh], k / v [Hkv][T][dh] in `dtype`
 * (MIA_BF16 | MIA_F16; rows taken as already rotated), HOST pointers.  The rows go through the prompt pass's cache writer for the given
 * cache mode -- bits 0: the 16-bit cache (KVCacheSimple); bits 4 | 8: QuantizedKVCache(groupSize: 64, bits:) (:182-201), see
 * mia_lm_set_kv_quant -- and that mode's attention kernel runs q at position T - 1 over keys [0, T).  out fp32 [Hq][dh].
 * dh 64 | 128, Hq % Hkv == 0, T <= 8192.  bits outside {0, 4, 8}: MIA_ERR_INVALID_ARGUMENT; another head_dim: MIA_ERR_UNSUPPORTED. */
int mia_op_kvq_attention(mia_ctx* ctx, const void* q, const void* k, const void* v, float* out, int Hq, int Hkv, int T, int dh, int bits,
                         int dtype);

/* The prompt pass's tiled causal grouped-query attention (lm_prefill_attn.hip, see mia_lm_set_prompt_attention) without a model around
 * it.  k / v [Hkv][T][dh] in `dtype` (MIA_BF16 | MIA_F16; rows taken as already rotated) go through the prompt pass's 16-bit cache
 * writer; q [n][Hq][dh] holds the rows at positions T - n .. T - 1, and the row at position p attends to keys [0, p] (n < T: queries
 * that start behind cached keys).  out fp32 [n][Hq][dh]: the kernel's 16-bit output widened.  HOST pointers.  dh 64 | 128,
 * Hq % Hkv == 0, 1 <= n <= T <= 8192; anything else is MIA_ERR_INVALID_ARGUMENT, another head_dim MIA_ERR_UNSUPPORTED. */
int mia_op_lm_prompt_attention(mia_ctx* ctx, const void* q, const void* k, const void* v, float* out, int Hq, int Hkv, int T, int n, int dh,
                               int dtype);

/* Test hook: the LM decode step's skinny GEMMs (csrc/skinny.h: skinny_gemm_launch on 16-bit weights, skinny_gemm_q_launch on packed 4- /
 * 6- / 8-bit weights) with every launch argument exposed, so each kernel form the two launchers choose from the shape can be compared with a
 * reference on its own.  DEVICE pointers, enqueued on the context's stream.  A [M][lda] and the 16-bit outputs are in `dtype`
 * (MIA_BF16 | MIA_F16); acc[m][n] = sum_k A[m][k] W[n][k] in fp32, summed in a fixed order that depends on the shape only.
 *   mode 1 (OUTF32):  out fp32 [M][ldo] = acc (* rstd[m]) + bias[n]
 *   mode 2 (PARTIAL): out fp32 [S][M][N], slice s = the K range [s K/S, (s+1) K/S) of acc (* rstd[m]); no bias
 *   mode 4 (SWIGLU):  W rows interleaved gate / up: out 16-bit [M][ldo], out[m][n/2] = silu(g) * u of v = acc (* rstd) + bias; S = 1
 *   mode 5 (RESID):   xres fp32 [M][N] += acc + bias; out 16-bit [M][ldo] = xres * nw[n]; ss_out[n/16][m] (fp32 [N/16][M]) = the sum of
 *                     xres^2 over the tile's 16 columns; S = 1, N % 16 == 0, ldo % 4 == 0
 *   ss_in != NULL (fp32 [ss_tiles][M], 1 <= ss_tiles <= 512): rstd[m] = rsqrt(sum_t ss_in[t][m] / ss_dim + eps) * rs_scale; else rstd = 1.
 * Weights: wfrag == NULL: W [N][K] row-major in `dtype`, K % (32 S) == 0; w_frag != 0 makes the op repack W into weight fragment order
 *   (dec_launch_repack_wfrag, into the context workspace) and run the fragment-order loads -- results are identical.  wfrag != NULL:
 *   the packed form, wfrag / stfrag as mia_quant_repack builds them for `bits` (4 | 6 | 8) and compute type `dtype`, K % (128 S) == 0.
 * M_cap (0 = M): the rows the caller's buffers are sized for.  The packed launcher picks its kernel form from max(M, M_cap), so that a
 *   row's result does not depend on how many rows the call carries (the LM step passes the handle's batch capacity).
 * lda % 8 == 0, lda >= K, ldo >= N (N / 2 for mode 4); S > 1 only in mode 2; A, W, wfrag, stfrag, out, xres and nw 16-byte aligned, bias
 * too in mode 5 (the other modes read it, like ss_in, one float at a time; ss_out is written so); W and the packed arrays below 4 GiB,
 * A too with 16-bit weights (32-bit byte offsets in the kernels).  Anything else, modes 0 and 3 and non-positive sizes included, is
 * MIA_ERR_INVALID_ARGUMENT and launches nothing. */
typedef struct {
  const void* A; int64_t lda;
  const void* W;
  const uint32_t* wfrag; const float* stfrag; int32_t bits;
  int32_t w_frag;
  const float* bias;
  void* out; int64_t ldo;
  int32_t M, N, K, S, mode, dtype;
  float* xres; const float* nw; float* ss_out;
  const float* ss_in; int32_t ss_tiles, ss_dim; float eps, rs_scale;
  int32_t M_cap;
} mia_skinny_desc;
int mia_op_skinny_gemm(mia_ctx* ctx, const mia_skinny_desc* d);

/* The many-row GEMM on packed weights (csrc/gemm_quant.hip), the kernel behind mia_lm_set_prompt_weights(lm, 1), without a model around
 * it: C fp32 [M][ldc] = A [M][lda] (`dtype`: MIA_BF16 | MIA_F16) . Wq^T (+ R fp32 [M][ldr]; R may be NULL, and may be C itself).  wfrag /
 * stfrag are the arrays mia_quant_repack builds for `bits` (4 | 6 | 8) and compute type `dtype` -- the ones mia_op_skinny_gemm reads.
 * Per 64-input group the result is scale * sum(code * a) + bias * sum(a) with fp32 sums, groups added in ascending order; no weight is
 * formed or rounded, and a row's result does not depend on M.  DEVICE pointers, enqueued on the context's stream.  Any M, N >= 1,
 * K % 128 == 0, lda % 8 == 0, lda >= K, ldc / ldr >= N; A, wfrag and stfrag 16-byte aligned.  Anything else is MIA_ERR_INVALID_ARGUMENT
 * and launches nothing.  The descriptor (include/mia_gemm_quant.h, included by the callers that fill one) follows mia_skinny_desc. */
typedef struct mia_gemm_quant_desc mia_gemm_quant_desc;    /* defined in include/mia_gemm_quant.h */
int mia_op_gemm_quant(mia_ctx* ctx, const mia_gemm_quant_desc* d);

/* ---- Whisper ---------------------------------------------------------------------------------- */
/* Model dimensions == ModelDimensions (STT/Whisper/Config/WhisperConfig.swift:9-86), read by the caller
 * from config.json. */
typedef struct {
  int32_t n_mels, n_audio_ctx, n_audio_state, n_audio_head, n_audio_layer;
  int32_t n_vocab, n_text_ctx, n_text_state, n_text_head, n_text_layer;
} mia_whisper_dims;

/* A named host tensor handed to the loader (safetensors entry, already mapped by the caller).
 * Names follow the reference's Module key schema (@ModuleInfo keys in STT/Whisper/Layers/ *.swift), e.g.
 *   encoder.conv1.weight [Cout,3,Cin]   encoder.blocks.0.attn.query.weight [D,D]
 *   decoder.token_embedding.weight [V,D]  decoder.positional_embedding [n_text_ctx,D]  decoder.ln.weight [D]
 * `encoder.positional_embedding` is optional (sinusoids, AudioEncoder.swift:78-96, are computed when absent). */
typedef struct {
  const char* name;
  int32_t dtype;      /* mia_dtype of `data` */
  int32_t ndim;
  int64_t shape[4];
  const void* data;   /* host pointer, C-contiguous */
} mia_tensor_view;

/* Decoding options == DecodingOptions + the integer tables the reference's tokenizer provides
 * (STT/Whisper/WhisperDecoding.swift:14-51,104-122,190-206; STT/Whisper/WhisperTokenizer.swift:72-96,489-532).
 * The tokenizer itself (a CPU text codec) stays on the caller's side; its outputs arrive as arrays. */
typedef struct {
  const int32_t* initial_tokens; /* [n_initial] shared by all clips, or [B][n_initial] if per_clip_initial:
                                    ([sot_prev]+prompt)? + sotSequence (+ no_timestamps when timestamps off) */
  int32_t n_initial;
  int32_t per_clip_initial;
  int32_t sot_index;             /* index of <|startoftranscript|> inside initial_tokens (no-speech probe) */
  const int32_t* suppress_ids;   /* nonSpeechTokens + {transcribe, translate, sot, sot_prev, sot_lm, no_speech} */
  int32_t n_suppress;
  const int32_t* blank_ids;      /* tokenizer.encode(" "): suppressed together with eot on the first step only */
  int32_t n_blank;
  int32_t eot, no_speech, no_timestamps, timestamp_begin;
  int32_t timestamps;            /* 0 = TimestampGranularity.none, 1 = segment/word rules active */
  int32_t max_tokens;            /* DecodingOptions.maxTokens (448): budget = max_tokens - n_initial */
  int32_t max_initial_timestamp_index; /* 50 (WhisperDecoding.swift:281) */
  int32_t max_new_tokens;        /* extra cap on generated tokens per clip (0 = none); benchmarking aid */
  float temperature;             /* 0 = greedy (argmax).  > 0: inverse-CDF sampling with caller-provided uniforms */
  const float* uniforms;         /* [B][max_tokens] in [0,1) when any temperature > 0 (explicit RNG), else NULL */
  /* optional per-clip overrides (NULL = use the scalar fields): prefixes of different length (prompt conditioning differs per
   * clip: initial_tokens is then [B][n_initial] with n_initial_per_clip[b] valid entries per row), the fallback temperature
   * of each clip (WhisperSTT.swift:195-250) and which clips take part in this call (inactive clips are left untouched). */
  const int32_t* n_initial_per_clip;
  const int32_t* sot_index_per_clip;
  const float* clip_temperature;
  const int32_t* clip_active;
} mia_decode_opts;

/* Replaces WhisperModel.load's tensor upload (STT/Whisper/WhisperModel.swift:184-206).  compute_dtype is MIA_BF16
 * or MIA_F16 (storage type of weights/activations; accumulation and the residual stream are fp32). */
mia_whisper* mia_whisper_load(mia_ctx* ctx, const mia_whisper_dims* dims, const mia_tensor_view* tensors, int n_tensors,
                              int compute_dtype);
void mia_whisper_free(mia_whisper* w);
/* A second handle on the same (read-only) weights with its own activations, KV caches, decode state and step graph, bound to another
 * context (= another HIP stream) of the same device -- for decoding different batches concurrently (the reference has one model per
 * actor; this is the serving-side counterpart).  Free every clone before the handle it was cloned from. */
mia_whisper* mia_whisper_clone(mia_whisper* src, mia_ctx* ctx);
/* MLX-affine quantised decoder weights for the decode step (group 64; 4- or 8-bit codes): the reference's default engine loads Whisper
 * in 4 bit and keeps every quantised module packed (STT/Whisper/WhisperModel.swift:189-196).  mia_whisper_attach_quantized takes the
 * decoder matrices the step reads as stored -- `<p>.weight` (MIA_U32 codes [N][K * bits / 32], little end first), `<p>.scales`,
 * `<p>.biases` ([N][K/64]; f16, bf16 or f32, one type for all) for p = decoder.blocks.L.{attn.{query,key,value,out},
 * cross_attn.{query,out}, mlp1, mlp2} and decoder.token_embedding -- onto a handle loaded from the de-quantised checkpoint; other
 * tensors (the encoder, cross_attn.{key,value}) are ignored and stay on the 16-bit copy.  n_text_state must be a multiple of 128.  One
 * attach per handle, on the handle that owns the weights and before it is cloned.  Errors: MIA_ERR_INVALID_ARGUMENT for anything wrong
 * with the call (a missing or mis-shaped tensor, bits, group size, a clone, a handle with clones, a second attach), MIA_ERR_OUT_OF_MEMORY
 * when the device refuses the buffers, MIA_ERR_DEVICE when an upload fails; after any of them the handle is unchanged.  mia_whisper_use_packed(w, 1) makes the decode step (mia_whisper_decode_greedy, mia_whisper_align,
 * mia_whisper_detect_language) stream the packed codes and multiply them as MLX's kernels do (per group: scale * sum(code * x) + bias *
 * sum(x), fp32 group sums, no weight rounded); 0 (the default) restores the 16-bit step exactly.  A clone inherits the packed weights and
 * the switch of the handle it was cloned from. */
int mia_whisper_attach_quantized(mia_whisper* w, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits);
int mia_whisper_use_packed(mia_whisper* w, int on);
/* Test hook: the host repack of one packed Linear [N][K] (K % 128 == 0) into the fragment-ordered arrays the packed step kernels read:
 * wfrag [ceil(N/16)][K/128][bits/4][64][4] uint32, stfrag [ceil(N/16)][K/128][16][4] float = (scale, bias - MAG * scale) per group, MAG =
 * 1024 (MIA_F16 compute) or 128 (MIA_BF16), x 17 for 6 and 8 bit.  bits 6: wfrag [ceil(N/16)][K/128][384], the low-nibble plane [64][4]
 * followed by the plane of 2-bit high parts [64][2] (csrc/skinny_quant.hip).  bits 4 | 6 | 8.  Host memory in and out; needs no device. */
int mia_quant_repack(const uint32_t* codes, const void* scales, const void* biases, int N, int K, int bits, int scale_dtype,
                     int compute_dtype, uint32_t* wfrag, float* stfrag);
/* Test hook: force the encoder GEMM tile variant (0 / 1: 128^2 register / LDS-DMA staged, 2: 256^2 two-buffer, 3: automatic
 * (default), 4: 256^2 8-phase).  Results are identical up to fp32 summation order; anything else is MIA_ERR_INVALID_ARGUMENT. */
int mia_whisper_set_gemm_variant(mia_whisper* w, int variant);

/* Test hooks of the decode step (never used by the product path).
 *   mia_whisper_set_debug: bit 0 = launch every step's kernels directly instead of replaying the captured hipGraph, bit 1 = the
 *     one-workgroup decode head at temperature 0 too (normally the split argmax head).  Results must not change.  Bit 2 = the step
 *     keeps every LayerNorm in its own reduce + LayerNorm kernel instead of carrying x * gamma across the attention output
 *     projections: the control chain of tests/test_norm_carry_gpu.py (same function, other 16-bit rounding points).  Bit 4 (16) =
 *     the step's cache policies as they were before the layer weights were kept resident: every weight load follows
 *     mia_whisper_set_weight_sharing, self-attention's K/V load with the default policy (the control of
 *     tests/test_decode_cache_policy_gpu.py and of A/B runs; results must not change).  Other bits, bit 3 (8) among them, are
 *     MIA_ERR_INVALID_ARGUMENT.  A changed flag re-captures the step graph at the next decode.
 *   mia_whisper_trace_logits: from now on every decode step ALSO copies the raw fp32 logits (before the logit rules) of the listed
 *     batch rows into a trace [n_clips][n_text_ctx][n_vocab], filed under the position of the token the step consumed -- the copy is a
 *     node of the same captured step graph, so the trace is what the graph computed.  n_clips = 0 switches it off (<= 8 rows).
 *   mia_whisper_read_logit_trace: rows [first_pos, first_pos + n_pos) of trace slot `slot` -> out (host float32 [n_pos][n_vocab]).
 * Used by tests/ to compare the step path's logits with the oracle's teacher-forced logits at every step (TextDecoder.swift:53-96). */
int mia_whisper_set_debug(mia_whisper* w, int flags);
int mia_whisper_trace_logits(mia_whisper* w, const int32_t* clips, int n_clips);
int mia_whisper_read_logit_trace(mia_whisper* w, int slot, int first_pos, int n_pos, float* out);

/* Replaces model.encode(mel) (WhisperDecoding.swift:98 -> AudioEncoder.swift:43-68) for a batch of 30 s windows and
 * primes the decoder's cross-attention K/V (MultiHeadAttention.swift:49-59).
 *   mel: [B][2*n_audio_ctx][n_mels] in the model's compute dtype. */
int mia_whisper_encode(mia_whisper* w, const void* mel, int B, int mem);
/* Copy the audio features of the last encode ([B][n_audio_ctx][n_audio_state]) out as `dtype` (test hook). */
int mia_whisper_get_audio_features(mia_whisper* w, void* out, int dtype, int mem);

/* Replaces GreedyDecoder.decode's loop (WhisperDecoding.swift:135-359) for the B clips of the last encode:
 * decoder forward with KV cache, logit rules, argmax / sampling, log-prob bookkeeping; all on device.
 *   tokens        int32 [B][max_tokens]: generated tokens (EOT stripped), zero padded
 *   n_tokens      int32 [B]
 *   avg_logprob   float [B]   sum logp / count(non-EOT)            (WhisperDecoding.swift:345-362)
 *   no_speech_prob float [B]  softmax(logits[sot_index])[no_speech] (WhisperDecoding.swift:158-169)
 * Output pointers are host or device according to `mem`. */
int mia_whisper_decode_greedy(mia_whisper* w, const mia_decode_opts* opts, int32_t* tokens, int32_t* n_tokens,
                              float* avg_logprob, float* no_speech_prob, int mem);

/* Language detection (WhisperModel.swift:223-260): one decoder step on [sot]; argmax/softmax over the language
 * token range [sot+1, sot+1+n_languages).  lang_idx int32 [B], prob float [B] (host pointers). */
int mia_whisper_detect_language(mia_whisper* w, int32_t sot, int32_t n_languages, int32_t* lang_idx, float* prob);

/* One 30 s window per clip, end to end (log-mel -> encode -> greedy decode), i.e. the body of the reference's
 * transcribe loop for a batch (WhisperSTT.swift:140-145,181-213).  pcm/offs as in mia_logmel_whisper; pcm and the
 * outputs live in `mem`. */
/* The first half of mia_whisper_transcribe_windows alone: log-mel + encoder (the cross K/V of every decoder layer are primed); follow
 * with mia_whisper_decode_greedy.  Lets a host that drives several handles run their (MFMA-bound) encoders and their
 * (latency-bound) decoders in separate phases: decoders of different batches overlap each other well, an encoder next to a decoder does
 * not. */
int mia_whisper_encode_windows(mia_whisper* w, const float* pcm, const int64_t* offs, int B, int64_t pad_right, int mem);
/* Serving-side scheduling aid: from now on the encoder half of mia_whisper_encode_windows / mia_whisper_transcribe_windows (log-mel,
 * encoder, cross K/V) is enqueued on `hip_stream` instead of the context's stream, ordered against it by events in both directions (the
 * order of a handle's own work does not change).  A host that drives several handles can then create the contexts (decode chains:
 * thousands of short dependent kernels) on HIGH-priority streams and hand every handle a normal-priority encode stream: the decode
 * kernels of one batch are then dispatched ahead of the queued tiles of another batch's encoder instead of taking turns with them.
 * NULL restores the single-stream form.  The stream must belong to the context's device and outlive the handle's use of it. */
int mia_whisper_set_encode_stream(mia_whisper* w, void* hip_stream);
/* Throughput hint for handles that share one weight copy (mia_whisper_clone) and decode CONCURRENTLY on their own streams.  The step
 * chooses its cache policies from the model's byte counts alone (layer weights kept resident in the 256 MiB Infinity Cache when
 * they fit beside a step's other cached bytes, everything read once per step non-temporal), for one reader and for several, so on a
 * model that fits (large-v3-turbo, packed or not) this call selects nothing.  It still decides the weight loads of a model whose layer
 * weights exceed that budget (large-v3) and of the earlier policies (mia_whisper_set_debug bit 4): default policy with
 * concurrent_readers > 1, non-temporal with 1.  Results are bit-identical
 * either way.  Call on every handle of the group; takes effect at the next decode. */
int mia_whisper_set_weight_sharing(mia_whisper* w, int concurrent_readers);
int mia_whisper_transcribe_windows(mia_whisper* w, const float* pcm, const int64_t* offs, int B, int64_t pad_right,
                                   const mia_decode_opts* opts, int32_t* tokens, int32_t* n_tokens, float* avg_logprob,
                                   float* no_speech_prob, int mem);

/* ---- device-resident log-mel for the seek loop ---------------------------------------------------
 * WhisperSTT.transcribe computes the log-mel of the WHOLE clip once (+ 30 s of zeros), keeps it on the device and slices every 30 s
 * window out of it there (STT/Whisper/WhisperSTT.swift:140-145 whisperLogMelSpectrogram(audio:nMels:padding: nSamples); :171-182
 * mel[seek ..< seek + segmentSize], padOrTrimMel, .asType(.float16)).  mia_whisper_audio is that tensor for a batch of clips, owned by
 * the library.
 *   mia_whisper_audio_create: log-mel of n_clips whole clips (pcm / offs as in mia_logmel_whisper, pcm in `mem`; pad_right zeros appended
 *     to each, the reference passes 480000) in ONE batched launch, kept in HBM as fp32 [n_clips][F][n_mels] with
 *     F = max_b (len_b + pad_right) / 160; frames past a clip's own count are 0.0 (as mia_logmel_whisper).  A clip's values do not
 *     depend on the batch it is computed in.  n_mels is the model's (a multiple of 8).  NULL on failure (mia_last_error of w's context).
 *     Free it before the context of `w`.
 *   mia_whisper_audio_frames: F.
 *   mia_whisper_audio_read (test hook): frames [first_frame, first_frame + n_frames) of `clip` -> out, host float32 [n_frames][n_mels]. */
typedef struct mia_whisper_audio mia_whisper_audio;
mia_whisper_audio* mia_whisper_audio_create(mia_whisper* w, const float* pcm, const int64_t* offs, int n_clips, int64_t pad_right,
                                            int mem);
void mia_whisper_audio_free(mia_whisper_audio* a);
int64_t mia_whisper_audio_frames(const mia_whisper_audio* a);
int mia_whisper_audio_read(mia_whisper_audio* a, int clip, int64_t first_frame, int64_t n_frames, float* out);
/* model.encode of B windows addressed inside a resident mel (the loop body's encode, WhisperSTT.swift:171-182 -> WhisperDecoding.swift:98;
 * findAlignment's own encoder pass, WhisperTiming.swift:590-598; detectLanguage's, WhisperSTT.swift:155-161): window b = frames
 * [seek[b], seek[b] + n_valid[b]) of clip clip[b], zero-padded to 2*n_audio_ctx rows (padOrTrimMel), rounded to the compute dtype
 * (round to nearest even) and written straight into the encoder's input layout by one gather kernel; then the encoder and the cross
 * K/V exactly as mia_whisper_encode.  Bit-identical to mia_whisper_encode of the same windows sliced, padded and rounded on the host.
 * clip / seek / n_valid are host arrays of B entries; clip[] may repeat an index.  MIA_ERR_INVALID_ARGUMENT (before anything is
 * launched) for B <= 0, clip[b] outside [0, n_clips), seek[b] < 0, n_valid[b] outside [0, 2*n_audio_ctx], seek[b] + n_valid[b] > F,
 * or an audio made for another n_mels or device.  Honours mia_whisper_set_encode_stream like mia_whisper_encode_windows; profiling
 * class of the gather: "mel_gather" (work = bytes). */
int mia_whisper_encode_audio_windows(mia_whisper* w, mia_whisper_audio* a, const int32_t* clip, const int64_t* seek,
                                     const int32_t* n_valid, int B);

/* Word-timestamp alignment: the tensor half of findAlignment (STT/Whisper/WhisperTiming.swift:558-748; model.forwardWithCrossQK,
 * STT/Whisper/WhisperModel.swift:95-99).  For every clip of the last encode: a teacher-forced decoder pass over
 * tokens[b][0..n_tokens[b]) = [sot sequence, no_timestamps, text tokens, eot] keeps the pre-softmax cross-attention scores of the
 * alignment heads (heads int32 [n_heads][2] = (layer, head), the model's alignment_heads); on the device: softmax over the first
 * num_frames[b] / 2 frames, standardisation over tokens, width-7 median filter (reflect), mean over heads; on the host like the
 * reference: DTW over rows [row_start, n_tokens[b] - 1) (row_start = index of no_timestamps) of the negated matrix.
 *   token_probs [B][stride]: P(tokens[p + 1]) under softmax(logits[p][0:eot]);  text_idx / time_idx [B][path_cap] + path_len [B]: the
 *   DTW path (row index relative to row_start, frame index);  matrix (nullable) [B][stride][n_audio_ctx]: the filtered, head-averaged
 *   weights.  All host pointers.  Word splitting and the jump-time arithmetic (:735-820) stay with the caller (tokenizer text). */
int mia_whisper_align(mia_whisper* w, const int32_t* tokens, int stride, const int32_t* n_tokens, const int32_t* heads, int n_heads,
                      const int32_t* num_frames, int row_start, int eot, float* token_probs, int32_t* text_idx, int32_t* time_idx,
                      int32_t* path_len, int path_cap, float* matrix);

/* ---- neural codec decoders (fp32, like the reference) ------------------------------------------ */
/* SNACConfig (TTS/Orpheus/SNAC/SNACConfig.swift:9-94); tensors use the checkpoint key schema the reference loads
 * (decoder.model.layers.N..., quantizer.quantizers.i.{codebook.weight,out_proj.{weight_g,weight_v,bias}};
 * SNACDecoder.swift:101-243,358-368), float32. */
typedef struct {
  int32_t latent_dim, decoder_dim;
  int32_t n_rates; int32_t decoder_rates[8];
  int32_t n_vq; int32_t vq_strides[4];
  int32_t codebook_size, codebook_dim;
  int32_t noise, depthwise;
} mia_snac_config;
/* DACConfig (Codec/DAC/DACModel.swift:169-203): decoder side only. */
typedef struct {
  int32_t latent_dim, decoder_dim;
  int32_t n_rates; int32_t decoder_rates[8];
  int32_t n_codebooks, codebook_size, codebook_dim;
} mia_dac_config;

mia_codec* mia_snac_load(mia_ctx* ctx, const mia_snac_config* cfg, const mia_tensor_view* tensors, int n_tensors);
mia_codec* mia_dac_load(mia_ctx* ctx, const mia_dac_config* cfg, const mia_tensor_view* tensors, int n_tensors);
void mia_codec_free(mia_codec* c);
/* Samples produced / Gaussian values consumed for a latent of `latent_len` steps (SNAC: max_i n_i*vq_stride_i; DAC: T). */
int64_t mia_codec_output_len(mia_codec* c, int64_t latent_len);
int64_t mia_codec_noise_len(mia_codec* c, int64_t latent_len);
/* Replaces SNACDecoder.decode(codes:) (TTS/Orpheus/SNAC/SNACDecoder.swift:281-289, called at
 * TTS/Orpheus/TTSEngine/OrpheusTTS.swift:361).  codes[i] -> n_codes[i] ids of VQ level i.  `noise`: the N(0,1) draws of
 * the NoiseBlocks (NoiseBlock.swift:33), block after block, mia_codec_noise_len() values in total, or NULL for none.
 * pcm: float32 mono 24 kHz. */
int mia_snac_decode(mia_codec* c, const int32_t* const* codes, const int32_t* n_codes, int n_levels, const float* noise,
                    int64_t n_noise, float* pcm, int64_t pcm_capacity, int64_t* n_samples, int mem);
/* Replaces DACCodec.decodeFromCodes (Codec/DAC/DACModel.swift:303-306) for one sequence: codes int32 [n_codebooks][T]. */
int mia_dac_decode(mia_codec* c, const int32_t* codes, int n_codebooks, int64_t T, float* pcm, int64_t pcm_capacity,
                   int64_t* n_samples, int mem);
/* n_utt utterances in one pass; utterance u = mia_snac_decode of its own codes / noise, bit for bit (every convolution runs once over
 * the stacked sequences; a sequence's rows past its own end read as zero, exactly the padding a single call sees).
 * codes: utterance after utterance, level after level, concatenated; n_codes[u*n_levels + i] ids of level i of utterance u (a level
 *        whose expansion differs from that utterance's latent length is skipped for that utterance only).
 * noise: each utterance's slab exactly as mia_snac_decode takes it, concatenated (slab u holds mia_codec_noise_len(T0_u) values), or NULL.
 * pcm:   utterance u at pcm + pcm_off[u]; pcm_off has n_utt + 1 entries, pcm_off[u+1] - pcm_off[u] >= mia_codec_output_len(T0_u);
 *        n_samples[u] receives the count.  1 <= n_utt <= 64.
 * n_codes, pcm_off and n_samples are HOST arrays whatever `mem` is; `mem` describes codes, noise and pcm.  Scratch: three buffers of
 * n_utt x (largest stage of the longest utterance), grow-only. */
int mia_snac_decode_batch(mia_codec* c, int n_utt, const int32_t* codes, const int32_t* n_codes, int n_levels, const float* noise,
                          int64_t n_noise, float* pcm, const int64_t* pcm_off, int64_t* n_samples, int mem);
/* The same for DAC: codes of utterance u are [n_codebooks][T[u]], utterances concatenated; T (host) has n_utt entries. */
int mia_dac_decode_batch(mia_codec* c, int n_utt, const int32_t* codes, int n_codebooks, const int64_t* T, float* pcm,
                         const int64_t* pcm_off, int64_t* n_samples, int mem);
/* Bytes of activations (all utterances, three buffers) up to which a stage of the batch entries runs stacked; from the first stage
 * above it every utterance runs the rest of the program on its own, with the single call's launches.  Stage 0 always runs stacked.
 * Default: 256 MiB (the Infinity Cache) for SNAC, whose late stages are memory-bound; no limit for DAC.  bytes < 0 restores the
 * handle's default.  The waveforms do not depend on it, only the time. */
int mia_codec_set_stack_budget(mia_codec* c, int64_t bytes);
/* Encoder side of the DAC codec: replaces DACCodec.encode (Codec/DAC/DACModel.swift:284-296): preprocess (right-pad to the hop
 * length :308-317) -> DACEncoder (:43-86; blocks :15-38) -> residual vector quantisation (DACQuantize.swift:147-190, nearest entry
 * on L2-normalised vectors :87-115, first index on ties).  mia_dac_load_encoder attaches the `encoder.*` and
 * `quantizer.quantizers.N.in_proj.*` tensors to a handle made by mia_dac_load (encoder_dim * 2^n_rates must equal its latent width).
 * mia_dac_encode: pcm float32 mono [n_samples] -> codes int32 [n_quantizers][codes_capacity] (row q holds *n_steps ids);
 * n_quantizers <= 0 = all codebooks.  mia_dac_code_len(n_samples) = steps produced. */
typedef struct {
  int32_t encoder_dim;
  int32_t n_rates; int32_t encoder_rates[8];
} mia_dac_encoder_config;
int mia_dac_load_encoder(mia_codec* c, const mia_dac_encoder_config* cfg, const mia_tensor_view* tensors, int n_tensors);
int64_t mia_dac_code_len(mia_codec* c, int64_t n_samples);
int mia_dac_encode(mia_codec* c, const float* pcm, int64_t n_samples, int n_quantizers, int32_t* codes, int64_t codes_capacity,
                   int64_t* n_steps, int mem);

/* ---- Mimi codec decode (TTS/Marvis/Mimi/, fp32 like the reference) ------------------------------------------------
 * mia_mimi_config (include/mia_mimi.h, included by the callers that fill one) carries the fields of MimiConfig / SeanetConfig /
 * MimiTransformerConfig (Mimi.swift:17-103) the decoder uses.  upsample_stride =
 * sample_rate / prod(ratios) / frame_rate (Mimi.swift:128-129).  Flags are 0 / 1: seanet_pad_constant = padMode == .constant,
 * layer_norm = norm == "layer_norm", layer_scale = a LayerScale is present, rope = positionalEmbedding == "rope".
 * Tensors: float32 under the names and layouts Mimi.sanitize produces (Mimi.swift:305-377; checkpoint.sanitize_mimi), decoder side only:
 * quantizer.rvq_{first,rest}.{vq.layers.N.codebook.{embedding_sum,cluster_usage},output_proj.weight}, upsample.convtr.convtr.weight,
 * decoder_transformer.transformer.layers.N.*, decoder.{init_conv1d,layers.N.upsample,layers.N.residuals.0.block.M,final_conv1d}.*.
 * The loader refuses, each with its own message (MIA_ERR_INVALID_ARGUMENT): head_dim != 64, kv_repeat != 1, gating, a norm other than
 * layer_norm, a non-causal / non-constant-padded / shortcut-convolution SEANet, more than one residual layer per stage, an upsample
 * stride other than 2, and channel counts that are not multiples of 32 (the tap GEMM's rule). */
typedef struct mia_mimi_config mia_mimi_config;        /* defined in include/mia_mimi.h */
typedef struct mia_mimi mia_mimi;
typedef struct mia_mimi_stream mia_mimi_stream;
mia_mimi* mia_mimi_load(mia_ctx* ctx, const mia_mimi_config* cfg, const mia_tensor_view* tensors, int n_tensors);
void mia_mimi_free(mia_mimi* m);
/* samples per n_frames code frames: n_frames * upsample_stride * prod(ratios) (1920 per frame for mimi_202407) */
int64_t mia_mimi_output_len(mia_mimi* m, int64_t n_frames);
/* Replaces Mimi.decode (Mimi.swift:184-192; MarvisTTS.swift:534): codes int32 [n_q][T] -> pcm float32 [T * samples per frame].  The
 * transformer runs full bidirectional attention over all 2 T positions at RoPE offset 0, as the reference's fresh cache with a nil mask
 * does.  1 <= n_q <= nq: the sum runs over the codebooks given.
 * `codes` is a HOST array in both entries; `pcm_mem` (a mia_mem) describes pcm alone.  Before anything is launched every id is checked:
 * an id outside [0, bins), n_q outside [1, nq], a pcm_capacity below mia_mimi_output_len(T) and, in a stream, an n_q other than the
 * stream's first call's are MIA_ERR_INVALID_ARGUMENT, and the handle / stream is unchanged.  T = 0 / n = 0 succeed with 0 samples. */
int mia_mimi_decode(mia_mimi* m, const int32_t* codes, int n_q, int64_t T, float* pcm, int64_t pcm_capacity, int64_t* n_samples,
                    int pcm_mem);
/* Replaces MimiStreamingDecoder (Mimi.swift:213-239; MarvisTTS.swift:536).  A stream owns, on the device, what the reference's step
 * carries: per transformer layer the last `context` positions of rotated keys and of values, the running position, and per
 * convolution the input rows its next call needs.  Several streams may share a handle; calls on one context are serialised by the
 * caller.  mia_mimi_stream_decode(n frames) equals n calls of decodeStep: the two positions of frame f attend to the keys at positions
 * [max(0, 2 f - context), 2 f + 2).  It runs ONE pass over the n frames.  Streamed and whole-clip decodes are different functions of
 * the same codes, as in the reference.  mia_mimi_stream_reset = MimiStreamingDecoder.reset().  Free a handle's streams before the handle. */
mia_mimi_stream* mia_mimi_stream_create(mia_mimi* m);
void mia_mimi_stream_free(mia_mimi_stream* s);
int mia_mimi_stream_reset(mia_mimi_stream* s);
int mia_mimi_stream_decode(mia_mimi_stream* s, const int32_t* codes, int n_q, int64_t n, float* pcm, int64_t pcm_capacity,
                           int64_t* n_samples, int pcm_mem);
/* Mimi encode (Mimi.encode, Mimi.swift:174-182; the codec call of MarvisTTS.tokenizeAudio, MarvisTTS.swift:318-348).  The encode side of
 * a handle is OPTIONAL: it is loaded when the tensors carry encoder.{init_conv1d,layers.N.residuals.0.block.M,layers.N.downsample,
 * final_conv1d}.conv.conv.*, encoder_transformer.transformer.layers.N.*, downsample.conv.conv.weight [D][2 stride][D] and
 * quantizer.rvq_{first,rest}.input_proj.weight [dq][1][D].  With none of them the handle is the decode-only one and every entry below
 * returns MIA_ERR_INVALID_ARGUMENT ("no encoder loaded"); with some but not all the load fails and names the missing tensor.  The encode
 * side additionally needs quantizer_dim to be a multiple of 8, at most 504.
 * Lengths: every strided stage maps L rows to ceil(L / r), so n_samples samples give P = the ceil chain over the SEANet ratios
 * positions and mia_mimi_encode_frames = ceil(P / upsample_stride) code frames (one frame per 1920 samples, rounded up, for
 * mimi_202407); 0 for a decode-only handle or n_samples < 1.
 * mia_mimi_encode: pcm float32 [n_samples] at the codec's rate (host or device, `pcm_mem`) -> codes int32 [n_q][T], a HOST array of
 * dense rows of T = *n_frames ids (codes_capacity, in frames, only has to cover T).  n_q in [1, nq] asks for the first n_q stages of the
 * split residual quantiser (row 0 = rvq_first); their codes do not depend on the later stages.  Equal distances go to the lowest index.
 * mia_mimi_encode_latent stops in front of the quantiser: the [T][d_model] rows it sees (`data_mem` describes pcm and latent alike;
 * capacity in frames).  mia_mimi_quantize is the quantiser alone on caller latents (`latent_mem` describes `latent`; `codes` is a
 * host array [n_q][T]).  As with pcm_mem above, the parameter names say what the memory kind covers.
 * mia_mimi_quantize(mia_mimi_encode_latent(x)) == mia_mimi_encode(x) bit for bit.
 * Refused with MIA_ERR_INVALID_ARGUMENT before anything is launched, the handle and its streams unchanged: a null pointer,
 * n_samples < 1, n_q outside [1, nq], a capacity below mia_mimi_encode_frames(n_samples), T outside [1, 2^21], and a clip of more than
 * 2^27 / seanet_nfilters samples (2^21 = 87 s at 24 kHz for mimi_202407: the three rotating SEANet buffers of n_samples x nfilters
 * floats are 512 MiB each at that length).  Mimi.encodeStep (streaming encode) has no caller in the reference and is not built. */
int64_t mia_mimi_encode_frames(mia_mimi* m, int64_t n_samples);
int mia_mimi_encode(mia_mimi* m, const float* pcm, int64_t n_samples, int n_q, int32_t* codes, int64_t codes_capacity, int64_t* n_frames,
                    int pcm_mem);
int mia_mimi_encode_latent(mia_mimi* m, const float* pcm, int64_t n_samples, float* latent, int64_t capacity, int64_t* n_frames,
                           int data_mem);
int mia_mimi_quantize(mia_mimi* m, const float* latent, int64_t T, int n_q, int32_t* codes, int latent_mem);

/* ---- OuteTTS speaker-profile audio (TTS/OuteTTS/OuteTTSAudioProcessor.swift) ------------------------------------
 * The sample arithmetic of createSpeakerFromTranscription (:363-453); the word / code slicing around it is host integer arithmetic
 * (outetts.py).  Caller arrays are HOST pointers in every entry point of this section.
 *   mia_speaker_audio_create: preprocessAudioForSpeaker (:289-336) of a host clip, kept in HBM as fp32 [n]: gain to target_loudness_db RMS
 *     (measured over max(n, 0.4 s) samples, the reference's zero padding) and the peak limiter at peak_limit_db, folded into one factor
 *     that multiplies once (the reference multiplies twice in fp32: one rounding apart).  target_loudness_db = NaN keeps the clip as
 *     given (features of raw samples).  n <= 2^24 (11.6 min at 24 kHz).  NULL on
 *     failure (mia_last_error of ctx).  Free it before ctx.
 *   mia_speaker_audio_data: DEVICE pointer of the clip; feeds mia_dac_encode in device mode.  mia_speaker_audio_read: test hook.
 *   mia_speaker_audio_features: extractAudioFeatures (:191-216) of S segments [start[s], start[s] + len[s]) of the clip.
 *     feat int32 [S][3] = energy, spectral_centroid, pitch, each Int(round(v * 100)) in 0..100; raw (nullable) float32 [S][3] = RMS,
 *     centroid in Hz, normalised pitch before that rounding.  len 0 or a non-finite sample -> (0, 0, 0).
 *     Centroid (:219-277): real DFT of N = 2^ceil(log2 n) points, vDSP's packed bins (bin 0 = sqrt(DC^2 + Nyquist^2), no Nyquist bin).
 *     Pitch (:15-161): the reference's forward + inverse vDSP round trip has no conjugate product, so its "autocorrelation" is
 *     C (w x)[2j] for j < 200 and 0 above; that closed form is computed.  A segment of n <= 240 samples has no
 *     frame and pitch 0 (the reference traps at n <= 80).  All sums run in double in a fixed order: a segment's result does not depend
 *     on the other segments of the call.  The number of launches depends on the set of FFT sizes present, not on S:
 *     statistics + pitch frames (if any segment has a frame) + one per size up to mia_op_rfft_block, two per larger size + finish;
 *     mia_speaker_audio_launches returns the last call's count.
 *   mia_op_rfft_pow2 (operator-level hook of the FFT): unscaled DFT of x [n] zero-padded to N, out float32 [N/2+1][2].
 *     mia_op_rfft_block: the largest N one workgroup transforms in LDS; above it the transform is a four-step split.
 * MIA_ERR_INVALID_ARGUMENT before anything is launched: null pointers, n <= 0, sample_rate <= 0, n > 2^24, a segment outside [0, len],
 * S <= 0 (or > 65535), N not a power of two or outside 2..2^24, n > N. */
typedef struct mia_speaker_audio mia_speaker_audio;
mia_speaker_audio* mia_speaker_audio_create(mia_ctx* ctx, const float* pcm, int64_t n, int sample_rate, float target_loudness_db,
                                            float peak_limit_db);
void mia_speaker_audio_free(mia_speaker_audio* a);
int64_t mia_speaker_audio_len(const mia_speaker_audio* a);
const float* mia_speaker_audio_data(const mia_speaker_audio* a);
int mia_speaker_audio_read(mia_speaker_audio* a, int64_t first, int64_t n, float* out);
int mia_speaker_audio_features(mia_speaker_audio* a, const int64_t* start, const int64_t* len, int S, int32_t* feat, float* raw);
int mia_speaker_audio_launches(const mia_speaker_audio* a);
int64_t mia_op_rfft_block(void);
int mia_op_rfft_pow2(mia_ctx* ctx, const float* x, int64_t n, int64_t N, float* out);

/* ---- reference-clip trimming (Utils/AudioTrimmer.swift) ----------------------------------------------------------
 * The sample arithmetic of AudioTrimmer: findSpeechBounds (:218-274), which trimSilence (:142-207) shares up to its fall-backs; called
 * from TTS/CosyVoice2/CosyVoice2Engine.swift:420-424 and TTS/OuteTTS/OuteTTSEngine.swift:250-254.  The word logic of the same file
 * (:285-567) is host code (trim.py).  Caller arrays are HOST pointers in every entry point of this section.
 *   mia_clip_create: uploads a host clip once and keeps it in HBM as fp32 [n], unchanged.  n <= 2^26.  NULL on failure
 *     (mia_last_error of ctx).  Free it before ctx.  mia_clip_data: DEVICE pointer of the clip.  mia_clip_read: test hook.
 *   mia_clip_num_frames (host arithmetic): max(1, (n - frame) / hop + 1), the division truncating toward zero; 0 for a non-positive
 *     argument.  Frame i covers [i hop, min(i hop + frame, n)): only the one frame of a clip shorter than `frame` is short, and samples
 *     behind the last whole frame are in no frame.
 *   mia_clip_speech_bounds: a frame qualifies when max(ms, 1e-20) >= max(ms_max, 1e-20) * 10^(-top_db / 10), ms its mean square: the
 *     reference's 20 log10(max(rms, 1e-10)) >= max_dB - top_db in the energy domain, the ratio computed once on the host in double.
 *     start = first qualifying frame * hop, end = min((last qualifying frame + 1) * hop, n); found = 0 when no frame qualifies
 *     (top_db < 0 only) or start >= end.  Mean squares are summed in double in a fixed order (element j of a frame on lane j % 64, a
 *     fixed shuffle tree): a frame's energy is the same bits wherever the frame sits.  Two launches whatever the clip length
 *     (mia_clip_launches: the last bounds call's count, 0 after a refused one); energies stay in the ctx workspace, three integers
 *     come back.  A frame with a non-finite energy (a NaN or Inf sample inside a frame) is MIA_ERR_INVALID_AUDIO: the reference's
 *     max() over NaN depends on operand order and is not copied.
 *   mia_clip_frame_energy (test hook): the mean squares of frames [first_frame, first_frame + n_frames) as doubles.
 * MIA_ERR_INVALID_ARGUMENT before anything is launched: null pointers, n <= 0, n > 2^26, sample_rate <= 0, frame <= 0, hop <= 0,
 * frame > 2^20, a non-finite top_db, a frame range outside the clip's frames.  More than 2^22 frames: MIA_ERR_UNSUPPORTED. */
typedef struct mia_clip mia_clip;
mia_clip* mia_clip_create(mia_ctx* ctx, const float* pcm, int64_t n, int sample_rate);
void mia_clip_free(mia_clip* c);
int64_t mia_clip_len(const mia_clip* c);
const float* mia_clip_data(const mia_clip* c);
int mia_clip_read(mia_clip* c, int64_t first, int64_t n, float* out);
int mia_clip_speech_bounds(mia_clip* c, int64_t frame, int64_t hop, float top_db, int64_t* start, int64_t* end, int* found);
int mia_clip_frame_energy(mia_clip* c, int64_t frame, int64_t hop, int64_t first_frame, int64_t n_frames, double* ms_out);
int64_t mia_clip_num_frames(int64_t n, int64_t frame, int64_t hop);
int mia_clip_launches(const mia_clip* c);

/* ---- autoregressive LMs (Llama-3 / Qwen2 / Qwen3 blocks) ---------------------------------------- */
/* OrpheusConfig (TTS/Orpheus/BuildingBlocks/TransformerBlock.swift:16-34) / Qwen2Config (TTS/CosyVoice2/LLM/Qwen2LM.swift:15-43).
 * Tensors use the Hugging Face key schema both ports load: model.embed_tokens.weight, model.layers.N.self_attn.{q,k,v,o}_proj.weight
 * (+ .bias for q,k,v when qkv_bias), model.layers.N.mlp.{gate,up,down}_proj.weight, model.layers.N.{input,post_attention}_layernorm.weight,
 * model.norm.weight, lm_head.weight (absent when tie_embeddings).
 * Optional tensors switch behaviour by their presence (the struct below keeps its layout):
 *  - llm_decoder.{weight,bias}, speech_embedding.weight: the CosyVoice2 head and speech embedding (mia_lm_generate_ras).
 *  - model.layers.N.self_attn.q_norm.weight and .k_norm.weight, [head_dim] each: Qwen3's per-head RMSNorm of every query and key head
 *    (Qwen3Attention, STT/FunASR/Layers/Qwen3Model.swift:32-35,57-59,88-95; eps = rms_eps).  Applied in fp32 between the projection
 *    (+ bias, if any) and RoPE, y = x * rsqrt(mean(x^2 over head_dim) + eps) * w, inside the two kernels that finish q|k|v (no extra
 *    launch); V is untouched.  Both tensors in every layer or in none: one of a pair, some layers only, or a wrong length fail the load
 *    with a message naming the tensor.  A handle without them launches exactly the kernels it launched before.  n_heads * head_dim need
 *    not equal hidden (Qwen3-0.6B: 16 x 128 against 1024; Qwen3Config's Swift default head_dim is 64, the published config says 128 --
 *    both widths are supported).  mia_lm_set_kv_quant(bits != 0) on such a handle is MIA_ERR_UNSUPPORTED (the reference's Qwen3 decoder
 *    uses KVCacheSimple only, FunASRSTT.swift:120); packed step weights (mia_lm_attach_quantized) work as on any handle. */
typedef struct {
  int32_t vocab, hidden, inter, n_layers, n_heads, n_kv_heads, head_dim, max_ctx;
  float rms_eps, rope_theta;
  int32_t rope_llama3;            /* 1: Llama3RoPE frequency scaling (TTS/Shared/Llama3RoPE.swift:27-66) */
  float rope_factor, rope_low, rope_high;
  int32_t rope_old_ctx;
  int32_t qkv_bias, tie_embeddings;
} mia_lm_config;

/* sampleNextToken parameters (TTS/Orpheus/TTSEngine/OrpheusTTS.swift:375-470): repetition penalty over the last
 * rep_window generated ids -> /temperature -> top-p (keeps the first token crossing p) -> categorical. */
typedef struct {
  float temperature, top_p, rep_penalty;
  int32_t rep_window, max_new_tokens;
  int32_t n_stop; int32_t stop_ids[4];
  int32_t reserved;
} mia_lm_sampler;

mia_lm* mia_lm_load(mia_ctx* ctx, const mia_lm_config* cfg, const mia_tensor_view* tensors, int n_tensors, int dtype);
/* MLX-affine quantised (group 64; 4-, 6- or 8-bit codes) weights for the decode step: the reference's default Orpheus / CosyVoice2
 * checkpoints are quantised (TTS/Orpheus/TTSEngine/OrpheusWeightLoader.swift:28-60; the bit width is a loader option,
 * Models/TranscriptionResult.swift:162-198) and MLX multiplies them packed (quantizedMatmul).  mia_lm_attach_quantized takes every step
 * Linear as stored -- `<name>.weight` (MIA_U32 codes [N][K * bits / 32], one little-endian bit stream per row), `<name>.scales`, `<name>.biases` ([N][K/64],
 * both f16 or both bf16) -- onto a handle loaded from the de-quantised checkpoint; the per-token step then streams the packed codes and
 * multiplies them as MLX's own kernels do (per group: scale * sum(code * x) + bias * sum(x), the codes exact in the MFMA's 16-bit
 * operands, fp32 group sums); the batched prompt pass multiplies the 16-bit copy until mia_lm_set_prompt_weights(lm, 1) moves it to the
 * packed weights too.  One attach per handle.  mia_lm_attach_q4 = bits 4.
 * mia_lm_use_q4 toggles the step between the packed and the 16-bit weights (0 = 16-bit). */
int mia_lm_attach_quantized(mia_lm* lm, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits);
int mia_lm_attach_q4(mia_lm* lm, const mia_tensor_view* tensors, int n_tensors, int group_size);
int mia_lm_use_q4(mia_lm* lm, int on);
/* Which weights the batched prompt pass multiplies.  0 (default): the 16-bit copy, exactly as without this call.  1: the attached packed
 * weights, through a many-row packed GEMM (csrc/gemm_quant.hip) with the step's arithmetic -- per 64-input group scale * sum(code * x) +
 * bias * sum(x), fp32 sums, no weight formed or rounded -- so that the K/V rows of a prompt and those of generated tokens come from the
 * same function of the weights (the reference runs quantizedMatmul for both).  Everything else of the prompt pass is unchanged, and the
 * mode does not depend on mia_lm_use_q4.  Mode 1 without attached weights, or another mode: MIA_ERR_INVALID_ARGUMENT.
 * mia_lm_release_dense (packed weights attached, else MIA_ERR_INVALID_ARGUMENT) sets mia_lm_use_q4(1) and prompt mode 1 and frees the
 * layers' 16-bit Linears -- q|k|v, o, gate|up, down, row-major and fragment order; the embedding table, norms, biases and the head stay.
 * Afterwards mia_lm_use_q4(lm, 0) and mia_lm_set_prompt_weights(lm, 0) are MIA_ERR_UNSUPPORTED; everything else works as before.
 * mia_lm_weight_bytes reports the device bytes of weight matrices the handle holds now: *dense the 16-bit ones (tables, head, Linears in
 * both orders), *packed the attached codes and (scale, offset) pairs. */
int mia_lm_set_prompt_weights(mia_lm* lm, int mode);
int mia_lm_release_dense(mia_lm* lm);
int mia_lm_weight_bytes(mia_lm* lm, int64_t* dense, int64_t* packed);
/* Test hook: bit 0 = launch every step's kernels directly (no hipGraph), bit 1 = feed prompts token by token (no batched prompt
 * pass).  Results agree up to fp32 summation order. */
int mia_lm_set_debug(mia_lm* lm, int flags);
/* Which attention kernel the batched prompt pass runs (every entry point that feeds a prompt: mia_lm_forward, mia_lm_generate and its
 * batch / RAS / greedy forms).  0 (default): the single-token kernel, one workgroup per (query head, prompt row).  1: the tiled causal
 * grouped-query kernel of lm_prefill_attn.hip -- Q K^T and P V on the matrix cores, the query heads of a KV group sharing each staged
 * K / V tile -- for every run on the 16-bit cache; meant for long prompts (OuteTTS repeats its ~1 900-token speaker profile for every
 * sentence, TTS/OuteTTS/OuteTTS.swift:327-340).  With mia_lm_set_kv_quant(bits != 0) active the prompt pass keeps the packed cache's row
 * kernel whatever the mode; the decode step is the same in both modes.  The modes agree to the 16-bit rounding of the attention
 * probabilities, not bit for bit; within mode 1 a row's result does not depend on the chunk or batch it sits in.  Any other mode:
 * MIA_ERR_INVALID_ARGUMENT. */
int mia_lm_set_prompt_attention(mia_lm* lm, int mode);
void mia_lm_free(mia_lm* lm);
int mia_lm_reset(mia_lm* lm);
/* model(ids, cache) then logits[0,-1] (OrpheusTTS.swift:245-251,289): appends n ids to the KV cache, returns the fp32
 * logits after the last one into last_logits [vocab] (host pointer, may be NULL). */
int mia_lm_forward(mia_lm* lm, const int32_t* ids, int n, float* last_logits);
/* The whole sampling loop of generateChunk (OrpheusTTS.swift:245-348) on device: prompt, then up to max_new_tokens sampled
 * ids (stops after emitting a stop id).  uniforms: max_new_tokens values in [0,1), one per draw (explicit RNG: inverse CDF
 * over the kept tokens in index order).  Host pointers. */
int mia_lm_generate(mia_lm* lm, const int32_t* prompt, int n_prompt, const mia_lm_sampler* sampler, const float* uniforms,
                    int32_t* out_tokens, int32_t* n_out);
/* Sentence-level batching (MI355X-side addition; the reference generates its sentences one after another, OrpheusTTS.swift:179-191):
 * mia_lm_set_batch sizes the per-sequence state (K/V caches, repetition windows, ...) for up to max_batch <= 32 sequences;
 * mia_lm_generate_batch runs mia_lm_generate's loop for n_seq prompts side by side -- one read of the weights per step for all of
 * them.  prompts: all ids back to back, prompt_offsets [n_seq + 1]; uniforms [n_seq][max_new_tokens]; out_tokens
 * [n_seq][max_new_tokens]; n_out [n_seq].  Sequence b's output equals mia_lm_generate(prompt b, uniforms row b) on the same handle
 * capacity: a sequence's ids never depend on the batch it sits in.  (The capacity selects the step's kernel chain -- up to 4 sequences
 * the low-latency chain with the RMSNorm carried across the GEMMs, above that the split-K chain -- so runs under capacities on
 * different sides of 4 agree to fp32 summation order, not bit for bit.)  Host pointers. */
int mia_lm_set_batch(mia_lm* lm, int max_batch);
int mia_lm_generate_batch(mia_lm* lm, const int32_t* prompts, const int32_t* prompt_offsets, int n_seq, const mia_lm_sampler* sampler,
                          const float* uniforms, int32_t* out_tokens, int32_t* n_out);
/* Quantised KV cache: OrpheusModel.newCache(quantized:groupSize:bits:) (TTS/Orpheus/BuildingBlocks/TransformerBlock.swift:182-201,
 * re-exported at :236-241) returns QuantizedKVCache(groupSize: 64, bits: 4) instead of KVCacheSimple, and attentionWithCacheUpdate
 * (:91-99) routes every attention call of the layer to it.  bits 4 | 8, group_size 64: each K row (after RoPE) and V row is rounded
 * to the handle's 16-bit type as before, then kept per 64 consecutive elements of the head dimension as codes (uint32, little end
 * first) plus one (scale, bias) pair in that 16-bit type: scale = (max - min) / (2^bits - 1) (1 for a constant group), bias = min,
 * code = clamp(rint((x - bias) / scale), 0, 2^bits - 1) with the ROUNDED pair, value read back = scale * code + bias in fp32.
 * Attention then sees only values read back, the current token's row included.  MLX's rule restated from its public documentation,
 * unpinned against MLX; its nudge that makes zero exactly representable is not reproduced.  The 16-bit caches are not allocated in
 * this mode: 0.28x (4 bit) / 0.53x (8 bit) of their bytes.  bits 0 restores them.  The call re-allocates the per-sequence state at the
 * current capacity (either order with mia_lm_set_batch), drops the step graph and resets every sequence; cache contents are not
 * converted.  Every other entry point works unchanged in either mode.  bits outside {0, 4, 8}: MIA_ERR_INVALID_ARGUMENT;
 * group_size != 64: MIA_ERR_UNSUPPORTED; nothing is launched or allocated then. */
int mia_lm_set_kv_quant(mia_lm* lm, int bits, int group_size);
/* Test hook: rows [pos0, pos0 + n) of every kv head of (layer, seq) as fp32 [Hkv][n][dh] -- scale * code + bias in quantised mode, the
 * 16-bit values widened otherwise.  Host pointers; layer / seq / rows outside the handle: MIA_ERR_INVALID_ARGUMENT. */
int mia_lm_read_kv(mia_lm* lm, int layer, int seq, int pos0, int n, float* k_out, float* v_out);
/* CosyVoice2 RAS sampling parameters (TTS/CosyVoice2/LLM/Qwen2LM.swift:433-488 defaults: top_p 0.8, top_k 25, win 10, tau 0.1;
 * eos = speech_token_size (6561); min_len / max_len = 2x / 20x the text length, :368-372). */
typedef struct { float top_p; int32_t top_k; int32_t win; float tau; int32_t eos; int32_t min_len; int32_t max_len; } mia_ras_params;
/* Qwen2LM.inference + inferenceLoop (Qwen2LM.swift:335-427) on device.  The model must have been loaded with the extra
 * tensors llm_decoder.{weight,bias} and speech_embedding.weight.  prompt_embeds: float32 [n_prompt][hidden] =
 * [llm_embedding[sos], embed_tokens(prompt_text + text), llm_embedding[task], speech_embedding(prompt tokens)], gathered by
 * the caller.  uniforms: the stream of explicit draws (one per categorical; rejected EOS trials consume more).  Host pointers. */
int mia_lm_generate_ras(mia_lm* lm, const float* prompt_embeds, int n_prompt, const mia_ras_params* rp, const float* uniforms,
                        int n_uniforms, int32_t* out_tokens, int32_t* n_out);
/* mia_lm_generate_ras for n_seq utterances side by side (after mia_lm_set_batch): prompt_embeds = the rows of all prompts back to back
 * [prompt_offsets[n_seq]][hidden]; rp [n_seq] (top_p, top_k, win, tau, eos must agree; min_len / max_len are per utterance); uniforms
 * [n_seq][n_uniforms]; out_tokens [n_seq][out_stride], out_stride >= max(max_len) + 1; n_out [n_seq].  Utterance b's ids equal
 * mia_lm_generate_ras(prompt b, rp[b], uniforms row b).  Host pointers. */
int mia_lm_generate_ras_batch(mia_lm* lm, const float* prompt_embeds, const int32_t* prompt_offsets, int n_seq, const mia_ras_params* rp,
                              const float* uniforms, int n_uniforms, int32_t* out_tokens, int out_stride, int32_t* n_out);
/* Fun-ASR's decoder loop (STT/FunASR/FunASRSTT.swift:118-156 with FunASRConfig.temperature 0, its default: sampleNextToken takes
 * MLX.argMax, FunASRModel.swift:160-163) on device.  prompt_embeds: float32 [n_prompt][hidden], the merged prompt
 * [text ... sos | audio embeddings | eos ... text] (FunASRModel.mergeEmbeddings, :71-141; gathered by the caller).  The rows go through
 * the batched prompt pass and the first step; every step then takes the argmax of the fp32 logits over the whole vocabulary (lowest
 * index on an exact tie, as MLX.argMax), embeds it through model.embed_tokens and projects through the tied embedding or lm_head.weight.
 * A sequence ends when it draws one of stop_ids (n_stop in 1..4) -- that id is NOT written to out_tokens and not counted in n_out
 * (:151-155) -- or after max_new_tokens ids.  out_tokens holds max_new_tokens ids.  The sampler is a node of the captured step graph; no
 * uniforms are involved.  The reference's temperature > 0 branch is mia_lm_generate_topk below.  MIA_ERR_INVALID_ARGUMENT,
 * before anything is launched: a null pointer, n_prompt <= 0, n_prompt + max_new_tokens > max_ctx, n_stop outside 1..4, a stop id
 * outside the vocabulary, a handle with llm_decoder / speech_embedding tensors.  Host pointers. */
int mia_lm_generate_greedy(mia_lm* lm, const float* prompt_embeds, int n_prompt, const int32_t* stop_ids, int n_stop,
                           int max_new_tokens, int32_t* out_tokens, int32_t* n_out);
/* mia_lm_generate_greedy for n_seq utterances side by side (after mia_lm_set_batch; n_seq above the capacity is
 * MIA_ERR_INVALID_ARGUMENT): prompt_embeds = the rows of all prompts back to back [prompt_offsets[n_seq]][hidden]; out_tokens
 * [n_seq][out_stride], out_stride >= max_new_tokens; n_out [n_seq].  Utterance b's ids equal mia_lm_generate_greedy(prompt b) on the
 * same handle capacity.  Host pointers. */
int mia_lm_generate_greedy_batch(mia_lm* lm, const float* prompt_embeds, const int32_t* prompt_offsets, int n_seq,
                                 const int32_t* stop_ids, int n_stop, int max_new_tokens, int32_t* out_tokens, int out_stride, int32_t* n_out);
/* The same loop with sampleNextToken's temperature > 0 branch (STT/FunASR/FunASRModel.swift:165-198: top-k, 50 when topK == 0, then
 * top-p inside the top-k set, then a categorical draw).  The reference leaves argPartition's ties, the order of the kept set when
 * topP >= 1 and MLXRandom open; here they are fixed by explicit uniforms, lowest index on ties and an inverse CDF.  For a row x[0..V) of
 * fp32 logits, temperature > 0, top_k >= 0, top_p > 0 and one uniform u in [0,1):
 *   1. k = min(top_k > 0 ? top_k : 50, V); 1 <= k <= 1024, a larger k is MIA_ERR_UNSUPPORTED.
 *   2. The kept set is the first k entries under "higher value first, then lower index" on the raw logits (-0 counts as +0); the selection
 *      is exact, ties at the k-th value included.  A NaN ranks below every number; a row whose best entry is NaN gives id 0.
 *   3. The kept entries are held in that order (the reference's argSort(-probs) order), also when top_p >= 1.
 *   4. top_p < 1: p_j = softmax((x_j - x_max) / temperature) over the k kept entries in fp32 (a kept NaN has p = 0),
 *      n = clamp(count(cumsum(p)_j < top_p) + 1, 1, k); otherwise n = k.
 *   5. q_j = softmax over the first n kept entries, w_j = q_j + 1e-10 (categorical(log(probs + 1e-10))); the pick is the first j with
 *      cumsum(w)_j > u * sum(w), or the last entry if rounding leaves none.  All sums run in a fixed order that depends on the row alone:
 *      a row's pick is the same bits in any batch, any call, captured graph or direct launch.
 *   6. Bookkeeping as mia_lm_generate_greedy (FunASRSTT.swift:132-156): a stop id ends the sequence and is neither emitted nor counted;
 *      the loop also ends after max_new_tokens ids.  Each draw of a sequence takes the next value of uniforms (max_new_tokens of them).
 * MIA_ERR_INVALID_ARGUMENT before anything is launched (the handle stays usable): what mia_lm_generate_greedy lists, a null uniforms
 * pointer, temperature or top_p not finite or <= 0, top_k < 0.  Host pointers. */
int mia_lm_generate_topk(mia_lm* lm, const float* prompt_embeds, int n_prompt, float temperature, int top_k, float top_p,
                         const int32_t* stop_ids, int n_stop, int max_new_tokens, const float* uniforms, int32_t* out_tokens, int32_t* n_out);
/* mia_lm_generate_topk for n_seq utterances side by side (see mia_lm_generate_greedy_batch): uniforms [n_seq][max_new_tokens]; utterance
 * b's ids equal mia_lm_generate_topk(prompt b, uniforms row b) on the same handle capacity.  Host pointers. */
int mia_lm_generate_topk_batch(mia_lm* lm, const float* prompt_embeds, const int32_t* prompt_offsets, int n_seq, float temperature,
                               int top_k, float top_p, const int32_t* stop_ids, int n_stop, int max_new_tokens, const float* uniforms,
                               int32_t* out_tokens, int out_stride, int32_t* n_out);
/* One sampleNextToken call of that branch (steps 1-5) on caller-provided logits [V]: *out = the picked id; kept_ids (may be NULL; room
 * for k ids) receives the n kept ids in kept order and *n_kept (may be NULL) their count.  Host pointers. */
int mia_sample_top_k_top_p(mia_ctx* ctx, const float* logits, int V, float temperature, int top_k, float top_p, float uniform,
                           int32_t* out, int32_t* kept_ids, int32_t* n_kept);
/* One sampleNextToken call on caller-provided logits (host pointers). */
int mia_sample_top_p(mia_ctx* ctx, const float* logits, int V, const int32_t* history, int n_hist, float rep_penalty,
                     float temperature, float top_p, float uniform, int32_t* out);

/* ---- Marvis TTS (CSM): backbone, depth decoder and frame sampler ----------------------------------------------- */
/* MarvisModel.generateFrame (TTS/Marvis/Models/MarvisModel.swift:466-545) and the loop of MarvisTTS.decodePrompt
 * (TTS/Marvis/MarvisTTS.swift:452-523) on device; the codes they produce are what mia_mimi_decode / mia_mimi_stream_decode take.
 * mia_marvis_config (include/mia_marvis.h, included by the callers that fill one) carries MarvisConfig and the two Llama stacks'
 * dimensions.  Tensors: 16-bit or float32 under the Module keys after the reference's stripModelPrefix + sanitize
 * (MarvisTTS.swift:249-282; checkpoint.sanitize_marvis): backbone.layers.N.self_attn.{q,k,v,o}_proj.weight, .mlp.{gate,up,down}_proj.weight,
 * .{input,post_attention}_layernorm.weight, backbone.norm.weight, the same under decoder., text_embeddings.weight [text_vocab][D],
 * audio_embeddings.weight [n_codebooks * audio_vocab][D], projection.weight [d_dec][D], codebook0_head.weight [audio_vocab][D],
 * audio_head [n_codebooks - 1][d_dec][audio_vocab] (applied as x @ W).  Weights are rounded to `dtype` (MIA_BF16 | MIA_F16); the residual
 * stream is fp32 as in the LM step.  A missing or mis-shaped tensor fails the load with a message naming it.  *status (may be NULL)
 * receives the code: MIA_ERR_UNSUPPORTED for attention_bias / mlp_bias and for audio_vocab > 8192 (the frame sampler holds a row in one
 * workgroup), MIA_ERR_INVALID_ARGUMENT for everything else wrong with the call.  head_dim 64 | 128, n_codebooks 2..32.
 *
 * A row is n_codebooks + 1 ids and a 0/1 mask of the same width; its embedding is
 *   sum_{c < K} mask[c] * audio_embeddings[c * audio_vocab + id[c]] + mask[K] * text_embeddings[id[K]]        (fp32, columns in that order).
 * RoPE is interleaved in the reference (pairs (x[2i], x[2i+1]), MarvisLlamaBackbone.swift:129-164); the loader permutes the rows of every
 * q_proj / k_proj head (new[i] = old[2i], new[i + dh/2] = old[2i+1]) and runs the LM step's split-half kernels: q.k is invariant under a
 * permutation applied to both.  The frequencies are Llama3ScaledRoPE.applyScaling's (:102-127) in its own fp32 operation order.
 * A frame: c0 = sample(codebook0_head(lastH)); the decoder starts on an empty cache at position 0, takes projection(lastH) and
 * projection(audio_emb(0, c0)) at positions 0 and 1 (as two single-row steps: row 0 contributes only its K/V), then
 * projection(audio_emb(i, c_i)) at position i + 1; the row at position i goes through audio_head[i - 1] and gives c_i;
 * codebooks = min(n_codebooks, max_codebooks), and codebooks = 1 runs no decoder step.
 *
 * The sampler (mia_sample_top_p_ascending is one draw of it) restates MLXLMCommon's TopPSampler -- the reference uses
 * TopPSampler(temperature: 0.9, topP: 0.8), MarvisTTS.swift:417 -- from that library's published source, which is not part of the reference
 * tree: the rule is unpinned against it.  Explicit uniforms replace its random draw.  For a row x[0..V) of fp32 logits, V <= 8192,
 * temperature > 0, 0 < top_p <= 1 and one uniform u in [0,1):
 *   1. p = softmax(x / temperature) in fp32 with the maximum subtracted; a NaN logit has p = 0.  A row without a positive finite sum gives id 0.
 *   2. The entries are ordered ascending by p, the lower index first on equal p; a NaN ranks below every number.
 *   3. c_j = the inclusive ascending cumulative sum.
 *   4. The kept entries are those from the first j with c_j > 1 - top_p (the subtraction in fp32) to the largest; if there is none, the
 *      largest alone.
 *   5. The pick is the first kept j whose cumulative sum over the kept entries, in that ascending order, exceeds u * (their sum); the
 *      last kept entry if rounding leaves none.
 *   6. Every sum runs in a fixed order that depends on the row alone: a pick is the same bits in a captured graph and in a direct launch.
 *
 * mia_marvis_frame = one generateFrame: appends T >= 1 rows (tokens, mask) [T][n_codebooks + 1] -- a fed-back frame narrower than the
 * prompt rows is written with mask 0 in its unused columns, which is the same sum -- draws `codebooks` ids with uniforms[codebooks], and
 * returns them in ids_out.  forced (may be NULL) [codebooks]: id i is replaced by forced[i] after its draw (teacher forcing).  logits_out
 * (may be NULL) [codebooks][audio_vocab] receives every head's fp32 logits.  The call applies no stop rule of its own.
 * mia_marvis_generate = decodePrompt: feeds the prompt [T][n_codebooks + 1], then draws up to max_frames frames, each fed back as
 * [frame | 0] with mask [1 .. 1 | 0]; a frame whose ids are all 0 ends the sentence and is not emitted.  uniforms [max_frames][codebooks],
 * frames_out [max_frames][codebooks], *n_frames = frames emitted.  T = 0 continues from the state the previous call left (the fed-back
 * row is the last emitted frame; the codebook count must not change): N frames per call, then the next N, for streaming.  A sequence
 * that has drawn the all-zero frame stays finished (0 frames) until mia_marvis_reset (= resetCaches).  The loop is one graph launch per
 * frame and reads the finished flags every 16th frame; for a finished sequence every kernel of the frames launched behind its all-zero
 * one is a no-op: nothing is drawn or emitted, no K/V row is written and no position advances.
 * Sentence-level batching (MI355X-side addition; the reference runs its sentences one after another, each behind the same voice prompt,
 * MarvisTTS.swift:421-445): mia_marvis_set_batch sizes the per-sequence state of the handle and of both stacks (K/V caches included) for up
 * to max_batch <= 32 sequences and resets them; mia_marvis_generate_batch runs mia_marvis_generate's loop for n_seq prompts side by side --
 * one read of the weights per step for all of them.  tokens / mask: the rows of all prompts back to back, prompt_offsets [n_seq + 1] (in
 * rows); uniforms [n_seq][max_frames][codebooks]; frames_out [n_seq][max_frames][codebooks]; n_frames [n_seq].  Sequence b's frames equal
 * mia_marvis_generate(prompt b, uniforms row b) on the same handle capacity (the capacity selects the step's kernel chain, as in
 * mia_lm_set_batch).  Sequences finish at different frames; the call returns when all have, or after max_frames.  It starts from and leaves
 * a reset handle (no continuation).  n_seq above the capacity, an empty prompt, or rows + max_frames > max_ctx for any prompt:
 * MIA_ERR_INVALID_ARGUMENT.
 * MIA_ERR_INVALID_ARGUMENT before anything is launched (the handle stays usable): null pointers, an id outside its table (text column
 * against text_vocab, audio columns against audio_vocab), a mask value other than 0 / 1, max_codebooks < 1, rows in the cache + T +
 * max_frames > max_ctx, a temperature that is not finite and positive, top_p outside (0, 1], T = 0 on a handle that has drawn no frame
 * since its reset.  A MIA_ERR_DEVICE after the first launch of a call (a failed launch or copy) resets the handle: its message says so.
 * Host pointers.
 * mia_marvis_set_debug: bit 0 launches every frame's kernels directly (no hipGraph), bit 1 walks prompts row by row through the step (no
 * batched prompt pass).  Ids are the same with bit 0; with bit 1 the logits agree up to fp32 summation order.
 * Packed weights (the published checkpoints are MLX-affine 6-bit, group 64, and the reference keeps every module that has a `.scales`
 * packed: MarvisTTS.installWeights, MarvisTTS.swift:220-226): mia_marvis_attach_quantized takes, onto a handle loaded from the
 * de-quantised checkpoint, `<p>.weight` (MIA_U32 codes [N][K * bits / 32]), `<p>.scales`, `<p>.biases` ([N][K/64], both f16 or both bf16)
 * for p = {backbone,decoder}.layers.L.self_attn.{q,k,v,o}_proj, .mlp.{gate,up,down}_proj and projection, and codebook0_head when the
 * checkpoint stores its `.scales`; bits 4 | 6 | 8, group_size 64.  q_proj / k_proj get the loader's row permutation on all three tensors
 * (packing runs along the input axis, so permuting rows is exact).  audio_head is never quantised and the embedding tables stay 16-bit
 * tables.  Hidden sizes, heads * head_dim and intermediate sizes of both stacks must be multiples of 128.  The frame's single-row steps
 * then stream the packed codes through the LM step's packed GEMMs (mia_lm_attach_quantized); prompts go through the 16-bit prompt pass
 * until mia_marvis_use_packed_prompt(m, 1) puts the backbone's prompt pass on the packed weights (mia_lm_set_prompt_weights; the decoder
 * has no prompt pass, and the frame graph does not hold the prompt pass, so nothing is dropped).  mia_marvis_release_dense frees the 16-bit
 * layer Linears of both stacks (mia_lm_release_dense) with both switches at 1; mia_marvis_use_packed(m, 0) and
 * mia_marvis_use_packed_prompt(m, 0) are MIA_ERR_UNSUPPORTED afterwards.  The projection's copies, audio_head and the tables stay.  One
 * attach per handle; the frame graph is dropped.  Errors as mia_lm_attach_quantized; after any of them the handle is exactly as before --
 * neither stack is packed unless both and the projection are.  mia_marvis_use_packed(m, 0 | 1) switches the frame between the 16-bit and
 * the packed weights (1 after a successful attach; 1 without an attach is MIA_ERR_INVALID_ARGUMENT) and drops the frame graph. */
typedef struct mia_marvis_config mia_marvis_config;    /* defined in include/mia_marvis.h */
typedef struct mia_marvis mia_marvis;
mia_marvis* mia_marvis_load(mia_ctx* ctx, const mia_marvis_config* cfg, const mia_tensor_view* tensors, int n_tensors, int dtype, int32_t* status);
void mia_marvis_free(mia_marvis* m);
int mia_marvis_reset(mia_marvis* m);
int mia_marvis_set_debug(mia_marvis* m, int flags);
int mia_marvis_set_batch(mia_marvis* m, int max_batch);
int mia_marvis_attach_quantized(mia_marvis* m, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits);
int mia_marvis_use_packed(mia_marvis* m, int on);
int mia_marvis_use_packed_prompt(mia_marvis* m, int on);
int mia_marvis_release_dense(mia_marvis* m);
int mia_marvis_frame(mia_marvis* m, const int32_t* tokens, const int32_t* mask, int T, int max_codebooks, float temperature, float top_p,
                     const float* uniforms, const int32_t* forced, int32_t* ids_out, float* logits_out);
int mia_marvis_generate(mia_marvis* m, const int32_t* tokens, const int32_t* mask, int T, int max_codebooks, float temperature, float top_p,
                        int max_frames, const float* uniforms, int32_t* frames_out, int32_t* n_frames);
int mia_marvis_generate_batch(mia_marvis* m, const int32_t* tokens, const int32_t* mask, const int32_t* prompt_offsets, int n_seq, int max_codebooks,
                              float temperature, float top_p, int max_frames, const float* uniforms, int32_t* frames_out, int32_t* n_frames);
/* One draw of the rule above on caller-provided logits [V]: *out = the picked id; kept_ids (may be NULL; room for V ids) receives the
 * kept ids in ascending order of p and *n_kept (may be NULL) their count.  V > 8192: MIA_ERR_UNSUPPORTED.  Host pointers. */
int mia_sample_top_p_ascending(mia_ctx* ctx, const float* logits, int V, float temperature, float top_p, float uniform, int32_t* out,
                               int32_t* kept_ids, int32_t* n_kept);

/* ---- Fun-ASR audio half: fbank + LFR + CMVN front end, SenseVoice SANM encoder, audio adaptor ------------------ */
/* FunASRModel.encodeAudio (STT/FunASR/FunASRModel.swift:41-58): waveform -> the audio rows mia_lm_generate_greedy's prompt takes.
 * SenseVoiceEncoderConfig + AudioAdaptorConfig (STT/FunASR/Config/FunASRConfig.swift:79-214).  Head dim is 128 in both stacks
 * (encoder_dim = n_heads * 128, llm_dim = adaptor_heads * 128); the adaptor blocks' ffn is llm_dim / 4; n_encoders0 = 1. */
typedef struct mia_sensevoice mia_sensevoice;
typedef struct { int32_t input_dim, encoder_dim, n_heads, ffn_dim, kernel_size, sanm_shift,
                 n_encoders0, n_encoders, n_tp_encoders;
                 int32_t adaptor_k, llm_dim, adaptor_ffn_dim, adaptor_layers, adaptor_heads; } mia_sensevoice_config;
/* float32 tensors under the reference's Module keys: audio_encoder.{encoders0,encoders,tp_encoders}.N.{norm1,norm2}.{weight,bias},
 * ....self_attn.{linear_q_k_v,linear_out}.{weight,bias}, ....self_attn.fsmn_block.weight ([D][1][K] as in the checkpoint or [D][K][1] as
 * FunASRModel.sanitize leaves it), ....feed_forward.{w_1,w_2}.{weight,bias}, audio_encoder.{after_norm,tp_norm}.{weight,bias},
 * audio_adaptor.{linear1,linear2}.{weight,bias}, audio_adaptor.blocks.N.self_attn.{linear_q,linear_k,linear_v,linear_out}.{weight,bias},
 * audio_adaptor.blocks.N.{norm1,norm2}.{weight,bias}, audio_adaptor.blocks.N.feed_forward.{w_1,w_2}.{weight,bias}.  Linear weights are
 * rounded to `dtype` (MIA_BF16 | MIA_F16); norms, biases and FSMN taps stay fp32.  NULL on failure: mia_last_error(ctx) names the
 * missing or mis-shaped tensor, or the config rule that failed (e.g. a sanm_shift that leaves a negative right context). */
mia_sensevoice* mia_sensevoice_load(mia_ctx* ctx, const mia_sensevoice_config* cfg, const mia_tensor_view* tensors, int n_tensors, int dtype);
void mia_sensevoice_free(mia_sensevoice* sv);
/* preprocessAudio (STT/FunASR/FunASRAudio.swift:197-216) for B clips of 16 kHz float32 audio laid back to back (offs: HOST int64 [B+1],
 * every clip longer than 200 samples): Hamming-window log-mel (1 + L/160 frames, natural log), LFR (7 frames stacked, every 6th kept:
 * t_lfr = ceil(frames / 6)), per-utterance CMVN.  feats_out float32 [sum t_lfr][stride] (stride >= 560), the clips' rows back to back;
 * t_lfr_out HOST int32 [B].  pcm / feats_out live in `mem`. */
int mia_sensevoice_features(mia_ctx* ctx, const float* pcm, const int64_t* offs, int B, float* feats_out, int32_t* t_lfr_out, int64_t stride, int mem);
/* Rows feats_out must hold for these clips (offs as above); < 0 on a bad argument. */
int64_t mia_sensevoice_feature_rows(const int64_t* offs, int B);
/* SenseVoiceEncoder + AudioAdaptor on B utterances stacked back to back: feats float32 [sum t_lfr[b]][input_dim]; t_lfr HOST int32 [B].
 * enc_out (nullable, the test tap) float32 [sum t_lfr[b]][encoder_dim]: the encoder's output after tp_norm.  emb_out float32
 * [sum n_out[b]][llm_dim] with n_out[b] = (t_lfr[b] - 1) / adaptor_k + 1 (HOST int32 [B]).  Every GEMM runs over all utterances at once;
 * utterance b's rows equal its own B = 1 call bit for bit.  feats / enc_out / emb_out live in `mem`. */
int mia_sensevoice_encode(mia_sensevoice* sv, const float* feats, const int32_t* t_lfr, int B, float* enc_out, float* emb_out, int32_t* n_out, int mem);
/* mia_sensevoice_features -> mia_sensevoice_encode with nothing leaving the device in between: emb_out float32 [sum n_out[b]][llm_dim]
 * (capacity: mia_sensevoice_feature_rows rows is always enough), n_out HOST int32 [B].  pcm / emb_out live in `mem`. */
int mia_sensevoice_encode_audio(mia_sensevoice* sv, const float* pcm, const int64_t* offs, int B, float* emb_out, int32_t* n_out, int mem);

/* ---- S3Tokenizer (speech -> 25 Hz token ids) ---------------------------------------------------- */
/* S3TokenizerModelConfig / V3 (Codec/S3Tokenizer/S3TokenizerConfig.swift:9-90): V2 = 6 blocks, V3 = 12. */
typedef struct { int32_t n_mels, n_audio_state, n_audio_head, n_audio_layer; } mia_s3_config;
/* float32 tensors, Module key schema of the reference: encoder.conv{1,2}.{weight,bias}, encoder.blocks.N.attn.{query,key,value,out}.*,
 * encoder.blocks.N.attn.fsmn_block.weight, encoder.blocks.N.{attn_ln,mlp_ln}.*, encoder.blocks.N.mlp.layers.{0,2}.*,
 * quantizer.fsq_codebook.project_down.{weight,bias}. */
mia_s3tok* mia_s3tok_load(mia_ctx* ctx, const mia_s3_config* cfg, const mia_tensor_view* tensors, int n_tensors);
void mia_s3tok_free(mia_s3tok* s3);
/* Replaces S3TokenizerV2.quantize(mel:melLen:) for clips of at most 30 s (Codec/S3Tokenizer/S3Tokenizer.swift:474-494; called at
 * TTS/CosyVoice2/CosyVoice2TTS.swift:391).  mel float32 [B][n_mels][T] (the layout mia_logmel_s3 emits), mel_len / tok_len host
 * int32 [B]; tokens int32 [B][tokens_stride], zero padded; token count = ((len-1)/2+1 - 1)/2 + 1. */
int mia_s3tok_encode(mia_s3tok* s3, const float* mel, const int32_t* mel_len, int B, int T, int32_t* tokens, int tokens_stride,
                     int32_t* tok_len, int mem);

/* ---- HiFT vocoder (80-bin mel @ 50 Hz -> 24 kHz waveform) ------------------------------------------ */
/* Constructor arguments of CosyHiFTGenerator (TTS/CosyVoice2/HiFiGAN/CosyHiFTGenerator.swift:283-300).  n_fft 16 / hop 4 are
 * fixed (istftParams).  The residual-block dilations are shared by every block ([1,3,5] in the reference). */
typedef struct {
  int32_t in_channels, base_channels, nb_harmonics, sampling_rate;
  int32_t n_ups; int32_t up_rates[4]; int32_t up_kernels[4];
  int32_t n_res_kernels; int32_t res_kernels[4];
  int32_t src_res_kernels[4];          /* one per upsample stage */
  int32_t n_dilations; int32_t dilations[4];
  float nsf_alpha, nsf_sigma, voiced_threshold, lrelu_slope, audio_limit;
} mia_hift_config;
typedef struct mia_hift mia_hift;
/* float32 tensors, Module key schema of the reference (CosyHiFTGenerator.swift:272-279): f0_predictor.condnet_{0,2,4,6,8}.*,
 * f0_predictor.classifier.*, m_source.l_linear.*, conv_pre.*, ups.N.*, source_downs.N.*, source_resblocks.N.{convs1,convs2}.M.*,
 * source_resblocks.N.{activations1,activations2}.M.alpha, resblocks.N.(same), conv_post.*  (Conv1d weight [Cout][K][Cin],
 * ConvTransposed1d weight [Cout][K][Cin]). */
mia_hift* mia_hift_load(mia_ctx* ctx, const mia_hift_config* cfg, const mia_tensor_view* tensors, int n_tensors);
void mia_hift_free(mia_hift* h);
/* samples produced per mel frame: prod(up_rates) * hop (480) */
int mia_hift_upsample_factor(const mia_hift* h);
/* CosyF0Predictor (CosyHiFTGenerator.swift:236-255): mel float32 [in_channels][T] (channel-major as in the reference) -> f0 [T]. */
int mia_hift_f0(mia_hift* h, const float* mel, int T, float* f0, int mem);
/* f0Upsample + SourceModuleHnNSF2 / SineGen2 (CosyHiFTGenerator.swift:96-153,190-203,408-410,487-495): f0 [T] -> source [480 T].
 * noise: the reference's MLXRandom.normal draw, float32 [480 T][nb_harmonics+1], or NULL for no additive noise.  The reference's
 * random initial phase (:103-111) only touches sample 0 of the full-rate `rad` track, which the 480:1 linear downsample never
 * reads (it reads samples 480 i + 239 / + 240), so it has no effect on the output and is not an input here.  T <= 17000. */
int mia_hift_source(mia_hift* h, const float* f0, int T, const float* noise, float* source, int mem);
/* CosyHiFTGenerator.decode(x:s:) (:412-475): mel [in_channels][T] + source [480 T] -> waveform [480 T], clipped to +-audio_limit. */
int mia_hift_decode(mia_hift* h, const float* mel, int T, const float* source, float* pcm, int mem);
/* CosyHiFTGenerator.callAsFunction (:482-505): f0 -> source (its first cache_len samples replaced by cache_source, the
 * streaming hand-over) -> decode.  source_out (nullable) receives the source actually used.  Every buffer lives in `mem`;
 * with MIA_MEM_DEVICE nothing is copied and the call returns after enqueueing on the ctx stream. */
int mia_hift_vocode(mia_hift* h, const float* mel, int T, const float* noise, const float* cache_source, int cache_len,
                    float* pcm, float* source_out, int mem);
/* mia_hift_vocode for n utterances in one pass (an MI355X-side addition, like mia_flow_inference_batch: the reference vocodes its
 * utterances one after another, CosyVoice2Model.swift:200-208).  mels: the utterances' [in_channels][T[u]] blocks back to back; noise
 * (nullable): their [480 T[u]][nb_harmonics+1] blocks back to back; pcm: 480 T[u] samples per utterance back to back.  Every
 * convolution runs once over the stacked sequences (a sequence's rows past its own end read as zero, the padding its single call
 * sees); each utterance's waveform equals its own mia_hift_vocode call bit for bit.  1 <= n <= 64.  The cache_source hand-over of
 * the streaming path stays with the single-utterance call.  Returns after the waveforms are in `pcm`. */
int mia_hift_vocode_batch(mia_hift* h, const float* mels, const int32_t* T, int n, const float* noise, float* pcm, int mem);

/* ---- CosyVoice2 flow (speech tokens -> 80-bin mel @ 50 Hz) ---------------------------------------- */
/* FlowConfig (TTS/CosyVoice2/Config/CosyVoice2Config.swift:79-127).  Built for the shapes the reference engine uses: head dim 64 in
 * both the conformer encoder (input_size = 64 * enc_heads) and the estimator, mel 80, dec_in_channels = 4 * 80, one U-Net level. */
typedef struct {
  int32_t input_size, output_size, spk_embed_dim, vocab_size, pre_lookahead_len, n_timesteps;
  int32_t enc_heads, enc_linear_units, enc_blocks, enc_up_blocks, upsample_stride;
  int32_t dec_in_channels, dec_channels, dec_heads, dec_n_blocks, dec_mid_blocks;
  float cfg_rate;   /* inference_cfg_rate, 0.7 */
} mia_flow_config;
typedef struct mia_flow mia_flow;
/* float32 tensors under the reference's (remapped) Module keys (CosyVoice2TTS.swift:320-336): input_embedding.weight,
 * spk_embed_affine_layer.*, encoder.{embed,up_embed}.{linear,norm}.*, encoder.pre_lookahead_layer.conv{1,2}.*, encoder.up_layer.conv.*,
 * encoder.{encoders,up_encoders}.N.{self_attn.{linear_q,linear_k,linear_v,linear_out,linear_pos}.*, self_attn.pos_bias_{u,v},
 * feed_forward.{w_1,w_2}.*, norm_mha.*, norm_ff.*}, encoder.after_norm.*, encoder_proj.*, decoder.estimator.time_mlp.linear_{1,2}.*,
 * decoder.estimator.{down_blocks.0,mid_blocks.N,up_blocks.0}.{resnet.{mlp_linear,block{1,2}.conv.conv,block{1,2}.norm,res_conv}.*,
 * transformers.K.{norm1,norm3,attn.{query_proj,key_proj,value_proj,out_proj},ff.layers.{0,1}}.*}, ...down_blocks.0.downsample.conv.*,
 * ...up_blocks.0.upsample.conv.*, decoder.estimator.final_block.{conv.conv,norm}.*, decoder.estimator.final_proj.*. */
mia_flow* mia_flow_load(mia_ctx* ctx, const mia_flow_config* cfg, const mia_tensor_view* tensors, int n_tensors);
void mia_flow_free(mia_flow* f);
/* input_embedding -> UpsampleConformerEncoder(streaming: false) -> encoder_proj (CosyVoice2Model.swift:496-522,
 * UpsampleConformerEncoder.swift:407-474): token int32 [n] -> mu float32 [upsample_stride * n][80]. */
int mia_flow_encode(mia_flow* f, const int32_t* token, int n_token, float* mu, int mem);
/* CosyVoice2FlowModule.inference(finalize: true) (CosyVoice2Model.swift:467-553) for one utterance:
 *   token [n_token], prompt_token [n_prompt] int32; prompt_feat float32 [prompt_feat_len][80] (the prompt's mel, time-major as in the
 *   reference); embedding float32 [spk_embed_dim]; z float32 [80][T], T = upsample_stride (n_token + n_prompt): the CFM's initial
 *   noise, which the reference draws internally (CosyVoice2CFM.swift:86) -- explicit here; n_timesteps <= 0 means cfg.n_timesteps.
 *   mel out float32 [80][T - prompt_feat_len] (channel-major, what CosyHiFTGenerator consumes).  Every buffer lives in `mem`. */
int mia_flow_inference(mia_flow* f, const int32_t* token, int n_token, const int32_t* prompt_token, int n_prompt, const float* prompt_feat,
                       int prompt_feat_len, const float* embedding, const float* z, int n_timesteps, float* mel, int mem);
/* n_utt utterances through ONE pass of the flow (an MI355X-side addition like mia_lm_generate_ras_batch: the reference synthesises its
 * sentences one after another, CosyVoice2Model.swift:155-208,467-553).  Every argument of mia_flow_inference becomes an array indexed by
 * utterance (prompt_token / prompt_feat may be null when every utterance has none; entry u may be null when n_prompt[u] /
 * prompt_feat_len[u] is 0); mel[u] receives float32 [80][T_u - prompt_feat_len[u]], T_u = upsample_stride (n_token[u] + n_prompt[u]).
 * The utterances run as stacked sequences padded to the longest one; padding never reaches a valid frame (per-sequence key masks and
 * zero look-ahead), so mel[u] is bit-identical to the utterance's own mia_flow_inference call.  1 <= n_utt <= 64. */
int mia_flow_inference_batch(mia_flow* f, int n_utt, const int32_t* const* token, const int32_t* n_token, const int32_t* const* prompt_token,
                             const int32_t* n_prompt, const float* const* prompt_feat, const int32_t* prompt_feat_len, const float* const* embedding,
                             const float* const* z, int n_timesteps, float* const* mel, int mem);
/* The same call with the two switches the modules carry for chunked synthesis:
 *   finalize = 0 drops the encoder's last pre_lookahead_len * upsample_stride frames before the CFM (CosyVoice2Model.swift:504-510), so
 *     T = upsample_stride (n_token + n_prompt) - that trim; z is [80][T] for THAT T and *mel_frames = T - prompt_feat_len;
 *   enc_static_chunk / dec_static_chunk > 0 turn on the block-causal "streaming" attention masks (query i sees keys below
 *     (i / chunk + 1) chunk: subsequentChunkMask, Codec/S3Gen/Transformer/UpsampleConformerEncoder.swift:124-195) of the conformer
 *     encoder (chunk, and chunk * upsample_stride after the up-sampling, :424-460) and of the estimator's transformer blocks
 *     (Codec/S3Gen/S3GenDecoder.swift:304-320); the checkpoint's values are encoder_static_chunk_size / decoder_static_chunk_size
 *     (TTS/CosyVoice2/Config/CosyVoice2Config.swift:155,166).  0 / 0 with finalize = 1 is mia_flow_inference. */
int mia_flow_inference_streaming(mia_flow* f, const int32_t* token, int n_token, const int32_t* prompt_token, int n_prompt, const float* prompt_feat,
                                 int prompt_feat_len, const float* embedding, const float* z, int n_timesteps, int finalize, int enc_static_chunk,
                                 int dec_static_chunk, float* mel, int* mel_frames, int mem);

/* ---- CAM++ speaker encoder (CosyVoice2 prepareConditionals, once per speaker) ---------------------------------
 * Replaces CAMPlusSpeakerEncoder (TTS/CosyVoice2/SpeakerEncoder/CAMPlusSpeakerEncoder.swift:12-150, called at
 * TTS/CosyVoice2/CosyVoice2TTS.swift:409) = Codec/S3Gen/CAMPPlus.swift: kaldiFbankCAMPPlus :32-108, CAMPPlus :687-785,
 * CAMPPlus.inference :788-818, in the one configuration that wrapper builds (80 fbank bins, 192-d embedding, growth 32,
 * bottleneck 4 x 32, 128 initial channels, "batchnorm-relu", segment output).  BatchNorm uses its running statistics. */
#define MIA_CAMPPLUS_DIM 192
typedef struct mia_campplus mia_campplus;
/* float32 tensors with the reference's Module key paths ("campplus." prefix already stripped, CAMPlusSpeakerEncoder.swift:93-104):
 * head.{conv1,conv2}.weight [32][3][3][Cin], head.{bn1,bn2}.{weight,bias,running_mean,running_var},
 * head.layer{1,2}.{0,1}.{conv1,conv2}.weight, .{bn1,bn2}.*, head.layer{1,2}.0.shortcut.{0.weight [32][1][1][32], 1.*},
 * tdnn.linear.weight [128][5][320], tdnn.nonlinear.0.*, blocks.B.layers.I.{nonlinear1.0.*, linear1.weight [128][1][Cin],
 * nonlinear2.0.*, cam_layer.linear_local.weight [32][3][128], cam_layer.linear1.{weight [64][1][128], bias},
 * cam_layer.linear2.{weight [32][1][64], bias}}, transits.B.{nonlinear.0.*, linear.weight}, out_nonlinear.0.*,
 * dense.linear.weight [192][1][1024], dense.nonlinear.0.{running_mean,running_var}. */
mia_campplus* mia_campplus_load(mia_ctx* ctx, const mia_tensor_view* tensors, int n_tensors);
void mia_campplus_free(mia_campplus* m);
/* kaldiFbankCAMPPlus (CAMPPlus.swift:32-108): pcm float32 mono 16 kHz [n_samples >= 400] -> fbank float32
 * [mia_kaldi_fbank_frames(n_samples)][80] (frame-major).  mean_norm != 0 also removes each bin's mean over time (:797-799),
 * which is what the encoder consumes; 0 gives extractFbank's raw features (CAMPlusSpeakerEncoder.swift:138-150). */
int64_t mia_kaldi_fbank_frames(int64_t n_samples);
int mia_campplus_fbank(mia_campplus* m, const float* pcm, int64_t n_samples, int mean_norm, float* fbank, int mem);
/* CAMPPlus.callAsFunction (:755-785) for one clip: feats float32 [n_frames][80] -> emb float32 [192]. */
int mia_campplus_forward(mia_campplus* m, const float* feats, int n_frames, float* emb, int mem);
/* CAMPPlus.inference (:788-818) for one clip: pcm float32 mono 16 kHz [n_samples] -> emb float32 [192]. */
int mia_campplus_embed(mia_campplus* m, const float* pcm, int64_t n_samples, float* emb, int mem);

/* ---- Kokoro: iSTFTNet decoder and F0 / N predictor blocks (prosody features + style -> 24 kHz waveform), fp32 -------------------
 * Replaces KokoroDecoder + Generator (TTS/Kokoro/Decoder/KokoroDecoder.swift:83-112, Generator.swift:133-192) with the harmonic
 * source (KokoroSineGen.swift, KokoroSourceModuleHnNSF.swift), the STFT pair (MLXSTFT.swift) and, when the tensors are there, the
 * part of Predictor.F0NTrain behind `shared` (TTSEngine/KokoroModel.swift:66-89).  mia_kokoro_config (include/mia_kokoro.h, included
 * by the callers that fill one) carries the constructor arguments; pred_dim = 0 means a handle without the F0 / N blocks.
 * Tensors: float32 under the reference's keys as KokoroWeightLoader.sanitizeWeights leaves them (checkpoint.sanitize_kokoro):
 * decoder.{encode,decode.N}.{conv1,conv2,conv1x1,pool}.{weight_g,weight_v,bias}, .{norm1,norm2}.fc.{weight,bias},
 * decoder.{F0_conv,N_conv,asr_res.0}.*, decoder.generator.{ups.N,conv_post}.*, .noise_convs.N.{weight,bias},
 * .{noise_res,resblocks}.N.{convs1,convs2}.K.*, .{adain1,adain2}.K.fc.*, .{alpha1,alpha2}.K [1][C][1], .m_source.l_linear.*, and
 * (optional, all or none) predictor.{F0,N}.N.* with predictor.{F0_proj,N_proj}.{weight,bias}.  Weight norm is folded at load
 * (w = g v / (||v|| + 1e-7) over every axis but 0 of the tensor as stored) and oriented by ConvWeighted's rule
 * (ConvWeighted.swift:118-122).  A missing tensor is an INVALID_ARGUMENT error that names it.
 * Channel-major arguments are [C][T], as the reference holds them; `data_mem` describes every buffer of a call (host or device, the HiFT entry points' convention).  Row counts: T in [1, 10000].
 *   mia_kokoro_output_len: samples of a T-row decode (600 T for the production shape).
 *   mia_kokoro_f0n: x [pred_dim][T] (the output of Predictor.shared), s_pred [style_dim] -> f0 [2 T], n [2 T].
 *   mia_kokoro_source: f0 [L] -> source [300 L] (f0 up-sampling, SineGen, l_linear + tanh) and har [60 L + 1][22] (STFT 20 / 5:
 *     11 magnitudes, then 11 phases; bins 0 and 10 have phase 0 or +pi).  noise float32 [300 L][9] stands in for
 *     MLXRandom.normal(sineWaves.shape), NULL = none; the random initial phase has no effect on the output and is not an input.
 *     Either output may be NULL.
 *   mia_kokoro_generate: Generator.callAsFunction from a given har: x [up_initial][L], s [style_dim], har [60 L + 1][22] -> pcm [300 L].
 *   mia_kokoro_decode: KokoroDecoder.callAsFunction: asr [dim_in][T], f0 [2 T], n [2 T], s [style_dim], noise as above for
 *     L = 2 T (nullable) -> pcm [600 T].
 * Out of scope: ALBERT, TextEncoder, DurationEncoder, the BiLSTMs and the alignment; voice packs; stacked utterances; 16-bit weights. */
typedef struct mia_kokoro_config mia_kokoro_config;    /* defined in include/mia_kokoro.h */
typedef struct mia_kokoro mia_kokoro;
mia_kokoro* mia_kokoro_load(mia_ctx* ctx, const mia_kokoro_config* cfg, const mia_tensor_view* tensors, int n_tensors);
void mia_kokoro_free(mia_kokoro* h);
int64_t mia_kokoro_output_len(const mia_kokoro* h, int64_t T);
int mia_kokoro_f0n(mia_kokoro* h, const float* x, int T, const float* s_pred, float* f0, float* n, int data_mem);
int mia_kokoro_source(mia_kokoro* h, const float* f0, int L, const float* noise, float* source, float* har, int data_mem);
int mia_kokoro_generate(mia_kokoro* h, const float* x, int L, const float* s, const float* har, float* pcm, int data_mem);
int mia_kokoro_decode(mia_kokoro* h, const float* asr, int T, const float* f0, const float* n, const float* s, const float* noise,
                      float* pcm, int data_mem);
/* Operator-level hook: per-channel mean and 1 / sqrt(var + 1e-5) over the T rows of a row-major x [T][ld] (population variance, as
 * MLX.variance gives; T = 1: variance 0).  Deterministic.  Device pointers; mean and rstd are [C]. */
int mia_op_instance_norm(mia_ctx* ctx, const float* x, int64_t ld, int64_t T, int C, float* mean, float* rstd);

#ifdef __cplusplus
}
#endif
#endif /* MIA_H */
