// codec_encode.hip -- DAC encoder + residual vector quantisation (Codec/DAC/DACModel.swift:13-86,284-296; DACQuantize.swift:54-116,147-190)
// over the encoder program built by mia_dac_load_encoder (codec_load.hip).
#include "codec_model.h"

// code steps of the encoder program for T0 (hop-padded) samples; max_floats: its widest activation, T * C
static int64_t encoder_steps(const mia_codec* c, int64_t T0, size_t* max_floats = nullptr) {
  int64_t T = T0; size_t mf = (size_t)T0 * c->enc_dim;
  for (const Op& op : c->enc_ops) {
    if (op.residual || op.side) continue;
    if (op.stride > 1) T = strided_rows(op, T);
    mf = std::max(mf, (size_t)T * op.N);
  }
  if (max_floats) *max_floats = mf;
  return T;
}

// preprocess: right-pad to the hop length (DACModel.swift:308-317)
static int64_t hop_padded(const mia_codec* c, int64_t n_samples) { return (n_samples + c->hop - 1) / c->hop * c->hop; }

extern "C" int64_t mia_dac_code_len(mia_codec* c, int64_t n_samples) {
  if (!c || !c->has_encoder || n_samples <= 0) return 0;
  return encoder_steps(c, hop_padded(c, n_samples));
}

extern "C" int mia_dac_encode(mia_codec* c, const float* pcm, int64_t n_samples, int n_quantizers, int32_t* codes, int64_t codes_capacity,
                              int64_t* n_steps, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 1 && c->has_encoder, "dac_encode: no encoder loaded (mia_dac_load_encoder)");
  MIA_CHECK_ARG(ctx, pcm && codes && n_samples > 0, "dac_encode: null pointer or empty audio");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "dac_encode: bad mem");
  HostIo io(ctx, mem);
  const int nq = n_quantizers <= 0 ? c->n_levels : std::min(n_quantizers, c->n_levels);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const int64_t T0 = hop_padded(c, n_samples);
  size_t max_floats;
  const int64_t Tc = encoder_steps(c, T0, &max_floats);
  MIA_CHECK_ARG(ctx, Tc > 0 && codes_capacity >= Tc, "dac_encode: codes buffer too small (%lld < %lld steps)", (long long)codes_capacity, (long long)Tc);
  MIA_CHECK_ARG(ctx, T0 < (1ll << 30), "dac_encode: audio too long for one call");
  int rc = codec_scratch(c, max_floats);
  if (rc != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, c->d_audio, c->audio_cap, (size_t)T0, "codec: hipMalloc failed")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, c->d_ze, c->ze_cap, (size_t)Tc * (size_t)std::max(c->cb_dim, 1), "codec: hipMalloc failed")) != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, c->d_codes, c->codes_cap, (size_t)nq * Tc, "codec: hipMalloc failed")) != MIA_OK) return rc;
  MIA_HIP(ctx, hipMemsetAsync(c->d_audio, 0, (size_t)T0 * 4, s));
  io.check(hipMemcpyAsync(c->d_audio, pcm, (size_t)n_samples * 4, io.from_caller(), s));
  float* x = c->buf[0]; float* h = c->buf[1]; float* y = c->buf[2];
  int64_t T = T0;
  if (codec_conv_in1_launch(c->d_audio, x, c->enc_in_w, c->enc_in_b, T, c->enc_dim, 7, 3, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "dac_encode: input conv launch failed");
  for (const Op& op : c->enc_ops) {
    const ConvGemmArgs g = codec_conv_args(op, x, h, y, T);
    if ((rc = codec_conv_gemm_run(ctx, g, 1, "dac_encode")) != MIA_OK) return rc;
    if (!op.residual && !op.side) { std::swap(x, y); T = g.T_out; }
  }
  // residual vector quantisation: x holds z [Tc][latent] and becomes the residual
  for (int i = 0; i < nq; ++i) {
    const ConvGemmArgs g = codec_conv_args(c->in_proj[i], x, h, c->d_ze, T);
    if ((rc = codec_conv_gemm_run(ctx, g, 1, "dac_encode")) != MIA_OK) return rc;
    if (codec_vq_assign_launch(c->d_ze, c->cbn[i], c->cbn_sq[i], c->codebook[i], c->weff[i], c->ebias[i], x, c->d_codes + (size_t)i * T, (int)T, c->latent,
                               c->cb_size, c->cb_dim, s)) return mia_fail(ctx, MIA_ERR_DEVICE, "dac_encode: vq launch failed");
  }
  if (n_steps) *n_steps = T;
  // codes [nq][T] -> caller's [nq][codes_capacity] rows
  io.check(hipMemcpy2DAsync(codes, (size_t)codes_capacity * 4, c->d_codes, (size_t)T * 4, (size_t)T * 4, nq, io.to_caller(), s));
  return io.finish();
}
