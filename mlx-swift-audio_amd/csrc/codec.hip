// codec.hip -- SNAC and DAC neural-codec decoders as layer programs over the fp32 kernels of codec_kernels.hip: the executor and the
// single-utterance entries.  (Programs are built in codec_load.hip; stacked decode: codec_batch.hip; DAC encoder: codec_encode.hip.)
//
// Replaces SNACDecoder.decode(codes:) (TTS/Orpheus/SNAC/SNACDecoder.swift:250-289,328-407 with WNConv1d.swift:64-88,
// ConvWeightedTranspose1d.swift:70-100, ResidualUnit.swift:58-95, NoiseBlock.swift:27-41) and
// DACCodec.decodeFromCodes (Codec/DAC/DACModel.swift:303-306 -> DACQuantize.swift:192-220 -> DACModel.swift:120-164,
// DACLayers.swift).  Weight normalisation g*v/(||v||+1e-12) is folded ONCE at load (the reference recomputes it on every
// forward, WNConv1d.swift:73-74).  The Gaussian of SNAC's NoiseBlock is an explicit input (null = no noise).
#include "codec_model.h"

// run ops [begin, end) of the program from cursor k (op 0: k.x holds the latent [T0][latent]); the output conv writes T_final samples to
// d_pcm.  Stacked: k.T = the longest utterance's rows.
int codec_run(mia_codec* c, Cursor& k, size_t begin, size_t end, const float* d_noise, float* d_pcm, const Stack& st) {
  mia_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  float*& x = k.x; float*& h = k.h; float*& y = k.y;
  int64_t& T = k.T; int& C = k.C; int64_t& noff = k.noff;
  int& stage = k.stage; int& nblock = k.nblock;
  auto seq = [&]() { SeqArgs q; if (st.U) { q.n = st.U; q.len = st.len + (size_t)stage * st.U; q.step = st.slab / C; } return q; };
  auto seq_gemm = [&](ConvGemmArgs& g) {
    if (!st.U) return;
    g.n_seq = st.U; g.x_seq_step = st.slab / g.ldx; g.y_seq_step = st.slab / g.ldy; g.seq_len = st.len + (size_t)stage * st.U;
  };
  for (size_t oi = begin; oi < end; ++oi) {
    const Op& op = c->ops[oi];
    switch (op.kind) {
      case OP_DW:
        if (codec_dwconv_launch(x, h, op.w, op.b, op.a_pre, op.a_post, (int)T, C, op.taps, op.dil, s, seq())) return mia_fail(ctx, MIA_ERR_DEVICE, "codec: dwconv launch failed");
        if (!op.residual) std::swap(x, h);     // plain depthwise layer: its output becomes the stream
        break;
      case OP_CONV: {
        ConvGemmArgs g = codec_conv_args(op, x, h, y, T);
        seq_gemm(g);
        if (int rc = codec_conv_gemm_run(ctx, g, 1, "codec")) return rc;
        if (!op.residual && !op.side) { std::swap(x, y); C = op.N; }
        break;
      }
      case OP_CONVT: {
        const int64_t T_out = convt_rows(op, T);
        ConvGemmArgs g;
        g.X = x; g.ldx = op.Cin; g.T_in = (int)T; g.W = op.w; g.w_phase_stride = (int64_t)op.N * 2 * op.Cin; g.bias = op.b; g.alpha = op.a_pre;
        g.M = (int)T + 1; g.N = op.N; g.Cin = op.Cin; g.taps = 2; g.dil = 1; g.pad = 1;
        g.Y = y; g.ldy = op.N; g.T_out = (int)T_out; g.y_row_mul = op.stride; g.y_row_off = -op.pad; g.y_phase_step = 1;
        seq_gemm(g);
        if (int rc = codec_conv_gemm_run(ctx, g, op.stride, "codec")) return rc;
        std::swap(x, y); C = op.N; T = T_out; ++stage;
        break;
      }
      case OP_NOISE1:
        if (d_noise) {
          SeqArgs q = seq();
          if (st.U) q.noise_off = st.noise_off + (size_t)nblock * st.U;
          if (codec_noise1_launch(x, op.w, st.U ? d_noise : d_noise + noff, (int)T, C, s, q)) return mia_fail(ctx, MIA_ERR_DEVICE, "codec: noise launch failed");
        }
        noff += T; ++nblock;
        break;
      case OP_NOISEC:
        if (d_noise) {
          ConvGemmArgs g;
          g.X = x; g.ldx = C; g.T_in = (int)T; g.W = op.w; g.M = (int)T; g.N = C; g.Cin = C; g.T_out = (int)T;
          g.R = x; g.ldr = C; g.noise = st.U ? d_noise : d_noise + noff; g.Y = y; g.ldy = C;
          seq_gemm(g);
          if (st.U) g.noise_seq_off = st.noise_off + (size_t)nblock * st.U;
          if (int rc = codec_conv_gemm_run(ctx, g, 1, "codec")) return rc;
          std::swap(x, y);
        }
        noff += T; ++nblock;
        break;
      case OP_OUT1: {
        SeqArgs q = seq();
        q.out_off = st.pcm_off;
        if (codec_conv_out1_launch(x, d_pcm, op.w, op.b, op.a_pre, (int)T, C, op.taps, s, q)) return mia_fail(ctx, MIA_ERR_DEVICE, "codec: output conv launch failed");
        break;
      }
    }
  }
  return MIA_OK;
}

// shared tail: codes already on the device, latent length T0 with geometry gm
static int decode_common(mia_codec* c, const EmbedArgs& ea, int64_t T0, const Geometry& gm, const float* noise, int64_t n_noise_given, float* pcm, int64_t* n_out, HostIo& io) {
  mia_ctx* ctx = c->ctx;
  int rc = codec_scratch(c, gm.max_floats);
  if (rc != MIA_OK) return rc;
  if ((rc = mia_grow(ctx, c->d_pcm, c->pcm_cap, (size_t)gm.T_final, "codec: hipMalloc failed")) != MIA_OK) return rc;
  const float* d_noise = nullptr;
  if (noise && gm.noise_total > 0) {
    MIA_CHECK_ARG(ctx, n_noise_given == gm.noise_total, "codec: noise must hold %lld values (got %lld)", (long long)gm.noise_total, (long long)n_noise_given);
    if (io.host() && (rc = mia_grow(ctx, c->d_noise, c->noise_cap, (size_t)gm.noise_total, "codec: hipMalloc failed")) != MIA_OK) return rc;
    d_noise = io.in(noise, c->d_noise, (size_t)gm.noise_total * 4);
  }
  if (codec_embed_launch(ea, c->buf[0], (int)T0, c->latent, ctx->stream)) return mia_fail(ctx, MIA_ERR_DEVICE, "codec: embed launch failed");
  float* dst = io.out(pcm, c->d_pcm, (size_t)gm.T_final * 4);
  Cursor k{c->buf[0], c->buf[1], c->buf[2], T0, c->latent};
  rc = codec_run(c, k, 0, c->ops.size(), d_noise, dst);
  if (rc != MIA_OK) return rc;
  if (n_out) *n_out = gm.T_final;
  return io.finish();
}

extern "C" int mia_codec_set_stack_budget(mia_codec* c, int64_t bytes) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  c->stack_budget = bytes < 0 ? c->stack_budget_default : bytes;
  return MIA_OK;
}

extern "C" int64_t mia_codec_noise_len(mia_codec* c, int64_t latent_len) {
  return !c || latent_len <= 0 ? 0 : codec_geometry(c, latent_len).noise_total;
}

extern "C" int64_t mia_codec_output_len(mia_codec* c, int64_t latent_len) {
  return !c || latent_len <= 0 ? 0 : codec_geometry(c, latent_len).T_final;
}

extern "C" int mia_snac_decode(mia_codec* c, const int32_t* const* codes, const int32_t* n_codes, int n_levels, const float* noise,
                               int64_t n_noise, float* pcm, int64_t pcm_capacity, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 0, "snac_decode: handle is not a SNAC model");
  MIA_CHECK_ARG(ctx, codes && n_codes && pcm && n_levels > 0, "snac_decode: null arguments");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "snac_decode: bad mem");
  HostIo io(ctx, mem);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  // expanded length = max_i n_i * stride_i; a level whose expansion differs is skipped, as embedCodes does (SNACDecoder.swift:337-402)
  int64_t T0 = 0; size_t total = 0;
  for (int i = 0; i < c->n_levels && i < n_levels; ++i) if (n_codes[i] > 0) { T0 = std::max<int64_t>(T0, (int64_t)n_codes[i] * c->vq_stride[i]); total += n_codes[i]; }
  MIA_CHECK_ARG(ctx, T0 > 0, "snac_decode: no codes");
  int rc = mia_grow(ctx, c->d_codes, c->codes_cap, total, "codec: hipMalloc failed");
  if (rc != MIA_OK) return rc;
  EmbedArgs ea = codec_embed_args(c, c->n_levels, c->vq_stride);
  size_t off = 0;
  for (int i = 0; i < c->n_levels; ++i) {
    if (i >= n_levels || n_codes[i] <= 0 || (int64_t)n_codes[i] * c->vq_stride[i] != T0) continue;
    for (int k = 0; k < n_codes[i] && io.host(); ++k)
      if (codes[i][k] < 0 || codes[i][k] >= c->cb_size) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "snac_decode: code %d out of range at level %d", codes[i][k], i);
    io.check(hipMemcpyAsync(c->d_codes + off, codes[i], (size_t)n_codes[i] * 4, io.from_caller(), ctx->stream));
    ea.codes[i] = c->d_codes + off; off += n_codes[i];
  }
  const Geometry gm = codec_geometry(c, T0);
  MIA_CHECK_ARG(ctx, pcm_capacity >= gm.T_final, "snac_decode: pcm buffer too small (%lld < %lld)", (long long)pcm_capacity, (long long)gm.T_final);
  return decode_common(c, ea, T0, gm, noise, n_noise, pcm, n_samples, io);
}

extern "C" int mia_dac_decode(mia_codec* c, const int32_t* codes, int n_codebooks, int64_t T, float* pcm, int64_t pcm_capacity, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 1, "dac_decode: handle is not a DAC model");
  MIA_CHECK_ARG(ctx, codes && pcm && T > 0 && n_codebooks > 0 && n_codebooks <= c->n_levels, "dac_decode: bad arguments");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "dac_decode: bad mem");
  HostIo io(ctx, mem);
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = mia_grow(ctx, c->d_codes, c->codes_cap, (size_t)n_codebooks * T, "codec: hipMalloc failed");
  if (rc != MIA_OK) return rc;
  if (io.host())
    for (int64_t k = 0; k < (int64_t)n_codebooks * T; ++k)
      if (codes[k] < 0 || codes[k] >= c->cb_size) return mia_fail(ctx, MIA_ERR_INVALID_ARGUMENT, "dac_decode: code %d out of range", codes[k]);
  io.check(hipMemcpyAsync(c->d_codes, codes, (size_t)n_codebooks * T * 4, io.from_caller(), ctx->stream));
  const int ones[MIA_MAX_LEVELS] = {1, 1, 1, 1};
  EmbedArgs ea = codec_embed_args(c, n_codebooks, ones);
  for (int i = 0; i < n_codebooks; ++i) ea.codes[i] = c->d_codes + (size_t)i * T;
  const Geometry gm = codec_geometry(c, T);
  MIA_CHECK_ARG(ctx, pcm_capacity >= gm.T_final, "dac_decode: pcm buffer too small");
  return decode_common(c, ea, T, gm, nullptr, 0, pcm, n_samples, io);
}
