// codec_batch.hip -- stacked decode: n_utt utterances in one pass of the SNAC / DAC program (mia_snac_decode_batch, mia_dac_decode_batch).
// The layout of the stacked buffers and tables is described at Stack (codec_model.h).
#include <numeric>

#include "codec_model.h"

namespace {

struct BatchUtt { int64_t T0 = 0; Geometry g; int64_t code_off[MIA_MAX_LEVELS] = {-1, -1, -1, -1}; };

// the call's tables in the handle's pinned staging, uploaded once: [pcm_off U | code_off U x MIA_MAX_LEVELS] int64, then
// [len stages x U | noise_off blocks x U] int32.  st gets the device addresses; code_off follows st.pcm_off, and the staging (c->h_tab) still
// starts with the host copy of pcm_off afterwards.
int upload_tables(mia_codec* c, const std::vector<BatchUtt>& ut, const Geometry& gmax, const int64_t* pcm_off, bool dev, Stack& st) {
  mia_ctx* ctx = c->ctx;
  hipStream_t s = ctx->stream;
  const int U = (int)ut.size();
  const size_t n_stages = gmax.n_stages, n_blocks = gmax.n_blocks;
  const size_t n64 = (size_t)U * (1 + MIA_MAX_LEVELS), n32 = (size_t)U * (n_stages + n_blocks), bytes = n64 * 8 + n32 * 4;
  if (!c->tab_ev) MIA_HIP(ctx, hipEventCreateWithFlags(&c->tab_ev, hipEventDisableTiming));
  else MIA_HIP(ctx, hipEventSynchronize(c->tab_ev));       // the previous call's upload has left the staging
  if (bytes > c->tab_cap) {
    MIA_HIP(ctx, hipStreamSynchronize(s));
    if (c->d_tab) (void)hipFree(c->d_tab);
    if (c->h_tab) (void)hipHostFree(c->h_tab);
    c->d_tab = c->h_tab = nullptr; c->tab_cap = 0;
    MIA_HIP(ctx, hipHostMalloc(&c->h_tab, bytes, hipHostMallocDefault));
    MIA_HIP(ctx, hipMalloc(&c->d_tab, bytes));
    c->tab_cap = bytes;
  }
  int64_t* h64 = (int64_t*)c->h_tab; int32_t* h32 = (int32_t*)(h64 + n64);
  int64_t po = 0, zo = 0;
  for (int u = 0; u < U; ++u) {
    const Geometry& g = ut[u].g;
    h64[u] = dev ? pcm_off[u] : po;                        // host: packed in d_pcm, copied out per utterance by the caller
    for (int l = 0; l < MIA_MAX_LEVELS; ++l) h64[U + (size_t)u * MIA_MAX_LEVELS + l] = ut[u].code_off[l];
    for (size_t k = 0; k < n_stages; ++k) h32[k * U + u] = (int32_t)g.rows[k];
    for (size_t k = 0; k < n_blocks; ++k) h32[(n_stages + k) * U + u] = (int32_t)(zo + g.noise_off[k]);
    po += g.T_final; zo += g.noise_total;
  }
  MIA_HIP(ctx, hipMemcpyAsync(c->d_tab, c->h_tab, bytes, hipMemcpyHostToDevice, s));
  MIA_HIP(ctx, hipEventRecord(c->tab_ev, s));
  st.pcm_off = (const int64_t*)c->d_tab;
  st.len = (const int32_t*)((const int64_t*)c->d_tab + n64);
  st.noise_off = st.len + n_stages * U;
  return MIA_OK;
}

// shared tail of the two batch entries: every argument has been checked, nothing has touched the GPU yet.  Host memory: the caller's
// codes / noise / pcm are behind asynchronous copies, and io keeps every return path, the failing ones included, from leaving one pending
// (the tables' staging belongs to the handle and needs no such care).
int decode_batch_common(mia_codec* c, std::vector<BatchUtt>& ut, const int strides[MIA_MAX_LEVELS], int n_levels, const int32_t* codes, size_t n_codes_total,
                       const float* noise, float* pcm, const int64_t* pcm_off, int64_t* n_samples, HostIo& io) {
  mia_ctx* ctx = c->ctx;
  const int U = (int)ut.size();
  const bool dev = !io.host();
  int64_t pcm_total = 0, noise_total = 0;
  const BatchUtt* longest = &ut[0];
  for (const BatchUtt& b : ut) { if (b.T0 > longest->T0) longest = &b; pcm_total += b.g.T_final; noise_total += b.g.noise_total; }
  if (noise_total == 0) noise = nullptr;
  const int64_t Tmax = longest->T0;
  const Geometry& gmax = longest->g;
  // floats per utterance per buffer: the largest stage of the longest utterance, rounded up to a whole number of rows at every stage
  int64_t row_lcm = c->latent;
  for (const Op& op : c->ops) if (op.kind == OP_CONVT || (op.kind == OP_CONV && !op.residual)) row_lcm = std::lcm<int64_t>(row_lcm, op.N);
  const int64_t slab = ((int64_t)gmax.max_floats + row_lcm - 1) / row_lcm * row_lcm;
  MIA_HIP(ctx, hipSetDevice(ctx->device));
  int rc = codec_scratch(c, (size_t)slab * (size_t)U);     // three buffers of n_utt x (largest stage of the longest utterance)
  if (rc != MIA_OK) return rc;
  if (!dev) {
    if ((rc = mia_grow(ctx, c->d_pcm, c->pcm_cap, (size_t)pcm_total, "codec: hipMalloc failed")) != MIA_OK) return rc;
    if ((rc = mia_grow(ctx, c->d_codes, c->codes_cap, n_codes_total, "codec: hipMalloc failed")) != MIA_OK) return rc;
    if (noise && (rc = mia_grow(ctx, c->d_noise, c->noise_cap, (size_t)noise_total, "codec: hipMalloc failed")) != MIA_OK) return rc;
  }
  Stack st; st.U = U; st.slab = slab;
  if ((rc = upload_tables(c, ut, gmax, pcm_off, dev, st)) != MIA_OK) return rc;
  const int64_t* h_pcm_off = (const int64_t*)c->h_tab;
  const int32_t* d_codes = io.in(codes, c->d_codes, n_codes_total * 4);
  const float* d_noise = io.in(noise, c->d_noise, (size_t)noise_total * 4);
  EmbedArgs ea = codec_embed_args(c, n_levels, strides);
  ea.codes_base = d_codes; ea.seq_code_off = st.pcm_off + U;
  SeqArgs q0; q0.n = U; q0.len = st.len; q0.step = slab / c->latent;
  if (codec_embed_launch(ea, c->buf[0], (int)Tmax, c->latent, ctx->stream, q0)) return mia_fail(ctx, MIA_ERR_DEVICE, "codec: embed launch failed");
  // Stages run stacked while all the utterances' activations there (three buffers) fit the budget.  SNAC: 256 MiB, the Infinity Cache.
  // Its early stages have too few rows per utterance to fill the CUs, and stacking fills them; from the first stage that does not fit,
  // every utterance runs the rest of the program on its own slab, one after the other, with the single call's launches.  A late
  // stage of ONE utterance fills the chip, and its depthwise + 1x1 layers are memory-bound and hand their activations over through
  // the cache, which a pass over all utterances per layer streams from HBM instead: every stage stacked measured 3-4 % SLOWER than
  // the loop of single calls at 8 and 32 chunks of 171 frames, this split 2 % faster.  DAC's dense 7-tap convolutions are
  // compute-bound and gain from the larger grids at every stage (8 x 750 steps: 10 % faster with every stage stacked, 1 % with the
  // split), so its default is no limit.  LABNOTES, "stacked codec decode".  Stage 0 is always stacked.
  size_t split = c->ops.size();
  { int stage = 0;
    for (size_t i = 0; i < c->ops.size(); ++i) {
      const Op& op = c->ops[i];
      if (op.kind != OP_CONVT) continue;
      if ((double)U * 3.0 * (double)gmax.rows[++stage] * op.N * 4.0 > (double)c->stack_budget) { split = i; break; }
    } }
  float* dst = dev ? pcm : c->d_pcm;
  Cursor k{c->buf[0], c->buf[1], c->buf[2], Tmax, c->latent};
  if ((rc = codec_run(c, k, 0, split, d_noise, dst, st)) != MIA_OK) return rc;
  if (split < c->ops.size()) {
    int64_t zo_u = 0;
    for (int u = 0; u < U; ++u) {
      const Geometry& g = ut[u].g;
      Cursor ku{k.x + (int64_t)u * slab, k.h + (int64_t)u * slab, k.y + (int64_t)u * slab, g.rows[k.stage], k.C};
      ku.noff = zo_u + (k.nblock < g.n_blocks ? g.noise_off[k.nblock] : 0); ku.stage = k.stage; ku.nblock = k.nblock;
      if ((rc = codec_run(c, ku, split, c->ops.size(), d_noise, dst + h_pcm_off[u])) != MIA_OK) return rc;
      zo_u += g.noise_total;
    }
  }
  if (n_samples) for (int u = 0; u < U; ++u) n_samples[u] = ut[u].g.T_final;
  int64_t po = 0;
  for (int u = 0; u < U && !dev; ++u) {                    // host: each utterance from the packed d_pcm to its place
    io.out(pcm + pcm_off[u], c->d_pcm + po, (size_t)ut[u].g.T_final * 4);
    po += ut[u].g.T_final;
  }
  return io.finish();
}

// the geometry of every utterance (one program walk each), and the checks both entries share; `what` prefixes the messages
int batch_lengths(mia_codec* c, std::vector<BatchUtt>& ut, const float* noise, int64_t n_noise, const int64_t* pcm_off, const char* what) {
  mia_ctx* ctx = c->ctx;
  int64_t noise_total = 0;
  MIA_CHECK_ARG(ctx, pcm_off[0] >= 0, "%s: pcm_off[0] is negative", what);
  for (size_t u = 0; u < ut.size(); ++u) {
    ut[u].g = codec_geometry(c, ut[u].T0);
    noise_total += ut[u].g.noise_total;
    MIA_CHECK_ARG(ctx, pcm_off[u + 1] - pcm_off[u] >= ut[u].g.T_final, "%s: pcm room of utterance %d too small (%lld < %lld)", what, (int)u,
                  (long long)(pcm_off[u + 1] - pcm_off[u]), (long long)ut[u].g.T_final);
  }
  MIA_CHECK_ARG(ctx, noise_total < (1ll << 31), "%s: too many noise values for one call", what);
  if (noise && noise_total > 0)
    MIA_CHECK_ARG(ctx, n_noise == noise_total, "%s: noise must hold %lld values, the sum over the utterances (got %lld)", what, (long long)noise_total, (long long)n_noise);
  return MIA_OK;
}

}  // namespace

extern "C" int mia_snac_decode_batch(mia_codec* c, int n_utt, const int32_t* codes, const int32_t* n_codes, int n_levels, const float* noise,
                                     int64_t n_noise, float* pcm, const int64_t* pcm_off, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 0, "snac_decode_batch: handle is not a SNAC model");
  MIA_CHECK_ARG(ctx, n_utt >= 1 && n_utt <= 64, "snac_decode_batch: n_utt must be 1..64 (got %d)", n_utt);
  MIA_CHECK_ARG(ctx, codes && n_codes && pcm && pcm_off && n_levels > 0, "snac_decode_batch: null arguments");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "snac_decode_batch: bad mem");
  HostIo io(ctx, mem);
  std::vector<BatchUtt> ut(n_utt);
  size_t off = 0;
  for (int u = 0; u < n_utt; ++u) {
    const int32_t* n = n_codes + (size_t)u * n_levels;
    // expanded length = max_i n_i * stride_i; a level whose expansion differs is skipped for this utterance, as embedCodes does
    for (int i = 0; i < c->n_levels && i < n_levels; ++i) if (n[i] > 0) ut[u].T0 = std::max<int64_t>(ut[u].T0, (int64_t)n[i] * c->vq_stride[i]);
    MIA_CHECK_ARG(ctx, ut[u].T0 > 0, "snac_decode_batch: utterance %d has no codes", u);
    for (int i = 0; i < n_levels; ++i) {
      if (n[i] <= 0) continue;
      if (i < c->n_levels && (int64_t)n[i] * c->vq_stride[i] == ut[u].T0) {
        for (int k = 0; k < n[i] && io.host(); ++k)
          MIA_CHECK_ARG(ctx, codes[off + k] >= 0 && codes[off + k] < c->cb_size, "snac_decode_batch: code %d out of range at level %d of utterance %d", codes[off + k], i, u);
        ut[u].code_off[i] = (int64_t)off;
      }
      off += n[i];
    }
  }
  if (int rc = batch_lengths(c, ut, noise, n_noise, pcm_off, "snac_decode_batch")) return rc;
  return decode_batch_common(c, ut, c->vq_stride, c->n_levels, codes, off, noise, pcm, pcm_off, n_samples, io);
}

extern "C" int mia_dac_decode_batch(mia_codec* c, int n_utt, const int32_t* codes, int n_codebooks, const int64_t* T, float* pcm,
                                    const int64_t* pcm_off, int64_t* n_samples, int mem) {
  if (!c) return MIA_ERR_MODEL_NOT_LOADED;
  mia_ctx* ctx = c->ctx;
  MIA_CHECK_ARG(ctx, c->kind == 1, "dac_decode_batch: handle is not a DAC model");
  MIA_CHECK_ARG(ctx, n_utt >= 1 && n_utt <= 64, "dac_decode_batch: n_utt must be 1..64 (got %d)", n_utt);
  MIA_CHECK_ARG(ctx, codes && T && pcm && pcm_off && n_codebooks > 0 && n_codebooks <= c->n_levels, "dac_decode_batch: bad arguments");
  MIA_CHECK_ARG(ctx, HostIo::valid(mem), "dac_decode_batch: bad mem");
  HostIo io(ctx, mem);
  std::vector<BatchUtt> ut(n_utt);
  size_t off = 0;
  for (int u = 0; u < n_utt; ++u) {
    MIA_CHECK_ARG(ctx, T[u] > 0 && T[u] < (1ll << 30), "dac_decode_batch: utterance %d has no codes (T = %lld)", u, (long long)T[u]);
    ut[u].T0 = T[u];
    for (int i = 0; i < n_codebooks; ++i) ut[u].code_off[i] = (int64_t)(off + (size_t)i * T[u]);
    const size_t n = (size_t)n_codebooks * T[u];
    for (size_t k = 0; k < n && io.host(); ++k)
      MIA_CHECK_ARG(ctx, codes[off + k] >= 0 && codes[off + k] < c->cb_size, "dac_decode_batch: code %d out of range in utterance %d", codes[off + k], u);
    off += n;
  }
  if (int rc = batch_lengths(c, ut, nullptr, 0, pcm_off, "dac_decode_batch")) return rc;
  const int ones[MIA_MAX_LEVELS] = {1, 1, 1, 1};
  return decode_batch_common(c, ut, ones, n_codebooks, codes, off, nullptr, pcm, pcm_off, n_samples, io);
}
