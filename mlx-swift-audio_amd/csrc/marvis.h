// marvis.h -- what marvis.hip (handle, frame graph, entry points) and marvis_kernels.hip (the frame's own kernels) share.
#pragma once
#include "lm.h"

// device record of the sequence: frames emitted by this call, the all-zero frame seen, the next uniform of this call
struct MvState { int n_frames; int finished; int u_cursor; int pad; };

constexpr int MV_MAX_VOCAB = 8192;       // the sampler sorts the whole row in one workgroup's LDS
constexpr int MV_MAX_CODEBOOKS = 32;

// row r of (ids, mask) [T][K+1] -> the fp32 embedding row of sequence rowmap[r].x at position rowmap[r].y, out[(seq * max_ctx + pos)][D]:
//   sum_{c<K} mask[c] * audio_emb[c * V + id[c]] + mask[K] * text_emb[id[K]], columns in that order; ids are clamped into their tables.
// bb_state[seq].n_embeds grows to cover the position
void mv_launch_embed_rows(hipStream_t s, int dtype, const int32_t* ids, const int32_t* mask, const int2* rowmap, int T, int K, int V, int text_vocab,
                          const void* audio_emb, const void* text_emb, float* out, int max_ctx, int D, LmState* bb_state);

struct MvSampleArgs {
  // workgroup b = sequence b: logits + b * ld_logits, uniforms + b * ld_uniforms, st + b, out / forced + b * ld_ids, emb_out + b * D
  int64_t ld_logits, ld_uniforms; int ld_ids;
  const float* logits; int V; float temperature, top_p;
  const float* uniforms; int n_uniforms;   // the draw reads uniforms[st->u_cursor] (clamped into the buffer) and advances the cursor
  MvState* st;                        // null: the standalone op (one uniform at uniforms[0], nothing skipped)
  int32_t* out;                       // the id (after forcing)
  const int32_t* forced;              // null or the id that replaces the draw
  int32_t* kept_ids; int32_t* n_kept; // null in the frame
  const uint16_t* emb; uint16_t* emb_out; int D;   // null or: this codebook's embedding table [V][D]; the picked row is copied to emb_out [D]
};
// one workgroup per sequence; V <= MV_MAX_VOCAB
void mv_launch_sample(hipStream_t s, const MvSampleArgs& a, int B);
// once per process before the first launch (raises the kernel's dynamic LDS limit); -1 on failure
int mv_sampler_init();

struct MvFrameEndArgs {
  MvState* st; LmState* bb_state; LmState* dec_state;
  const int32_t* frame; int ld_ids; int cb; int32_t* frames_out; int frames_cap;      // frame + b * ld_ids; frames_out + b * frames_cap * ld_ids
  const void* audio_emb; int V; int D; float* embeds; int max_ctx;                    // embeds + b * max_ctx * D
};
// end of a frame, one workgroup per sequence: decoder position back to 0; all-zero frame -> finished, and both stacks' states frozen
// (lm.h: the sequence's further steps are no-ops); otherwise the frame joins the record and its embedding sum
// becomes the backbone's next input row (position bb_state->pos, already advanced)
void mv_launch_frame_end(hipStream_t s, int dtype, const MvFrameEndArgs& a, int B);
