// decode.h -- internal interface between whisper_decode.hip (host loop) and the Whisper step's kernels (decode_kernels.hip, skinny_frag.hip).
#pragma once
#include "skinny.h"
#include "whisper.h"

int dec_launch_embed_ln(mia_whisper* w, const LNW& ln, hipStream_t s);
int dec_launch_reduce_ln(mia_whisper* w, int S, const float* bias, const LNW& ln, hipStream_t s);
// Whisper step: a.A in activation fragment order, a.W in weight fragment order (LinearW::wf)
int dec_launch_skinny(mia_whisper* w, const SkinnyArgs& a, int mode, hipStream_t s);
// the same on packed 4- / 8-bit weights (skinny_frag_quant.hip; LinearW::qw / qst): a.W is ignored, K % (128 S) == 0, modes SK_QKV /
// SK_OUT16 / SK_PARTIAL / SK_OUTF32, no carried LayerNorm (a.ss_in / a.c1 must be null)
int dec_launch_skinny_q(mia_whisper* w, const SkinnyArgs& a, const uint32_t* wfrag, const float* stfrag, int bits, int mode, hipStream_t s);
// c1[n] = sum_k W[n][k] gamma[k], c2[n] = sum_k W[n][k] beta[k] for a row-major 16-bit [N][K] matrix (fp32 sums in k order)
int dec_launch_lnfold(const void* w16, int N, int K, const float* gamma, const float* beta, float* c1, float* c2, int dtype, hipStream_t s, const float* bias = nullptr);
// qk_out (optional): pre-softmax scores of the heads with head_slot[h] >= 0 -> qk_out[b][slot][pos[b]][key] (word-timestamp alignment)
int dec_launch_attention(mia_whisper* w, const void* q, const void* kc, const void* vc, void* out, int fixed_keys, int cap_keys,
                         hipStream_t s, float* qk_out = nullptr, const int32_t* head_slot = nullptr, int n_slots = 0, int qk_ctx = 0,
                         bool self_nt = false);     // self attention (fixed_keys == 0): load the cached K/V non-temporal (cross K/V always are)
bool dec_head_is_split(const DecodeParams& p);
// test hook: logits of the traced clips -> w->trace[slot][pos[clip]][0:V]
int dec_launch_trace(mia_whisper* w, hipStream_t s);
int dec_launch_head(mia_whisper* w, int32_t* last_ts, const DecodeParams& p, hipStream_t s);
int dec_launch_finalize(mia_whisper* w, int32_t* out_n, const DecodeParams& p, hipStream_t s);
