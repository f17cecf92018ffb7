/* mia_marvis.h -- the configuration record of mia_marvis_load (include/mia.h, "Marvis TTS"): MarvisConfig and the two
 * MarvisBackboneConfig records of TTS/Marvis/Models/MarvisModel.swift:305-361 (backbone = bb_*, depth decoder = dec_*) as flat scalars.
 * The rope_* fields are Llama3ScaledRoPE's (MarvisLlamaBackbone.swift:31-39) and apply to both stacks; rope_llama3 = 0 leaves the
 * frequencies unscaled.  attention_bias / mlp_bias must be 0 (MIA_ERR_UNSUPPORTED otherwise).  max_ctx is the backbone's cache length
 * (the reference's 2048).  mia.h declares the type; a caller that fills one includes this file as well.  The ctypes mirror is
 * _abi.MarvisConfig (tests/test_marvis_abi.py compares the two field for field). */
#ifndef MIA_MARVIS_H
#define MIA_MARVIS_H
#include "mia.h"

struct mia_marvis_config {
  int32_t text_vocab, audio_vocab, n_codebooks, max_ctx;
  int32_t bb_hidden, bb_inter, bb_layers, bb_heads, bb_kv_heads, bb_head_dim;
  int32_t dec_hidden, dec_inter, dec_layers, dec_heads, dec_kv_heads, dec_head_dim;
  float bb_rms_eps, dec_rms_eps, bb_rope_theta, dec_rope_theta;
  int32_t rope_llama3;
  float rope_factor, rope_low, rope_high, rope_old_ctx;
  int32_t attention_bias, mlp_bias;
};

#endif
