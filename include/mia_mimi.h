/* mia_mimi.h -- the configuration record of mia_mimi_load (include/mia.h, "Mimi codec decode"): the fields of MimiConfig, SeanetConfig
 * and MimiTransformerConfig (TTS/Marvis/Mimi/Mimi.swift:17-103) that the decoder uses, all int32.  Flags are 0 / 1:
 * seanet_pad_constant = padMode == .constant, layer_norm = norm == "layer_norm", layer_scale = a LayerScale is present,
 * rope = positionalEmbedding == "rope".  upsample_stride = sample_rate / prod(ratios) / frame_rate (Mimi.swift:128-129).
 * mia.h declares the type; a caller that fills one includes this file as well.  The ctypes mirror is _abi.MimiConfig
 * (tests/test_mimi_abi.py compares the two field for field). */
#ifndef MIA_MIMI_H
#define MIA_MIMI_H
#include "mia.h"

struct mia_mimi_config {
  int32_t sample_rate, upsample_stride;
  int32_t nq, bins, quantizer_dim;
  int32_t seanet_dimension, seanet_nfilters;
  int32_t seanet_n_ratios; int32_t seanet_ratios[8];
  int32_t seanet_ksize, seanet_residual_ksize, seanet_last_ksize, seanet_n_residual_layers, seanet_dilation_base, seanet_compress;
  int32_t seanet_causal, seanet_true_skip, seanet_pad_constant;
  int32_t d_model, n_heads, n_layers, dim_feedforward, context, kv_repeat, gating, layer_norm, layer_scale, rope;
  int32_t max_period;
};

#endif
