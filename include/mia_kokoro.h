/* mia_kokoro.h -- the configuration record of mia_kokoro_load (include/mia.h, "Kokoro"): the constructor arguments of KokoroDecoder and
 * Predictor (TTS/Kokoro/TTSEngine/KokoroModel.swift:26-64,116-129), all int32.  hidden = the width of the encode / decode blocks (1024),
 * asr_res_dim = the channels of asr_res (64), up_initial = upsampleInitialChannel, which is also what the last decode block puts out;
 * n_harmonics = harmonicNum (8: nine sine tracks with the fundamental); pred_dim = Predictor's dModel, 0 = no F0 / N blocks.
 * mia.h declares the type; a caller that fills one includes this file as well.  The ctypes mirror is _abi.KokoroConfig
 * (tests/test_kokoro_abi.py compares the two field for field). */
#ifndef MIA_KOKORO_H
#define MIA_KOKORO_H
#include "mia.h"

struct mia_kokoro_config {
  int32_t dim_in, style_dim, hidden, asr_res_dim, pred_dim;
  int32_t up_initial, n_ups; int32_t up_rates[4]; int32_t up_kernels[4];
  int32_t n_res_kernels; int32_t res_kernels[4];
  int32_t n_dilations; int32_t dilations[4];
  int32_t n_fft, hop, n_harmonics, voiced_threshold, sample_rate;
};

#endif
