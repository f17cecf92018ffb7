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

/* The configuration record of mia_kokoro_text_load: Predictor's dModel (= TextEncoder's channels), the style width, and TextEncoder's
 * nSymbols, kernelSize and depth (TTSEngine/KokoroModel.swift:109-116).  The ctypes mirror is _abi.KokoroTextConfig. */
struct mia_kokoro_text_config {
  int32_t d_model, style_dim, n_symbols, kernel, depth;
};

/* The configuration record of mia_kokoro_bert_load: AlbertConfig (TTS/Kokoro/Albert/AlbertConfig.swift) without the dropout rates and the
 * layer-norm eps (1e-12, fixed), and out_dim = bert_encoder's output width (Predictor's dModel).  One layer group with one inner layer.
 * The ctypes mirror is _abi.KokoroBertConfig (tests/test_kokoro_bert_abi.py compares the two field for field). */
struct mia_kokoro_bert_config {
  int32_t vocab, embed, hidden, heads, intermediate, n_layers, max_positions, type_vocab, out_dim;
};

#endif
