// kokoro_text.h -- launch interface of Kokoro's text half: the bidirectional LSTM (kokoro_lstm.hip) and the small kernels around it
// (kokoro_text.hip: AdaLayerNorm / LayerNorm, duration head, alignment gather, embedding gather).  Activations are time-major fp32
// [rows][ld]; the channel counts here (d_model, d_model + style_dim) are multiples of 32, so no padding column exists.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mia_internal.h"

constexpr int KOKORO_LSTM_U = 16;            // hidden units a workgroup of the step kernel owns
constexpr int KOKORO_LSTM_MAX_H = 256, KOKORO_LSTM_MAX_IN = 1024;
constexpr int KOKORO_MAX_ROWS = 10000;       // the decoder's row limit
constexpr int KOKORO_MAX_TOKENS = 512;

// One BiLSTM as the kernels read it, one device block of kokoro_lstm_floats(In, H) floats:
//   wih  [8 H][In]   weight_ih of the forward direction above that of the reverse one (the tap GEMM's W)
//   bias [8 H]       bias_ih + bias_hh, same order
//   whh  [2][H / 16][4][16][H]   weight_hh by direction, unit block, gate (i, f, g, o), unit: a workgroup's 64 rows are contiguous
struct KokoroLstm { float* wih = nullptr; float* bias = nullptr; float* whh = nullptr; int In = 0, H = 0; };
struct KokoroLstmRaw { const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2]; };     // [0] forward, [1] reverse; device pointers

inline size_t kokoro_lstm_floats(int In, int H) { return (size_t)8 * H * In + (size_t)8 * H + (size_t)8 * H * H; }
inline bool kokoro_lstm_shape_ok(int In, int H) {
  return H >= KOKORO_LSTM_U && H <= KOKORO_LSTM_MAX_H && H % KOKORO_LSTM_U == 0 && In >= 32 && In <= KOKORO_LSTM_MAX_IN && In % 32 == 0;
}
// floats of scratch a run over T rows needs: xproj [T][8 H] and the cell state [2][H]
inline size_t kokoro_lstm_scratch(int64_t T, int H) { return (size_t)T * 8 * H + (size_t)2 * H; }

// block: kokoro_lstm_floats floats, 16-byte aligned.  Fills it from the eight tensors of a BiLSTM and returns the views in `w`.
int kokoro_lstm_pack_launch(const KokoroLstmRaw& raw, int In, int H, float* block, KokoroLstm& w, hipStream_t st);
// x [T][ldx] (columns [0, In)) -> out [T][ldo], columns [0, H) forward and [H, 2 H) reverse.  One tap-GEMM launch, then T step
// launches on the context's stream; no launch waits on another workgroup.  x and out must not overlap.
int kokoro_lstm_run(mia_ctx* ctx, const KokoroLstm& w, const float* x, int64_t ldx, int64_t T, float* scratch, float* out, int64_t ldo);
