// align_dtw.h -- the DTW of the word-timestamp alignment (WhisperTiming.swift:46-130): the host form and the device form (align_dtw.hip).
#pragma once
#include <vector>

#include "mia_internal.h"

// the largest n_text_ctx / n_audio_ctx of any published Whisper: what the device form is built for
constexpr int DTW_MAX_ROWS = 448, DTW_MAX_COLS = 1500;

// dtw + backtrace on the host; cost is [N][ld] with M valid columns
void dtw_host(const float* cost, int N, int M, int64_t ld, std::vector<int32_t>& ti, std::vector<int32_t>& tj);

// One launch for a ragged batch.  Clip b reads cost + b * clip_stride as [N_b][ld] with N_b = n_rows[b] - row_sub rows and M_b =
// n_cols[b] valid columns (device arrays); max_rows / max_cols bound every N_b / M_b and size the trace.  Outputs (device): text_idx /
// time_idx [B][path_cap] in forward order, path_len [B]; a clip whose path is longer than path_cap gets its length and nothing else.
struct DtwArgs {
  const float* cost = nullptr;
  int64_t clip_stride = 0, ld = 0;
  const int32_t* n_rows = nullptr;
  const int32_t* n_cols = nullptr;
  int row_sub = 0, B = 0, max_rows = 0, max_cols = 0;
  uint32_t* trace = nullptr;          // dtw_trace_bytes(B, max_rows, max_cols) of scratch
  int32_t* text_idx = nullptr;
  int32_t* time_idx = nullptr;
  int32_t* path_len = nullptr;
  int path_cap = 0;
};
size_t dtw_trace_bytes(int B, int max_rows, int max_cols);
const char* dtw_check(const DtwArgs& a);           // nullptr, or why the launch is refused
int dtw_launch(const DtwArgs& a, hipStream_t s);   // 0, or -1 when the arguments fail dtw_check or the launch fails
