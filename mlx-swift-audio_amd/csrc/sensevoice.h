// sensevoice.h -- internal interface between the Fun-ASR front end (funasr_frontend.hip) and the SenseVoice handle (sensevoice.hip).
#pragma once
#include <stdint.h>

#include <vector>

#include "mia_internal.h"

struct FunasrPlan {
  int B = 0;
  int64_t frames = 0, rows = 0, max_frames = 0;   // mel frames and LFR rows over all clips; the longest clip's frames
  std::vector<int32_t> t_lfr;                     // LFR rows per clip
};
// lengths of a call (host only); MIA_ERR_INVALID_AUDIO for a clip of <= 200 samples
int funasr_plan(mia_ctx* ctx, const int64_t* offs, int B, FunasrPlan& plan);
size_t funasr_scratch_bytes(const FunasrPlan& plan);
// pcm_dev: the clips back to back on the device; feats_dev fp32 [plan.rows][stride]; scratch: funasr_scratch_bytes(plan) device bytes.
// Returns after the stream has drained.
int funasr_features_device(mia_ctx* ctx, const float* pcm_dev, const int64_t* offs, const FunasrPlan& plan, float* feats_dev, int64_t stride, void* scratch);
