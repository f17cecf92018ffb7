#!/usr/bin/env python3
"""Fun-ASR's audio half (FunASRModel.encodeAudio: front end -> SenseVoice encoder 1 + 49 + 20 layers of 512 / 4 heads -> adaptor) on one
MI355X with random-init full-size bf16 weights: clips of 10 s and 60 s, 1 and 8 of them per call.  Prints one JSON line: wall ms per
encode_audio call (host pointers: the waveform goes up, the audio rows come back) and, from a separate profiled call, the per-class
split of the device time (mia_profile_read: logmel = the whole front end, enc_gemm, enc_attention = attn128, enc_norm, fsmn)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import funasr, synthetic

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
cfg = funasr.SENSEVOICE_CONFIGS["sensevoice"]
ctx = m.Context(0)
model = funasr.SenseVoiceEncoder.load(ctx, cfg, synthetic.sensevoice_weights(cfg, seed=0), m.BF16)
CLASSES = ("logmel", "enc_gemm", "enc_attention", "enc_norm", "fsmn")
res = {"model": "sensevoice 1+49+20 x 512/4 + adaptor 2 x 1024/8, bf16, random init", "reps": reps, "cases": []}
for seconds in (10, 60):
    for B in (1, 8):
        clips = [synthetic.synth_clip(i, seconds * 16000) for i in range(B)]
        out = model.encode_audio(clips)                      # warm-up: buffers grow, tables are built
        ts = []
        for _ in range(reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            model.encode_audio(clips)
            ts.append((time.perf_counter() - t0) * 1e3)
        ctx.profile(True)
        ctx.profile_reset()
        model.encode_audio(clips)
        split = {}
        for c in CLASSES:
            n, ms, _ = ctx.profile_read(c)
            split[c] = {"launches": n, "ms": round(ms, 3)}
        ctx.profile(False)
        ctx.profile_reset()
        res["cases"].append({"clip_s": seconds, "B": B, "audio_rows_per_clip": int(out[0].shape[0]), "ms_per_call_median": round(float(np.median(ts)), 2),
                             "ms_per_call_min": round(min(ts), 2), "device_ms_by_class": split,
                             "device_ms_total": round(sum(v["ms"] for v in split.values()), 2)})
model.close()
print(json.dumps(res))
