#!/usr/bin/env python3
"""mia_whisper_align with its DTW on the host (mode 0) against the device (mode 1, csrc/align_dtw.hip), same process, interleaved.

Workload: large-v3-turbo bf16 with random-init weights (as tools/bench_transcribe.py builds them), --clips (32) windows of random mel,
full 30 s of frames each, one teacher-forced sequence of --lengths (100, 224, 440) text tokens per clip, the six alignment heads the
published large-v3-turbo checkpoint lists.  Timed: the WHOLE timing.align call, host wall clock -- the call returns with its outputs on
the host, so it ends in a stream synchronise, and the tail under test is partly host work that device events would miss.  Per length:
one untimed call per mode, then --runs (7) timed pairs, mode 0 and mode 1 alternating; median, min and max per mode.  The paths of the
two modes are compared on every length.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import synthetic as S
from mlx_swift_audio_amd import timing as HT
from mlx_swift_audio_amd import whisper as HW

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="large-v3-turbo")
ap.add_argument("--clips", type=int, default=32)
ap.add_argument("--lengths", type=int, nargs="+", default=[100, 224, 440])
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--seed", type=int, default=0)
args = ap.parse_args()

HEADS = {"large-v3-turbo": [(2, 4), (2, 11), (3, 3), (3, 6), (3, 11), (3, 14)]}

dims = S.DIMS[args.model]
ctx = m.Context(0)
model = HW.WhisperModel.load(ctx, dims, S.synthetic_weights(dims, seed=args.seed, style="survey"), m.BF16)
print("model loaded", file=sys.stderr, flush=True)
st = model.special
heads = HEADS.get(args.model, [(dims.n_text_layer - 1, h) for h in range(min(6, dims.n_text_head))])
rng = np.random.default_rng(args.seed)
model.encode((0.5 * rng.standard_normal((args.clips, 2 * dims.n_audio_ctx, dims.n_mels))).astype(np.float32))
sot = st.sot_sequence(0, "transcribe")
frames = [2 * dims.n_audio_ctx] * args.clips


def call(mode, seqs):
    model.set_align_dtw(mode)
    ctx.synchronize()
    t0 = time.perf_counter()
    _, paths, _ = HT.align(model, seqs, heads, frames, len(sot), st.eot)
    ctx.synchronize()
    return time.perf_counter() - t0, paths


out = {"model": args.model, "dtype": "bf16", "clips": args.clips, "runs": args.runs, "lengths": {}}
for n in args.lengths:
    n = min(n, dims.n_text_ctx - len(sot) - 2)
    seqs = [sot + [st.no_timestamps] + rng.integers(300, 5000, n).tolist() + [st.eot] for _ in range(args.clips)]
    same = call(0, seqs)[1] == call(1, seqs)[1]               # untimed: workspace growth, first launches
    secs = {0: [], 1: []}
    for _ in range(args.runs):
        for mode in (0, 1):
            secs[mode].append(call(mode, seqs)[0])
    entry = {"paths_identical": same}
    for mode, name in ((0, "host_dtw"), (1, "device_dtw")):
        ms = [1e3 * s for s in secs[mode]]
        entry[name] = {"ms_median": round(float(np.median(ms)), 2), "ms_min": round(min(ms), 2), "ms_max": round(max(ms), 2)}
    entry["device_over_host"] = round(entry["device_dtw"]["ms_median"] / entry["host_dtw"]["ms_median"], 4)
    out["lengths"][str(n)] = entry
    print(n, entry, file=sys.stderr, flush=True)
model.set_align_dtw(0)
print(json.dumps(out))
model.close()
ctx.close()
