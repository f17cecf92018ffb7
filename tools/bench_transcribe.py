#!/usr/bin/env python3
"""WhisperSTT.transcribe over MULTI-window clips on one MI355X: the host mel path against the device-resident one, same process.

Workload: --clips (32) synthetic clips of --seconds (120) on large-v3-turbo bf16 with random-init weights (as bench.py builds them),
the reference's thresholds on (no_speech 0.6, logprob -1.0, compression ratio 2.4), segment timestamps, max_tokens 448, language 0.
With random-init weights most windows climb the temperature ladder, so passes per clip are printed beside the throughput: the number
means nothing without them.  Every run of a path uses the same np.random.default_rng(seed), so both paths do the same decoding work
(their results are identical; checked here on the first run of each).

  --path host|resident|both   resident = WhisperAudio + encode_audio_windows; host = per-clip log-mel to numpy, numpy slice / round,
                              one upload per window (resident=False)
  --runs N                    timed runs per path after one untimed run (default 3), reported individually with min / max
  --gen64                     also the single-window "64 generated tokens" run of SURVEY 8(d): mia_whisper_transcribe_windows on the
                              first 30 s of every clip with max_new_tokens=64

Prints one JSON line.  encodes per clip = encoder launches of the run / clips (every launch covers a sub-batch); the gather kernel's time
per call comes from mia_profile_read("mel_gather") in a separate, untimed profiled run (event recording perturbs the timed ones)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import synthetic as S
from mlx_swift_audio_amd import transcribe as HT
from mlx_swift_audio_amd import whisper as HW

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="large-v3-turbo")
ap.add_argument("--clips", type=int, default=32)
ap.add_argument("--seconds", type=float, default=120.0)
ap.add_argument("--path", choices=["host", "resident", "both"], default="both")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--max-tokens", type=int, default=448)
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--gen64", action="store_true")
args = ap.parse_args()


class Tok:
    def decode(self, toks):
        return "".join(" w%d" % t for t in toks)


dims = S.DIMS[args.model]
ctx = m.Context(0)
model = HW.WhisperModel.load(ctx, dims, S.synthetic_weights(dims, seed=args.seed, style="survey"), m.BF16)
print("model loaded", file=sys.stderr, flush=True)
sup = S.synthetic_suppress_list(model.special)
stt = HT.WhisperSTT(ctx, model, Tok(), sup, [220])
n = int(args.seconds * 16000)
clips = []
for i in range(args.clips):                              # synth_clip is 30 s: tile distinct ones to the asked length
    parts = [S.synth_clip(i * 16 + k) for k in range((n + 479999) // 480000)]
    clips.append(np.concatenate(parts)[:n])
audio_s = args.clips * args.seconds

counts = {"encode": 0, "windows": 0}
_ragged = model.decode_ragged


def _count_windows(o, inits, sot_index, temperatures, *a, **k):     # a window's first pass is the one at temperature 0
    counts["windows"] += sum(1 for t in temperatures if t == 0.0)
    return _ragged(o, inits, sot_index, temperatures, *a, **k)


model.decode_ragged = _count_windows
for name in ("encode", "encode_audio_windows"):
    def wrap(fn):
        def counted(*a, **k):
            counts["encode"] += 1
            return fn(*a, **k)
        return counted
    setattr(model, name, wrap(getattr(model, name)))


def run(path):
    counts["encode"] = counts["windows"] = 0
    ctx.synchronize()
    t0 = time.perf_counter()
    res = stt.transcribe(clips, max_tokens=args.max_tokens, rng=np.random.default_rng(3), resident=path == "resident")
    ctx.synchronize()
    dt = time.perf_counter() - t0
    print(f"{path}: {dt:.3f} s, {counts['encode']} encodes, {counts['windows']} windows", file=sys.stderr, flush=True)
    return dt, res, (counts["encode"], counts["windows"])


def signature(res):
    return [(r.passes, [(s.tokens, s.start, s.end) for s in r.segments]) for r in res]


out = {"model": args.model, "dtype": "bf16", "clips": args.clips, "clip_seconds": args.seconds, "max_tokens": args.max_tokens, "paths": {}}
sigs = {}
for path in (["host", "resident"] if args.path == "both" else [args.path]):
    _, res, (enc, wins) = run(path)                       # untimed: allocations, graph capture, workspace growth
    sigs[path] = signature(res)
    secs = [run(path)[0] for _ in range(args.runs)]
    rate = [audio_s / s for s in secs]
    passes = sum(r.passes for r in res)
    entry = {"seconds": [round(s, 4) for s in secs], "audio_s_per_s": [round(r, 1) for r in rate], "audio_s_per_s_median": round(float(np.median(rate)), 1),
             "spread_pct": round(100.0 * (max(rate) - min(rate)) / float(np.median(rate)), 2), "windows_per_clip": round(wins / args.clips, 2),
             "passes_per_clip": round(passes / args.clips, 2),
             "encodes_per_run": enc, "encodes_per_clip": round(enc / args.clips, 2), "segments": sum(len(r.segments) for r in res)}
    if path == "resident":
        ctx.profile(True)
        ctx.profile_reset()
        run(path)
        calls, ms, work = ctx.profile_read("mel_gather")
        ctx.profile(False)
        ctx.profile_reset()
        entry["mel_gather"] = {"calls": calls, "us_per_call": round(1e3 * ms / max(calls, 1), 2), "gb_per_s": round(work / max(ms, 1e-9) / 1e6, 1),
                               "mb_per_call": round(work / max(calls, 1) / 1e6, 2)}
    out["paths"][path] = entry
if len(sigs) == 2:
    out["results_identical"] = sigs["host"] == sigs["resident"]
    h, r = out["paths"]["host"]["audio_s_per_s_median"], out["paths"]["resident"]["audio_s_per_s_median"]
    out["resident_over_host"] = round(r / h, 4)

if args.gen64:
    o = HW.DecodingOptions(suppress_ids=sup, blank_ids=[220], max_new_tokens=64)
    first = [c[:480000] for c in clips]
    model.transcribe_windows(first, o)
    ctx.synchronize()
    secs = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        r64 = model.transcribe_windows(first, o)
        ctx.synchronize()
        secs.append(time.perf_counter() - t0)
    a64 = sum(min(c.shape[0], 480000) for c in first) / 16000.0
    out["gen64_single_window"] = {"seconds": [round(s, 4) for s in secs], "audio_s_per_s": [round(a64 / s, 1) for s in secs],
                                  "generated_tokens_per_clip": round(sum(len(r.tokens) for r in r64) / len(r64), 1)}
print(json.dumps(out))
model.close()
ctx.close()
