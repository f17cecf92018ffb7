#!/usr/bin/env python3
"""Reference-clip trimming on one MI355X: Clip creation (the upload) and speech_bounds (energy pass + finish + a 24-byte download), timed
separately, for a 30 s / 24 kHz clip and for 2^24 samples, frames 600 / 300, top_db 60.

Each figure is a synchronised host clock around the call: create returns after its upload has completed and speech_bounds after its
download, so both are host-inclusive call times, not kernel times.  Three warm-ups of each call, then --repeats batches of --calls calls
(the bounds call is tens of microseconds: a batch keeps the window well above the clock's resolution); min / median / max of the
per-call batch means in microseconds.  The clip is seeded noise between two quiet floors; the bounds are printed so that a changed
result shows.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mlx_swift_audio_amd as m  # noqa: E402
from mlx_swift_audio_amd import trim as T  # noqa: E402


def spread(us):
    us = sorted(us)
    return {"min": round(us[0], 1), "median": round(us[len(us) // 2], 1), "max": round(us[-1], 1)}


def clip_of(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    x = (1e-5 * rng.standard_normal(n)).astype(np.float32)
    lo, hi = n // 50, n - n // 40
    x[lo:hi] += (0.1 * rng.standard_normal(hi - lo)).astype(np.float32)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    ctx = m.Context(0)
    out = {"frame": 600, "hop": 300, "top_db": 60.0, "repeats": a.repeats, "calls_per_batch": a.calls, "unit": "us per call, host inclusive"}
    for label, n in (("30s_24k", 30 * 24000), ("2^24", 1 << 24)):
        x = clip_of(n, a.seed)
        creates = max(a.calls // 20, 5)

        def create_batch(k):
            total = 0.0
            for _ in range(k):
                t0 = time.perf_counter()
                c = T.Clip(ctx, x, 24000)                   # returns after the upload has completed
                total += time.perf_counter() - t0
                c.close()                                   # not timed: hipFree behind a device synchronise
            return total / k * 1e6
        create_batch(3)
        create_us = [create_batch(creates) for _ in range(a.repeats)]
        clip = T.Clip(ctx, x, 24000)

        def bounds_batch(k):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(k):
                b = clip.bounds(600, 300, 60.0)
            return (time.perf_counter() - t0) / k * 1e6, b
        bounds_batch(3)
        runs = [bounds_batch(a.calls) for _ in range(a.repeats)]
        out[label] = {"samples": n, "frames": T.num_frames(n, 600, 300), "upload_mb": round(n * 4 / 1e6, 2), "create_us": spread(create_us),
                      "speech_bounds_us": spread([r[0] for r in runs]), "launches": clip.launches, "bounds": list(runs[0][1][:2])}
        clip.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
