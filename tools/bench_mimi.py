#!/usr/bin/env python3
"""Mimi decode on one MI355X, random-init mimi_202407 (32 codebooks): the whole-clip decode of --frames frames (125 = 10 s) and the
streamed decode of the same frames in chunks of 1 (the reference's schedule: one decodeStep per frame), 4 and 25 frames.

Every figure is a synchronised host clock around host-memory calls (codes up, samples back), so it is what a caller waits for, not
kernel time.  --warmup untimed passes over the whole clip per schedule, then --repeats timed passes; a pass of a streamed schedule is
reset + all its calls.  Reported per schedule: min / median / max over the passes of milliseconds per call and per frame, and the
median's multiple of real time (one frame is 80 ms of audio).  The chunk-of-1 row is the baseline the larger chunks are read against.
Nothing is asserted.  Prints one JSON line.

--encode measures Mimi encode instead: clips of --seconds seconds (10 and 30) of noise through encode (32 codebooks), encode_latent,
and quantize on that latent with 32 codebooks and with 1.  The same warm-up / repeats / median rule, host-inclusive like the rest.
Derived rows: the chain's time per stage = (quantize 32 - quantize 1) / 31; the encoder transformer = 8/7 of the difference between
encode_latent on this handle and on one with a single transformer layer (same SEANet, same clip); the SEANet encoder and the latent
downsample = encode_latent minus that."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mlx_swift_audio_amd as m  # noqa: E402
from mlx_swift_audio_amd import synthetic  # noqa: E402
from mlx_swift_audio_amd.mimi import MimiCodec  # noqa: E402


def spread(v):
    v = sorted(v)
    return {"min": round(v[0], 4), "median": round(v[len(v) // 2], 4), "max": round(v[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=125)
    ap.add_argument("--chunks", type=int, nargs="*", default=[1, 4, 25])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--encode", action="store_true")
    ap.add_argument("--seconds", type=float, nargs="*", default=[10.0, 30.0])
    a = ap.parse_args()
    if a.encode:
        return encode_main(a)
    cfg = synthetic.MIMI_CONFIGS["mimi_202407"]
    ctx = m.Context(0)
    codec = MimiCodec.load(ctx, cfg, synthetic.mimi_weights(cfg, a.seed))
    rng = np.random.Generator(np.random.PCG64(a.seed))
    codes = rng.integers(0, cfg.quantizer_bins, (cfg.quantizer_nq, a.frames)).astype(np.int32)
    frame_ms = 1000.0 / cfg.frame_rate
    out = {"config": "mimi_202407", "frames": a.frames, "n_q": cfg.quantizer_nq, "warmup": a.warmup, "repeats": a.repeats,
           "unit": "ms, host inclusive", "schedules": {}}

    def timed(fn, calls):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        per_frame = spread([x / a.frames for x in ms])
        return {"calls": calls, "ms_per_call": spread([x / calls for x in ms]), "ms_per_frame": per_frame,
                "x_real_time": round(frame_ms / per_frame["median"], 1)}

    out["schedules"]["whole"] = timed(lambda: codec.decode(codes), 1)
    stream = codec.new_stream()
    for c in a.chunks:
        parts = [np.ascontiguousarray(codes[:, i:i + c]) for i in range(0, a.frames, c)]

        def run():
            stream.reset()
            for p in parts:
                stream.decode_frames(p)
        out["schedules"][f"stream_chunk_{c}"] = timed(run, len(parts))
    stream.close()
    codec.close()
    ctx.close()
    print(json.dumps(out))


def encode_main(a):
    import dataclasses
    cfg = synthetic.MIMI_CONFIGS["mimi_202407"]
    one = dataclasses.replace(cfg, transformer=dataclasses.replace(cfg.transformer, num_layers=1))
    ctx = m.Context(0)
    codec = MimiCodec.load(ctx, cfg, synthetic.mimi_weights(cfg, a.seed, encoder=True))
    shallow = MimiCodec.load(ctx, one, synthetic.mimi_weights(one, a.seed, encoder=True))
    rng = np.random.Generator(np.random.PCG64(a.seed))
    L = cfg.transformer.num_layers
    out = {"config": "mimi_202407", "mode": "encode", "n_q": cfg.quantizer_nq, "warmup": a.warmup, "repeats": a.repeats, "unit": "ms, host inclusive",
           "clips": {}}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ms = []
        for _ in range(a.repeats):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return spread(ms)

    for sec in a.seconds:
        pcm = (0.3 * rng.standard_normal(int(sec * cfg.sample_rate))).astype(np.float32)
        lat = codec.encode_latent(pcm).copy()
        row = {"samples": pcm.size, "frames": codec.encode_frames(pcm.size),
               "encode": timed(lambda: codec.encode(pcm)),
               "encode_latent": timed(lambda: codec.encode_latent(pcm)),
               "encode_latent_1_layer": timed(lambda: shallow.encode_latent(pcm)),
               "quantize_32": timed(lambda: codec.quantize(lat)),
               "quantize_1": timed(lambda: codec.quantize(lat, n_q=1))}
        tf = (row["encode_latent"]["median"] - row["encode_latent_1_layer"]["median"]) * L / (L - 1)
        row["derived"] = {"transformer": round(tf, 4), "seanet_and_downsample": round(row["encode_latent"]["median"] - tf, 4),
                          "chain_per_stage": round((row["quantize_32"]["median"] - row["quantize_1"]["median"]) / (cfg.quantizer_nq - 1), 5),
                          "x_real_time": round(sec * 1e3 / row["encode"]["median"], 1)}
        out["clips"][f"{sec:g}s"] = row
    shallow.close()
    codec.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
