"""Times Kokoro's waveform half on one GPU: random-init kokoro_82m, T rows of aligned text features (default 400: 10 s of audio), host
memory in and out, median of 7 calls after one warm-up.  Prints one JSON line: ms per call and x real time for the whole decode, and
the split the entry points allow -- predictor blocks (f0n), source + STFT (source), generator (generate), and the decoder blocks as
decode - source - generate.  The generator's stages carry no timers of their own, so they are not split further; AdaIN exists in the
materialised form only, so there is no fused / materialised comparison to report.

    python tools/bench_kokoro.py [--T 400] [--config kokoro_82m] [--repeat 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, repeat):
    fn()
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=400)
    ap.add_argument("--config", default="kokoro_82m")
    ap.add_argument("--repeat", type=int, default=7)
    a = ap.parse_args()
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import synthetic
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS, KokoroDecoder
    cfg = KOKORO_CONFIGS[a.config]
    ctx = m.Context(0)
    model = KokoroDecoder.load(ctx, cfg, synthetic.kokoro_weights(cfg, 2))
    rng = np.random.default_rng(0)
    T, L = a.T, 2 * a.T
    asr = rng.standard_normal((cfg.dim_in, T)).astype(np.float32)
    xp = rng.standard_normal((cfg.pred_dim, T)).astype(np.float32)
    s = rng.standard_normal(cfg.style_dim).astype(np.float32)
    f0 = np.where(rng.random(L) < 0.3, 0.0, rng.uniform(80, 300, L)).astype(np.float32)
    n = rng.standard_normal(L).astype(np.float32)
    noise = rng.standard_normal((L * cfg.upsample_scale, cfg.n_harmonics + 1)).astype(np.float32)
    xg = rng.standard_normal((cfg.up_initial, L)).astype(np.float32)
    _, har = model.source(f0, noise)
    ms = {"decode": _median_ms(lambda: model.decode(asr, f0, n, s, noise), a.repeat),
          "predictor_blocks": _median_ms(lambda: model.f0n(xp, s), a.repeat),
          "source_stft": _median_ms(lambda: model.source(f0, noise), a.repeat),
          "generator": _median_ms(lambda: model.generate(xg, s, har), a.repeat)}
    ms["decoder_blocks"] = ms["decode"] - ms["source_stft"] - ms["generator"]
    audio_s = model.output_len(T) / cfg.sample_rate
    print(json.dumps({"config": a.config, "T": T, "audio_s": audio_s, "ms": {k: round(v, 3) for k, v in ms.items()},
                      "x_real_time": round(audio_s / (ms["decode"] * 1e-3), 1), "adain": "materialised"}))
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
