"""Times Kokoro's waveform half on one GPU: random-init kokoro_82m, T rows of aligned text features (default 400: 10 s of audio), host
memory in and out, median of 7 calls after one warm-up.  Prints one JSON line: ms per call and x real time for the whole decode, and
the split the entry points allow -- predictor blocks (f0n), source + STFT (source), generator (generate), and the decoder blocks as
decode - source - generate.  The generator's stages carry no timers of their own, so they are not split further; AdaIN exists in the
materialised form only, so there is no fused / materialised comparison to report.

    python tools/bench_kokoro.py [--T 400] [--config kokoro_82m] [--repeat 7]

--text times the text half instead (N tokens, default 100, durations forced to sum to T): ms for durations, encode, align, shared and
the whole KokoroPipeline.synthesize beside decode alone, and the per-step cost of the recurrent kernel as `shared` ms / T (its input
projection included) against the 1.5 us floor of a dependent launch.

--bert times ALBERT + bert_encoder (N padded ids, default 100, and 512): ms for KokoroBert.encode alone, host memory in and out, and for
synthesize_ids beside synthesize from a host d_en in the same process (durations forced to sum to T).

--w16 is the A/B of KokoroDecoder.use_w16 (the tap GEMMs on bf16 copies of the weights, conv_gemm_w16.hip): one process, one handle,
f0n / generate / decode with the switch off, on, and off again (the third column shows what the first two differ by when nothing
changed), same protocol, clocks as found.
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
    ap.add_argument("--text", action="store_true")
    ap.add_argument("--N", type=int, default=100)
    ap.add_argument("--bert", action="store_true")
    ap.add_argument("--w16", action="store_true")
    a = ap.parse_args()
    if a.text:
        return text_main(a)
    if a.bert:
        return bert_main(a)
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
    if a.w16:
        calls = {"f0n": lambda: model.f0n(xp, s), "generate": lambda: model.generate(xg, s, har), "decode": lambda: model.decode(asr, f0, n, s, noise)}
        ms = {}
        for col, on in (("fp32", False), ("w16", True), ("fp32_again", False)):
            model.use_w16(on)
            ms[col] = {k: round(_median_ms(fn, a.repeat), 3) for k, fn in calls.items()}
        print(json.dumps({"config": a.config, "T": T, "audio_s": model.output_len(T) / cfg.sample_rate, "ms": ms}))
        model.close()
        ctx.close()
        return
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


def text_main(a):
    import torch  # noqa: F401  (before the HIP library loads: the pipeline holds its device buffers as torch tensors)

    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import synthetic
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS, KokoroDecoder, KokoroPipeline, KokoroText
    cfg = KOKORO_CONFIGS[a.config]
    ctx = m.Context(0)
    w = synthetic.kokoro_weights(cfg, 2, text=True)
    text, dec = KokoroText.load(ctx, cfg, w), KokoroDecoder.load(ctx, cfg, w)
    rng = np.random.default_rng(0)
    N, T = a.N, a.T
    d_en = rng.standard_normal((N, cfg.d_model)).astype(np.float32)
    ids = rng.integers(0, cfg.n_symbols, N).astype(np.int32)
    voice = rng.standard_normal(2 * cfg.style_dim).astype(np.float32)
    s_dec, s_pred = voice[:cfg.style_dim], voice[cfg.style_dim:]
    dur = np.full(N, T // N, np.int32)
    dur[:T - int(dur.sum())] += 1
    noise = rng.standard_normal((2 * T * cfg.upsample_scale, cfg.n_harmonics + 1)).astype(np.float32)
    d, _, _ = text.durations(d_en, s_pred)
    t_en = text.encode(ids)
    en, asr = text.align(d, t_en, dur)
    f0, n = dec.f0n(text.shared(en), s_pred)
    pipe = KokoroPipeline(text, dec)
    ms = {"durations": _median_ms(lambda: text.durations(d_en, s_pred), a.repeat),
          "encode": _median_ms(lambda: text.encode(ids), a.repeat),
          "align": _median_ms(lambda: text.align(d, t_en, dur), a.repeat),
          "shared": _median_ms(lambda: text.shared(en), a.repeat),
          "synthesize": _median_ms(lambda: pipe.synthesize(d_en, ids, voice, noise=noise, durations=dur), a.repeat),
          "decode": _median_ms(lambda: dec.decode(asr, f0, n, s_dec, noise), a.repeat)}
    print(json.dumps({"config": a.config, "N": N, "T": T, "ms": {k: round(v, 3) for k, v in ms.items()},
                      "lstm_step_us": round(ms["shared"] * 1e3 / T, 2), "launch_floor_us": 1.5, "persistent_lstm": "not built"}))
    for h in (text, dec):
        h.close()
    ctx.close()


def bert_main(a):
    import torch  # noqa: F401  (before the HIP library loads: the pipeline holds its device buffers as torch tensors)

    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import synthetic
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS, KokoroBert, KokoroDecoder, KokoroPipeline, KokoroText, voice_row
    cfg = KOKORO_CONFIGS[a.config]
    ctx = m.Context(0)
    w = synthetic.kokoro_weights(cfg, 2, text=True, bert=True)
    bert, text, dec = KokoroBert.load(ctx, cfg, w), KokoroText.load(ctx, cfg, w), KokoroDecoder.load(ctx, cfg, w)
    pipe = KokoroPipeline(text, dec, bert)
    rng = np.random.default_rng(0)
    pack = rng.standard_normal((510, 1, 2 * cfg.style_dim)).astype(np.float32)
    out = {"config": a.config, "T": a.T, "launches": 3 + 7 * cfg.bert_layers, "estimate_ms_at_N100": "< 1", "ms": {}}
    for N in (a.N, 512):
        ids = rng.integers(1, cfg.n_symbols, N - 2).astype(np.int32)
        padded = np.concatenate([[0], ids, [0]]).astype(np.int32)
        dur = np.full(N, a.T // N, np.int32)
        dur[:a.T - int(dur.sum())] += 1
        noise = rng.standard_normal((2 * a.T * cfg.upsample_scale, cfg.n_harmonics + 1)).astype(np.float32)
        d_en = bert.encode(padded)
        row = voice_row(pack, N - 2)
        out["ms"][f"N={N}"] = {
            "bert_encode": round(_median_ms(lambda: bert.encode(padded), a.repeat), 3),
            "synthesize_ids": round(_median_ms(lambda: pipe.synthesize_ids(ids, pack, noise=noise, durations=dur), a.repeat), 3),
            "synthesize_from_host_d_en": round(_median_ms(lambda: pipe.synthesize(d_en, padded, row, noise=noise, durations=dur), a.repeat), 3)}
    print(json.dumps(out))
    for h in (bert, text, dec):
        h.close()
    ctx.close()


if __name__ == "__main__":
    main()
