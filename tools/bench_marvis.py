#!/usr/bin/env python3
"""Marvis frame generation on one MI355X, random-init CSM-1B shapes (llama-1B backbone, llama-100M depth decoder, audio vocabulary 2051,
32 codebooks; the text vocabulary is cut to --text-vocab rows, which only shortens the host-side checkpoint generation): a voice prompt
of --prompt rows, then --frames frames per pass at each of the reference's quality levels (8 / 16 / 24 / 32 codebooks).

Every figure is a synchronised host clock around host-memory calls, so it is what a caller waits for.  A pass is reset + prompt +
frames; the prompt's share is measured by a pass of one frame and subtracted.  --warmup untimed passes, then --repeats timed ones; the
median is reported with min and max, and its multiple of real time (a frame is 80 ms of audio).  Random weights with uniforms at 0.999
do not draw the all-zero frame in practice; a pass that ends early is reported in `frames_emitted`.  Nothing is asserted.  Prints one
JSON line.

--packed {4,6,8}: every Linear of the checkpoint (both stacks, projection, codebook0_head) is quantised to that width (group 64, as the
published checkpoints store them), the handle is loaded through MarvisModel.load_quantized's steps, and the same handle is timed with
the switch off (16-bit copy of the de-quantised weights) and on (packed codes): the figures appear under "weights": {"16bit", "packed"}."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mlx_swift_audio_amd as m  # noqa: E402
from mlx_swift_audio_amd import marvis, synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--prompt", type=int, default=300)
    ap.add_argument("--text-vocab", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--codebooks", type=int, nargs="*", default=[8, 16, 24, 32])
    ap.add_argument("--batch", type=int, default=8, help="sentences side by side in the generate_batch rows (0: skip them)")
    ap.add_argument("--direct", action="store_true", help="launch every frame's kernels directly instead of the captured graph")
    ap.add_argument("--packed", type=int, choices=[4, 6, 8], default=0, help="quantise the Linears to this width and time the handle on the 16-bit copy and on the packed codes")
    a = ap.parse_args()
    cfg = dataclasses.replace(synthetic.MARVIS_CONFIGS["marvis-csm-1b"], text_vocab=a.text_vocab)
    t0 = time.perf_counter()
    w = synthetic.marvis_weights(cfg, seed=0)
    ctx = m.Context(0)
    if a.packed:
        from mlx_swift_audio_amd import checkpoint
        for k in [k for k in w if k.endswith("_proj.weight") or k in ("projection.weight", "codebook0_head.weight")]:
            w[k], w[k[:-7] + ".scales"], w[k[:-7] + ".biases"] = checkpoint.quantize_affine(w[k], 64, a.packed, np.float16)
        model = marvis.MarvisModel.load(ctx, cfg, checkpoint.expand_checkpoint(ctx, w), m.BF16)
        model.attach_quantized(w)
    else:
        model = marvis.MarvisModel.load(ctx, cfg, w, m.BF16)
    gen_s = time.perf_counter() - t0
    del w
    if a.direct:
        model.set_debug(1)
    rng = np.random.Generator(np.random.PCG64(0))
    n_text = min(40, a.prompt // 2)
    rows, mask = marvis.tokenize_start(rng.integers(0, a.text_vocab, n_text), rng.integers(1, cfg.audio_vocab, (cfg.n_codebooks, a.prompt - n_text)))
    out = {"config": "csm-1b shapes, bf16, random init", "prompt_rows": int(rows.shape[0]), "frames": a.frames, "warmup": a.warmup, "repeats": a.repeats,
           "launch": "direct" if a.direct else "graph", "unit": "ms, host inclusive", "checkpoint_generation_s": round(gen_s, 1)}

    def one_pass(cb, n):
        model.reset()
        ctx.synchronize()
        t = time.perf_counter()
        f = model.generate(rows, mask, cb, np.full((n, min(cb, cfg.n_codebooks)), 0.999, np.float32))
        return (time.perf_counter() - t) * 1e3, f.shape[0]

    def measure():
        res = {"codebooks": {}}
        for cb in a.codebooks:
            for _ in range(a.warmup):
                one_pass(cb, a.frames)
            first = sorted(one_pass(cb, 1)[0] for _ in range(a.repeats))[a.repeats // 2]
            runs = [one_pass(cb, a.frames) for _ in range(a.repeats)]
            per = sorted((ms - first) / max(a.frames - 1, 1) for ms, _ in runs)
            res["codebooks"][str(cb)] = {"prompt_plus_first_frame_ms": round(first, 3), "ms_per_frame": {"min": round(per[0], 4), "median": round(per[len(per) // 2], 4),
                                                                                                      "max": round(per[-1], 4)},
                                         "x_real_time": round(80.0 / per[len(per) // 2], 1), "frames_emitted": [n for _, n in runs]}
        if a.batch > 1:          # the same prompt for every sentence, as the reference's sentences share their voice prompt
            model.set_batch(a.batch)
            res["batch"] = {"sentences": a.batch, "codebooks": {}}
            for cb in a.codebooks:
                def bpass(n):
                    ctx.synchronize()
                    t = time.perf_counter()
                    f = model.generate_batch([(rows, mask)] * a.batch, cb, np.full((a.batch, n, min(cb, cfg.n_codebooks)), 0.999, np.float32))
                    return (time.perf_counter() - t) * 1e3, [x.shape[0] for x in f]
                for _ in range(a.warmup):
                    bpass(a.frames)
                first = sorted(bpass(1)[0] for _ in range(a.repeats))[a.repeats // 2]
                runs = [bpass(a.frames) for _ in range(a.repeats)]
                per = sorted((ms - first) / max(a.frames - 1, 1) for ms, _ in runs)
                med = per[len(per) // 2]
                res["batch"]["codebooks"][str(cb)] = {"prompts_plus_first_frame_ms": round(first, 3), "ms_per_frame_step": round(med, 4),
                                                       "audio_seconds_per_second": round(a.batch * 0.08 / (med * 1e-3), 1), "frames_emitted": runs[-1][1]}
        if a.batch > 1:
            model.set_batch(1)
        return res

    if a.packed:
        out["packed_bits"] = a.packed
        out["weights"] = {}
        for label, on in (("16bit", False), ("packed", True)):
            model.use_packed(on)
            out["weights"][label] = measure()
    else:
        out.update(measure())
    print(json.dumps(out))
    model.close()
    ctx.close()


if __name__ == "__main__":
    main()
