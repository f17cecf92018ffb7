#!/usr/bin/env python3
"""Whisper decode step on packed 4- / 8-bit weights against the 16-bit step: same process, same handle, the switch off and on.

Workload: large-v3-turbo dims (--model), synthetic 'survey' checkpoint whose DECODER matrices and token embedding are quantised at load
(checkpoint.quantize_affine, group 64, f16 scales; the handle is loaded from their de-quantisation and gets the packed tensors attached),
B in --batches (1, 4, 32) random mel windows, --steps (64) generated tokens per decode with EOT suppressed so that every clip runs every
step.  Per B and per mode: --warmup untimed decodes (the first captures the step graphs), then --repeats timed ones, the two modes
ALTERNATING so that drift of the shared machine hits both alike.  Time = the library's device events around the step loop of a decode
(mia_profile_read("decode"): the per-call set-up copies and the output copies are outside them) over the steps that loop ran; the host
clock around the whole call, which ends in a device synchronise, is printed beside it.  The encoder is outside both windows.

Prints one JSON line: per B and mode the median / min / max ms per step, and the algorithmic bytes of a step computed from the shapes
(weights + fp32 (s, t) pairs, cross K/V of every clip, self K/V at the mean position, logits written and read) -- not measured traffic."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import synthetic as S
from mlx_swift_audio_amd import whisper as HW
from mlx_swift_audio_amd.checkpoint import quantize_affine

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="large-v3-turbo")
ap.add_argument("--bits", type=int, default=4, choices=[4, 8])
ap.add_argument("--batches", default="1,4,32")
ap.add_argument("--steps", type=int, default=64)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--dtype", default="bf16", choices=["bf16", "f16"])
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--out", default=None, help="also write the JSON line to this file")
args = ap.parse_args()


def step_bytes(d, B, bits, n_init, steps):
    """Algorithmic bytes one decode step moves, from the shapes (16-bit activations are noise beside these and are left out)."""
    D, L, V, T = d.n_text_state, d.n_text_layer, d.n_vocab, d.n_audio_ctx
    n_w = 14 * D * D * L + V * D                                    # q|k|v 3, out 1, cross q / out 2, mlp 8 per layer; the tied embedding
    w = n_w * 2 if bits == 16 else n_w * bits / 8 + n_w / 64 * 8    # packed: codes + one fp32 (s, t) pair per 64 inputs
    cross = B * L * 2 * T * D * 2
    self_kv = B * L * 2 * (n_init + steps / 2) * D * 2
    logits = 2 * B * V * 4
    return {"weights": int(w), "cross_kv": int(cross), "self_kv": int(self_kv), "logits": int(logits), "total": int(w + cross + self_kv + logits)}


dims = S.DIMS[args.model]
dense = S.synthetic_weights(dims, seed=args.seed, style="survey")
packed = {}
for name in list(dense):
    a = dense[name]
    if name.startswith("decoder.") and name.endswith(".weight") and a.ndim == 2 and a.shape[1] % 64 == 0:      # the Linears and the embedding
        codes, sc, bi = quantize_affine(a, 64, args.bits, np.float16)
        base = name[:-7]
        packed[base + ".weight"], packed[base + ".scales"], packed[base + ".biases"] = codes, sc, bi
        per = 32 // args.bits
        q = ((codes[:, :, None] >> (np.arange(per, dtype=np.uint32) * np.uint32(args.bits))) & np.uint32((1 << args.bits) - 1)).reshape(a.shape[0], -1, 64)
        dense[name] = (sc.astype(np.float32)[..., None] * q.astype(np.float32) + bi.astype(np.float32)[..., None]).reshape(a.shape)
ctx = m.Context(0)
model = HW.WhisperModel.load(ctx, dims, dense, m.BF16 if args.dtype == "bf16" else m.F16)
model.attach_quantized(packed, bits=args.bits)
del dense
print("model loaded, packed weights attached", file=sys.stderr, flush=True)
ctx.profile(True)

st = model.special
opts = HW.DecodingOptions(timestamps=False, suppress_ids=S.synthetic_suppress_list(st) + [st.eot], blank_ids=[220], max_new_tokens=args.steps)
n_init = len(st.sot_sequence(0, "transcribe")) + 1      # + <|notimestamps|>
rng = np.random.default_rng(args.seed)
result = {"model": args.model, "bits": args.bits, "dtype": args.dtype, "generated_per_decode": args.steps, "forced_prefix": n_init, "warmup": args.warmup, "repeats": args.repeats, "batches": {}}
for B in [int(x) for x in args.batches.split(",")]:
    mel = (0.5 * rng.standard_normal((B, 2 * dims.n_audio_ctx, dims.n_mels))).astype(np.float32)
    model.encode(mel)
    times = {0: [], 1: []}
    wall = {0: [], 1: []}
    tokens = {}
    for it in range(args.warmup + args.repeats):
        for on in (0, 1):
            model.use_packed(bool(on))
            ctx.profile_reset()
            t0 = time.perf_counter()
            res = model.decode_greedy(opts)             # ends in a device synchronise (results are copied to the host)
            dt = time.perf_counter() - t0
            calls, ms, steps_run = ctx.profile_read("decode")               # device events around the step loop; work = steps run
            assert calls == 1 and steps_run > 0, (calls, steps_run)
            tokens[on] = [r.tokens for r in res]
            if it >= args.warmup:
                times[on].append(ms / steps_run)
                wall[on].append(1e3 * dt / steps_run)
    agree = sum(a == b for a, b in zip(tokens[0], tokens[1]))
    entry = {"clips_with_identical_ids": agree, "steps_run_last_decode": int(steps_run)}
    for on, key in ((0, "16bit"), (1, "packed")):
        t = times[on]
        entry[key] = {"ms_per_step_median": round(statistics.median(t), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                      "host_wall_ms_per_step_median": round(statistics.median(wall[on]), 5), "bytes_per_step": step_bytes(dims, B, args.bits if on else 16, n_init, args.steps)}
    entry["packed_over_16bit_time"] = round(entry["packed"]["ms_per_step_median"] / entry["16bit"]["ms_per_step_median"], 4)
    result["batches"][str(B)] = entry
    print(f"B {B}: 16-bit {entry['16bit']['ms_per_step_median']} ms/step, packed {entry['packed']['ms_per_step_median']} ms/step", file=sys.stderr, flush=True)
model.use_packed(False)
model.close()
line = json.dumps(result)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
