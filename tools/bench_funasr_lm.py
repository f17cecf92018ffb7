#!/usr/bin/env python3
"""Fun-ASR's decoder loop (FunASRSTT.swift:111-156) on one MI355X: Qwen3-0.6B with random-init bf16 weights, a prompt of 24 text rows +
250 audio rows + 8 text rows merged as FunASRModel.mergeEmbeddings does, then argv[1] greedy tokens (default 128).  Prints one JSON
line: prompt pass + first step, ms per generated token and its fraction of the HBM roofline (the bf16 weights are read once per step:
tied embedding + 28 layers, as tools/bench_orpheus.py counts them), at batch 1 and with 8 and 32 utterances side by side.
--no-qk-norm drops the q_norm / k_norm tensors from the checkpoint: same dims on the kernel instances without the norm (the A/B of
what the norm costs).
--temperature T [--top-k K] [--top-p P] (T > 0) also times the sampled loop (sampleNextToken's second branch: top-k, top-p, draw) against
the greedy loop in the same process, same prompts, at batch 1 and 8: the "sampled" entry holds ms per step of both and their difference,
which is what the six sampler launches cost over the greedy sampler's two."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import lm as HL
from mlx_swift_audio_amd import synthetic as S

qk_norm = "--no-qk-norm" not in sys.argv
args = [a for a in sys.argv[1:] if a != "--no-qk-norm"]


def _flag(name, default, kind):
    if name not in args:
        return default
    i = args.index(name)
    value = kind(args[i + 1])
    del args[i:i + 2]
    return value


temperature, top_k, top_p = _flag("--temperature", 0.0, float), _flag("--top-k", 0, int), _flag("--top-p", 0.95, float)
n_new = int(args[0]) if args else 128
cfg = S.LM_CONFIGS["qwen3-0.6b"]
ctx = m.Context(0)
w = S.lm_weights(cfg, seed=0, dtype=np.float16)
if not qk_norm:
    w = {k: v for k, v in w.items() if "q_norm" not in k and "k_norm" not in k}
model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
emb = w["model.embed_tokens.weight"]
dec = HL.FunASRDecoder(model, emb)
rng = np.random.default_rng(0)
SOS, EOS, STOP = cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1
spread = float(emb[:4096].astype(np.float32).std())


def prompt():
    ids = rng.integers(0, cfg.vocab - 3, 23).tolist() + [SOS, EOS] + rng.integers(0, cfg.vocab - 3, 7).tolist()
    audio = (rng.standard_normal((250, cfg.hidden)) * spread).astype(np.float32)
    return dec.merge_embeddings(ids, audio, SOS, EOS)


x = prompt()
assert x.shape == (24 + 250 + 8, cfg.hidden)


def run(n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate_greedy(x, (STOP,), n)
    return time.perf_counter() - t0, out


params = cfg.vocab * cfg.hidden + cfg.n_layers * ((cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim * cfg.hidden +
                                                  cfg.hidden * cfg.n_heads * cfg.head_dim + 3 * cfg.inter * cfg.hidden)
bytes_per_step = 2.0 * params
run(8)
d1, _ = run(1)
dt, out = run(n_new)
steps = max(len(out) - 1, 1)
ms_tok = (dt - d1) / steps * 1e3
res = {"model": "qwen3-0.6b (Fun-ASR decoder, greedy)", "qk_norm": qk_norm, "prompt_rows": int(x.shape[0]), "generated_tokens": len(out),
       "distinct_ids": len(set(out)), "prompt_pass_plus_first_step_ms": round(d1 * 1e3, 2), "ms_per_token": round(ms_tok, 4),
       "weight_GB_per_step": round(bytes_per_step / 1e9, 3), "hbm_frac_of_8TBs": round(bytes_per_step / (ms_tok * 1e-3) / 8e12, 4), "batch": []}
for batch in (8, 32):
    model.set_batch(batch)
    xs = [prompt() for _ in range(batch)]
    model.generate_greedy_batch(xs, (STOP,), 8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate_greedy_batch(xs, (STOP,), 1)
    b1 = time.perf_counter() - t0
    t0 = time.perf_counter()
    outs = model.generate_greedy_batch(xs, (STOP,), n_new)
    db = time.perf_counter() - t0
    bsteps = max(max(len(o) for o in outs) - 1, 1)
    ms_step = (db - b1) / bsteps * 1e3
    res["batch"].append({"utterances": batch, "generated_tokens": sum(len(o) for o in outs), "prompt_pass_plus_first_step_ms": round(b1 * 1e3, 2),
                         "ms_per_step": round(ms_step, 4), "ms_per_token": round(ms_step / batch, 4), "tokens_per_s": round(batch / (ms_step * 1e-3), 1),
                         "hbm_frac_of_8TBs": round(bytes_per_step / (ms_step * 1e-3) / 8e12, 4)})
if temperature > 0:
    # greedy against sampled, interleaved in one process on the same prompts; a run that draws the stop id early counts its own steps
    def step_ms(call, n):
        call(8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(1)
        t1 = time.perf_counter()
        outs = call(n)
        t2 = time.perf_counter()
        return ((t2 - t1) - (t1 - t0)) / max(max(len(o) for o in outs) - 1, 1) * 1e3

    res["sampled"] = {"temperature": temperature, "top_k": top_k, "top_p": top_p, "batch": []}
    for batch in (1, 8):
        model.set_batch(batch)
        xs = [prompt() for _ in range(batch)]
        us = rng.random((batch, n_new)).astype(np.float32)
        greedy = lambda n: model.generate_greedy_batch(xs, (STOP,), n)
        sampled = lambda n: model.generate_topk_batch(xs, us, (STOP,), n, temperature, top_p, top_k)
        g, s_ = [], []
        for _ in range(3):
            g.append(step_ms(greedy, n_new))
            s_.append(step_ms(sampled, n_new))
        res["sampled"]["batch"].append({"utterances": batch, "greedy_ms_per_step": round(min(g), 4), "sampled_ms_per_step": round(min(s_), 4),
                                        "sampler_extra_us_per_step": round((min(s_) - min(g)) * 1e3, 1),
                                        "greedy_runs": [round(v, 4) for v in g], "sampled_runs": [round(v, 4) for v in s_]})
model.set_batch(1)
print(json.dumps(res))
