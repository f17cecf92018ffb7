"""What `bench_outetts.py --split-step` and `bench_orpheus.py --split-step` share: the decode step's time per generated token at fixed
contexts on one handle, the step-attention switch off, then on, then off again (the form of bench_outetts.py --kv-bits).  `toggle` is
the setter that is switched: CausalLM.set_step_attention on the 16-bit cache, CausalLM.set_kvq_step_attention on the packed one.

A reading is the median of `reps` (>= 7) timed runs after one warm-up, clocks as found, synchronised host clock.  One run times
generate(prompt of `ctx` random ids, n_new tokens) and generate(the same prompt, 1 token) -- both end in a synchronise -- and reports
(t_n - t_1) / (tokens - 1): the prompt pass and the first step cancel, what is left is n_new - 1 decode steps at contexts ctx + 1 ..
ctx + n_new - 1.  Side by side: generate_batch of B such prompts, the same difference per STEP (all B sequences advance in one step)."""
import time

import numpy as np
import torch


def _spread(ms):
    ms = sorted(ms)
    return {"min": round(ms[0], 4), "median": round(ms[len(ms) // 2], 4), "max": round(ms[-1], 4)}


def _per_step_ms(run, n_new):
    """run(k) generates k tokens per sequence and returns the ids of sequence 0"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(1)
    t1 = time.perf_counter()
    gen = run(n_new)
    t2 = time.perf_counter()
    if len(gen) != n_new:
        raise SystemExit(f"a sequence stopped after {len(gen)} of {n_new} tokens: pick another --seed")
    return ((t2 - t1) - (t1 - t0)) * 1e3 / (n_new - 1)


def _off_on_off(toggle, run, n_new, reps):
    out = {}
    for name, on in (("off", False), ("on", True), ("off_again", False)):
        toggle(on)
        ts = [_per_step_ms(run, n_new) for _ in range(reps + 1)]        # one warm-up (it also re-captures the step graph)
        out[name] = _spread(ts[1:])
    out["off_minus_on_median"] = round(min(out["off"]["median"], out["off_again"]["median"]) - out["on"]["median"], 4)
    out["off_spread_median"] = round(abs(out["off"]["median"] - out["off_again"]["median"]), 4)
    return out


def measure(model, cfg, contexts, batches, batch_ctx, n_new, reps, seed, log, toggle=None):
    """-> {"ms_per_token": {ctx: off / on / off_again}, "ms_per_step_side_by_side": {B: ...}}"""
    toggle = toggle or model.set_step_attention
    rng = np.random.default_rng(seed)
    kw = dict(temperature=0.6, top_p=0.9, rep_penalty=1.1, rep_window=16, stop_ids=(cfg.vocab - 1,))
    u = rng.random(n_new).astype(np.float32)
    res = {"new_tokens": n_new, "repeats": reps, "ms_per_token": {}, "ms_per_step_side_by_side": {}}
    for n in contexts:
        ids = rng.integers(0, cfg.vocab - 1, n).tolist()
        res["ms_per_token"][str(n)] = r = _off_on_off(toggle, lambda k: model.generate(ids, u, max_new_tokens=k, **kw), n_new, reps)
        log(f"split-step context {n}: {r}")
    for B in batches:
        model.set_batch(B)
        prompts = [rng.integers(0, cfg.vocab - 1, batch_ctx).tolist() for _ in range(B)]
        ub = rng.random((B, n_new)).astype(np.float32)
        r = _off_on_off(toggle, lambda k: model.generate_batch(prompts, ub, max_new_tokens=k, **kw)[0], n_new, reps)
        r["context"] = batch_ctx
        res["ms_per_step_side_by_side"][str(B)] = r
        log(f"split-step {B} sentences at context {batch_ctx}: {r}")
    toggle(False)
    model.set_batch(1)
    return res
