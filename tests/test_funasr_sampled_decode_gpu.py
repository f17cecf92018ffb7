"""Fun-ASR's sampled decode on the GPU (mia_lm_generate_topk / _batch: the step graph ending in the top-k / top-p sampler) on the micro
Qwen3 checkpoints: top_k = 1 equals the greedy loop, a captured step equals a direct launch, a batch equals its single runs, the draw
reads its uniform, the ids equal the fp32 oracle's (tests/_qwen3_ref.py + tests/_funasr_sampler_ref.py) wherever the oracle's own run
leaves a derived margin, and FunASRModel.transcribe_tokens routes temperature > 0 here.

The oracle margin (test_sampled_ids_match_oracle).  eps = TOL["f16"] * logit std is tests/test_lm_qwen3_gpu.py's f16 logit bound against
the fp32 oracle.  Logits within eps of the oracle's can
  (a) change the kept set only if the k-th and (k+1)-th largest values are closer than 2 eps;
  (b) change which kept entries come before the picked one only if the pick's value is closer than 2 eps to a kept neighbour's
      (entries that swap places among themselves, before or after the pick, leave its interval where it is);
  (c) move a cumulative probability or a CDF edge by at most exp(2 eps / T) - 1 (every exp(x / T) moves by a factor within
      exp(+-eps / T), numerator and denominator alike), and a swap of two neighbours closer than 2 eps moves the cumulative value between
      them by at most as much again: delta = 2 (exp(2 eps / T) - 1).
So a step is safe when (a) and (b) hold, every cumulative value is >= delta from top_p and u * sum(w) is >= delta (of sum(w)) from the
pick's edges.  The uniforms are chosen on the CPU, step by step on the oracle alone (the midpoint of an interval that clears all four, a
new id where one is on offer); the test re-derives the four margins from the oracle's run with those uniforms, asserts them, prints the
smallest, and then demands exact ids.  Sampler: temperature 4, top_k 5, top_p 0.7 (the micro checkpoints' logits have std 1: five nearly
equal candidates, of which the nucleus keeps four).  Chosen seeds with two uniform rows each (the `choice` seeds of _oracle_uniforms), 10
steps and 10 distinct ids per row, smallest margins as multiples of the requirement ((a), (b), top_p, CDF edge):
  qwen3-micro    seed 53, choices 0 / 7: 1.03, 1.12, 3.6, 7.6 / 1.01, 1.97, 4.4, 7.6 (the rows part at the fifth id)
  qwen3-micro128 seed 49, choices 2 / 6: 1.27, 1.30, 4.8, 7.8 / 1.02, 1.08, 4.6, 7.6 (they part at the first id)"""
import dataclasses
import functools

import numpy as np
import pytest

import _funasr_sampler_ref as F
import _qwen3_ref as R
from mlx_swift_audio_amd import synthetic as S

pytestmark = pytest.mark.gpu

TOL_F16 = 0.015                     # tests/test_lm_qwen3_gpu.py: TOL["f16"]
T_ORA, K_ORA, P_ORA, N_ORA = 4.0, 5, 0.7, 10
ORACLE_CASES = [("qwen3-micro", 53, (0, 7)), ("qwen3-micro128", 49, (2, 6))]


@functools.lru_cache(maxsize=None)
def _case(cfg_name, seed, dtype_name="f16"):
    """Untied head, weights rounded to the storage type, a prompt of 3 text rows + 9 random "audio" rows + 3 text rows (the greedy tests' shape)."""
    cfg = dataclasses.replace(S.LM_CONFIGS[cfg_name], tie_embeddings=False)
    w = S.lm_weights(cfg, seed=seed, round_to=dtype_name)
    emb = w["model.embed_tokens.weight"]
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, cfg.vocab, 6)
    audio = (rng.standard_normal((9, cfg.hidden)) * emb.std()).astype(np.float32)
    prompt = np.concatenate([emb[ids[:3]], audio, emb[ids[3:]]]).astype(np.float32)
    prompt.setflags(write=False)
    return cfg, w, prompt


def _margins(logits, d, temperature, top_p):
    """The four margins of one oracle draw as multiples of what the module docstring requires: (a), (b), top_p, CDF edge."""
    x = np.asarray(logits, np.float64)
    eps = TOL_F16 * x.std()
    top = x[F.kept_order(logits, min(d.k + 1, x.size))]
    a = (top[d.k - 1] - top[d.k]) / (2 * eps) if d.k < x.size else np.inf
    near = [top[d.slot - 1] - top[d.slot]] if d.slot > 0 else []
    if d.slot + 1 < d.k:
        near.append(top[d.slot] - top[d.slot + 1])
    b = min(near) / (2 * eps) if near else np.inf
    delta = 2 * (np.exp(2 * eps / temperature) - 1)
    d_p = np.abs(d.cum - float(np.float32(top_p))).min() if d.cum.size else np.inf
    lo = d.cw[d.slot - 1] if d.slot > 0 else 0.0
    d_u = min(d.goal - lo, d.cw[d.slot] - d.goal) / d.cw[-1]
    return float(a), float(b), float(d_p / delta), float(d_u / delta)


@functools.lru_cache(maxsize=None)
def _oracle_uniforms(cfg_name, seed, choice):
    """N_ORA uniforms chosen on the oracle alone: at every step the midpoint of an interval whose draw clears the four margins, a new id
    where one is on offer, `choice` seeding which.  None when a step has no such interval."""
    cfg, w, prompt = _case(cfg_name, seed)
    emb = w["model.embed_tokens.weight"]
    ora = R.Qwen3Oracle(cfg, w)
    ora.reset()
    rng = np.random.default_rng(choice)
    logits = ora.logits_of_rows(prompt)
    us, out = [], []
    for _ in range(N_ORA):
        d0 = F.sample(logits, 0.0, T_ORA, P_ORA, K_ORA)
        edges = np.concatenate([[0.0], d0.cw]) / d0.cw[-1]
        ok = []
        for j in range(len(d0.kept)):
            u = float(np.float32((edges[j] + edges[j + 1]) / 2))
            d = F.sample(logits, u, T_ORA, P_ORA, K_ORA)
            if d.slot == j and min(_margins(logits, d, T_ORA, P_ORA)) >= 1.0:
                ok.append((u, d.pick))
        if not ok:
            return None
        new = [c for c in ok if c[1] not in out] or ok
        u, pick = new[rng.integers(len(new))]
        us.append(u)
        out.append(pick)
        logits = ora.logits_of_rows(emb[pick][None])
    return tuple(us)


def _oracle_ids(cfg_name, seed, us, trace=None):
    cfg, w, prompt = _case(cfg_name, seed)
    ora = R.Qwen3Oracle(cfg, w)
    ora.reset()
    return F.generate(ora.logits_of_rows, w["model.embed_tokens.weight"], prompt, us, (cfg.vocab - 1,), len(us), T_ORA, P_ORA, K_ORA, trace)


@pytest.mark.parametrize("cfg_name,seed,choices", ORACLE_CASES)
def test_sampled_ids_match_oracle(ctx, cfg_name, seed, choices):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg, w, prompt = _case(cfg_name, seed)
    rows = [_oracle_uniforms(cfg_name, seed, c) for c in choices]
    assert all(r is not None for r in rows)
    want = []
    for us in rows:                                                       # precondition, on the oracle alone: no step may be excused
        trace = []
        ids = _oracle_ids(cfg_name, seed, us, trace)
        worst = np.min([_margins(lg, d, T_ORA, P_ORA) for lg, d in trace], axis=0)
        print(cfg_name, "smallest margins (a), (b), top_p, CDF edge, as multiples of the requirement:", worst, "ids", ids)
        assert len(trace) == N_ORA >= 8 and len(ids) == N_ORA and len(set(ids)) >= 5
        assert worst.min() >= 1.0, worst
        want.append(ids)
    assert want[0] != want[1]                                             # the second row was chosen to draw other ids
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    got = [model.generate_topk(prompt, us, (cfg.vocab - 1,), N_ORA, T_ORA, P_ORA, K_ORA) for us in rows]
    assert got[0] == want[0] and got[1] == want[1]
    assert got[0] != got[1]                                               # the draw reads its uniform
    assert model.generate_topk(prompt, rows[0], (cfg.vocab - 1,), 4, T_ORA, P_ORA, K_ORA) == want[0][:4]      # the budget
    model.close()


@pytest.mark.parametrize("cfg_name,seed", [("qwen3-micro", 13), ("qwen3-micro128", 127)])
def test_top_k_one_equals_greedy(ctx, cfg_name, seed):
    """k = 1 keeps the argmax alone: whatever the temperature, top_p and uniforms, the loop is the greedy one, stop ids included."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg, w, prompt = _case(cfg_name, seed)
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    last = cfg.vocab - 1
    us = np.random.default_rng(seed).random(24).astype(np.float32)
    want = model.generate_greedy(prompt, (last,), 24)
    assert len(want) == 24
    for t, p in ((0.3, 0.95), (2.5, 0.2), (1.0, 1.0)):
        assert model.generate_topk(prompt, us, (last,), 24, t, p, 1) == want
    stop = next(t for i, t in enumerate(want) if i >= 3 and t not in want[:i])        # an id that first appears at step >= 3
    first = want.index(stop)
    assert model.generate_greedy(prompt, (stop, last), 24) == want[:first]
    assert model.generate_topk(prompt, us, (stop, last), 24, 0.7, 0.95, 1) == want[:first]             # not emitted, not counted
    assert model.generate_topk(prompt, us, (last, want[0]), 24, 0.7, 0.95, 1) == []                    # a stop id as the first pick
    assert model.generate_topk(prompt, us, (last,), 24, 0.7, 0.95, 1) == want                          # and the handle decodes on
    assert model.generate_greedy(prompt, (last,), 24) == want                                          # the greedy graph is re-captured
    model.close()


def test_direct_launch_equals_graph(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg, w, prompt = _case("qwen3-micro", 53)
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    us = np.random.default_rng(1).random(20).astype(np.float32)
    params = [(T_ORA, P_ORA, K_ORA), (0.8, 0.95, 0), (1.5, 1.0, 1024), (0.8, 0.95, 0)]      # a change of temperature, k or p re-captures
    graph = [model.generate_topk(prompt, us, (cfg.vocab - 1,), 20, t, p, k) for t, p, k in params]
    assert graph[1] == graph[3] and len({tuple(g) for g in graph}) == 3
    model.set_debug(1)
    assert [model.generate_topk(prompt, us, (cfg.vocab - 1,), 20, t, p, k) for t, p, k in params] == graph
    # the prompt walked through the step (debug bit 1): the sampler idles for 14 steps, then draws -- captured and direct alike
    model.set_debug(2)
    walked = [model.generate_topk(prompt, us, (cfg.vocab - 1,), 20, t, p, k) for t, p, k in params]
    assert walked[1] == walked[3]
    model.set_debug(3)
    assert [model.generate_topk(prompt, us, (cfg.vocab - 1,), 20, t, p, k) for t, p, k in params] == walked
    model.close()


def test_batch_equals_single_runs(ctx):
    """Six prompts of 1 .. 40 rows side by side on a capacity-6 handle, each with its own uniform row: every sequence equals its own
    generate_topk on the same capacity -- the one-row prompt and the sequences that stop at different steps included."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = dataclasses.replace(S.LM_CONFIGS["qwen3-micro"], tie_embeddings=False)
    w = S.lm_weights(cfg, seed=8, round_to="bf16")
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    model.set_batch(6)
    rng = np.random.default_rng(5)
    spread = w["model.embed_tokens.weight"].std()
    prompts = [(rng.standard_normal((n, cfg.hidden)) * spread).astype(np.float32) for n in (1, 3, 9, 17, 40, 12)]
    n_new, last = 20, cfg.vocab - 1
    us = rng.random((6, n_new)).astype(np.float32)
    args = (n_new, 1.0, 0.95, 0)
    free = [model.generate_topk(p, u, (last,), *args) for p, u in zip(prompts, us)]
    assert all(len(f) == n_new for f in free) and len({tuple(f) for f in free}) == 6
    assert model.generate_topk(prompts[2], us[3], (last,), *args) != free[2]          # another uniform row, other ids
    stops = (free[1][5], free[4][11])
    solo = [model.generate_topk(p, u, stops, *args) for p, u in zip(prompts, us)]
    assert len(solo[1]) <= 5 and len(solo[4]) <= 11 and len({len(s) for s in solo}) >= 2, [len(s) for s in solo]
    for b, s in enumerate(solo):
        k = next((i for i, t in enumerate(free[b]) if t in stops), n_new)
        assert s == free[b][:k], b
    assert model.generate_topk_batch(prompts, us, stops, *args) == solo
    assert model.generate_topk_batch(prompts[:2], us[:2], stops, *args) == solo[:2]   # a smaller batch on the same state
    assert model.generate_topk_batch(prompts, us, (last,), *args) == free
    model.close()


def test_errors_leave_the_handle_usable(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    INV, UNS = m._lib.ERR_INVALID_ARGUMENT, m._lib.ERR_UNSUPPORTED
    cfg, w, prompt = _case("qwen3-micro", 53)
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    us = np.random.default_rng(2).random(64).astype(np.float32)
    last = cfg.vocab - 1

    def gen(p=prompt, stops=(last,), n=6, t=0.8, top_p=0.95, k=0):
        return model.generate_topk(p, us[:max(n, 1)] if n <= 64 else np.zeros(n, np.float32), stops, n, t, top_p, k)

    good = gen()
    assert len(good) == 6
    bad = [(dict(t=0.0), INV), (dict(t=-0.5), INV), (dict(t=float("nan")), INV), (dict(t=float("inf")), INV),
           (dict(top_p=0.0), INV), (dict(top_p=-1.0), INV), (dict(top_p=float("nan")), INV), (dict(top_p=float("inf")), INV),
           (dict(k=-1), INV), (dict(k=1025), UNS), (dict(k=cfg.vocab), UNS),
           (dict(stops=()), INV), (dict(stops=(1, 2, 3, 4, 5)), INV), (dict(stops=(cfg.vocab,)), INV), (dict(stops=(-1,)), INV),
           (dict(n=cfg.max_ctx - prompt.shape[0] + 1), INV), (dict(n=0), INV), (dict(p=prompt[:0]), INV)]
    for kw, code in bad:
        with pytest.raises(m.MiaError) as e:
            gen(**kw)
        assert e.value.code == code, kw
        assert gen() == good
    with pytest.raises(m.MiaError) as e:
        model.generate_topk_batch([prompt, prompt], np.stack([us[:6], us[:6]]), (last,), 6, 0.8)        # 2 sequences on capacity 1
    assert e.value.code == INV
    # straight through the C ABI: null pointers, and an out_stride that cannot hold max_new_tokens ids
    lib = ctx.lib
    stop, out, n = np.array([last], np.int32), np.zeros(16, np.int32), np.zeros(2, np.int32)
    offs = np.array([0, prompt.shape[0]], np.int32)
    P, U = prompt.ctypes.data, us.ctypes.data
    assert lib.mia_lm_generate_topk(model.h, None, prompt.shape[0], 0.8, 0, 0.95, stop.ctypes.data, 1, 6, U, out.ctypes.data, n.ctypes.data) == INV
    assert lib.mia_lm_generate_topk(model.h, P, prompt.shape[0], 0.8, 0, 0.95, stop.ctypes.data, 1, 6, None, out.ctypes.data, n.ctypes.data) == INV
    assert lib.mia_lm_generate_topk_batch(model.h, P, offs.ctypes.data, 1, 0.8, 0, 0.95, stop.ctypes.data, 1, 6, U, out.ctypes.data, 5, n.ctypes.data) == INV
    assert lib.mia_lm_generate_topk_batch(model.h, P, offs.ctypes.data, 1, 0.8, 0, 0.95, stop.ctypes.data, 1, 6, U, out.ctypes.data, 6, n.ctypes.data) == 0
    assert out[:n[0]].tolist() == good
    model.close()
    # a CosyVoice2-style handle (speech_embedding / llm_decoder) has its own loop
    ccfg = S.LM_CONFIGS["qwen-micro"]
    cw = S.lm_weights(ccfg, seed=1, round_to="bf16")
    cw.update(S.qwen2lm_extra_weights(ccfg, 61, seed=0, round_to="bf16"))
    cosy = HL.CausalLM.load(ctx, ccfg, cw, m.BF16)
    x = (np.random.default_rng(1).standard_normal((5, ccfg.hidden)) * 0.3).astype(np.float32)
    with pytest.raises(m.MiaError) as e:
        cosy.generate_topk(x, us, (1,), 6, 0.8)
    assert e.value.code == INV
    cosy.close()


SOS, EOS = 2990, 2991
PROMPTS = ([5, 17, SOS, EOS, 256, 999], [42, SOS, EOS, 7, 7, 1500, 3])


def test_through_the_model(ctx):
    """FunASRModel.transcribe_tokens on the micro pipeline (sensevoice-micro + qwen3-micro256): temperature > 0 equals generate_topk on the
    same merged prompt, temperature 0 equals the call without the new arguments, a list of clips takes uniforms [n, max_tokens]."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import funasr, lm as HL
    scfg = funasr.SENSEVOICE_CONFIGS["sensevoice-micro"]
    enc = funasr.SenseVoiceEncoder.load(ctx, scfg, S.sensevoice_weights(scfg, seed=3, round_to="bf16"), m.BF16)
    lcfg = S.LM_CONFIGS["qwen3-micro256"]
    lw = S.lm_weights(lcfg, seed=4, round_to="bf16")
    lm = HL.CausalLM.load(ctx, lcfg, lw, m.BF16)
    lm.set_batch(2)
    dec = HL.FunASRDecoder(lm, lw["model.embed_tokens.weight"])
    model = funasr.FunASRModel(enc, dec)
    clips = [(S.synth_clip(i, n) + 0.01 * np.random.default_rng(70 + i).standard_normal(n)).astype(np.float32) for i, n in enumerate((16000, 23456))]
    stops = (lcfg.vocab - 1,)
    us = np.random.default_rng(9).random((2, 8)).astype(np.float32)
    solo = []
    for x, ids, u in zip(clips, PROMPTS, us):
        merged = dec.merge_embeddings(ids, model.encode_audio(x), SOS, EOS)
        want = lm.generate_topk(merged, u, stops, 8, 0.9, 0.95, 0)
        got = model.transcribe_tokens(x, ids, SOS, EOS, stops, 8, temperature=0.9, uniforms=u)
        assert len(want) == 8 and got == want
        assert model.transcribe_tokens(x, ids, SOS, EOS, stops, 8, temperature=0.9, top_p=0.95, top_k=1, uniforms=u) == lm.generate_greedy(merged, stops, 8)
        assert model.transcribe_tokens(x, ids, SOS, EOS, stops, 8, temperature=0.0) == model.transcribe_tokens(x, ids, SOS, EOS, stops, 8)
        assert model.transcribe_tokens(x, ids, SOS, EOS, stops, 8) == lm.generate_greedy(merged, stops, 8)
        solo.append(got)
    assert solo[0] != lm.generate_greedy(dec.merge_embeddings(PROMPTS[0], model.encode_audio(clips[0]), SOS, EOS), stops, 8)     # it does sample
    assert model.transcribe_tokens(list(clips), list(PROMPTS), SOS, EOS, stops, 8, temperature=0.9, uniforms=us) == solo
    with pytest.raises(ValueError):
        model.transcribe_tokens(clips[0], PROMPTS[0], SOS, EOS, stops, 8, temperature=0.9)
    with pytest.raises(ValueError):
        dec.transcribe_tokens(PROMPTS[0], model.encode_audio(clips[0]), SOS, EOS, stops, 8, temperature=0.9)
    lm.close(); enc.close()
