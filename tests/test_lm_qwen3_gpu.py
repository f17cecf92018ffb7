"""GPU parity of the Qwen3 decoder blocks (per-head q / k RMSNorm before RoPE, n_heads * head_dim != hidden) and of the greedy decode
from embedding rows (Fun-ASR's decoder loop) against the fp32 CPU reference of tests/_qwen3_ref.py, which tests/test_qwen3_ref.py pins
against transformers' Qwen3ForCausalLM.  Every model is a 2-layer micro checkpoint rounded to the handle's storage type.

Tolerances are the project's own (tests/test_lm_gpu.py): logits max |delta| <= 0.08 (bf16) / 0.015 (f16) of the logit standard deviation;
prompt pass against stepping 0.02; greedy ids exact, on prompts whose every step has an oracle top-2 margin of at least 0.03 (twice
the f16 tolerance: no logit error inside the tolerance can change the argmax).

Measured on an MI355X (max |delta| / std, forward of 10 ids then one step): bf16 0.022 / 0.018 (head_dim 64) and 0.031 / 0.033 (128), f16
0.0030 / 0.0028 and 0.0030 / 0.0039; with the scaled gains at most 0.058 (bf16) / 0.0034 (f16); prompt pass against stepping at most 0.017."""
import dataclasses
import functools

import numpy as np
import pytest

import _qwen3_ref as R
from mlx_swift_audio_amd import synthetic as S

pytestmark = pytest.mark.gpu

IDS = [5, 17, 256, 999, 2048, 3, 42, 7, 7, 1500]
TOL = {"bf16": 0.08, "f16": 0.015}


def _dt(name):
    import mlx_swift_audio_amd as m
    return m.BF16 if name == "bf16" else m.F16


def _scaled(w):
    """A checkpoint whose norm gains matter: q_norm of layer 0 times 4, k_norm of layer 1 times 0.25 (exact in 16 bit)."""
    w = dict(w)
    w["model.layers.0.self_attn.q_norm.weight"] = w["model.layers.0.self_attn.q_norm.weight"] * np.float32(4.0)
    w["model.layers.1.self_attn.k_norm.weight"] = w["model.layers.1.self_attn.k_norm.weight"] * np.float32(0.25)
    return w


@functools.lru_cache(maxsize=None)
def _logit_case(cfg_name, dtype_name, scaled=False):
    """(cfg, weights, oracle logits after IDS, oracle logits after one more id) -- computed once, shared, never written to."""
    cfg = S.LM_CONFIGS[cfg_name]
    w = S.lm_weights(cfg, seed=2, round_to=dtype_name)
    if scaled:
        w = _scaled(w)
    ora = R.Qwen3Oracle(cfg, w)
    ref = ora.forward(IDS).numpy()[-1]
    ref2 = ora.forward([11]).numpy()[-1]
    for a in (ref, ref2):
        a.setflags(write=False)
    return cfg, w, ref, ref2


def _check_forward(model, ref, ref2, dtype_name, label):
    got, nxt = model.forward(IDS), model.forward([11])        # 9 rows through the prompt pass + the step, then a step on the cache
    tol = TOL[dtype_name] * ref.std()
    d1, d2 = np.abs(got - ref).max(), np.abs(nxt - ref2).max()
    print(f"{label}: max |delta| / std = {d1 / ref.std():.4f} (10 ids), {d2 / ref.std():.4f} (next step); bound {TOL[dtype_name]}")
    assert d1 <= tol, (d1, tol)
    assert d2 <= tol, (d2, tol)


@pytest.mark.parametrize("cfg_name", ["qwen3-micro", "qwen3-micro128"])
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_forward_logits_match_oracle(ctx, cfg_name, dtype_name):
    """Fails on a build that ignores q_norm / k_norm: the logits then sit more than one standard deviation off."""
    from mlx_swift_audio_amd import lm as HL
    cfg, w, ref, ref2 = _logit_case(cfg_name, dtype_name)
    model = HL.CausalLM.load(ctx, cfg, w, _dt(dtype_name))
    _check_forward(model, ref, ref2, dtype_name, f"{cfg_name} {dtype_name}")
    model.reset()
    again = model.forward(IDS)
    model.reset()
    np.testing.assert_array_equal(model.forward(IDS), again)      # deterministic (fixed-order sums, no atomics)
    model.close()


def test_forward_logits_split_k_chain(ctx):
    """A capacity above 4 sequences takes the split-K + reduce / norm chain instead of the carried norm."""
    from mlx_swift_audio_amd import lm as HL
    cfg, w, ref, ref2 = _logit_case("qwen3-micro", "bf16")
    model = HL.CausalLM.load(ctx, cfg, w, _dt("bf16"))
    model.set_batch(6)
    _check_forward(model, ref, ref2, "bf16", "qwen3-micro bf16, capacity 6")
    model.close()


@pytest.mark.parametrize("cfg_name", ["qwen3-micro", "qwen3-micro128"])
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_norm_weights_matter(ctx, cfg_name, dtype_name):
    """q_norm of layer 0 scaled by 4 and k_norm of layer 1 by 0.25: a build that normalises but drops a gain, or swaps q and k, fails."""
    from mlx_swift_audio_amd import lm as HL
    cfg, w, ref, ref2 = _logit_case(cfg_name, dtype_name, True)
    plain = _logit_case(cfg_name, dtype_name)[2]
    assert np.abs(plain - ref).max() > 4 * TOL[dtype_name] * ref.std()       # the scaled gains do move the logits
    model = HL.CausalLM.load(ctx, cfg, w, _dt(dtype_name))
    _check_forward(model, ref, ref2, dtype_name, f"{cfg_name} {dtype_name} scaled gains")
    model.close()


@pytest.mark.parametrize("cfg_name", ["qwen3-micro", "qwen3-micro128"])
def test_prompt_pass_matches_stepping(ctx, cfg_name):
    """forward(40 ids) through the batched prompt pass (lm_rope_cache normalises q and k) against the same ids walked through the step
    (debug bit 1: the fused preamble of lm_attention normalises them)."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = S.LM_CONFIGS[cfg_name]
    w = S.lm_weights(cfg, seed=6, round_to="bf16")
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    ids = np.random.default_rng(40).integers(0, cfg.vocab, 40).tolist()
    batched, nxt_b = model.forward(ids), model.forward([9])
    model.reset()
    model.set_debug(2)
    stepped, nxt_s = model.forward(ids), model.forward([9])
    scale = stepped.std()
    print(cfg_name, "prompt pass vs stepping:", np.abs(batched - stepped).max() / scale, np.abs(nxt_b - nxt_s).max() / scale)
    assert np.abs(batched - stepped).max() <= 0.02 * scale
    assert np.abs(nxt_b - nxt_s).max() <= 0.02 * scale
    ref = R.Qwen3Oracle(cfg, w).forward(ids).numpy()[-1]
    assert np.abs(batched - ref).max() <= 0.08 * ref.std()
    model.close()


@functools.lru_cache(maxsize=None)
def _greedy_case(cfg_name, seed, n_new):
    """Untied head (tied random-init embeddings collapse a greedy run onto a handful of ids), f16-rounded weights, a prompt of 3 text
    rows + 9 random "audio" rows at the embedding's spread + 3 text rows.  Returns (cfg, weights, prompt rows, oracle ids, margins)."""
    cfg = dataclasses.replace(S.LM_CONFIGS[cfg_name], tie_embeddings=False)
    w = S.lm_weights(cfg, seed=seed, round_to="f16")
    emb = w["model.embed_tokens.weight"]
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, cfg.vocab, 6)
    audio = (rng.standard_normal((9, cfg.hidden)) * emb.std()).astype(np.float32)
    prompt = np.concatenate([emb[ids[:3]], audio, emb[ids[3:]]]).astype(np.float32)
    prompt.setflags(write=False)
    margins = []
    want = R.greedy(R.Qwen3Oracle(cfg, w), prompt, (cfg.vocab - 1,), n_new, margins)
    return cfg, w, prompt, tuple(want), tuple(margins)


# seeds chosen on the CPU so that the oracle's own top-2 margin is >= 0.03 of the logit std at each of the 24 steps (head_dim 64: seed 13,
# smallest margin 0.045, 24 distinct ids; head_dim 128: seed 127, 0.046, 19 distinct ids), and so that the 10th id is new at position 9
GREEDY_CASES = [("qwen3-micro", 13), ("qwen3-micro128", 127)]


@pytest.mark.parametrize("cfg_name,seed", GREEDY_CASES)
def test_greedy_ids_match_oracle(ctx, cfg_name, seed):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg, w, prompt, want, margins = _greedy_case(cfg_name, seed, 24)
    assert len(want) == 24 and min(margins) >= 0.03, min(margins)        # precondition, on the oracle alone: no step may be excused
    assert len(set(want)) >= 12
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    got = model.generate_greedy(prompt, (cfg.vocab - 1,), 24)
    assert got == list(want)
    assert model.generate_greedy(prompt, (cfg.vocab - 1,), 7) == list(want[:7])      # the budget
    model.close()


@pytest.mark.parametrize("cfg_name,seed", GREEDY_CASES)
def test_greedy_stop_id_ends_the_run_and_is_not_emitted(ctx, cfg_name, seed):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg, w, prompt, want, margins = _greedy_case(cfg_name, seed, 24)
    assert min(margins) >= 0.03
    stop = want[9]
    first = want.index(stop)
    assert first == 9                                                    # the seed's 10th id is new there
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    got = model.generate_greedy(prompt, (stop, cfg.vocab - 1), 24)
    assert len(got) == first and got == list(want[:first]) and stop not in got
    assert model.generate_greedy(prompt, (cfg.vocab - 1, want[0]), 24) == []         # a stop id as the first pick: nothing is emitted
    assert model.generate_greedy(prompt, (cfg.vocab - 1,), 24) == list(want)         # and the handle decodes on
    model.close()


def test_direct_launch_equals_graph(ctx):
    """Debug bit 0 launches every step's kernels directly: same kernels, same arguments, so logits and greedy ids are bit-identical."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg, w, prompt, want, _ = _greedy_case("qwen3-micro", 13, 24)
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    lg, ids = model.forward(IDS), model.generate_greedy(prompt, (cfg.vocab - 1,), 16)
    model.set_debug(1)
    model.reset()
    np.testing.assert_array_equal(model.forward(IDS), lg)
    assert model.generate_greedy(prompt, (cfg.vocab - 1,), 16) == ids == list(want[:16])
    model.close()


def test_greedy_batch_equals_single_runs(ctx):
    """Six prompts of 1 .. 40 rows side by side on a capacity-6 handle (the split-K chain): every sequence equals its own generate_greedy
    on the same capacity, the one-row prompt (no prompt-pass rows) and the sequences that stop at different steps included."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = dataclasses.replace(S.LM_CONFIGS["qwen3-micro"], tie_embeddings=False)
    w = S.lm_weights(cfg, seed=8, round_to="bf16")
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    model.set_batch(6)
    rng = np.random.default_rng(5)
    spread = w["model.embed_tokens.weight"].std()
    prompts = [(rng.standard_normal((n, cfg.hidden)) * spread).astype(np.float32) for n in (1, 3, 9, 17, 40, 12)]
    n_new = 20
    free = [model.generate_greedy(p, (cfg.vocab - 1,), n_new) for p in prompts]
    assert all(len(f) == n_new for f in free)
    stops = (free[1][5], free[4][11])                                    # sequences 1 and 4 stop early (others may, at their own step)
    solo = [model.generate_greedy(p, stops, n_new) for p in prompts]
    assert len(solo[1]) <= 5 and len(solo[4]) <= 11 and len({len(s) for s in solo}) >= 2, [len(s) for s in solo]
    for b, s in enumerate(solo):
        k = next((i for i, t in enumerate(free[b]) if t in stops), n_new)
        assert s == free[b][:k], b
    assert model.generate_greedy_batch(prompts, stops, n_new) == solo
    assert model.generate_greedy_batch(prompts[:2], stops, n_new) == solo[:2]        # a smaller batch on the same state
    assert model.generate_greedy_batch(prompts, (cfg.vocab - 1,), n_new) == free
    with pytest.raises(m.MiaError) as e:
        model.generate_greedy_batch(prompts + prompts[:1], stops, n_new)             # 7 sequences > set_batch(6)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.close()


def test_packed_step_with_qk_norm(ctx):
    """The packed 4-bit step (mia_lm_attach_quantized) replaces the GEMMs only and shares lm_attention's fused preamble, q / k norm
    included.  Dims: qwen3-micro128 widened to hidden 256, inter 512, 4 heads x 128 (n_heads * head_dim = 512), 2 kv heads -- every K a
    multiple of 128.  Tolerances as test_packed_step_matches_oracle_and_expanded_checkpoint (bf16)."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    from oracle import quant as OQ
    cfg = dataclasses.replace(S.LM_CONFIGS["qwen3-micro128"], hidden=256, inter=512, n_heads=4, n_kv_heads=2)
    w = S.lm_weights(cfg, seed=11)
    packed, dense = {}, dict(w)
    names = ["model.embed_tokens"]
    for l in range(cfg.n_layers):
        p = f"model.layers.{l}"
        names += [p + ".self_attn." + n + "_proj" for n in "qkvo"] + [p + ".mlp." + n + "_proj" for n in ("gate", "up", "down")]
    for n in names:
        pk, sc, bi = OQ.quantize_affine(w[n + ".weight"], 64, 4)
        sc, bi = sc.astype(np.float16), bi.astype(np.float16)
        packed[n + ".weight"], packed[n + ".scales"], packed[n + ".biases"] = pk, sc, bi
        dense[n + ".weight"] = OQ.dequantize_affine(pk, sc.astype(np.float32), bi.astype(np.float32), 64, 4)
    model = HL.CausalLM.load(ctx, cfg, dense, m.BF16)
    model.attach_q4(packed, bits=4)
    ids = np.random.default_rng(2).integers(0, cfg.vocab, 9).tolist()
    model.use_q4(False)
    ref_steps = [model.forward([t]).copy() for t in ids]                 # the 16-bit step of the same handle, token by token
    model.use_q4(True)
    model.reset()
    q_steps = [model.forward([t]).copy() for t in ids]
    ref = R.Qwen3Oracle(cfg, dense).forward(ids).numpy()
    for i, (got, want) in enumerate(zip(q_steps, ref_steps)):
        sd = ref[i].std()
        assert np.isfinite(got).all()
        assert np.abs(got - want).max() <= 0.06 * sd, (i, np.abs(got - want).max(), sd)
        assert np.abs(got - ref[i]).max() <= 0.08 * sd, (i, np.abs(got - ref[i]).max(), sd)
    model.close()


def test_errors_leave_the_handle_usable(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    INV, UNS = m._lib.ERR_INVALID_ARGUMENT, m._lib.ERR_UNSUPPORTED
    cfg, w, ref, _ = _logit_case("qwen3-micro", "bf16")
    qn, kn = "model.layers.%d.self_attn.q_norm.weight", "model.layers.%d.self_attn.k_norm.weight"

    def load_fails(weights, name):
        with pytest.raises(m.MiaError) as e:
            HL.CausalLM.load(ctx, cfg, weights, m.BF16)
        assert e.value.code == INV and name in str(e.value), str(e.value)

    load_fails({k: v for k, v in w.items() if k != kn % 1}, kn % 1)                          # one of a pair
    load_fails({k: v for k, v in w.items() if k not in (qn % 1, kn % 1)}, qn % 1)            # some layers only
    load_fails({**w, qn % 0: np.ones(cfg.head_dim + 1, np.float32)}, qn % 0)                 # wrong length
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)                                            # ... and a valid load follows
    logits = model.forward(IDS)
    assert np.abs(logits - ref).max() <= TOL["bf16"] * ref.std()

    def still_decodes():
        model.reset()
        np.testing.assert_array_equal(model.forward(IDS), logits)

    with pytest.raises(m.MiaError) as e:
        model.new_cache(quantized=True, bits=4)
    assert e.value.code == UNS
    still_decodes()
    model.new_cache(quantized=False)                                                         # bits 0 stays legal
    still_decodes()
    prompt = (np.random.default_rng(0).standard_normal((5, cfg.hidden)) * 0.3).astype(np.float32)
    good = model.generate_greedy(prompt, (1,), 6)
    bad_calls = [lambda: model.generate_greedy(prompt, (), 6),                               # n_stop = 0
                 lambda: model.generate_greedy(prompt, (1, 2, 3, 4, 5), 6),                  # n_stop = 5
                 lambda: model.generate_greedy(prompt, (cfg.vocab,), 6),                     # stop id outside the vocabulary
                 lambda: model.generate_greedy(prompt, (-1,), 6),
                 lambda: model.generate_greedy(prompt, (1,), cfg.max_ctx - 4),               # 5 rows + budget > max_ctx
                 lambda: model.generate_greedy(prompt, (1,), 0),
                 lambda: model.generate_greedy(prompt[:0], (1,), 6),                         # n_prompt = 0
                 lambda: model.generate_greedy_batch([prompt, prompt], (1,), 6)]             # 2 sequences on capacity 1
    for call in bad_calls:
        with pytest.raises(m.MiaError) as e:
            call()
        assert e.value.code == INV
        assert model.generate_greedy(prompt, (1,), 6) == good
    # straight through the C ABI: a null pointer, and an out_stride that cannot hold max_new_tokens ids
    lib = ctx.lib
    stop, out, n = np.array([1], np.int32), np.zeros(16, np.int32), np.zeros(2, np.int32)
    offs = np.array([0, 5], np.int32)
    assert lib.mia_lm_generate_greedy(model.h, None, 5, stop.ctypes.data, 1, 6, out.ctypes.data, n.ctypes.data) == INV
    assert lib.mia_lm_generate_greedy_batch(model.h, prompt.ctypes.data, offs.ctypes.data, 1, stop.ctypes.data, 1, 6, out.ctypes.data, 5, n.ctypes.data) == INV
    assert lib.mia_lm_generate_greedy_batch(model.h, prompt.ctypes.data, offs.ctypes.data, 1, stop.ctypes.data, 1, 6, out.ctypes.data, 6, n.ctypes.data) == 0
    assert out[:n[0]].tolist() == good
    model.close()
    # a CosyVoice2-style handle (speech_embedding / llm_decoder) has its own loop
    ccfg = S.LM_CONFIGS["qwen-micro"]
    cw = S.lm_weights(ccfg, seed=1, round_to="bf16")
    cw.update(S.qwen2lm_extra_weights(ccfg, 61, seed=0, round_to="bf16"))
    cosy = HL.CausalLM.load(ctx, ccfg, cw, m.BF16)
    x = (np.random.default_rng(1).standard_normal((5, ccfg.hidden)) * 0.3).astype(np.float32)
    with pytest.raises(m.MiaError) as e:
        cosy.generate_greedy(x, (1,), 6)
    assert e.value.code == INV
    u = np.random.default_rng(2).random(64).astype(np.float32)
    assert len(cosy.generate_ras(x, u, 2, 6, 61)) <= 6                                       # its own loop still runs
    cosy.close()
