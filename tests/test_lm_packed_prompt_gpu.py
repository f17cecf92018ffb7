"""The LM handle with its batched prompt pass on the packed weights (mia_lm_set_prompt_weights(lm, 1): csrc/gemm_quant.hip under
lm_prefill_rows) and with the 16-bit Linears released (mia_lm_release_dense), on the micro Llama / Qwen2 (q|k|v bias) configs that
tests/test_lm_gpu.py and tests/test_quant6_gpu.py pack, at 4, 6 and 8 bits.

Bounds (none taken from GPU output):
 * logits behind a packed prompt pass against the fp32 oracle on the de-quantised, UNROUNDED weights: the project's 16-bit LM tolerance,
   0.08 (bf16) / 0.015 (f16) of the logit std (tests/test_lm_gpu.py: test_forward_logits_match_oracle; LOGIT_TOL of test_lm_kvq_gpu.py) --
   the tighter of the bounds the packed tests carry, not the 0.02 f16 "behind the default prompt pass".  The same handle with the prompt
   walked through the packed step (debug bit 1) is held to the same bound as a control.
 * K/V rows of a packed prompt pass against the rows of the walked packed step: tests/test_lm_gpu.py compares prompt pass and step
   (test_batched_prompt_pass_matches_stepping: "same K/V rows up to fp32 summation order") at 0.02 of the spread of the compared
   quantity, and that is the tolerance here, on the rows themselves: 0.02 x std of the walked rows, per layer, K and V apart.  (The two
   paths round their activations to 16 bit at different points -- the step's fused chain stores x * gain before the division by the
   rms, the prompt pass after -- so the rows are one or two 16-bit roundings apart, not fp32 roundings: a float64-against-fp32 gap of
   the oracle, ~1e-6, says nothing about them.)
Measured on an MI355X 2026-10-21 (worst over the cases): logits 0.0378 (bf16) / 0.0037 (f16) of the std through the packed prompt pass,
0.0349 / 0.0037 walked; K/V rows 505..519: f16 0.0000 x std at layer 0 (bit-equal) and 0.0024 at layer 1, bf16 0.0020 at layer 0 and
0.0198 at layer 1 (llama-micro128, 4 bit: just inside the 0.02; every kernel on both paths sums in a fixed order, so the figure repeats)."""
import dataclasses

import numpy as np
import pytest

import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import lm as HL
from mlx_swift_audio_amd import synthetic as S
from oracle import lm as OL
from test_lm_gpu import _quantized_checkpoint
from test_quant6_gpu import _quantized_checkpoint6

pytestmark = pytest.mark.gpu

LOGIT_TOL = {"bf16": 0.08, "f16": 0.015}
KV_TOL = 0.02
CASES = [(c, d, b) for (c, d) in (("llama-micro128", "bf16"), ("qwen-micro", "f16")) for b in (4, 6, 8)]


def _dt(name):
    return m.BF16 if name == "bf16" else m.F16


def _checkpoint(cfg, bits, seed=11):
    return _quantized_checkpoint6(cfg, seed) if bits == 6 else _quantized_checkpoint(cfg, seed, bits=bits)


def _load(ctx, cfg_name, dtype_name, bits, max_ctx=None, attach=True):
    cfg = S.LM_CONFIGS[cfg_name]
    if max_ctx:
        cfg = dataclasses.replace(cfg, max_ctx=max_ctx)
    packed, dense = _checkpoint(cfg, bits)
    model = HL.CausalLM.load(ctx, cfg, dense, _dt(dtype_name))
    if attach:
        model.attach_q4(packed, bits=bits)
    return cfg, dense, model


@pytest.mark.parametrize("cfg_name,dtype_name,bits", CASES)
def test_logits_behind_a_packed_prompt_meet_the_step_bound(ctx, cfg_name, dtype_name, bits):
    cfg, dense, model = _load(ctx, cfg_name, dtype_name, bits)
    ids = np.random.default_rng(40 + bits).integers(0, cfg.vocab, 41).tolist()      # 40 rows through the prompt pass, the last through the step
    ora = OL.LMOracle(cfg, dense)
    want = [ora.forward(ids).numpy()[-1], ora.forward([9]).numpy()[-1]]
    tol = LOGIT_TOL[dtype_name]

    def run():
        model.reset()
        return [model.forward(ids).copy(), model.forward([9]).copy()]

    default = run()                                  # the default: prompt rows on the 16-bit copy
    model.set_prompt_weights(True)
    packed = run()
    model.set_debug(2)                               # control: the prompt walked through the packed step
    walked = run()
    model.set_debug(0)
    for name, got in (("packed prompt pass", packed), ("walked", walked)):
        for i in range(2):
            e = np.abs(got[i] - want[i]).max() / want[i].std()
            print(f"{cfg_name} {dtype_name} q{bits} {name} step {i}: {e:.4f} of the logit std (bound {tol})")
            assert np.isfinite(got[i]).all() and e <= tol, (name, i, e)
    assert not np.array_equal(packed[0], default[0])          # the mode does reach the prompt pass
    # mode 0 after mode 1: bit-identical to a handle that never switched
    model.set_prompt_weights(False)
    again = run()
    assert np.array_equal(again[0], default[0]) and np.array_equal(again[1], default[1])
    model.close()


@pytest.mark.parametrize("cfg_name,dtype_name,bits", [("llama-micro128", "bf16", 4), ("qwen-micro", "f16", 6), ("qwen-micro", "f16", 8)])
def test_kv_rows_across_the_chunk_boundary_agree_with_the_walked_step(ctx, cfg_name, dtype_name, bits):
    """521 ids: 520 prompt-pass rows = one chunk of 512 and one of 8; rows 505..519 straddle the boundary"""
    cfg, dense, model = _load(ctx, cfg_name, dtype_name, bits, max_ctx=1024)
    ids = np.random.default_rng(520 + bits).integers(0, cfg.vocab, 521).tolist()
    model.set_prompt_weights(True)
    model.forward(ids)
    got = [model.read_kv(l, 0, 505, 15) for l in range(cfg.n_layers)]
    model.reset()
    model.set_debug(2)
    model.forward(ids)
    want = [model.read_kv(l, 0, 505, 15) for l in range(cfg.n_layers)]
    for l in range(cfg.n_layers):
        for name, g, w in (("k", got[l][0], want[l][0]), ("v", got[l][1], want[l][1])):
            e = np.abs(g - w).max() / w.std()
            print(f"{cfg_name} {dtype_name} q{bits} layer {l} {name}: {e:.5f} x std (bound {KV_TOL})")
            assert np.isfinite(g).all() and w.std() > 0 and e <= KV_TOL, (l, name, e)
    model.close()


def _embeds(dense, ids):
    return dense["model.embed_tokens.weight"][np.asarray(ids)].astype(np.float32)


@pytest.mark.parametrize("cfg_name,dtype_name,bits", [("llama-micro128", "bf16", 6), ("qwen-micro", "f16", 4)])
def test_two_prompts_side_by_side_equal_their_single_calls(ctx, cfg_name, dtype_name, bits):
    cfg, dense, model = _load(ctx, cfg_name, dtype_name, bits)
    model.set_prompt_weights(True)
    rng = np.random.default_rng(7)
    prompts = [_embeds(dense, rng.integers(0, cfg.vocab, n)) for n in (40, 23)]
    model.set_batch(2)
    both = model.generate_greedy_batch(prompts, (cfg.vocab - 1,), 8)
    for b in range(2):
        assert model.generate_greedy(prompts[b], (cfg.vocab - 1,), 8) == both[b], b
    assert all(len(x) > 0 for x in both)
    model.close()


def _greedy_margin(cfg, dense, ids, n_new):
    """the oracle's greedy run from embedding rows: (ids, smallest top-1 margin / logit std over the steps)"""
    ora = OL.LMOracle(cfg, dense)
    emb = ora.w["model.embed_tokens.weight"]
    head = emb if cfg.tie_embeddings else ora.w["lm_head.weight"]
    x, out, worst = emb[np.asarray(ids)], [], np.inf
    for _ in range(n_new):
        lg = (ora.hidden(x)[-1] @ head.t()).numpy()
        top = np.sort(lg)[-2:]
        worst = min(worst, float(top[1] - top[0]) / float(lg.std()))
        out.append(int(lg.argmax()))
        x = emb[np.asarray(out[-1:])]
    return out, worst


def test_quantised_kv_cache_takes_the_packed_prompt_pass(ctx):
    """new_cache(quantized=True, bits=8): the packed prompt pass feeds the cache quantiser; ids equal the walked prompt's.  Each run is a
    perturbation of the oracle's logits; the prompt is the first (searched on the CPU, on the oracle alone) whose top-1 margin at every
    step is more than twice 0.08 of the logit std, the loosest logit bound the project's LM tests carry."""
    cfg_name, dtype_name, bits, n_new = "qwen-micro", "f16", 4, 4
    cfg = S.LM_CONFIGS[cfg_name]
    _, dense = _checkpoint(cfg, bits)
    ids, want, margin = None, None, 0.0
    for seed in range(200):
        cand = np.random.default_rng(9000 + seed).integers(0, cfg.vocab - 1, 40).tolist()
        w, mg = _greedy_margin(cfg, dense, cand, n_new)
        if mg > 2 * 0.08 and cfg.vocab - 1 not in w:
            ids, want, margin = cand, w, mg
            break
    assert ids is not None and margin > 2 * 0.08, "no prompt with a safe margin among 200 seeds"
    print(f"prompt seed {seed}: smallest top-1 margin {margin:.3f} of the logit std")
    cfg, dense, model = _load(ctx, cfg_name, dtype_name, bits)
    model.new_cache(quantized=True, bits=8)
    model.set_prompt_weights(True)
    got = model.generate_greedy(_embeds(dense, ids), (cfg.vocab - 1,), n_new)
    model.set_debug(2)
    walked = model.generate_greedy(_embeds(dense, ids), (cfg.vocab - 1,), n_new)
    assert got == walked == want, (got, walked, want)
    model.close()


def test_mode_1_needs_attached_weights(ctx):
    cfg, dense, model = _load(ctx, "llama-micro128", "bf16", 4, attach=False)
    for call in (lambda: model.set_prompt_weights(True), model.release_dense):
        with pytest.raises(m.MiaError) as e:
            call()
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.set_prompt_weights(False)                  # the default is always accepted
    dense_b, packed_b = model.weight_bytes()
    assert packed_b == 0 and dense_b > 0
    model.close()


@pytest.mark.parametrize("cfg_name,dtype_name,bits", [("llama-micro128", "bf16", 8), ("qwen-micro", "f16", 6)])
def test_release_dense(ctx, cfg_name, dtype_name, bits):
    cfg, dense, model = _load(ctx, cfg_name, dtype_name, bits)
    rng = np.random.default_rng(3)
    ids = rng.integers(0, cfg.vocab, 40).tolist()
    u = rng.random(12).astype(np.float32)
    kw = dict(temperature=0.7, top_p=0.9, rep_penalty=1.2, rep_window=16, max_new_tokens=12, stop_ids=(cfg.vocab - 1,))
    model.set_prompt_weights(True)
    model.use_q4(True)
    before = model.generate(ids, u, **kw)
    d0, q0 = model.weight_bytes()
    model.release_dense()
    d1, q1 = model.weight_bytes()
    D, Nq, Nk, inter = cfg.hidden, cfg.n_heads * cfg.head_dim, cfg.n_kv_heads * cfg.head_dim, cfg.inter
    pad16 = lambda n: (n + 15) // 16 * 16
    linears = [(Nq + 2 * Nk, D), (D, Nq), (2 * inter, D), (D, inter)]
    held = sum(N * K * 2 + pad16(N) * K * 2 for N, K in linears) * cfg.n_layers       # two copies each: row-major and fragment order
    assert d0 - d1 == held and q1 == q0 and q0 > 0, (d0, d1, held, q0, q1)
    print(f"{cfg_name} q{bits}: dense {d0} -> {d1} bytes, packed {q0}")
    assert model.generate(ids, u, **kw) == before
    for call in (lambda: model.use_q4(False), lambda: model.set_prompt_weights(False)):
        with pytest.raises(m.MiaError) as e:
            call()
        assert e.value.code == m._lib.ERR_UNSUPPORTED
    model.use_q4(True); model.set_prompt_weights(True); model.release_dense()          # what is already so stays accepted
    model.reset()
    assert model.generate(ids, u, **kw) == before
    model.set_batch(2)
    ub = np.stack([u, u])
    two = model.generate_batch([ids, ids[:17]], ub, **kw)
    model.set_batch(1)
    assert model.generate(ids[:17], u, **kw) == two[1]
    model.close()
