"""lm_step_attn_kvq.hip -- the decode step's split-key attention on the quantised KV cache's codes, shared across a KV group -- at the
operator (mia_op_lm_step_attention_kvq) against an fp64 softmax(q k^T dh^-0.5) v over the rows read back by tests/_kvq_rule.py, and in
the model (CausalLM.set_kvq_step_attention(1)) against the oracle attending over the device's own rows, mode 0's quantiser bits, the
batch == single contract and the switch's hygiene.

Lengths and heads are test_lm_step_attn_gpu.py's (MFMA tile, wave and slice edges, the new row alone in a slice, a multi-slice tail);
inputs carry one outlier channel per 64-group (K + 9, V - 7), so the bias terms dominate the scale terms.  Bound per element, the one
lm_prefill_attn_kvq.hip is held to for the same reasons: 1 ulp of the output type at the output's magnitude + rel * max(max|dq(V)|,
R_V), rel = 2^-8 (bf16) | 2^-11 (f16), R_V = the largest max - min of a 64-group of the rounded V rows.  The model's bounds are
test_lm_kvq_gpu.py's: logits within LOGIT_TOL of the forced-cache oracle, every new K/V row within 0.5 scale + d.

Measured on the MI355X (worst error / bound over a case's lengths): mode 1 bf16 0.17 .. 0.26, f16 0.18 .. 0.28 over all heads, head dims
and bit widths; mode 0 0.13 .. 0.29; ramp and spike 0.10 .. 0.19.  Model, mode 1 with p * scale_V as a hi + lo pair: new rows at most
0.90 .. 0.99 (4 bit), 0.57 .. 0.90 (8 bit) of 0.5 scale + d, logits 0.009 .. 0.021 sigma."""
import dataclasses

import numpy as np
import pytest

import _kvq_rule as R
from mlx_swift_audio_amd import synthetic as S
from test_lm_kvq_gpu import CONFIGS, LOGIT_TOL, _check_logits_and_new_rows, _load, _weights      # noqa: F401  (LOGIT_TOL: the bound _check_logits_and_new_rows applies)
from test_lm_prompt_attn_gpu import _bound, _kinds
from test_lm_step_attn_gpu import HEADS, LENGTHS

pytestmark = pytest.mark.gpu


def _data(seed, T, Hq, Hkv, dh):
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal(s).astype(np.float32) for s in ((Hq, dh), (Hkv, T, dh), (Hkv, T, dh)))
    for g in range(dh // 64):
        k[:, :, 64 * g + 7 + g] += np.float32(9.0)
        v[:, :, 64 * g + 21 + g] -= np.float32(7.0)
    return q, k, v


def _ratio(ctx, q, k, v, bits, kind, mode):
    """worst |error| / bound of one operator call against fp64 over the rows the cache reads back (q rounded to `kind`)"""
    from mlx_swift_audio_amd import ops
    dtype, rel, mant = _kinds()[kind]
    got = ops.lm_step_attention_kvq(ctx, q, k, v, bits=bits, mode=mode, dtype=dtype)
    qd = S.round_array(q, kind).astype(np.float64)
    kd, vd = R.dq_rows(k, bits, kind).astype(np.float64), R.dq_rows(v, bits, kind).astype(np.float64)
    (Hq, dh), (Hkv, T, _) = q.shape, k.shape
    ref = np.zeros((Hq, dh))
    for h in range(Hq):
        s = kd[h // (Hq // Hkv)] @ qd[h] * dh ** -0.5
        p = np.exp(s - s.max())
        ref[h] = (p / p.sum()) @ vd[h // (Hq // Hkv)]
    g = S.round_array(v, kind).reshape(Hkv, T, dh // 64, 64)
    vterm = max(float(np.abs(vd).max()), float((g.max(-1) - g.min(-1)).max()))
    assert np.isfinite(got).all()
    return float((np.abs(got - ref) / _bound(ref, got, vterm, rel, mant)).max())


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_kvq_split_step_attention_matches_reference(ctx, heads, dh, bits, kind):
    worst = {T: _ratio(ctx, *_data(1000 * T + 10 * heads[0] + dh, T, *heads, dh), bits, kind, 1) for T in LENGTHS}
    print(f"lm_step_attention_kvq mode 1 {kind} q{bits} dh={dh} heads={heads}: worst err/bound {max(worst.values()):.3f} (T={max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("heads", [(4, 2), (3, 1)])
@pytest.mark.parametrize("T", [2, 65, 257])
def test_kvq_mode0_through_the_same_operator(ctx, T, heads, bits):
    """lm_kvq_attention's fused form keeps P in fp32 and de-quantises on the vector pipe: inside the same bound."""
    for dh, kind in ((64, "bf16"), (128, "f16")):
        r = _ratio(ctx, *_data(50 + T + dh, T, *heads, dh), bits, kind, 0)
        print(f"lm_step_attention_kvq mode 0 {kind} q{bits} dh={dh} heads={heads} T={T}: worst err/bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("spike_at", ["last", "first"])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dh", [64, 128])
def test_kvq_rescale_and_merge_branches(ctx, dh, bits, kind, spike_at):
    """test_lm_step_attn_gpu.py's ramp and spike: scores of each group's first head ramp from 0 to 4 with the key index -- the maximum
    moves upward inside every wave, between the waves of a slice and between slices -- and one key scores 34: the new row, or key 0."""
    T, Hq, Hkv = 600, 4, 2
    q, k, v = _data(77 + dh, T, Hq, Hkv, dh)
    score = 4.0 * np.arange(T) / T
    score[T - 1 if spike_at == "last" else 0] = 34.0
    for j in range(Hkv):
        qh = S.round_array(q[2 * j], kind).astype(np.float64)
        k[j] = 0.05 * k[j] + np.outer(score * dh ** 0.5 / (qh @ qh), qh)
    r = _ratio(ctx, q, k, v, bits, kind, 1)
    print(f"lm_step_attention_kvq mode 1 {kind} q{bits} dh={dh} spike {spike_at}: worst err/bound {r:.3f}")
    assert r <= 1.0


CONTEXTS = (1, 2, 64, 65, 255, 256, 257, 513, 700)


def _steps(model, cfg):
    """per context n: forward(n ids), forward([11]) -> (the step's logits, layer 0's K and V rows [0, n])"""
    out = []
    for n in CONTEXTS:
        model.reset()
        model.forward(np.random.default_rng(n).integers(0, cfg.vocab, n).tolist())
        out.append((model.forward([11]),) + tuple(model.read_kv(0, 0, 0, n + 1)))
    return out


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("cfg_name", ["llama-micro", "llama-micro128", "qwen-micro"])
def test_kvq_mode1_model_against_forced_oracle_and_mode0_rows(ctx, cfg_name, bits):
    """Logits within LOGIT_TOL of the oracle over the device's rows and every new K/V row of every layer within 0.5 scale + d; layer 0's
    rows (they do not depend on attention) equal mode 0's bit for bit: the writer's quantiser; the captured graph equals direct launches."""
    cfg = CONFIGS[cfg_name]
    plain, quant = _load(ctx, cfg_name, "bf16"), _load(ctx, cfg_name, "bf16", bits)
    mode0 = _steps(quant, cfg)
    quant.set_kvq_step_attention(1)
    _check_logits_and_new_rows(plain, quant, R.ForcedCacheOracle(cfg, _weights(cfg_name, "bf16")), cfg, "bf16", bits, CONTEXTS)
    graph = _steps(quant, cfg)
    for a, b in zip(graph, mode0):
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    quant.set_debug(1)
    for a, b in zip(_steps(quant, cfg), graph):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    plain.close()
    quant.close()


@pytest.mark.parametrize("bits", [4, 8])
def test_kvq_mode1_batch_hygiene_and_errors(ctx, bits):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    from mlx_swift_audio_amd import ops
    cfg = CONFIGS["llama-micro"]
    model = _load(ctx, "llama-micro", "bf16")
    rng = np.random.default_rng(3)
    ids, u = rng.integers(0, cfg.vocab - 1, 260).tolist(), rng.random(16).astype(np.float32)

    def run():
        gen = model.generate(ids, u, max_new_tokens=16, stop_ids=(cfg.vocab - 1,))
        model.reset()
        return gen, model.forward(ids), model.forward([7])

    def same(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])

    plain = run()
    model.new_cache(quantized=True, bits=bits)
    off = run()
    model.set_kvq_step_attention(1)
    run()
    model.set_kvq_step_attention(0)
    assert same(run(), off)
    model.set_kvq_step_attention(1)
    model.new_cache(quantized=False)                 # the 16-bit cache keeps its own step kernel whatever this switch says
    assert same(run(), plain)
    with pytest.raises(m.MiaError) as e:
        model.set_kvq_step_attention(2)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.set_batch(4)                               # the workspace follows the capacity and the cache mode
    model.new_cache(quantized=True, bits=bits)
    prompts = [rng.integers(0, cfg.vocab - 1, n).tolist() for n in (9, 70, 255, 300)]
    ub = rng.random((4, 24)).astype(np.float32)
    kw = dict(temperature=0.8, top_p=0.9, rep_penalty=1.2, rep_window=16, max_new_tokens=24, stop_ids=(cfg.vocab - 1,))
    both = model.generate_batch(prompts, ub, **kw)
    for b, p in enumerate(prompts):
        assert model.generate(p, ub[b], **kw) == both[b], b
    model.close()
    wcfg = dataclasses.replace(cfg, n_heads=17, n_kv_heads=1)
    wide = HL.CausalLM.load(ctx, wcfg, S.lm_weights(wcfg, seed=6, round_to="bf16"), m.BF16)
    with pytest.raises(m.MiaError, match="at most 16 query heads") as e:
        wide.set_kvq_step_attention(1)
    assert e.value.code == m._lib.ERR_UNSUPPORTED
    wide.close()
    with pytest.raises(m.MiaError):
        ops.lm_step_attention_kvq(ctx, np.zeros((4, 96), np.float32), np.zeros((2, 3, 96), np.float32), np.zeros((2, 3, 96), np.float32), bits=bits)
