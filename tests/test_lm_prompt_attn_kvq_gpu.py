"""lm_prefill_attn_kvq.hip -- the prompt pass's tiled causal GQA attention on the quantised KV cache's codes -- at the operator
(mia_op_lm_prompt_attention_kvq) against an fp64 softmax(q k^T dh^-0.5, causal) v over the rows read back by tests/_kvq_rule.py, and in
the model (CausalLM.set_kvq_prompt_attention(1)) against the oracle attending over the device's own rows.

Lengths, heads and the ulp term are test_lm_prompt_attn_gpu.py's.  Inputs carry one outlier channel per 64-group (K + 9, V - 7, as in
test_lm_kvq_gpu.py), so the bias terms are large against the scale terms.  Bound per element: 1 ulp of the output type at the output's
magnitude + rel * max(max|dq(V)|, R_V), rel = 2^-8 (bf16) | 2^-11 (f16), R_V = the largest max - min of a 64-group of the rounded V rows:
p * scale_V is rounded to the 16-bit type (relative half-spacing 2^-9 | 2^-12) and multiplies a code with scale * code <= max - min, sum p
= 1, times the factor 2 the 16-bit kernel's bound keeps.  The scores are exact products in fp32 sums and get no term of their own.

Measured on the MI355X (worst error / bound over a case's lengths): bf16 0.253 .. 0.285, f16 0.223 .. 0.289 over all heads, head dims and
bit widths; the spiked case 0.191 .. 0.192 (dh 64), 0.268 .. 0.274 (dh 128).  Model, mode 1: K/V rows at most 0.72 .. 0.98 of 0.5 scale
+ d (d 0.021 .. 0.024; the row kernel on the same prompts: 0.71 .. 0.98), logits 0.013 .. 0.025 sigma."""
import dataclasses

import numpy as np
import pytest

import _kvq_rule as R
from mlx_swift_audio_amd import synthetic as S
from test_lm_kvq_gpu import LOGIT_TOL
from test_lm_prompt_attn_gpu import EDGES, HEADS, KEY_TILE, _bound, _kinds, _qtile

pytestmark = pytest.mark.gpu


def _data(seed, T, n, Hq, Hkv, dh):
    rng = np.random.default_rng(seed)
    q, k, v = (rng.standard_normal(s).astype(np.float32) for s in ((n, Hq, dh), (Hkv, T, dh), (Hkv, T, dh)))
    for g in range(dh // 64):
        k[:, :, 64 * g + 7 + g] += np.float32(9.0)
        v[:, :, 64 * g + 21 + g] -= np.float32(7.0)
    return q, k, v


def _ref(q, k, v, bits, kind):
    """fp64 causal attention of q (rounded to `kind`) at positions T - n .. T - 1 over the rows the cache reads back; the bound's V term"""
    q = S.round_array(q, kind).astype(np.float64)
    kd, vd = R.dq_rows(k, bits, kind).astype(np.float64), R.dq_rows(v, bits, kind).astype(np.float64)
    n, Hq, dh = q.shape
    Hkv, T, _ = k.shape
    out = np.zeros((n, Hq, dh))
    mask = np.arange(T)[None, :] > np.arange(T - n, T)[:, None]
    for h in range(Hq):
        kv = h // (Hq // Hkv)
        s = q[:, h] @ kd[kv].T * dh ** -0.5
        s[mask] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h] = (p / p.sum(axis=1, keepdims=True)) @ vd[kv]
    g = S.round_array(v, kind).reshape(Hkv, T, dh // 64, 64)
    return out, max(float(np.abs(vd).max()), float((g.max(-1) - g.min(-1)).max())), vd


def _check(ctx, q, k, v, bits, kind):
    """worst err / bound, asserted <= 1"""
    from mlx_swift_audio_amd import ops
    dtype, rel, mant = _kinds()[kind]
    got = ops.lm_prompt_attention_kvq(ctx, q, k, v, bits=bits, dtype=dtype)
    ref, vterm, _ = _ref(q, k, v, bits, kind)
    ratio = float((np.abs(got - ref) / _bound(ref, got, vterm, rel, mant)).max())
    assert ratio <= 1.0, (q.shape, k.shape, ratio)
    return got, ratio


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_kvq_prompt_attention_matches_reference(ctx, heads, dh, bits, kind):
    """n = T over every edge length, then n < T: one row behind a full key tile, and a query tile + 1 rows behind 100 cached keys."""
    Hq, Hkv = heads
    qt = _qtile(Hq, Hkv)
    worst = 0.0
    for T, n in [(T, T) for T in EDGES] + [(KEY_TILE + 1, 1), (100 + qt + 1, qt + 1)]:
        q, k, v = _data(1000 * T + 10 * Hq + dh + n, T, n, Hq, Hkv, dh)
        worst = max(worst, _check(ctx, q, k, v, bits, kind)[1])
    print(f"lm_prompt_attention_kvq {kind} q{bits} dh={dh} Hq={Hq} Hkv={Hkv}: worst err/bound {worst:.3f}")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dh", [64, 128])
def test_kvq_prompt_attention_rescale_branch(ctx, dh, bits, kind):
    """test_prompt_attention_rescale_branch's spikes: key 150 = 8 x query 170 and key 70 = 8 x query 100 move the running maximum after
    the first tile; key 180 = 8 x query 5 lies above position 5 and must have no effect there."""
    T, Hq, Hkv = 193, 4, 2
    q, k, v = _data(7, T, T, Hq, Hkv, dh)
    k[:, 150] = 8.0 * q[170, ::2]
    k[:, 70] = 8.0 * q[100, ::2]
    k[:, 180] = 8.0 * q[5, ::2]
    got, ratio = _check(ctx, q, k, v, bits, kind)
    print(f"lm_prompt_attention_kvq {kind} q{bits} dh={dh} spiked: worst err/bound {ratio:.3f}")
    ref, _, vd = _ref(q, k, v, bits, kind)
    assert np.abs(ref[170, 0] - vd[0, 150]).max() < 0.05
    assert np.abs(got[5, 0] - vd[0, 180]).max() > 0.5


@pytest.mark.parametrize("bits,dh,kind", [(4, 64, "bf16"), (8, 128, "f16")])
def test_kvq_prompt_attention_row_independence(ctx, bits, dh, kind):
    from mlx_swift_audio_amd import ops
    Hq, Hkv = 4, 2
    qt = _qtile(Hq, Hkv)
    T = 2 * qt + 37
    q, k, v = _data(23, T, T, Hq, Hkv, dh)
    kw = dict(bits=bits, dtype=_kinds()[kind][0])
    full = ops.lm_prompt_attention_kvq(ctx, q, k, v, **kw)
    assert np.array_equal(full, ops.lm_prompt_attention_kvq(ctx, q, k, v, **kw))
    for n in (1, 37, qt + 1):
        assert np.array_equal(full[T - n:], ops.lm_prompt_attention_kvq(ctx, q[T - n:], k, v, **kw)), n


def _load(ctx, cfg, w, bits=0, mode=0):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    if bits:
        model.new_cache(quantized=True, bits=bits)
    model.set_kvq_prompt_attention(mode)
    return model


def _rows_against_oracle(model, ora, cfg, ids):
    """forward(ids): per layer and K / V, (device rows, the oracle's own un-quantised rows over the device's rows) [Hkv, n, dh]; the
    last-position logits and the next step's, each with step_logits over the device's rows"""
    import torch
    n, t = len(ids), 11
    model.reset()
    got = model.forward(ids)
    cache = [model.read_kv(l, 0, 0, n) for l in range(cfg.n_layers)]
    ora.offset = 0
    _, own = ora.hidden(ora.w["model.embed_tokens.weight"][torch.as_tensor(ids)], cache)
    nxt = model.forward([t])
    cache1 = [model.read_kv(l, 0, 0, n + 1) for l in range(cfg.n_layers)]
    logits = [(got, ora.step_logits(ids[-1], n - 1, cache)[0]), (nxt, ora.step_logits(t, n, cache1)[0])]
    return [(cache[l][i], own[l][i]) for l in range(cfg.n_layers) for i in (0, 1)], logits


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("cfg_name", ["llama-micro", "llama-micro128", "qwen-micro"])
def test_kvq_mode1_rows_and_logits_against_forced_oracle(ctx, cfg_name, bits):
    """Every K/V row the prompt pass writes (they depend on the new kernel's output from layer 1 on) within 0.5 scale + d of the oracle's
    own row, d = the largest deviation the 16-bit handle shows in the same procedure; logits within LOGIT_TOL of the oracle."""
    cfg = dataclasses.replace(S.LM_CONFIGS[cfg_name], max_ctx=1024)
    w = S.lm_weights(cfg, seed=2, round_to="bf16")
    plain, quant = _load(ctx, cfg, w), _load(ctx, cfg, w, bits, 1)
    ora = R.ForcedCacheOracle(cfg, w)
    prompts = [np.random.default_rng(n).integers(0, cfg.vocab, n).tolist() for n in (40, 131, 700)]
    d = max(float(np.abs(dev - own).max()) for ids in prompts for dev, own in _rows_against_oracle(plain, ora, cfg, ids)[0])
    for ids in prompts:
        rows, logits = _rows_against_oracle(quant, ora, cfg, ids)
        worst = 0.0
        for dev, own in rows:
            _, s, _ = R.quantise(S.round_array(own, "bf16"), bits, "bf16")
            delta = np.abs(dev - own).reshape(*s.shape, 64)
            worst = max(worst, float((delta / (0.5 * s[..., None] + d)).max()))
        errs = [float(np.abs(got - ref).max() / ref.std()) for got, ref in logits]
        print(f"kvq mode 1 {cfg_name} q{bits} n={len(ids)}: rows at most {worst:.3f} of 0.5 scale + d (d {d:.3e}); logits {errs[0]:.4f}, next {errs[1]:.4f} sigma")
        assert worst <= 1.0 and max(errs) <= LOGIT_TOL["bf16"], (len(ids), worst, errs)
    plain.close()
    quant.close()


@pytest.mark.parametrize("bits", [4, 8])
def test_kvq_mode1_batch_switch_back_and_errors(ctx, bits):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    cfg = dataclasses.replace(S.LM_CONFIGS["llama-micro"], max_ctx=1024)
    w = S.lm_weights(cfg, seed=8, round_to="bf16")
    rng = np.random.default_rng(31)
    ids = rng.integers(0, cfg.vocab, 90).tolist()
    never = _load(ctx, cfg, w, bits)
    want = never.forward(ids)
    never.close()
    model = _load(ctx, cfg, w, bits, 1)
    assert not np.array_equal(model.forward(ids), want)          # (the switch was really on)
    model.set_kvq_prompt_attention(0)
    model.reset()
    assert np.array_equal(model.forward(ids), want)
    with pytest.raises(m.MiaError) as e:
        model.set_kvq_prompt_attention(2)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    # four prompts, 579 rows: the 512-row chunk boundary falls inside the last one
    model.set_batch(4)
    model.set_kvq_prompt_attention(1)
    prompts = [rng.integers(0, cfg.vocab - 1, n).tolist() for n in (9, 70, 200, 300)]
    u = rng.random((4, 24)).astype(np.float32)
    kw = dict(temperature=0.8, top_p=0.9, rep_penalty=1.2, rep_window=16, max_new_tokens=24, stop_ids=(cfg.vocab - 1,))
    both = model.generate_batch(prompts, u, **kw)
    for b, p in enumerate(prompts):
        assert model.generate(p, u[b], **kw) == both[b], b
    model.close()
    z = np.zeros((2, 2, 64), np.float32)
    for q, k in ((np.zeros((2, 4, 96), np.float32), np.zeros((2, 2, 96), np.float32)), (np.zeros((2, 3, 64), np.float32), z)):      # head dim 96; Hq % Hkv != 0
        with pytest.raises(m.MiaError):
            ops.lm_prompt_attention_kvq(ctx, q, k, k, bits=bits)
