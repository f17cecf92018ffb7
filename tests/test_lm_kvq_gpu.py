"""GPU: the LM's quantised KV cache (mia_lm_set_kv_quant / CausalLM.new_cache(quantized=True): QuantizedKVCache(groupSize: 64, bits: 4 | 8),
TransformerBlock.swift:182-201) against the rule in tests/_kvq_rule.py.

What is compared with what:
  * the kernel alone (mia_op_kvq_attention) against float64 softmax attention over the helper's de-quantised rows of the same inputs;
  * the quantiser bit for bit: layer 0's K/V rows do not depend on the cache, so the quantised handle's read_kv(0, ...) must equal the
    helper's dq(quantise(.)) of the 16-bit handle's rows;
  * logits with the DEVICE's own cache rows forced into the oracle (both sides attend over the same rows, so no quantisation flip enters
    and the project's 16-bit LM tolerances apply: 0.08 std bf16, 0.015 std f16) -- never against an oracle that quantises its own K/V:
    a 16-bit pre-rounding of K/V alone moves 4-bit logits by 0.2 - 0.5 std on these random-init configs;
  * the new rows of deeper layers against the oracle's own un-quantised rows, within half a quantisation step plus the 16-bit path's own
    error measured in the same test;
  * invariants (batch == solo, reset, back to the 16-bit cache, packed weights, RAS) bit for bit."""
import dataclasses
import functools

import numpy as np
import pytest

import _kvq_rule as R
from mlx_swift_audio_amd import synthetic as S
from mlx_swift_audio_amd.synthetic import round_array
from oracle import lm as OL

pytestmark = pytest.mark.gpu

# the three micro configs plus two non-power-of-two GQA ratios (Orpheus-3B: 24 / 8 = 3, Qwen2-0.5B: 14 / 2 = 7); max_ctx 1024 so the
# context lengths below fit
CONFIGS = {name: dataclasses.replace(S.LM_CONFIGS[name], max_ctx=1024) for name in ("llama-micro", "llama-micro128", "qwen-micro")}
CONFIGS["gqa3"] = S.LMConfig(3000, 384, 512, 2, 6, 2, 64, 1024)
CONFIGS["gqa7"] = dataclasses.replace(S.LM_CONFIGS["qwen-micro"], hidden=448, n_heads=14, n_kv_heads=2, head_dim=64, max_ctx=1024)
CFG_NAMES = list(CONFIGS)
# on and around the key loop's sweep (16 waves x keys per wave instruction x 4 = 512 keys at head_dim 64, 256 at 128) and the sub-wave edges
CONTEXTS = (1, 2, 9, 64, 65, 257, 513, 700)
LOGIT_TOL = {"bf16": 0.08, "f16": 0.015}      # x logit std: the project's LM tolerances (tests/test_lm_gpu.py)


def _dt(name):
    import mlx_swift_audio_amd as m
    return m.BF16 if name == "bf16" else m.F16


@functools.lru_cache(maxsize=None)
def _weights(cfg_name, dtype_name):
    return S.lm_weights(CONFIGS[cfg_name], seed=2, round_to=dtype_name)


def _load(ctx, cfg_name, dtype_name, bits=0):
    from mlx_swift_audio_amd import lm as HL
    model = HL.CausalLM.load(ctx, CONFIGS[cfg_name], _weights(cfg_name, dtype_name), _dt(dtype_name))
    if bits:
        model.new_cache(quantized=True, bits=bits)
    return model


def _ids(cfg, n, seed=0):
    return np.random.default_rng(1000 * seed + n).integers(0, cfg.vocab, n).tolist()


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
# Bound: |out - ref| <= r * |ref| + a * max|dq(V)|.
# r: the kernel computes in fp32 and rounds ONCE, its output, to the 16-bit type (RNE): half a spacing = 2^-8 relative for bf16 (7 stored
#    mantissa bits), 2^-11 for f16 (10).
# a: measured with this test's own inputs and reference at bits = 0, which runs the 16-bit cache's kernels (lm_rope_cache + lm_attention,
#    untouched by the quantised cache): largest |out - ref| / max|V| over every shape and context length below was
#        bf16  3.41e-3      f16  3.67e-4          (test_kernel_alone_16bit_yardstick prints them)
#    and a is twice that, because the packed path has one more fp32 multiply-add per element (scale * code + bias).
R_REL = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
A_MEASURED = {"bf16": 3.41e-3, "f16": 3.67e-4}
A_ABS = {k: 2.0 * v for k, v in A_MEASURED.items()}
KERNEL_SHAPES = [(4, 2, 64), (2, 1, 128), (6, 2, 64), (14, 2, 64), (24, 8, 128)]      # (Hq, Hkv, dh): the five configs' GQA ratios + Orpheus' heads


def _kernel_inputs(Hq, Hkv, dh, T, dtype_name):
    rng = np.random.default_rng(Hq * 1000 + dh + T)
    q = rng.standard_normal((Hq, dh)).astype(np.float32)
    k = rng.standard_normal((Hkv, T, dh)).astype(np.float32)
    v = rng.standard_normal((Hkv, T, dh)).astype(np.float32)
    for g in range(dh // 64):                          # one outlier channel per group: it sets the group's range, as in trained K/V
        k[:, :, 64 * g + 7 + g] += np.float32(9.0)
        v[:, :, 64 * g + 21 + g] -= np.float32(7.0)
    return round_array(q, dtype_name), round_array(k, dtype_name), round_array(v, dtype_name)


def _attention_f64(q, k, v):
    Hq, dh = q.shape
    rep = Hq // k.shape[0]
    out = np.empty((Hq, dh), np.float64)
    for h in range(Hq):
        kk, vv = k[h // rep].astype(np.float64), v[h // rep].astype(np.float64)
        s = kk @ q[h].astype(np.float64) / np.sqrt(float(dh))
        p = np.exp(s - s.max())
        out[h] = (p / p.sum()) @ vv
    return out


def _kernel_case(ctx, Hq, Hkv, dh, T, dtype_name, bits):
    """(largest |out - ref|, largest excess over the bound's relative part, max|dq(V)|)"""
    from mlx_swift_audio_amd import ops
    q, k, v = _kernel_inputs(Hq, Hkv, dh, T, dtype_name)
    out = ops.kvq_attention(ctx, q, k, v, bits=bits, dtype=_dt(dtype_name))
    if bits:
        k, v = R.dq_rows(k, bits, dtype_name), R.dq_rows(v, bits, dtype_name)
    ref = _attention_f64(q, k, v)
    err = np.abs(out.astype(np.float64) - ref)
    return float(err.max()), float((err - R_REL[dtype_name] * np.abs(ref)).max()), float(np.abs(v).max())


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_kernel_alone_16bit_yardstick(ctx, dtype_name):
    """bits = 0: the existing kernels through the same op, inputs and reference -- the measurement behind A_MEASURED, and a check that
    it still stands (within the 2x the quantised bound allows itself).  The figure is dominated by the one rounding of the output: half a
    bf16 / f16 spacing of the planted value channel (|out| ~ 7 of max|V| ~ 10), which is why the two types differ by ~2^3."""
    worst = 0.0
    for Hq, Hkv, dh in KERNEL_SHAPES:
        for T in CONTEXTS:
            e, _, vmax = _kernel_case(ctx, Hq, Hkv, dh, T, dtype_name, 0)
            worst = max(worst, e / vmax)
    print(f"kvq yardstick {dtype_name}: largest |out - ref| / max|V| at bits 0 = {worst:.3e}")
    assert worst <= A_ABS[dtype_name], worst


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_alone_matches_float64_over_dequantised_rows(ctx, shape, dtype_name, bits):
    Hq, Hkv, dh = shape
    for T in CONTEXTS:
        e, excess, vmax = _kernel_case(ctx, Hq, Hkv, dh, T, dtype_name, bits)
        print(f"kvq kernel {shape} {dtype_name} q{bits} T={T}: max|err| {e:.3e}, beyond r|ref| {excess:.3e}, allowed {A_ABS[dtype_name] * vmax:.3e}")
        assert excess <= A_ABS[dtype_name] * vmax, (T, e, excess, A_ABS[dtype_name] * vmax)


# ---- 2. the quantiser, bit for bit ----------------------------------------------------------------------------------------------
def _same_bits(got, want, what):
    assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)), \
        (what, float(np.abs(got - want).max()), int((got != want).sum()))


def _assert_layer0_rows(plain, quant, seq, n, bits, dtype_name, what):
    k16, v16 = plain.read_kv(0, seq, 0, n)
    kq, vq = quant.read_kv(0, seq, 0, n)
    np.testing.assert_array_equal(round_array(k16, dtype_name), k16)      # (the 16-bit rows really are 16-bit values)
    _same_bits(kq, R.dq_rows(k16, bits, dtype_name), what + " K")
    _same_bits(vq, R.dq_rows(v16, bits, dtype_name), what + " V")
    assert np.abs(k16).max() > 0 and np.abs(v16).max() > 0


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("cfg_name", CFG_NAMES)
def test_quantiser_bit_exact_on_layer0_rows(ctx, cfg_name, dtype_name, bits):
    cfg = CONFIGS[cfg_name]
    plain, quant = _load(ctx, cfg_name, dtype_name), _load(ctx, cfg_name, dtype_name, bits)
    ids = _ids(cfg, 70)
    for m_ in (plain, quant):                          # rows 0 .. 68 by the batched prompt pass, row 69 by the step, 70 .. 72 by single steps
        m_.forward(ids)
        for t in (5, 6, 7):
            m_.forward([t])
    _assert_layer0_rows(plain, quant, 0, 73, bits, dtype_name, "prompt pass + steps")
    for m_ in (plain, quant):                          # every row by a directly launched step (no prompt pass, no graph)
        m_.set_debug(3)
        m_.reset()
        m_.forward(ids[:11])
    _assert_layer0_rows(plain, quant, 0, 11, bits, dtype_name, "stepped")
    for m_ in (plain, quant):                          # prompts token by token through the step GRAPH
        m_.set_debug(2)
        m_.reset()
        m_.forward(ids[:9])
    _assert_layer0_rows(plain, quant, 0, 9, bits, dtype_name, "stepped, graph")
    # sequence slots b > 0 of a capacity-5 handle (the split-K + reduce chain); the cache mode survives set_batch, and set_batch then
    # new_cache gives the same handle as new_cache then set_batch
    other = _load(ctx, cfg_name, dtype_name)
    other.set_batch(5)
    other.new_cache(quantized=True, bits=bits)
    prompts = [_ids(cfg, n, seed=3) for n in (3, 12, 1, 30, 9)]
    u = np.random.default_rng(4).random((5, 4)).astype(np.float32)
    kw = dict(max_new_tokens=4, stop_ids=(cfg.vocab - 1,))
    for m_ in (plain, quant):
        m_.set_debug(0)
        m_.set_batch(5)
    plain.generate_batch(prompts, u, **kw)
    got = quant.generate_batch(prompts, u, **kw)
    assert other.generate_batch(prompts, u, **kw) == got
    for b in (1, 3, 4):                                # the prompt's rows: ids past it may differ between the two cache modes
        _assert_layer0_rows(plain, quant, b, len(prompts[b]), bits, dtype_name, f"slot {b}")
        _same_bits(other.read_kv(0, b, 0, len(prompts[b]))[0], quant.read_kv(0, b, 0, len(prompts[b]))[0], f"either order, slot {b}")
    for m_ in (plain, quant, other):
        m_.close()


# ---- 3. + 4. logits over the device's own rows; new rows of every layer -------------------------------------------------------------
def _step_against_forced_oracle(model, ora, cfg, n, seed):
    """forward(n ids), forward([t]); the oracle takes t at position n over the DEVICE's rows [0, n] of every layer.  Returns the device
    logits, the oracle logits, and per layer (device new k / v row, oracle's own new k / v row)."""
    ids, t = _ids(cfg, n, seed), 11
    model.reset()
    model.forward(ids)
    got = model.forward([t])
    cache = [model.read_kv(l, 0, 0, n + 1) for l in range(cfg.n_layers)]
    ref, own = ora.step_logits(t, n, cache)
    rows = [((cache[l][0][:, n], cache[l][1][:, n]), (own[l][0][:, 0], own[l][1][:, 0])) for l in range(cfg.n_layers)]
    return got, ref, rows


def _check_logits_and_new_rows(plain, quant, ora, cfg, dtype_name, bits, contexts, seed=0):
    # d: the largest |device new row - oracle's own new row| of the same procedure on the 16-bit handle, over the whole test (every
    # context, layer, K and V): the existing path as yardstick for what is not quantisation error
    d = 0.0
    for n in contexts:
        got16, ref16, rows16 = _step_against_forced_oracle(plain, ora, cfg, n, seed)
        d = max([d] + [float(np.abs(dev[i] - own[i]).max()) for dev, own in rows16 for i in (0, 1)])
        assert np.abs(got16 - ref16).max() <= LOGIT_TOL[dtype_name] * ref16.std(), n
    for n in contexts:
        got, ref, rows = _step_against_forced_oracle(quant, ora, cfg, n, seed)
        sd = float(ref.std())
        err = float(np.abs(got - ref).max())
        worst = 0.0
        for l, (dev, own) in enumerate(rows):
            for i, name in enumerate("KV"):
                _, s, _ = R.quantise(round_array(own[i], dtype_name), bits, dtype_name)             # the group's scale, from the oracle's own row
                delta = np.abs(dev[i] - own[i]).reshape(cfg.n_kv_heads, cfg.head_dim // 64, 64)
                bound = 0.5 * s[..., None] + d
                worst = max(worst, float((delta / bound).max()))
        print(f"kvq logits q{bits} {dtype_name} n={n}: max|delta| {err / sd:.4f} std; new rows at most {worst:.3f} of 0.5 scale + d, d {d:.3e}")
        assert np.isfinite(got).all() and err <= LOGIT_TOL[dtype_name] * sd, (n, err / sd)
        assert worst <= 1.0, (n, worst, d)


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
@pytest.mark.parametrize("cfg_name", CFG_NAMES)
def test_logits_and_new_rows_with_device_cache_forced_into_oracle(ctx, cfg_name, dtype_name, bits):
    cfg = CONFIGS[cfg_name]
    plain, quant = _load(ctx, cfg_name, dtype_name), _load(ctx, cfg_name, dtype_name, bits)
    ora = R.ForcedCacheOracle(cfg, _weights(cfg_name, dtype_name))
    _check_logits_and_new_rows(plain, quant, ora, cfg, dtype_name, bits, CONTEXTS)
    plain.close()
    quant.close()


# ---- 5. invariants, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,dtype_name,bits", [("llama-micro128", "bf16", 4), ("gqa3", "f16", 8), ("gqa7", "bf16", 8), ("llama-micro", "f16", 4)])
def test_batch_equals_solo_reset_and_back_to_16bit(ctx, cfg_name, dtype_name, bits):
    cfg = CONFIGS[cfg_name]
    model, never = _load(ctx, cfg_name, dtype_name, bits), _load(ctx, cfg_name, dtype_name)
    rng = np.random.default_rng(5)
    # prompt lengths: 1 (no prompt-pass rows in either entry point) or >= 9 (the pass in both).  With 2 .. 8 ids generate() walks the
    # step where generate_batch() takes the pass -- two fp32 summation orders by design (lm.hip, LmGenCall::pf_min_rows), equal ids in
    # neither cache mode
    prompts = [rng.integers(0, cfg.vocab - 1, n).tolist() for n in (12, 40, 1, 17, 9)]
    n_new = 24
    u = rng.random((len(prompts), n_new)).astype(np.float32)
    kw = dict(temperature=0.8, top_p=0.9, rep_penalty=1.2, rep_window=16, max_new_tokens=n_new, stop_ids=(int(rng.integers(0, cfg.vocab)),))
    ids = _ids(cfg, 20)
    for cap in (5, 3):                                 # the split-K + reduce chain, then the carried-norm chain
        model.set_batch(cap)
        solo = [model.generate(p, u[b], **kw) for b, p in enumerate(prompts[:cap])]
        assert all(len(s_) > 0 for s_ in solo)
        assert model.generate_batch(prompts[:cap], u[:cap], **kw) == solo, cap
        assert model.generate_batch(prompts[:cap], u[:cap], **kw) == solo, cap             # the same call reproduces itself
        model.reset()                                  # (forward starts where sequence 0 stands)
        again = model.forward(ids)
        model.reset()
        _same_bits(model.forward(ids), again, f"reset + forward, capacity {cap}")
    # back to the 16-bit cache: identical to a handle that never left it
    want_gen = never.generate(prompts[1], u[1], **kw)
    never.reset()
    want = never.forward(ids)
    model.set_batch(1)
    model.reset()
    quant_logits = model.forward(ids)
    model.new_cache(quantized=False)
    assert model.generate(prompts[1], u[1], **kw) == want_gen
    model.reset()
    _same_bits(model.forward(ids), want, "16-bit cache after a quantised run")
    assert not np.array_equal(quant_logits, want)      # (the quantised run did differ: the mode was really on)
    model.close()
    never.close()


@pytest.mark.parametrize("cfg_name,dtype_name,bits", [("llama-micro128", "bf16", 4), ("qwen-micro", "f16", 8)])
def test_packed_weights_with_quantised_cache(ctx, cfg_name, dtype_name, bits):
    """attach_q4 + use_q4(True) with the quantised cache: item 3's check against the oracle on the de-quantised checkpoint."""
    from mlx_swift_audio_amd import lm as HL
    from test_lm_gpu import _quantized_checkpoint
    cfg = CONFIGS[cfg_name]
    packed, dense = _quantized_checkpoint(cfg, seed=11)
    plain, quant = (HL.CausalLM.load(ctx, cfg, dense, _dt(dtype_name)) for _ in range(2))
    for m_ in (plain, quant):
        m_.attach_q4(packed)
        m_.use_q4(True)
    quant.new_cache(quantized=True, bits=bits)
    ora = R.ForcedCacheOracle(cfg, dense)
    _check_logits_and_new_rows(plain, quant, ora, cfg, dtype_name, bits, (2, 9, 65), seed=1)
    plain.close()
    quant.close()


@pytest.mark.parametrize("bits", [4, 8])
def test_generate_ras_runs_and_reproduces_itself(ctx, bits):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = CONFIGS["qwen-micro"]
    S_TOK = 200
    w = S.lm_weights(cfg, seed=5, round_to="f16")
    w.update(S.qwen2lm_extra_weights(cfg, S_TOK, seed=5, round_to="f16"))
    model = HL.CausalLM.load(ctx, cfg, w, m.F16)
    model.new_cache(quantized=True, bits=bits)
    rng = np.random.default_rng(11)
    xs = [rng.standard_normal((n, cfg.hidden)).astype(np.float32) for n in (15, 4, 33)]
    mins, maxs = [12, 3, 20], [60, 25, 90]
    u = rng.random((3, 600)).astype(np.float32)
    solo = [model.generate_ras(xs[b], u[b], mins[b], maxs[b], S_TOK) for b in range(3)]
    assert all(mins[b] - 1 <= len(solo[b]) <= maxs[b] and all(0 <= t < S_TOK for t in solo[b]) for b in range(3))
    assert [model.generate_ras(xs[b], u[b], mins[b], maxs[b], S_TOK) for b in range(3)] == solo
    model.set_batch(3)
    assert model.generate_ras_batch(xs, u, mins, maxs, S_TOK) == solo
    model.close()


# ---- 6. arguments ----------------------------------------------------------------------------------------------------------------------
def test_arguments_are_rejected_before_anything_runs(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    model = _load(ctx, "llama-micro", "bf16")
    ids = _ids(CONFIGS["llama-micro"], 12)
    want = model.forward(ids)

    def code(fn):
        with pytest.raises(m.MiaError) as e:
            fn()
        return e.value.code

    for bits in (1, 2, 3, 5, 16, -4):
        assert code(lambda: model.new_cache(quantized=True, bits=bits)) == m._lib.ERR_INVALID_ARGUMENT, bits
    for gs in (32, 128, 0):
        assert code(lambda: model.new_cache(quantized=True, group_size=gs, bits=4)) == m._lib.ERR_UNSUPPORTED, gs
    # the rejected calls left the handle alone: same mode, same cache contents, same position
    k, _ = model.read_kv(0, 0, 0, 12)
    assert np.abs(k).max() > 0
    model.reset()
    _same_bits(model.forward(ids), want, "after rejected calls")
    c = CONFIGS["llama-micro"]
    for args in ((-1, 0, 0, 1), (c.n_layers, 0, 0, 1), (0, 1, 0, 1), (0, -1, 0, 1), (0, 0, -1, 1), (0, 0, 0, 0), (0, 0, c.max_ctx, 1), (0, 0, c.max_ctx - 3, 4), (0, 0, 0, c.max_ctx + 1)):
        assert code(lambda: model.read_kv(*args)) == m._lib.ERR_INVALID_ARGUMENT, args
    model.new_cache(quantized=True, bits=8)
    assert code(lambda: model.read_kv(0, 0, c.max_ctx - 3, 4)) == m._lib.ERR_INVALID_ARGUMENT
    model.close()
    q = np.zeros((4, 64), np.float32)
    for dh in (32, 96, 256):
        assert code(lambda: ops.kvq_attention(ctx, np.zeros((4, dh), np.float32), np.zeros((2, 5, dh), np.float32), np.zeros((2, 5, dh), np.float32), bits=4)) == m._lib.ERR_UNSUPPORTED, dh
    for bits in (2, 16):
        assert code(lambda: ops.kvq_attention(ctx, q, np.zeros((2, 5, 64), np.float32), np.zeros((2, 5, 64), np.float32), bits=bits)) == m._lib.ERR_INVALID_ARGUMENT, bits
    assert code(lambda: ops.kvq_attention(ctx, np.zeros((3, 64), np.float32), np.zeros((2, 5, 64), np.float32), np.zeros((2, 5, 64), np.float32), bits=4)) == m._lib.ERR_INVALID_ARGUMENT
