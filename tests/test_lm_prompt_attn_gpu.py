"""lm_prefill_attn.hip -- the prompt pass's tiled causal GQA attention -- at the operator (mia_op_lm_prompt_attention) against an fp64
softmax(q k^T dh^-0.5, causal) v of the same 16-bit-rounded inputs, and in the model (CausalLM.set_prompt_attention(1)) against stepping,
the oracle and the batch == single contract.

The kernel's tiles: keys are walked in KEY TILES of 64 anchored at key 0; a wave owns 32 positions of one query head (the WAVE WIDTH);
a workgroup's QUERY TILE is 128 / GW positions of GW heads of one KV group, GW = 4 | 2 | 1 for a group size that is a multiple of 4 | even
| odd: (Hq, Hkv) = (1, 1) -> 128 positions, (4, 2) -> 64, (8, 2) -> 32.  T covers 1, 2 and one below, at and one above 32, 64 and 128
(every one of which is a query tile, the key tile or the wave width of some case), plus 193 (three full key tiles and a one-key tail).

Bound, per element (test_attn128_gpu.py's, for the same reason): 1 ulp of the output type at the output's magnitude + 2^-8 (bf16) | 2^-11
(f16) of the largest |v| (P is rounded to the 16-bit type before P V).  Measured on the MI355X (worst error / bound): n = T over all
heads, head dims and lengths bf16 0.29 (dh 128, (4, 2), T = 2), f16 0.30 (dh 64, (8, 2), T = 193), smallest 0.00 (T = 1: the output is
the value row); queries behind cached keys 0.06 .. 0.18 (bf16), 0.07 .. 0.22 (f16); the spiked case 0.41 (bf16), 0.38 / 0.47 (f16, dh
64 / 128).  Model, mode 1 against stepping: 0.011 .. 0.015 sigma at the last position, 0.008 .. 0.016 sigma on the next step."""
import dataclasses

import numpy as np
import pytest

from mlx_swift_audio_amd import synthetic as S

pytestmark = pytest.mark.gpu

KEY_TILE = 64
EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193]
HEADS = [(1, 1), (4, 2), (8, 2)]


def _qtile(Hq, Hkv):
    g = Hq // Hkv
    return 128 // (4 if g % 4 == 0 else 2 if g % 2 == 0 else 1)


def _kinds():
    import mlx_swift_audio_amd as m
    return {"bf16": (m.BF16, 2.0 ** -8, 7), "f16": (m.F16, 2.0 ** -11, 10)}


def _ref(q, k, v, kind):
    """q [n, Hq, dh] at positions T - n .. T - 1, k / v [Hkv, T, dh] -> fp64 [n, Hq, dh], max |v|"""
    q, k, v = (S.round_array(a, kind).astype(np.float64) for a in (q, k, v))
    n, Hq, dh = q.shape
    Hkv, T, _ = k.shape
    out = np.zeros((n, Hq, dh))
    pos = np.arange(T - n, T)
    mask = np.arange(T)[None, :] > pos[:, None]
    for h in range(Hq):
        kv = h // (Hq // Hkv)
        s = q[:, h] @ k[kv].T * dh ** -0.5
        s[mask] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h] = (p / p.sum(axis=1, keepdims=True)) @ v[kv]
    return out, float(np.abs(v).max())


def _bound(ref, got, vmax, rel, mant_bits):
    mag = np.maximum(np.abs(ref), np.abs(got))
    expo = np.floor(np.log2(np.maximum(mag, 2.0 ** -14)))          # (f16 subnormals share the ulp of 2^-14)
    return 2.0 ** (expo - mant_bits) + rel * vmax


def _data(seed, T, n, Hq, Hkv, dh):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, Hq, dh)).astype(np.float32), rng.standard_normal((Hkv, T, dh)).astype(np.float32),
            rng.standard_normal((Hkv, T, dh)).astype(np.float32))


def _check(ctx, q, k, v, kind, label):
    from mlx_swift_audio_amd import ops
    dtype, rel, mant = _kinds()[kind]
    got = ops.lm_prompt_attention(ctx, q, k, v, dtype=dtype)
    ref, vmax = _ref(q, k, v, kind)
    err, bound = np.abs(got - ref), _bound(ref, got, vmax, rel, mant)
    print(f"lm_prompt_attention {label}: max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    return got


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_prompt_attention_matches_reference(ctx, heads, dh, kind):
    """n = T over every edge length: one case per (heads, dh, type), the lengths inside it (each is one small launch)."""
    Hq, Hkv = heads
    for T in EDGES:
        q, k, v = _data(1000 * T + 10 * Hq + dh, T, T, Hq, Hkv, dh)
        _check(ctx, q, k, v, kind, f"{kind} dh={dh} Hq={Hq} Hkv={Hkv} T=n={T}")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_prompt_attention_queries_behind_cached_keys(ctx, heads, dh, kind):
    """n < T: a single query row behind one full key tile of cached keys, and one query tile + 1 rows behind 100 cached keys."""
    Hq, Hkv = heads
    for T, n in ((KEY_TILE + 1, 1), (100 + _qtile(Hq, Hkv) + 1, _qtile(Hq, Hkv) + 1)):
        q, k, v = _data(7000 + T + Hq + dh, T, n, Hq, Hkv, dh)
        _check(ctx, q, k, v, kind, f"{kind} dh={dh} Hq={Hq} Hkv={Hkv} T={T} n={n}")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("dh", [64, 128])
def test_prompt_attention_rescale_branch(ctx, dh, kind):
    """The running maximum has to move after the first tile: key 150 (third key tile) is 8 x query 170, and key 70 (second tile) 8 x query
    100 -- raw scores about 60 x dh^0.5 above the rest, far past the lazy-rescale threshold.  Key 180 is 8 x query 5 but lies ABOVE
    position 5: it must have no effect there (the fp64 reference masks it; an unmasked spike would take the whole row)."""
    T, Hq, Hkv = 193, 4, 2
    q, k, v = _data(7, T, T, Hq, Hkv, dh)
    k[:, 150] = 8.0 * q[170, ::2]          # kv head j <- query head 2 j (the first of its group)
    k[:, 70] = 8.0 * q[100, ::2]
    k[:, 180] = 8.0 * q[5, ::2]
    got = _check(ctx, q, k, v, kind, f"{kind} dh={dh} spiked")
    ref, _ = _ref(q, k, v, kind)
    assert np.abs(ref[170, 0] - S.round_array(v, kind)[0, 150]).max() < 0.05      # the spike does own its row in the reference ...
    assert np.abs(got[5, 0] - S.round_array(v, kind)[0, 180]).max() > 0.5         # ... and key 180 does not own row 5


def test_prompt_attention_row_independence(ctx):
    """A row's bits depend on its own q row and keys / values [0, p] only: the last n' rows of the n = T call equal the n = n' call (other
    query tiling, other tile mates) bit for bit, and a repeat call returns the same bits."""
    from mlx_swift_audio_amd import ops
    import mlx_swift_audio_amd as m
    Hq, Hkv, dh = 4, 2, 64
    qt = _qtile(Hq, Hkv)
    T = 2 * qt + 37
    q, k, v = _data(23, T, T, Hq, Hkv, dh)
    for dtype in (m.BF16, m.F16):
        full = ops.lm_prompt_attention(ctx, q, k, v, dtype=dtype)
        assert np.array_equal(full, ops.lm_prompt_attention(ctx, q, k, v, dtype=dtype))
        for n in (1, 37, qt + 1):
            assert np.array_equal(full[T - n:], ops.lm_prompt_attention(ctx, q[T - n:], k, v, dtype=dtype)), n


@pytest.mark.parametrize("cfg_name,n,max_ctx", [("llama-micro", 40, 256), ("llama-micro128", 131, 256), ("qwen-micro", 700, 1024), ("qwen3-micro", 131, 256)])
def test_mode1_prompt_pass_matches_stepping(ctx, cfg_name, n, max_ctx):
    """test_lm_gpu.py's test_batched_prompt_pass_matches_stepping with set_prompt_attention(1), same tolerances: the last-position logits
    and the next step on the cache within 0.02 sigma of stepping, within 0.08 sigma of the oracle for n <= 200 (Llama / Qwen2 configs; the
    q/k-norm handle is compared with its own stepping)."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    from oracle import lm as OL
    cfg = dataclasses.replace(S.LM_CONFIGS[cfg_name], max_ctx=max_ctx)
    w = S.lm_weights(cfg, seed=6, round_to="bf16")
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    model.set_prompt_attention(1)
    ids = np.random.default_rng(n).integers(0, cfg.vocab, n).tolist()
    batched = model.forward(ids)
    nxt_b = model.forward([9])                      # a decode step on the K/V rows the prompt pass wrote
    model.reset()
    for t in ids[:-1]:
        model.forward([t])
    stepped = model.forward([ids[-1]])
    nxt_s = model.forward([9])
    scale = stepped.std()
    print(f"mode 1 {cfg_name} n={n}: |batched - stepped| / sigma {np.abs(batched - stepped).max() / scale:.4f}, next step {np.abs(nxt_b - nxt_s).max() / scale:.4f}")
    assert np.abs(batched - stepped).max() <= 0.02 * scale, np.abs(batched - stepped).max() / scale
    assert np.abs(nxt_b - nxt_s).max() <= 0.02 * scale
    if n <= 200 and not cfg.qk_norm:
        ref = OL.LMOracle(cfg, w).forward(ids).numpy()[-1]
        assert np.abs(batched - ref).max() <= 0.08 * ref.std()
    model.close()


def test_mode1_batch_equals_single(ctx):
    """generate_batch with the tiled kernel: four prompts of 9, 70, 200 and 300 ids (579 rows: the 512-row chunk boundary falls inside the
    last sequence, and every chunk holds runs of several sequences) -- sequence b's ids equal generate(prompt b, uniforms row b) exactly."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = dataclasses.replace(S.LM_CONFIGS["llama-micro"], max_ctx=1024)
    model = HL.CausalLM.load(ctx, cfg, S.lm_weights(cfg, seed=8, round_to="bf16"), m.BF16)
    model.set_batch(4)
    model.set_prompt_attention(1)
    rng = np.random.default_rng(31)
    prompts = [rng.integers(0, cfg.vocab - 1, n).tolist() for n in (9, 70, 200, 300)]
    n_new = 24
    u = rng.random((4, n_new)).astype(np.float32)
    kw = dict(temperature=0.8, top_p=0.9, rep_penalty=1.2, rep_window=16, max_new_tokens=n_new, stop_ids=(cfg.vocab - 1,))
    both = model.generate_batch(prompts, u, **kw)
    for b, p in enumerate(prompts):
        assert model.generate(p, u[b], **kw) == both[b], b
    model.close()


def test_switch_hygiene(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL, ops
    cfg = S.LM_CONFIGS["llama-micro"]
    w = S.lm_weights(cfg, seed=6, round_to="bf16")
    ids = np.random.default_rng(3).integers(0, cfg.vocab, 90).tolist()
    fresh = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    want = fresh.forward(ids)
    fresh.close()
    model = HL.CausalLM.load(ctx, cfg, w, m.BF16)
    model.set_prompt_attention(1)
    tiled = model.forward(ids)
    assert np.abs(tiled - want).max() <= 0.02 * want.std()
    model.set_prompt_attention(0)
    model.reset()
    assert np.array_equal(model.forward(ids), want)          # mode 1 then mode 0: a fresh handle's bits
    # the quantised cache keeps its own row kernel whatever the mode
    model.new_cache(quantized=True, bits=4)
    q0 = model.forward(ids)
    model.set_prompt_attention(1)
    model.reset()
    assert np.array_equal(model.forward(ids), q0)
    with pytest.raises(m.MiaError) as e:
        model.set_prompt_attention(2)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.close()
    z = np.zeros((2, 4, 96), np.float32)
    with pytest.raises(m.MiaError):                          # head dim 96
        ops.lm_prompt_attention(ctx, z, np.zeros((2, 2, 96), np.float32), np.zeros((2, 2, 96), np.float32))
    with pytest.raises(m.MiaError):                          # Hq % Hkv != 0
        ops.lm_prompt_attention(ctx, np.zeros((2, 3, 64), np.float32), np.zeros((2, 2, 64), np.float32), np.zeros((2, 2, 64), np.float32))
