"""lm_step_attn.hip -- the decode step's split-key attention shared across a KV group -- at the operator (mia_op_lm_step_attention)
against an fp64 softmax(q k^T dh^-0.5) v over keys [0, T) of the same 16-bit-rounded inputs, and in the model
(CausalLM.set_step_attention(True)) against the default step, the batch == single contract and the switch's hygiene.

The kernel's edges: a 16-key MFMA tile, 64 keys per wave, 256 keys per workgroup (slice); T sits one below, at and one above each, plus
1 (no cached key), 257 (the new row alone in the second slice) and a many-slice tail.  Bound, per element (test_lm_prompt_attn_gpu.py's,
for the same reason): 1 ulp of the output type at the output's magnitude + 2^-8 (bf16) | 2^-11 (f16) of the largest |v| (P is rounded
to the 16-bit type before P V; the kernel also carries the rounding's remainder, so it sits well inside).  Measured on the MI355X (worst
error / bound over the thirteen lengths): mode 1 bf16 0.18 .. 0.29, f16 0.18 .. 0.28 over the twenty (heads, dh) cases, the worst always
at T = 2 or 16; mode 0 0.03 .. 0.28; the ramp-and-spike case 0.013 (dh 64), 0.13 .. 0.14 (dh 128).  Model, mode 1 against mode 0 over
21 steps: every logit equal on all four configs (0.0000 sigma; with P alone, no remainder, it read 0.027 sigma on llama-micro)."""
import dataclasses

import numpy as np
import pytest

from mlx_swift_audio_amd import synthetic as S

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513, 600]
HEADS = [(1, 1), (4, 2), (3, 1), (14, 2), (16, 1)]
KINDS = {"bf16": (2.0 ** -8, 7), "f16": (2.0 ** -11, 10)}


def _ref(q, k, v, kind):
    """q [Hq, dh] at position T - 1, k / v [Hkv, T, dh] -> fp64 [Hq, dh], max |v|"""
    q, k, v = (S.round_array(a, kind).astype(np.float64) for a in (q, k, v))
    Hq, dh = q.shape
    out = np.zeros((Hq, dh))
    for h in range(Hq):
        kv = h // (Hq // k.shape[0])
        s = k[kv] @ q[h] * dh ** -0.5
        p = np.exp(s - s.max())
        out[h] = (p / p.sum()) @ v[kv]
    return out, float(np.abs(v).max())


def _ratio(ctx, q, k, v, kind, mode):
    """worst |error| / bound of one operator call"""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    rel, mant = KINDS[kind]
    got = ops.lm_step_attention(ctx, q, k, v, mode=mode, dtype=m.BF16 if kind == "bf16" else m.F16)
    ref, vmax = _ref(q, k, v, kind)
    assert np.isfinite(got).all()
    expo = np.floor(np.log2(np.maximum(np.maximum(np.abs(ref), np.abs(got)), 2.0 ** -14)))      # (f16 subnormals share the ulp of 2^-14)
    return float((np.abs(got - ref) / (2.0 ** (expo - mant) + rel * vmax)).max())


def _data(seed, T, Hq, Hkv, dh):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((Hq, dh), (Hkv, T, dh), (Hkv, T, dh)))


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("heads", HEADS)
def test_split_step_attention_matches_reference(ctx, heads, dh, kind):
    worst = {T: _ratio(ctx, *_data(1000 * T + 10 * heads[0] + dh, T, *heads, dh), kind, 1) for T in LENGTHS}
    print(f"lm_step_attention mode 1 {kind} dh={dh} heads={heads}: worst err/bound {max(worst.values()):.3f} (T={max(worst, key=worst.get)})")
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("heads", [(4, 2), (3, 1)])
@pytest.mark.parametrize("T", [2, 65, 257])
def test_mode0_through_the_same_operator(ctx, T, heads):
    """The fused lm_attention the step runs today keeps P in fp32: inside the same bound a fortiori."""
    for dh, kind in ((64, "bf16"), (128, "f16")):
        r = _ratio(ctx, *_data(50 + T + dh, T, *heads, dh), kind, 0)
        print(f"lm_step_attention mode 0 {kind} dh={dh} heads={heads} T={T}: worst err/bound {r:.3f}")
        assert r <= 1.0


@pytest.mark.parametrize("spike_at", ["last", "first"])
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("dh", [64, 128])
def test_rescale_and_merge_branches(ctx, dh, kind, spike_at):
    """Scores of each group's first head ramp from 0 to 4 with the key index -- the maximum moves upward inside every wave, between the
    waves of a slice and between slices -- and one key scores 34: the new row (key T - 1), or key 0 of the first slice."""
    T, Hq, Hkv = 600, 4, 2
    q, k, v = _data(77 + dh, T, Hq, Hkv, dh)
    score = 4.0 * np.arange(T) / T
    score[T - 1 if spike_at == "last" else 0] = 34.0
    for j in range(Hkv):
        qh = S.round_array(q[2 * j], kind).astype(np.float64)
        k[j] = 0.05 * k[j] + np.outer(score * dh ** 0.5 / (qh @ qh), qh)
    r = _ratio(ctx, q, k, v, kind, 1)
    print(f"lm_step_attention mode 1 {kind} dh={dh} spike {spike_at}: worst err/bound {r:.3f}")
    assert r <= 1.0


def _load(ctx, cfg_name, **over):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = dataclasses.replace(S.LM_CONFIGS[cfg_name], **over)
    return HL.CausalLM.load(ctx, cfg, S.lm_weights(cfg, seed=6, round_to="bf16"), m.BF16), cfg


def _run(model, ids, steps):
    """a 250-id prompt, then teacher-forced single steps: the logits after every call"""
    model.reset()
    return [model.forward(ids)] + [model.forward([t]) for t in steps]


@pytest.mark.parametrize("cfg_name", ["llama-micro", "llama-micro128", "qwen-micro", "qwen3-micro"])
def test_model_mode1_matches_mode0(ctx, cfg_name):
    """Contexts 250 .. 270 cross the 256-key slice edge.  test_lm_gpu.py's test_batched_prompt_pass_matches_stepping tolerance (0.02
    sigma) on every step's logits; mode 1 under the captured graph equals mode 1 launched directly bit for bit."""
    model, cfg = _load(ctx, cfg_name, max_ctx=1024)
    ids = np.random.default_rng(250).integers(0, cfg.vocab, 250).tolist()
    base = _run(model, ids, [])
    steps = []
    for _ in range(20):                              # greedy under mode 0; both modes are then fed the same ids
        steps.append(int(base[-1].argmax()))
        base.append(model.forward([steps[-1]]))
    model.set_step_attention(True)
    split = _run(model, ids, steps)
    worst = max(np.abs(a - b).max() / b.std() for a, b in zip(split, base))
    print(f"split step {cfg_name}: worst |mode 1 - mode 0| / sigma over 21 steps {worst:.4f}")
    assert worst <= 0.02
    model.set_debug(1)
    direct = _run(model, ids, steps)
    assert all(np.array_equal(a, b) for a, b in zip(split, direct))
    model.close()


def test_mode1_batch_equals_single(ctx):
    model, cfg = _load(ctx, "llama-micro", max_ctx=1024)
    model.set_batch(4)
    model.set_step_attention(True)
    rng = np.random.default_rng(31)
    prompts = [rng.integers(0, cfg.vocab - 1, n).tolist() for n in (9, 70, 255, 300)]
    u = rng.random((4, 24)).astype(np.float32)
    kw = dict(temperature=0.8, top_p=0.9, rep_penalty=1.2, rep_window=16, max_new_tokens=24, stop_ids=(cfg.vocab - 1,))
    both = model.generate_batch(prompts, u, **kw)
    for b, p in enumerate(prompts):
        assert model.generate(p, u[b], **kw) == both[b], b
    model.close()


def test_switch_hygiene(ctx):
    import mlx_swift_audio_amd as m
    model, cfg = _load(ctx, "llama-micro", max_ctx=512)
    rng = np.random.default_rng(3)
    ids, u = rng.integers(0, cfg.vocab - 1, 260).tolist(), rng.random(16).astype(np.float32)
    kw = dict(max_new_tokens=16, stop_ids=(cfg.vocab - 1,))

    def run():
        gen = model.generate(ids, u, **kw)
        model.reset()
        return gen, model.forward(ids), model.forward([7])

    off = run()
    model.set_step_attention(True)
    run()
    model.set_step_attention(False)
    again = run()
    assert again[0] == off[0] and np.array_equal(again[1], off[1]) and np.array_equal(again[2], off[2])
    model.new_cache(quantized=True, bits=4)          # the packed cache keeps its own step kernel whatever the mode
    q_off = run()
    model.set_step_attention(True)
    q_on = run()
    assert q_on[0] == q_off[0] and np.array_equal(q_on[1], q_off[1]) and np.array_equal(q_on[2], q_off[2])
    model.close()
    wide, _ = _load(ctx, "llama-micro", n_heads=17, n_kv_heads=1)
    with pytest.raises(m.MiaError, match="at most 16 query heads") as e:
        wide.set_step_attention(True)
    assert e.value.code == m._lib.ERR_UNSUPPORTED
    wide.close()
