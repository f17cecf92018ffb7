"""Marvis on packed 6-bit weights (mia_marvis_attach_quantized / mia_marvis_use_packed) against the float64 oracle on the de-quantised
checkpoint.  Cases, bounds and the oracle-side choice of uniforms: tests/_marvis6_cases.py.

(a) Six teacher-forced frames with the prompt walked through the packed step (set_debug(2)): no weight is rounded anywhere, every head's
    logits within the step chain's own TOL (0.08 bf16, 0.015 f16), and the packed run at least as close to the oracle as the 16-bit frame
    of the same handle.  "As close" is measured by the root mean square of error / std over all logits of the run: both runs round the
    same activations, and the 16-bit copy adds the rounding of every weight as an independent error, so its mean SQUARE error is the
    packed run's plus that term -- an inequality of expectations, which a sum over 6 x 5 x 67 logits resolves and the maximum of 30
    per-head figures does not (marvis-micro f16 on an MI355X: worst head 0.00555 packed against 0.00532 on the 16-bit copy; the
    per-head figures of both runs are printed).
(b) The same frames behind the default prompt pass (16-bit copy): the LM packed-step test's 0.08 / 0.02.  What the rule for a wider bound
    would allow, derived on the CPU (tests/_marvis6_cases.py: DERIVED_PROMPT_PASS; recomputed by tests/test_marvis6_ref.py), is on record
    and not used:  marvis-micro f16 0.0236, bf16 0.1386; marvis-micro128 f16 0.0178, bf16 0.1862.
(c) generate == frame-by-frame calls; four sentences side by side == their single calls on the same capacity, finishing at different frames.
(d) Sampled frames equal the oracle's exactly on uniforms chosen from the oracle alone; no draw left out.
(e) load_quantized on the file's own keys (embedding tables quantised too) == load + attach on the expanded dict.
(f) Refusals leave the handle exactly as it was."""
import numpy as np
import pytest

import _marvis6_cases as M6
import _marvis_cases as MC

pytestmark = pytest.mark.gpu


def _dt(name):
    import mlx_swift_audio_amd as m
    return {"f16": m.F16, "bf16": m.BF16}[name]


def _load(ctx, name, dtype, seed=3, peaked=False, attach=True):
    from mlx_swift_audio_amd import marvis
    stored, dense = M6.checkpoint(name, dtype, seed, peaked)
    model = marvis.MarvisModel.load(ctx, MC.config(name), dense, _dt(dtype))
    if attach:
        model.attach_quantized(stored)
    return model


def _forced_frames(model, codebooks=MC.N_CODEBOOKS):
    tk, mk = MC.prompt()
    out = []
    for f in range(6):
        ids, lg = model.frame(tk, mk, codebooks, np.full(codebooks, 0.5, np.float32), forced=MC.FORCED[f][:codebooks], return_logits=True)
        assert ids.tolist() == MC.FORCED[f][:codebooks].tolist()
        out.append(lg)
        tk, mk = MC.feedback(MC.FORCED[f][:codebooks])
    return np.stack(out)


def _ratio(got, ref):
    assert np.isfinite(got).all()
    return np.abs(got - ref).max(-1) / ref.std(-1)          # [6][codebooks]


def _rms(got, ref):
    return float(np.sqrt((((got - ref) / ref.std(-1, keepdims=True)) ** 2).mean()))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["marvis-micro", "marvis-micro128"])
def test_teacher_forced_logits_packed_and_16_bit(ctx, name, dtype):
    ref = M6.forced_run(name, dtype)
    model = _load(ctx, name, dtype)
    # (a) nothing rounded: the prompt through the packed step
    model.set_debug(2)
    lp = _forced_frames(model)
    model.use_packed(False)
    model.reset()
    l16 = _forced_frames(model)
    packed, plain = _ratio(lp, ref), _ratio(l16, ref)
    print(f"{name} {dtype} prompt through the step: packed max |delta| / std per head = {packed.max(0).round(4).tolist()}, 16-bit copy {plain.max(0).round(4).tolist()}; bound {MC.TOL[dtype]}")
    print(f"{name} {dtype} rms of error / std over the run: packed {_rms(lp, ref):.5f}, 16-bit copy {_rms(l16, ref):.5f}")
    assert (packed <= MC.TOL[dtype]).all(), packed
    assert _rms(lp, ref) <= _rms(l16, ref), (_rms(lp, ref), _rms(l16, ref))
    # (b) the default prompt pass (16-bit copy) in front of the packed frame
    model.set_debug(0)
    model.use_packed(True)
    model.reset()
    mixed = _ratio(_forced_frames(model), ref)
    print(f"{name} {dtype} default prompt pass: max |delta| / std per head = {mixed.max(0).round(4).tolist()}; bound {M6.TOL_PROMPT_PASS[dtype]} (derived, not used: {M6.DERIVED_PROMPT_PASS[(name, dtype)]})")
    assert (mixed <= M6.TOL_PROMPT_PASS[dtype]).all(), mixed
    # fewer codebooks re-capture the frame: one (no decoder step) and two
    for cb in (1, 2):
        model.reset()
        assert (_ratio(_forced_frames(model, cb), M6.forced_run(name, dtype, cb)) <= M6.TOL_PROMPT_PASS[dtype]).all(), cb
    model.close()


def test_generate_equals_frame_by_frame_calls(ctx):
    model = _load(ctx, "marvis-micro128", "bf16")
    uni = np.random.default_rng(5).random((10, 5), dtype=np.float32)
    tk, mk = MC.prompt()
    whole = model.generate(tk, mk, 5, uni)
    assert whole.shape == (10, 5) and len({tuple(f) for f in whole.tolist()}) > 5
    model.reset()
    rows, steps = (tk, mk), []
    for f in range(10):
        steps.append(model.frame(*rows, 5, uni[f]))
        rows = MC.feedback(steps[-1])
    assert np.stack(steps).tolist() == whole.tolist()
    model.set_debug(1)                                        # no hipGraph: the same kernels, the same bits
    model.reset()
    assert model.generate(tk, mk, 5, uni).tolist() == whole.tolist()
    model.set_debug(0)
    model.use_packed(False)                                   # the switch is read: the 16-bit frame draws from other logits
    model.reset()
    plain = model.generate(tk, mk, 5, uni)
    model.use_packed(True)
    model.reset()
    assert model.generate(tk, mk, 5, uni).tolist() == whole.tolist()
    print("frames that differ between the packed and the 16-bit frame:", int((plain != whole).any(-1).sum()), "of 10")
    model.close()


def test_batch_rows_equal_single_rows_and_finish_at_different_frames(ctx):
    s = M6.STOP
    chosen = M6.choose_uniforms(s["name"], s["dtype"], s["codebooks"], 8, s["temperature"], s["top_p"], 0, s["weight_seed"], M6.stop_want, tol=M6.TOL_PROMPT_PASS[s["dtype"]])
    assert chosen is not None
    u0, frames, margin = chosen
    print("oracle frames", frames.tolist(), "smallest margin of a draw", round(float(margin), 5))
    assert margin > 4 * MC.SAMPLER_SLACK and frames[-1].sum() == 0 and len(frames) == 3 and all(f.sum() > 0 for f in frames[:-1])
    uni = np.random.default_rng(21).random((4, 8, s["codebooks"]), dtype=np.float32)
    uni[0, :len(u0)] = u0
    prompts = [MC.prompt(), MC.prompt(11, 1), MC.prompt(20, 2), MC.prompt(5, 3)]
    model = _load(ctx, s["name"], s["dtype"], s["weight_seed"], True)
    model.set_batch(4)
    kw = dict(temperature=s["temperature"], top_p=s["top_p"])
    singles = []
    for b, (tk, mk) in enumerate(prompts):
        model.reset()
        singles.append(model.generate(tk, mk, s["codebooks"], uni[b], **kw))
    batch = model.generate_batch(prompts, s["codebooks"], uni, **kw)
    print("frames per sentence", [len(f) for f in batch])
    assert [f.tolist() for f in batch] == [f.tolist() for f in singles]
    assert batch[0].tolist() == frames[:2].tolist() and max(len(f) for f in batch[1:]) > 2
    model.close()


def test_sampled_frames_equal_the_oracle_exactly(ctx):
    s = M6.SAMPLED
    tol = M6.TOL_PROMPT_PASS[s["dtype"]]
    runs = [M6.choose_uniforms(s["name"], s["dtype"], 5, 6, s["temperature"], s["top_p"], cs, s["weight_seed"], tol=tol) for cs in s["choice_seeds"]]
    assert all(r is not None for r in runs)                   # the share of draws left out is zero
    for u, frames, margin in runs:
        print("oracle frames", frames.tolist(), "smallest margin of a draw", round(float(margin), 5))
        assert u.shape == (6, 5) and frames.shape == (6, 5) and margin > 4 * MC.SAMPLER_SLACK
        assert all(len(set(frames[:, c].tolist())) >= 2 for c in range(5))
    assert runs[0][1].tolist() != runs[1][1].tolist()
    # the bound the choice rests on holds on this checkpoint
    model = _load(ctx, s["name"], s["dtype"], s["weight_seed"], True)
    ratio = _ratio(_forced_frames(model), M6.forced_run(s["name"], s["dtype"], 5, None, s["weight_seed"], True))
    assert (ratio <= tol).all(), ratio
    tk, mk = MC.prompt()
    for u, frames, _ in runs:
        model.reset()
        got = model.generate(tk, mk, 5, u, temperature=s["temperature"], top_p=s["top_p"])
        assert got.tolist() == frames.tolist()
    model.close()


def test_load_quantized_equals_load_plus_attach(ctx):
    from mlx_swift_audio_amd import checkpoint as CK, marvis
    name, dtype = "marvis-micro", "f16"
    stored, _ = M6.checkpoint(name, dtype, quantise_embeddings=True)
    assert "text_embeddings.scales" in stored and "audio_embeddings.scales" in stored and "audio_head" in stored
    raw = {M6.raw_name(k): v for k, v in stored.items()}
    assert CK.sanitize_marvis(list(raw)) == list(stored) and any(".attn.output_proj." in k for k in raw) and any(k.endswith("sa_norm.scale") for k in raw)
    a = marvis.MarvisModel.load_quantized(ctx, MC.config(name), raw, _dt(dtype))
    b = marvis.MarvisModel.load(ctx, MC.config(name), CK.expand_checkpoint(ctx, stored), _dt(dtype))
    b.attach_quantized(stored)
    la, lb = _forced_frames(a), _forced_frames(b)
    assert np.array_equal(la, lb)
    a.use_packed(False); b.use_packed(False)
    a.reset(); b.reset()
    assert np.array_equal(_forced_frames(a), _forced_frames(b))
    a.close(); b.close()


def test_refusals_leave_the_handle_as_it_was(ctx):
    import mlx_swift_audio_amd as m
    name, dtype = "marvis-micro", "f16"
    stored, _ = M6.checkpoint(name, dtype)
    model = _load(ctx, name, dtype, attach=False)

    def refused(fn, text=None):
        with pytest.raises(m.MiaError) as e:
            fn()
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, e.value
        assert text is None or text in str(e.value), e.value

    before = _forced_frames(model)
    refused(lambda: model.use_packed(True))                                                   # nothing attached
    lacking = {k: v for k, v in stored.items() if not k.startswith("decoder.layers.1.mlp.down_proj.")}
    refused(lambda: model.attach_quantized(lacking), "decoder.layers.1.mlp.down_proj")        # the backbone was ready: nothing of it stays
    refused(lambda: model.attach_quantized({k: v for k, v in stored.items() if not k.startswith("projection.")}), "projection")
    refused(lambda: model.attach_quantized({k: v for k, v in stored.items() if not k.startswith("backbone.layers.0.self_attn.k_proj.s")}), "backbone.layers.0.self_attn.k_proj")
    for bits in (3, 5, 7):
        refused(lambda: model.attach_quantized(stored, bits=bits))
    refused(lambda: model.attach_quantized(stored, group_size=32))
    refused(lambda: model.use_packed(True))
    model.reset()
    assert np.array_equal(_forced_frames(model), before)                                      # the 16-bit frame, bit for bit
    model.attach_quantized(stored)
    refused(lambda: model.attach_quantized(stored))                                           # one attach per handle
    model.reset()
    ref = M6.forced_run(name, dtype)
    assert (_ratio(_forced_frames(model), ref) <= M6.TOL_PROMPT_PASS[dtype]).all()
    model.close()
