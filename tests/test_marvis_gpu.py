"""Marvis on the GPU against the float64 oracle of tests/_marvis_ref.py (cases, bounds and uniform choices: tests/_marvis_cases.py).

1. Logits of every head over six teacher-forced frames: max |got - ref64| <= TOL * std(ref64) per head, TOL = the step chain's own bound
   (tests/test_lm_qwen3_gpu.py).  The second stack chained behind the first did not need more; what the rule for a wider bound would have
   allowed (derived on the CPU from the oracle alone: 4 x its float64 run against its run with 16-bit activations) is on record in
   tests/_marvis_cases.py and recomputed by tests/test_marvis_ref.py:
       config            dtype   TOL (asserted)   derived (not used)   measured on an MI355X, worst head
       marvis-micro      f16     0.015            0.0194               0.0044
       marvis-micro      bf16    0.08             0.1754               0.0364
       marvis-micro128   f16     0.015            0.0139               0.0039
       marvis-micro128   bf16    0.08             0.1383               0.0388
   codebooks 1 (no decoder step), 2 and 5; frames 2 .. 6 start the decoder at position 0 over the previous frame's cache rows.
2. mia_sample_top_p_ascending equals the oracle's pick and kept list exactly on the constructed rows and on 200 random rows whose margins
   the oracle clears.
3. Sampled frames equal the oracle's exactly, with no draw excused (test_sampled_frames_equal_the_oracle_exactly).
4. The loop: the stop rule on a checkpoint and uniforms for which the oracle draws the all-zero frame as its fourth (peaked checkpoint seed
   29, 3 codebooks, temperature 1.5, top_p 0.8; every draw's smallest margin is re-derived and asserted), the T = 0 continuation, a captured
   graph against direct launches, the 40-row prompt through the prompt pass, argument checks, and the pipeline into the Mimi decoder.
5. Sentences side by side equal their single calls on the same capacity and finish at different frames; a finished sentence's further
   frames touch nothing of it."""
import dataclasses

import numpy as np
import pytest

import _marvis_cases as MC
import _marvis_ref as R

pytestmark = pytest.mark.gpu


def _dt(name):
    import mlx_swift_audio_amd as m
    return {"f16": m.F16, "bf16": m.BF16}[name]


def _load(ctx, name, dtype, seed=3, peaked=False):
    from mlx_swift_audio_amd import marvis
    return marvis.MarvisModel.load(ctx, MC.config(name), MC.weights(name, dtype, seed, peaked), _dt(dtype))


def _forced_frames(model, codebooks, n_audio=9):
    tk, mk = MC.prompt(n_audio)
    out = []
    for f in range(6):
        ids, lg = model.frame(tk, mk, codebooks, np.full(codebooks, 0.5, np.float32), forced=MC.FORCED[f][:codebooks], return_logits=True)
        assert ids.tolist() == MC.FORCED[f][:codebooks].tolist()
        out.append(lg)
        tk, mk = MC.feedback(MC.FORCED[f][:codebooks])
    return np.stack(out)


@pytest.mark.parametrize("codebooks", [1, 2, 5])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["marvis-micro", "marvis-micro128"])
def test_logits_at_every_head_teacher_forced(ctx, name, dtype, codebooks):
    ref = MC.forced_run(name, dtype, codebooks)
    model = _load(ctx, name, dtype)
    got = _forced_frames(model, codebooks)
    model.close()
    ratio = np.abs(got - ref).max(-1) / ref.std(-1)          # [6][codebooks]
    print(f"{name} {dtype} codebooks {codebooks}: max |delta| / std per head = {ratio.max(0).round(4).tolist()}; bound {MC.bound(name, dtype)}")
    assert np.isfinite(got).all()
    assert (ratio <= MC.bound(name, dtype)).all(), ratio


PEAKED = [("marvis-micro", "f16", 5, 393), ("marvis-micro", "f16", 3, 29)]      # the checkpoints of the sampled-frames and stop-rule tests


@pytest.mark.parametrize("name,dtype,codebooks,seed", PEAKED)
def test_logits_on_the_peaked_checkpoints(ctx, name, dtype, codebooks, seed):
    """The draws of the two loop tests are chosen to be safe within the logit bound: it has to hold on their checkpoints too."""
    ref = MC.forced_run(name, dtype, codebooks, None, 9, seed, True)
    model = _load(ctx, name, dtype, seed, True)
    got = _forced_frames(model, codebooks)
    model.close()
    ratio = np.abs(got - ref).max(-1) / ref.std(-1)
    print(f"{name} {dtype} peaked seed {seed}: max |delta| / std per head = {ratio.max(0).round(4).tolist()}; bound {MC.bound(name, dtype)}")
    assert (ratio <= MC.bound(name, dtype)).all(), ratio


SAMPLED = dict(name="marvis-micro", dtype="f16", temperature=0.9, top_p=0.6, weight_seed=393, choice_seeds=(0, 1))


def test_sampled_frames_equal_the_oracle_exactly(ctx):
    """6 frames x 5 codebooks, no draw excused.  The uniforms are chosen on the oracle alone, frame by frame and draw by draw
    (MC.choose_uniforms): every draw keeps its kept set, the pick's place among its neighbours and its CDF interval for logits anywhere
    within the bound of the logits test.  Checkpoint: peaked, seed 393 (found on the CPU among seeds 0 .. 400 at temperature 0.9, top_p
    0.6); choice seeds 0 and 1 give two uniform tables whose frames part; smallest margin of a draw 0.139 (re-derived and printed below)."""
    s = SAMPLED
    runs = [MC.choose_uniforms(s["name"], s["dtype"], 5, 6, s["temperature"], s["top_p"], cs, s["weight_seed"], True) for cs in s["choice_seeds"]]
    assert all(r is not None for r in runs)                   # the share of draws left out is zero
    for u, frames, margin in runs:
        print("oracle frames", frames.tolist(), "smallest margin of a draw", round(margin, 5))
        assert u.shape == (6, 5) and frames.shape == (6, 5) and margin > 4 * MC.SAMPLER_SLACK
        assert all(len(set(frames[:, c].tolist())) >= 2 for c in range(5))
    assert runs[0][1].tolist() != runs[1][1].tolist()         # two uniform tables part: the draws read their uniforms
    model = _load(ctx, s["name"], s["dtype"], s["weight_seed"], True)
    tk, mk = MC.prompt()
    for u, frames, _ in runs:
        model.reset()
        got = model.generate(tk, mk, 5, u, temperature=s["temperature"], top_p=s["top_p"])
        assert got.tolist() == frames.tolist()
    model.close()


def test_sampler_op_equals_the_oracle(ctx):
    from mlx_swift_audio_amd import marvis
    for label, x, t, p, u in MC.sampler_rows():
        want, kept, _ = R.sample_top_p_ascending(x, t, p, u)
        got, gkept = marvis.sample_top_p_ascending(ctx, x, t, p, u)
        assert (got, gkept.tolist()) == (want, kept.tolist()), label
    rows = MC.random_sampler_rows()
    assert len(rows) == 200
    for i, (x, t, p, u) in enumerate(rows):
        want, kept, mg = R.sample_top_p_ascending(x, t, p, u)
        got, gkept = marvis.sample_top_p_ascending(ctx, x, t, p, u)
        assert got == want and gkept.tolist() == kept.tolist(), (i, mg)
    # a different uniform on the same row picks a different entry: the draw reads it
    x = np.zeros(4, np.float32)
    assert marvis.sample_top_p_ascending(ctx, x, 1.0, 1.0, 0.1)[0] == 0 and marvis.sample_top_p_ascending(ctx, x, 1.0, 1.0, 0.9)[0] == 3


def test_sampler_op_refuses_bad_arguments(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import marvis
    x = np.zeros(8, np.float32)
    for t, p in ((0.0, 0.5), (float("nan"), 0.5), (1.0, 0.0), (1.0, 1.5)):
        with pytest.raises(m.MiaError) as e:
            marvis.sample_top_p_ascending(ctx, x, t, p, 0.5)
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    with pytest.raises(m.MiaError) as e:
        marvis.sample_top_p_ascending(ctx, np.zeros(8193, np.float32), 1.0, 0.5, 0.5)
    assert e.value.code == m._lib.ERR_UNSUPPORTED
    assert marvis.sample_top_p_ascending(ctx, x, 1.0, 1.0, 0.99)[0] == 7


STOP = dict(name="marvis-micro", dtype="f16", codebooks=3, temperature=1.5, top_p=0.8, weight_seed=29)


def _stop_want(f, i, ids):
    if f >= 2 and 0 in ids:
        return 0
    nz = [t for t in ids if t != 0]
    return nz[0] if f < 2 and nz else None


def test_stop_rule_and_finished_state(ctx):
    s = STOP
    chosen = MC.choose_uniforms(s["name"], s["dtype"], s["codebooks"], 8, s["temperature"], s["top_p"], 0, s["weight_seed"], True, _stop_want)
    assert chosen is not None                                 # every draw of the oracle's run is safe within the logit bound
    u, frames, margin = chosen
    print("oracle frames", frames.tolist(), "smallest margin of a draw", margin)
    assert margin > 4 * MC.SAMPLER_SLACK and frames[-1].sum() == 0 and len(frames) - 1 >= 2 and all(f.sum() > 0 for f in frames[:-1])
    n = len(frames) - 1
    uni = np.full((8, s["codebooks"]), 0.5, np.float32)
    uni[:len(u)] = u
    model = _load(ctx, s["name"], s["dtype"], s["weight_seed"], True)
    tk, mk = MC.prompt()
    got = model.generate(tk, mk, s["codebooks"], uni, temperature=s["temperature"], top_p=s["top_p"])
    assert got.tolist() == frames[:n].tolist()                # the all-zero frame ends the sentence and is not emitted
    assert model.generate(None, None, s["codebooks"], uni[:2], temperature=s["temperature"], top_p=s["top_p"]).shape[0] == 0      # finished until reset
    # the frames launched behind the all-zero one (8 - 4 here) were no-ops: no cache row, no position moved.  A new row on the finished
    # handle gives the logits of the oracle whose cache holds the prompt and the three fed-back frames only
    ref = R.MarvisRef(MC.config(s["name"]), MC.weights(s["name"], s["dtype"], s["weight_seed"], True))
    rk, rm = tk, mk
    for f in range(len(frames)):
        ref.generate_frame(s["codebooks"], rk, rm, lambda lg, i: int(frames[f][i]))
        rk, rm = np.concatenate([frames[f], [0]])[None, :], np.array([[1] * s["codebooks"] + [0]])
    _, want = ref.generate_frame(s["codebooks"], np.array([[1, 2, 3, 0]]), np.array([[1, 1, 1, 0]]), lambda lg, i: 0, [4, 5, 6])
    _, lg = model.frame(*MC.feedback([1, 2, 3]), s["codebooks"], uni[0], forced=[4, 5, 6], return_logits=True)
    ratio = np.abs(lg - want).max(-1) / want.std(-1)
    print("a row behind the finished sentence: max |delta| / std per head =", ratio.round(4).tolist())
    assert (ratio <= MC.bound(s["name"], s["dtype"])).all(), ratio
    model.reset()
    model.reset()
    again = model.generate(tk, mk, s["codebooks"], uni, temperature=s["temperature"], top_p=s["top_p"])
    assert again.tolist() == frames[:n].tolist()
    # 20 frames allowed: the loop reads the flag behind the 16th launched frame and stops there; 12 of them ran as no-ops
    model.reset()
    assert model.generate(tk, mk, s["codebooks"], np.concatenate([uni, np.full((12, s["codebooks"]), 0.5, np.float32)]), temperature=s["temperature"],
                          top_p=s["top_p"]).tolist() == frames[:n].tolist()
    # the same sentence cut before its end: max_frames emitted, and the continuation reaches the same end
    model.reset()
    head = model.generate(tk, mk, s["codebooks"], uni[:2], temperature=s["temperature"], top_p=s["top_p"])
    tail = model.generate(None, None, s["codebooks"], uni[2:], temperature=s["temperature"], top_p=s["top_p"])
    assert np.concatenate([head, tail]).tolist() == frames[:n].tolist()
    model.close()


@pytest.mark.parametrize("capacity", [3, 8])
def test_batch_rows_equal_single_rows_and_finish_at_different_frames(ctx, capacity):
    """Three sentences side by side (prompts of 12, 14 and 23 rows): each one's frames equal its own single call on the same capacity -- 3: the
    chain with the carried norm, 8: the split-K chain.  Sentence 0 is the stop-rule case and ends after 3 frames while the others go on."""
    s = STOP
    u0, frames, _ = MC.choose_uniforms(s["name"], s["dtype"], s["codebooks"], 8, s["temperature"], s["top_p"], 0, s["weight_seed"], True, _stop_want)
    uni = np.random.default_rng(21).random((3, 8, s["codebooks"]), dtype=np.float32)
    uni[0, :len(u0)] = u0
    prompts = [MC.prompt(), MC.prompt(11, 1), MC.prompt(20, 2)]
    model = _load(ctx, s["name"], s["dtype"], s["weight_seed"], True)
    model.set_batch(capacity)
    kw = dict(temperature=s["temperature"], top_p=s["top_p"])
    singles = []
    for b, (tk, mk) in enumerate(prompts):
        model.reset()
        singles.append(model.generate(tk, mk, s["codebooks"], uni[b], **kw))
    batch = model.generate_batch(prompts, s["codebooks"], uni, **kw)
    print("frames per sentence", [len(f) for f in batch])
    assert [f.tolist() for f in batch] == [f.tolist() for f in singles]
    assert len(batch[0]) == len(frames) - 1 == 3 and max(len(f) for f in batch[1:]) > 3
    if capacity == 3:
        assert batch[0].tolist() == frames[:3].tolist()
    assert [f.tolist() for f in model.generate_batch(prompts[1:], s["codebooks"], uni[1:], **kw)] == [f.tolist() for f in singles[1:]]      # any slot, any n_seq
    assert model.generate(*prompts[1], s["codebooks"], uni[1], **kw).tolist() == singles[1].tolist()          # the call leaves a reset handle
    import mlx_swift_audio_amd as m
    for bad in (lambda: model.generate_batch(prompts * 3, s["codebooks"], np.tile(uni, (3, 1, 1)), **kw),                 # n_seq above the capacity
                lambda: model.generate_batch([prompts[0], (prompts[1][0][:0], prompts[1][1][:0])], s["codebooks"], uni[:2], **kw),      # an empty prompt
                lambda: model.set_batch(33), lambda: model.set_batch(0)):
        with pytest.raises(m.MiaError) as e:
            bad()
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.close()


def test_continuation_and_direct_launches_give_the_same_frames(ctx):
    model = _load(ctx, "marvis-micro128", "bf16")
    uni = np.random.default_rng(5).random((12, 5), dtype=np.float32)
    tk, mk = MC.prompt()
    whole = model.generate(tk, mk, 5, uni)
    assert whole.shape == (12, 5) and (whole >= 0).all() and (whole < MC.AUDIO_VOCAB).all() and len({tuple(f) for f in whole.tolist()}) > 6
    model.reset()
    parts = [model.generate(tk, mk, 5, uni[:5])] + [model.generate(None, None, 5, uni[a:b]) for a, b in ((5, 6), (6, 12))]
    assert np.concatenate(parts).tolist() == whole.tolist()
    other = np.random.default_rng(6).random((12, 5), dtype=np.float32)
    model.reset()
    assert model.generate(tk, mk, 5, other).tolist() != whole.tolist()          # the draws read their uniforms
    model.set_debug(1)                                                           # no hipGraph: the same kernels, the same bits
    model.reset()
    assert model.generate(tk, mk, 5, uni).tolist() == whole.tolist()
    model.set_debug(0)
    model.reset()
    assert model.generate(tk, mk, 2, uni[:, :2].copy()).shape == (12, 2)         # another codebook count re-captures the frame
    model.close()


@pytest.mark.parametrize("debug", [0, 2, 3])
def test_forty_row_prompt_through_the_prompt_pass_and_row_by_row(ctx, debug):
    name, dtype = "marvis-micro", "f16"
    ref = MC.forced_run(name, dtype, 5, None, 37)
    model = _load(ctx, name, dtype)
    model.set_debug(debug)
    got = _forced_frames(model, 5, 37)
    model.close()
    ratio = np.abs(got - ref).max(-1) / ref.std(-1)
    print(f"40-row prompt, debug {debug}: max |delta| / std per head = {ratio.max(0).round(4).tolist()}; bound {MC.bound(name, dtype)}")
    assert (ratio <= MC.bound(name, dtype)).all(), ratio


def test_argument_checks_leave_the_handle_usable(ctx):
    import mlx_swift_audio_amd as m
    model = _load(ctx, "marvis-micro", "f16")
    tk, mk = MC.prompt()
    uni = np.full((4, 5), 0.5, np.float32)

    def refused(fn):
        with pytest.raises(m.MiaError) as e:
            fn()
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, e.value

    refused(lambda: model.generate(None, None, 5, uni))                                      # T = 0 on a fresh handle
    bad = tk.copy(); bad[0, -1] = 300
    refused(lambda: model.generate(bad, mk, 5, uni))                                         # text id outside text_vocab
    bad = tk.copy(); bad[5, 0] = 67
    refused(lambda: model.generate(bad, mk, 5, uni))                                         # audio id outside audio_vocab
    bad = tk.copy(); bad[5, 1] = -1
    refused(lambda: model.frame(bad, mk, 5, uni[0]))
    badm = mk.copy(); badm[2, 2] = 2
    refused(lambda: model.generate(tk, badm, 5, uni))                                        # mask other than 0 / 1
    refused(lambda: model.generate(tk, mk, 0, uni))                                          # max_codebooks < 1
    refused(lambda: model.generate(tk, mk, 5, np.full((90, 5), 0.5, np.float32)))            # T + max_frames > max_ctx
    for t, p in ((0.0, 0.8), (float("inf"), 0.8), (-1.0, 0.8), (0.9, 0.0), (0.9, 1.01), (0.9, float("nan"))):
        refused(lambda: model.generate(tk, mk, 5, uni, temperature=t, top_p=p))
    refused(lambda: model.frame(tk, mk, 5, uni[0], forced=[0, 1, 2, 3, 67]))
    ref = MC.forced_run("marvis-micro", "f16", 5)
    got = _forced_frames(model, 5)[:1]                                                       # ... and a valid call follows
    assert (np.abs(got - ref[:1]).max(-1) / ref[:1].std(-1) <= MC.bound("marvis-micro", "f16")).all()
    refused(lambda: model.generate(None, None, 2, uni[:, :2].copy()))                        # a continuation keeps its codebook count
    model.close()


def test_load_refusals(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import marvis
    cfg, w = MC.config("marvis-micro"), MC.weights("marvis-micro", "f16")

    def fails(cfg_, w_, code, text):
        with pytest.raises(m.MiaError) as e:
            marvis.MarvisModel.load(ctx, cfg_, w_, m.F16)
        assert e.value.code == code and text in str(e.value), e.value

    fails(dataclasses.replace(cfg, attention_bias=True), w, m._lib.ERR_UNSUPPORTED, "attention_bias")
    fails(dataclasses.replace(cfg, mlp_bias=True), w, m._lib.ERR_UNSUPPORTED, "mlp_bias")
    fails(dataclasses.replace(cfg, audio_vocab=8193), w, m._lib.ERR_UNSUPPORTED, "8192")
    for name in ("audio_head", "projection.weight", "backbone.layers.1.self_attn.q_proj.weight", "decoder.layers.0.mlp.down_proj.weight", "decoder.norm.weight"):
        fails(cfg, {k: v for k, v in w.items() if k != name}, m._lib.ERR_INVALID_ARGUMENT, name)
        fails(cfg, {**w, name: w[name][..., :-1]}, m._lib.ERR_INVALID_ARGUMENT, name)


def test_pipeline_into_the_mimi_decoder(ctx):
    from mlx_swift_audio_amd import marvis, mimi, synthetic
    mcfg = dataclasses.replace(synthetic.MIMI_CONFIGS["mimi_micro"], quantizer_nq=5, quantizer_bins=128)
    codec = mimi.MimiCodec.load(ctx, mcfg, synthetic.mimi_weights(mcfg, seed=1))
    model = _load(ctx, "marvis-micro", "f16")
    tts = marvis.MarvisTTS(model, codec)
    tk, mk = MC.prompt()
    uni = np.random.default_rng(9).random((12, 5), dtype=np.float32)
    model.reset()
    frames = model.generate(tk, mk, 8, uni)
    pcm = tts.generate(tk, mk, "low", uni)
    assert pcm.shape == (frames.shape[0] * mcfg.samples_per_frame,) and np.isfinite(pcm).all() and np.abs(pcm).max() > 0
    assert np.array_equal(pcm, codec.decode(np.ascontiguousarray(frames.T)))
    chunks = list(tts.generate_streaming(tk, mk, "low", uni, interval=0.4))              # int(0.4 * 12.5) = 5 frames per chunk
    assert [c.size for c in chunks] == [n * mcfg.samples_per_frame for n in (5, 5, 2)][:len(chunks)] and sum(c.size for c in chunks) == pcm.size
    stream = codec.new_stream()
    assert np.array_equal(np.concatenate(chunks), np.concatenate([stream.decode_frames(np.ascontiguousarray(frames[a:b].T)) for a, b in ((0, 5), (5, 10), (10, 12))]))
    model.close()
    codec.close()
