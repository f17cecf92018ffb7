"""The decode step's cache policies (csrc/whisper_decode.hip: dec_cache_policy) change no bit and follow the budget rule.

The step keeps the decoder layers' weights resident in the Infinity Cache (default-policy loads) and loads what it reads once per step
non-temporal: the vocabulary matrix, the cross K/V and self-attention's cached K/V.  mia_whisper_set_debug bit 4 (16) restores the
earlier policies (one policy for every weight load, from mia_whisper_set_weight_sharing; self K/V default).  A cache policy is an
instruction immediate, so the library is compared with itself: tokens, avg_logprob (NaN-equal) and every traced logit row must be
bit-identical with the control bit off and on and with 1 and 3 declared readers.

Which policy a decode ran with is read from the profile classes: "decode_kept" has a record for every "decode" record whose step kept
the layer weights."""
import numpy as np
import pytest

from oracle import whisper as OW

from _whisper_packed import quantised_checkpoint

pytestmark = pytest.mark.gpu

CONTROL = 16                                      # mia_whisper_set_debug bit 4


def _dt(name):
    import mlx_swift_audio_amd as m
    return m.BF16 if name == "bf16" else m.F16


def _mel(dims, B, seed, dtype_name):
    rng = np.random.default_rng(seed)
    return OW.round_array((0.5 * rng.standard_normal((B, 2 * dims.n_audio_ctx, dims.n_mels))).astype(np.float32), dtype_name)


def _options(dims, n_new):
    from mlx_swift_audio_amd import whisper as HW
    st = OW.SpecialTokens.for_vocab(dims.n_vocab)
    return HW.DecodingOptions(timestamps=False, suppress_ids=OW.synthetic_suppress_list(st), blank_ids=[220, 50255], max_new_tokens=n_new)


def _run(model, mel, opts, traced):
    """(tokens, avg_logprob, traced rows of every traced clip) of one encode + decode.  The trace is re-allocated (NaN-filled) per
    run; rows 0 .. len(tokens) - 1 of a clip are positions it consumed (the forced prefix has at least one token)."""
    model.trace_logits(traced)
    model.encode(mel)
    res = model.decode_greedy(opts)
    rows = [model.read_logit_trace(slot, 0, max(1, len(res[b].tokens))).copy() for slot, b in enumerate(traced)]
    return [r.tokens for r in res], np.asarray([np.float32(r.avg_logprob) for r in res]), rows


def _assert_identical(runs):
    base = runs[0]
    for key, other in enumerate(runs[1:], 1):
        assert other[0] == base[0], key
        assert np.array_equal(other[1], base[1], equal_nan=True), key
        for a, b in zip(other[2], base[2]):
            assert a.shape == b.shape, key
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), key          # bit for bit, NaN rows included


def _four_runs(model, mel, opts, traced):
    runs = []
    for flags, readers in ((0, 1), (CONTROL, 1), (0, 3), (CONTROL, 3)):
        model.set_debug(flags)
        model.set_weight_sharing(readers)
        runs.append(_run(model, mel, opts, traced))
    model.set_debug(0)
    model.set_weight_sharing(1)
    model.trace_logits([])
    return runs


@pytest.mark.parametrize("dtype_name", ["bf16", "f16"])
def test_micro_policies_change_no_bits(ctx, dtype_name):
    """3 clips x 136 new tokens: self attention runs at 1 .. 136 + prefix keys, across 127, 128 and 129 (128 = one workgroup trip of
    32 U keys at U = 4), with non-temporal and with default-policy K/V loads."""
    from mlx_swift_audio_amd import whisper as HW
    dims = OW.DIMS["micro"]
    weights = OW.synthetic_weights(dims, seed=157, style="peaky", round_to=dtype_name)
    model = HW.WhisperModel.load(ctx, dims, weights, _dt(dtype_name))
    runs = _four_runs(model, _mel(dims, 3, 1, dtype_name), _options(dims, 136), [0, 2])
    assert max(len(t) for t in runs[0][0]) >= 130, [len(t) for t in runs[0][0]]       # some clip's key count passes 129
    assert all(r.shape[0] >= 1 and np.isfinite(r).all() for r in runs[0][2])
    _assert_identical(runs)
    model.close()


def test_tiny_en_policies_change_no_bits(ctx):
    """tiny.en, f16, 2 clips x 8 tokens: cross attention at the full 1500 keys, GEMM shapes other than micro's (D = 384)."""
    from mlx_swift_audio_amd import whisper as HW
    dims = OW.DIMS["tiny.en"]
    weights = OW.synthetic_weights(dims, seed=5, round_to="f16")
    model = HW.WhisperModel.load(ctx, dims, weights, _dt("f16"))
    runs = _four_runs(model, _mel(dims, 2, 1, "f16"), _options(dims, 8), [0, 1])
    _assert_identical(runs)
    model.close()


@pytest.mark.parametrize("bits,seed", [(4, 49), (8, 21)])
def test_micro_packed_policies_change_no_bits(ctx, bits, seed):
    """The packed step (csrc/skinny_frag_quant.hip) takes its policies from the same rule: control bit off and on, bit-identical."""
    from mlx_swift_audio_amd import whisper as HW
    dims = OW.DIMS["micro"]
    dense, packed = quantised_checkpoint(dims, seed, bits, "f16")
    model = HW.WhisperModel.load(ctx, dims, dense, _dt("f16"))
    model.attach_quantized(packed, bits=bits)
    model.use_packed(True)
    mel, opts = _mel(dims, 3, 1, "f16"), _options(dims, 40)
    runs = []
    for flags in (0, CONTROL):
        model.set_debug(flags)
        runs.append(_run(model, mel, opts, [0, 2]))
    model.set_debug(0)
    model.trace_logits([])
    assert all(np.isfinite(r).all() for r in runs[0][2])
    _assert_identical(runs)
    model.close()


def _kept(ctx, model, mel, opts):
    """(decode records, of them with the layer weights kept) of one encode + decode."""
    ctx.profile(True)
    ctx.profile_reset()
    try:
        model.encode(mel)
        model.decode_greedy(opts)
        return ctx.profile_read("decode")[0], ctx.profile_read("decode_kept")[0]
    finally:
        ctx.profile_reset()
        ctx.profile(False)


@pytest.mark.parametrize("dims_name", ["micro", "tiny.en"])
def test_budget_rule_keeps_what_fits(ctx, dims_name):
    """micro (0.9 MB of layer weights) and tiny.en (16.5 MB) fit the 230 MB budget: kept; under the control bit: not."""
    from mlx_swift_audio_amd import whisper as HW
    dims = OW.DIMS[dims_name]
    model = HW.WhisperModel.load(ctx, dims, OW.synthetic_weights(dims, seed=5, round_to="f16"), _dt("f16"))
    mel, opts = _mel(dims, 2, 1, "f16"), _options(dims, 2)
    assert _kept(ctx, model, mel, opts) == (1, 1)
    model.set_debug(CONTROL)
    assert _kept(ctx, model, mel, opts) == (1, 0)
    model.set_debug(0)
    model.close()


def test_budget_rule_streams_what_does_not_fit(ctx):
    """128 decoder layers at D = 256: 128 x 14 x 256^2 x 2 B = 234.9 MB of layer weights exceed the budget on their own, as large-v3's
    1.47 GB do: the step must run with the earlier policies (streamed weights), not thrash the cache.  Every layer shares layer 0's
    arrays (the loader uploads each), B = 1, two steps launched directly."""
    from mlx_swift_audio_amd import whisper as HW
    from mlx_swift_audio_amd.synthetic import ModelDimensions
    one = ModelDimensions(80, 100, 256, 4, 1, 51864, 448, 256, 4, 1)
    dims = ModelDimensions(80, 100, 256, 4, 1, 51864, 448, 256, 4, 128)
    assert dims.n_text_layer * 14 * dims.n_text_state ** 2 * 2 > 230e6
    weights = dict(OW.synthetic_weights(one, seed=5, round_to="f16"))
    layer0 = {k: v for k, v in weights.items() if k.startswith("decoder.blocks.0.")}
    for l in range(1, dims.n_text_layer):
        for k, v in layer0.items():
            weights[f"decoder.blocks.{l}." + k[len("decoder.blocks.0."):]] = v
    model = HW.WhisperModel.load(ctx, dims, weights, _dt("f16"))
    model.set_debug(1)                            # no step graph: 2 steps of 128 layers are not worth two captures
    mel, opts = _mel(dims, 1, 1, "f16"), _options(dims, 2)
    assert _kept(ctx, model, mel, opts) == (1, 0)
    model.set_weight_sharing(3)                   # the hint still decides how a model that does not fit loads its weights; nothing is "kept"
    assert _kept(ctx, model, mel, opts) == (1, 0)
    model.close()
