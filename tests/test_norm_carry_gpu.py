"""The carried-norm GEMM chains on scaled and shifted checkpoints.

Three hot paths store a not-yet-normalised 16-bit operand x * gamma and finish the norm in the consuming GEMM's epilogue: the LM step
(fused_norm, handle capacity <= 4), the Whisper decode step (fused_ln) and the Whisper encoder's out-proj -> mlp1 hand-over (gemm.hip,
ln_out).  On the synthetic checkpoints that operand is O(1) with a zero row mean, so neither its f16 range nor its common-mode rounding
is exercised.  tests/_equiv_checkpoints.py rewrites the checkpoints with exact power-of-two transforms; the variants are defined by
what the ORACLE measures at the hand-overs:

  near   largest |x gamma| over all rows and hand-overs in [0.25, 0.5] x 65504
  over   in every row of at least one hand-over per layer largest |x gamma| >= 2 x 65504, every stored tensor still finite in f16
  down   residual scaled down by the smallest 2^-k whose oracle logit std is still >= 0.5 x the base's (eps matters: own oracle only)
  shift  (Whisper) c = largest |x - row mean|, rounded up to a power of two, added to every positional channel

Every case first asserts its recipe on the oracle alone (test_recipe_holds_on_the_oracle runs without a GPU), then the HIP chain
against the oracle of the transformed, rounded checkpoint at the tolerances of the existing parity tests: the transforms are powers of
two and 16-bit rounding is relative, so nothing about the expected error changes.  The unfused chains (LM capacity 8, Whisper
set_debug bit 2, encoder tile variant 1) run the same checkpoints as controls."""
import functools

import numpy as np
import pytest
import torch

from mlx_swift_audio_amd import synthetic as S
from oracle import lm as OL
from oracle import quant as OQ
from oracle import whisper as OW

import _equiv_checkpoints as E
from _whisper_trace import check_clip

IDS = [5, 17, 256, 999, 2048, 3, 42, 7, 7, 1500]          # the ids of test_lm_gpu.py::test_forward_logits_match_oracle
NEXT = [11]
EQUIV_TOL = 2e-3                                            # exact transforms: |oracle(transformed) - oracle(base)| / std(base), the eps term

LM_CASES = [(c, d, v) for c in ("llama-micro", "qwen-micro") for d in ("f16", "bf16") for v in ("near", "over", "down")]
WD_CASES = [(d, v) for d in ("f16", "bf16") for v in ("near", "over", "down", "shift")]
WE_CASES = [(d, v) for d in ("f16", "bf16") for v in ("near", "over")]


def _dt(name):
    import mlx_swift_audio_amd as m
    return m.BF16 if name == "bf16" else m.F16


def _finite_stored(exact, dtype_name):
    assert E.all_finite_in(exact, "f16") and E.all_finite_in(exact, dtype_name), "a transformed tensor leaves the storage type"


# ---- causal LM ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lm_case(cfg_name, dtype_name, variant):
    """-> (cfg, rounded tensors, oracle logits [11, V] of IDS then NEXT); asserts the CPU-side conditions."""
    cfg = E.lm_untied(S.LM_CONFIGS[cfg_name])
    base = E.round_weights(S.lm_weights(cfg, seed=2, round_to=dtype_name), dtype_name)
    exact, info = E.lm_variant(OL.LMOracle, cfg, base, variant, [IDS, NEXT])
    _finite_stored(exact, dtype_name)
    base_logits = info["base_logits"]
    if variant != "down":
        lg, _ = E.lm_run(OL.LMOracle, cfg, exact, [IDS, NEXT])
        assert np.abs(lg - base_logits).max() <= EQUIV_TOL * base_logits.std(), (info["s"], info["G"])
    w = E.round_weights(exact, dtype_name)
    ref, taps = E.lm_run(OL.LMOracle, cfg, w, [IDS, NEXT])
    E.check_variant_position(variant, E.operand_rows(taps, w), cfg.n_layers)
    if variant == "down":
        assert ref.std() >= 0.5 * base_logits.std()
        half, _ = E.lm_run(OL.LMOracle, cfg, E.lm_transform(cfg, base, info["s"] / 2), [IDS, NEXT])
        assert half.std() < 0.5 * base_logits.std()          # the smallest such scale
    return cfg, w, ref


def _lm_check(got, want, dtype_name, frac=None):
    assert np.isfinite(got).all(), "non-finite logits"
    tol = (frac if frac is not None else (0.08 if dtype_name == "bf16" else 0.015)) * want.std()
    err = np.abs(got - want).max()
    assert err <= tol, (float(err / want.std()), "of the logit std")


@pytest.mark.gpu
@pytest.mark.parametrize("chain", ["capacity1", "stepwise", "capacity8"])
@pytest.mark.parametrize("cfg_name,dtype_name,variant", LM_CASES)
def test_lm_step_on_transformed_checkpoint(ctx, cfg_name, dtype_name, variant, chain):
    """capacity1: batched prompt pass, then the fused step (RMSNorm carried across o-proj / down-proj); stepwise: set_debug(2), every
    position through the fused step; capacity8: set_batch(8), the split-K + reduce / norm chain -- the control, which normalises
    before it rounds."""
    from mlx_swift_audio_amd import lm as HL
    cfg, w, ref = _lm_case(cfg_name, dtype_name, variant)
    model = HL.CausalLM.load(ctx, cfg, w, _dt(dtype_name))
    if chain == "stepwise":
        model.set_debug(2)
    if chain == "capacity8":
        model.set_batch(8)
    _lm_check(model.forward(IDS), ref[len(IDS) - 1], dtype_name)
    _lm_check(model.forward(NEXT), ref[len(IDS)], dtype_name)
    model.close()


def _quantize(cfg, w, bits):
    """tests/test_lm_gpu.py::_quantized_checkpoint on GIVEN tensors (untied head): group-64 affine codes, f16 scales / biases."""
    packed, dense = {}, dict(w)
    names = ["lm_head"]
    for l in range(cfg.n_layers):
        p = f"model.layers.{l}"
        names += [p + ".self_attn." + n + "_proj" for n in "qkvo"] + [p + ".mlp." + n + "_proj" for n in ("gate", "up", "down")]
    for n in names:
        pk, sc, bi = OQ.quantize_affine(w[n + ".weight"], 64, bits)
        sc, bi = sc.astype(np.float16), bi.astype(np.float16)
        assert np.isfinite(sc).all() and np.isfinite(bi).all()
        packed[n + ".weight"], packed[n + ".scales"], packed[n + ".biases"] = pk, sc, bi
        dense[n + ".weight"] = OQ.dequantize_affine(pk, sc.astype(np.float32), bi.astype(np.float32), 64, bits)
    return packed, dense


@functools.lru_cache(maxsize=None)
def _packed_case():
    cfg, w, _ = _lm_case("llama-micro128", "f16", "over")
    packed, dense = _quantize(cfg, w, 4)
    _finite_stored(dense, "f16")
    ref, taps = E.lm_run(OL.LMOracle, cfg, dense, [[t] for t in IDS + NEXT])
    E.check_variant_position("over", E.operand_rows(taps, dense), cfg.n_layers)      # the de-quantised model is still 'over'
    return cfg, packed, dense, ref


@pytest.mark.gpu
def test_lm_packed_step_on_over_checkpoint(ctx):
    """The SK_RESID epilogue of the packed 4-bit step (skinny_quant.hip) on the 'over' checkpoint, token by token, against the fp32
    oracle on the de-quantised weights at the packed tolerance of test_lm_gpu.py (0.02 of the logit std, f16)."""
    from mlx_swift_audio_amd import lm as HL
    cfg, packed, dense, ref = _packed_case()
    model = HL.CausalLM.load(ctx, cfg, dense, _dt("f16"))
    model.attach_q4(packed, bits=4)
    model.use_q4(True)
    for i, t in enumerate(IDS + NEXT):
        _lm_check(model.forward([t]), ref[i], "f16", frac=0.02)
    model.close()


# ---- Whisper --------------------------------------------------------------------------------------------------------------------------
DIMS = OW.DIMS["micro.en"]
N_NEW = 16


def _mel(dtype_name):
    rng = np.random.default_rng(1)
    return OW.round_array((0.5 * rng.standard_normal((2, 2 * DIMS.n_audio_ctx, DIMS.n_mels))).astype(np.float32), dtype_name)


def _decode_opts():
    st = OW.SpecialTokens.for_vocab(DIMS.n_vocab)
    kw = dict(timestamps=True, suppress_ids=OW.synthetic_suppress_list(st), blank_ids=[220, 50255], max_new_tokens=N_NEW)
    return st, kw, OW.DecodingOptions(**kw)


@functools.lru_cache(maxsize=None)
def _whisper_base(dtype_name):
    base = OW.synthetic_weights(DIMS, seed=77, style="peaky", round_to=dtype_name)
    ora = OW.WhisperOracle(DIMS, base)
    st, _, oo = _decode_opts()
    xa = ora.encode(_mel(dtype_name))
    init, _ = OW.initial_tokens(st, oo)
    toks = [list(init) + list(OW.greedy_decode(ora, st, xa[b:b + 1], oo).tokens) for b in range(2)]
    return base, xa, toks


@functools.lru_cache(maxsize=None)
def _decoder_case(dtype_name, variant):
    """-> rounded tensors of the transformed decoder; asserts the CPU-side conditions on the oracle's own run of the base checkpoint
    (teacher-forced over its 2 x 16 greedy tokens)."""
    base, xa, toks = _whisper_base(dtype_name)
    exact, info = E.whisper_decoder_variant(OW.WhisperOracle, DIMS, base, variant, xa, toks)
    _finite_stored(exact, dtype_name)
    base_logits = info["base_logits"]
    if variant != "down":
        lg, _ = E.whisper_decoder_run(OW.WhisperOracle, DIMS, exact, xa, toks)
        assert np.abs(lg - base_logits).max() <= EQUIV_TOL * base_logits.std(), info["s"]
    w = E.round_weights(exact, dtype_name)
    ref, taps = E.whisper_decoder_run(OW.WhisperOracle, DIMS, w, xa, toks)
    rows = E.operand_rows(taps, w)
    top = E.check_variant_position(variant, rows, DIMS.n_text_layer)
    if variant == "down":
        assert ref.std() >= 0.5 * base_logits.std()
        half, _ = E.whisper_decoder_run(OW.WhisperOracle, DIMS, E.whisper_decoder_transform(DIMS, base, info["s"] / 2), xa, toks)
        assert half.std() < 0.5 * base_logits.std()
    if variant == "shift":
        # the row mean really moved to c (>= the largest deviation), and the operand grew by no more than c x the largest gain
        dev = max(float((x - x.mean(dim=-1, keepdim=True)).abs().max()) for _, x in taps)
        mean = min(float(x.mean(dim=-1).abs().min()) for _, x in taps)
        gmax = max(float(np.abs(w[n + ".weight"]).max()) for n in rows)
        base_top = max(float(v.max()) for v in info["base_rows"].values())
        assert info["c"] >= dev * 0.99 and info["c"] < 2.05 * dev and mean >= 0.75 * info["c"], (info["c"], dev, mean)
        assert top <= base_top + info["c"] * gmax * 1.01, (top, base_top, info["c"], gmax)
    return w


WD_CHAINS = [(d, v, c) for d, v in WD_CASES for c in ("graph", "direct")] + [(d, v, "split") for d, v in WD_CASES if v in ("near", "over")]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype_name,variant,chain", WD_CHAINS)
def test_whisper_decode_step_on_transformed_checkpoint(ctx, dtype_name, variant, chain):
    """2 clips x 16 tokens through the step path (graph: the captured step graph; direct: set_debug(1); split: set_debug(4), the
    reduce + LayerNorm chain -- the control): the traced logits of every position against the transformed checkpoint's oracle on the
    handle's own audio features, the head replayed on them (tests/_whisper_trace.py), and the ids equal to the oracle's free run where
    its smallest top-2 margin is >= 10 x the measured logit noise (the rule of test_whisper_steps_gpu.py).  shift: tol_scale 2.0 --
    the operand's magnitude at most doubles against its spread, one bit of the 16-bit mantissa."""
    from mlx_swift_audio_amd import whisper as HW
    w = _decoder_case(dtype_name, variant)
    st, kw, oo = _decode_opts()
    ora = OW.WhisperOracle(DIMS, w)
    model = HW.WhisperModel.load(ctx, DIMS, w, _dt(dtype_name))
    model.set_debug({"graph": 0, "direct": 1, "split": 4}[chain])
    model.trace_logits([0, 1])
    res = HW.GreedyDecoder(model, HW.DecodingOptions(**kw)).decode(_mel(dtype_name))
    feats = model.audio_features()
    for b in range(2):
        xa = torch.from_numpy(feats[b:b + 1])
        info = check_clip(model, ora, st, oo, res[b], b, xa, dtype_name, N_NEW, tol_scale=2.0 if variant == "shift" else 1.0)
        ref = OW.greedy_decode(ora, st, xa, oo)
        print(dtype_name, variant, chain, b, "rel_rms", info["rel_rms_max"], "rel_max", info["rel_max_max"], "margin", min(ref.margins), "noise", info["noise_rms"])
        if min(ref.margins) >= 10 * info["noise_rms"]:
            assert res[b].tokens == ref.tokens, (b, res[b].tokens, ref.tokens)
    model.close()


@functools.lru_cache(maxsize=None)
def _encoder_case(dtype_name, variant):
    base, _, _ = _whisper_base(dtype_name)
    mel = _mel(dtype_name)
    exact, info = E.whisper_encoder_variant(OW.WhisperOracle, DIMS, base, variant, mel)
    _finite_stored(exact, dtype_name)
    w = E.round_weights(exact, dtype_name)
    ora = OW.WhisperOracle(DIMS, w)
    ref, taps = E.whisper_taps(ora, lambda: ora.encode(mel), "encoder.")
    E.check_variant_position(variant, E.operand_rows(taps, w), DIMS.n_audio_layer)
    ref = ref.numpy()
    fb = OW.WhisperOracle(DIMS, base).encode(mel).numpy()
    # the features still depend on the audio: two mels differ at least half as much as on the base checkpoint
    assert np.abs(ref[0] - ref[1]).mean() >= 0.5 * np.abs(fb[0] - fb[1]).mean()
    return w, ref


@pytest.mark.gpu
@pytest.mark.parametrize("gemm_variant", [1, 4])
@pytest.mark.parametrize("dtype_name,variant", WE_CASES)
def test_whisper_encoder_handover_on_transformed_checkpoint(ctx, dtype_name, variant, gemm_variant):
    """Tile variant 4 (8-phase kernel) carries mlp_ln through the out-proj's ln_out epilogue (D = 128 meets mia_gemm_ln_ok: N % 64 == 0,
    K >= 128); variant 1 runs the LayerNorm kernel -- the control.  Tolerance of test_whisper_gpu.py::test_encoder_matches_oracle."""
    from mlx_swift_audio_amd import whisper as HW
    w, ref = _encoder_case(dtype_name, variant)
    model = HW.WhisperModel.load(ctx, DIMS, w, _dt(dtype_name))
    model.set_gemm_variant(gemm_variant)
    model.encode(_mel(dtype_name))
    got = model.audio_features()
    assert np.isfinite(got).all(), "non-finite audio features"
    err = np.abs(got - ref)
    mx, mean = (0.06, 0.008) if dtype_name == "bf16" else (0.01, 0.0015)
    print(dtype_name, variant, gemm_variant, "max", err.max(), "mean", err.mean())
    assert err.max() <= mx and err.mean() <= mean, (err.max(), err.mean())
    model.close()


# ---- the recipes themselves, on the oracle alone (no GPU) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,dtype_name,variant", LM_CASES)
def test_lm_recipe_holds_on_the_oracle(cfg_name, dtype_name, variant):
    _lm_case(cfg_name, dtype_name, variant)


def test_lm_packed_recipe_holds_on_the_oracle():
    _packed_case()


@pytest.mark.parametrize("dtype_name,variant", WD_CASES)
def test_whisper_decoder_recipe_holds_on_the_oracle(dtype_name, variant):
    _decoder_case(dtype_name, variant)


@pytest.mark.parametrize("dtype_name,variant", WE_CASES)
def test_whisper_encoder_recipe_holds_on_the_oracle(dtype_name, variant):
    _encoder_case(dtype_name, variant)
