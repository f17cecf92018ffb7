"""The SenseVoice SANM encoder and the audio adaptor on the GPU (mia_sensevoice_encode) against the fp32 CPU restatement of
tests/_sensevoice_ref.py, on the micro configs (1 + 2 + 2 SANM layers of 256 / 2 heads, adaptor k 2 with one block of 256 / 2 heads),
sanm_shift 0 and 2, weights rounded to the handle's 16-bit type on both sides.

Bounds (tests/_sensevoice_ref.BOUNDS): enc_out is LayerNorm-ed, so the Whisper encoder's max / mean |d| <= 0.06 / 0.008 (bf16) and
0.01 / 0.0015 (f16) carry over; the adaptor's output is held to the same two numbers times the reference output's standard deviation.
tests/test_sensevoice_ref.py shows on the CPU that 16-bit rounding alone stays inside them and that a missing FSMN term, a residual on
layer 0 or a missing input scale do not -- the last two at different feature amplitudes, which is why every length runs at amplitude 1
and at 1e-3 here.  Lengths 1, 7, 64, 65, 201: odd T (the adaptor pads a zero row), one key tile, one row past it, two query tiles.

Measured on the MI355X, worst over both configs, all lengths and both amplitudes (enc_out max / mean; adaptor over std max / mean):
    bf16  0.0209 / 0.0037; 0.0230 / 0.0051        f16  0.0025 / 0.0005; 0.0028 / 0.0007
-- the figures of the rounded CPU reference (tests/test_sensevoice_ref.py): the device adds nothing visible to the 16-bit rounding."""
import functools

import numpy as np
import pytest

import _sensevoice_ref as R

pytestmark = pytest.mark.gpu

LENGTHS = (1, 7, 64, 65, 201)
AMPS = (1.0, 1e-3)


def _dt(kind):
    import mlx_swift_audio_amd as m
    return m.BF16 if kind == "bf16" else m.F16


def _feats(T, amp):
    return (amp * np.random.default_rng(T).standard_normal((T, 560))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """(cfg, weights, {(T, amp): (enc, emb)}) -- the reference runs once per config and type, is shared and never written to."""
    from mlx_swift_audio_amd import funasr, synthetic
    cfg = funasr.SENSEVOICE_CONFIGS[name]
    w = synthetic.sensevoice_weights(cfg, seed=1, round_to=kind)
    ref = R.SenseVoiceRef(cfg, w)
    outs = {}
    for T in LENGTHS:
        for amp in AMPS:
            outs[(T, amp)] = ref.encode_audio(_feats(T, amp))
            for a in outs[(T, amp)]:
                a.setflags(write=False)
    return cfg, w, outs


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["sensevoice-micro", "sensevoice-micro-shift2"])
def test_encoder_and_adaptor_match_reference(ctx, name, kind):
    from mlx_swift_audio_amd import funasr
    cfg, w, outs = _case(name, kind)
    model = funasr.SenseVoiceEncoder.load(ctx, cfg, w, _dt(kind))
    b_max, b_mean = R.BOUNDS[kind]
    worst = np.zeros(4)
    for (T, amp), (enc_ref, emb_ref) in outs.items():
        encs, embs = model.encode([_feats(T, amp)], want_encoder_out=True)
        assert encs[0].shape == (T, cfg.encoder_dim) and embs[0].shape == ((T - 1) // cfg.adaptor_k + 1, cfg.llm_dim)
        de, da = np.abs(encs[0] - enc_ref), np.abs(embs[0] - emb_ref) / emb_ref.std()
        worst = np.maximum(worst, [de.max(), de.mean(), da.max(), da.mean()])
        print(f"{name} {kind} T={T} amp={amp}: enc max/mean {de.max():.4f}/{de.mean():.5f}, adaptor/std max/mean {da.max():.4f}/{da.mean():.5f}")
        assert de.max() <= b_max and de.mean() <= b_mean, (T, amp, de.max(), de.mean())
        assert da.max() <= b_max and da.mean() <= b_mean, (T, amp, da.max(), da.mean())
    print(f"{name} {kind} worst: enc {worst[0]:.4f}/{worst[1]:.5f}, adaptor/std {worst[2]:.4f}/{worst[3]:.5f}; bound {b_max}/{b_mean}")
    model.close()


@pytest.mark.parametrize("name,kind", [("sensevoice-micro", "bf16"), ("sensevoice-micro-shift2", "f16")])
def test_ragged_stack_equals_single_calls(ctx, name, kind):
    """Three utterances of 201, 1 and 65 rows in one pass: utterance b's encoder rows and audio rows are those of its own call, bit for bit;
    so is a repeat of the stacked call."""
    from mlx_swift_audio_amd import funasr
    cfg, w, _ = _case(name, kind)
    model = funasr.SenseVoiceEncoder.load(ctx, cfg, w, _dt(kind))
    feats = [_feats(201, 1.0), _feats(1, 1.0), _feats(65, 1e-3)]
    encs, embs = model.encode(feats, want_encoder_out=True)
    for b, f in enumerate(feats):
        e1, a1 = model.encode([f], want_encoder_out=True)
        assert np.array_equal(encs[b], e1[0]), b
        assert np.array_equal(embs[b], a1[0]), b
    encs2, embs2 = model.encode(feats, want_encoder_out=True)
    assert all(np.array_equal(a, b) for a, b in zip(encs + embs, encs2 + embs2))
    assert np.array_equal(model.encode(feats)[2], embs[2])                       # without the tap
    model.close()


def test_fsmn_layouts_load_alike(ctx):
    """fsmn_block.weight as [D][K][1] (after FunASRModel.sanitize) gives the bits of [D][1][K] (the checkpoint)."""
    from mlx_swift_audio_amd import funasr
    cfg, w, _ = _case("sensevoice-micro", "bf16")
    w2 = {k: (np.ascontiguousarray(v.transpose(0, 2, 1)) if k.endswith("fsmn_block.weight") else v) for k, v in w.items()}
    a, b = funasr.SenseVoiceEncoder.load(ctx, cfg, w, _dt("bf16")), funasr.SenseVoiceEncoder.load(ctx, cfg, w2, _dt("bf16"))
    assert np.array_equal(a.encode([_feats(7, 1.0)])[0], b.encode([_feats(7, 1.0)])[0])
    a.close(); b.close()


def test_load_failures_are_named(ctx):
    import dataclasses
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import funasr
    cfg, w, _ = _case("sensevoice-micro", "bf16")
    missing = "audio_encoder.tp_encoders.1.self_attn.fsmn_block.weight"
    with pytest.raises(m.MiaError, match=missing.replace(".", r"\.")):
        funasr.SenseVoiceEncoder.load(ctx, cfg, {k: v for k, v in w.items() if k != missing}, _dt("bf16"))
    bad = dict(w)
    bad["audio_adaptor.linear1.weight"] = bad["audio_adaptor.linear1.weight"][:, :-1]
    with pytest.raises(m.MiaError, match=r"audio_adaptor\.linear1\.weight"):
        funasr.SenseVoiceEncoder.load(ctx, cfg, bad, _dt("bf16"))
    with pytest.raises(m.MiaError, match="negative right context"):             # left = 5 + 6 > K - 1
        funasr.SenseVoiceEncoder.load(ctx, dataclasses.replace(cfg, sanm_shift=6), w, _dt("bf16"))
