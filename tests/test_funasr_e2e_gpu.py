"""Fun-ASR from the waveform to token ids on the GPU, micro models (sensevoice-micro + a 2-layer Qwen3 of hidden 256): the fused
encode_audio equals features -> encode bit for bit, FunASRModel.transcribe_tokens returns what FunASRDecoder.transcribe_tokens returns on
the device's own audio rows (8 new tokens), and the list-of-clips form equals the per-clip form."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SOS, EOS = 2990, 2991
PROMPTS = ([5, 17, SOS, EOS, 256, 999], [42, SOS, EOS, 7, 7, 1500, 3])


@functools.lru_cache(maxsize=None)
def _clips():
    from mlx_swift_audio_amd import synthetic
    out = []
    for i, n in enumerate((16000, 23456)):
        x = (synthetic.synth_clip(i, n) + 0.01 * np.random.default_rng(70 + i).standard_normal(n)).astype(np.float32)
        x.setflags(write=False)
        out.append(x)
    return out


def _models(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import funasr, synthetic, lm as HL
    scfg = funasr.SENSEVOICE_CONFIGS["sensevoice-micro"]
    enc = funasr.SenseVoiceEncoder.load(ctx, scfg, synthetic.sensevoice_weights(scfg, seed=3, round_to="bf16"), m.BF16)
    lcfg = synthetic.LM_CONFIGS["qwen3-micro256"]
    lw = synthetic.lm_weights(lcfg, seed=4, round_to="bf16")
    lm = HL.CausalLM.load(ctx, lcfg, lw, m.BF16)
    lm.set_batch(2)
    return enc, lm, HL.FunASRDecoder(lm, lw["model.embed_tokens.weight"]), lcfg


def test_encode_audio_equals_features_then_encode(ctx):
    enc, lm, _, _ = _models(ctx)
    clips = _clips()
    for group in ([clips[0]], clips):
        fused = enc.encode_audio(group)
        staged = enc.encode(enc.features(group))
        assert len(fused) == len(staged) == len(group)
        for a, b, x in zip(fused, staged, group):
            assert a.shape == (((1 + len(x) // 160 + 5) // 6 - 1) // 2 + 1, 256)
            assert np.array_equal(a, b)
    assert np.array_equal(enc.encode_audio(clips)[1], enc.encode_audio([clips[1]])[0])     # a clip does not depend on its neighbours
    lm.close(); enc.close()


def test_transcribe_tokens_from_the_waveform(ctx):
    from mlx_swift_audio_amd import funasr
    enc, lm, dec, lcfg = _models(ctx)
    model = funasr.FunASRModel(enc, dec)
    clips = _clips()
    stops = (lcfg.vocab - 1,)
    solo = []
    for x, ids in zip(clips, PROMPTS):
        rows = model.encode_audio(x)
        want = dec.transcribe_tokens(ids, rows, SOS, EOS, stops, 8)
        got = model.transcribe_tokens(x, ids, SOS, EOS, stops, 8)
        assert len(want) == 8 and got == want
        solo.append(got)
    assert solo[0] != solo[1]
    assert model.transcribe_tokens(list(clips), list(PROMPTS), SOS, EOS, stops, 8) == solo
    lm.close(); enc.close()
