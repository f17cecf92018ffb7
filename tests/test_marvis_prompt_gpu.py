"""Marvis voice prompts from audio on the GPU: tokenize_audio / tokenize_segment / tokenize_start on a clip equal the rows built from
the oracle's codes (tests/_mimi_encode_ref.py), and MarvisTTS.reference_prompt (resample, encode, rows) drives the same generation as
the prompt built from those codes.  The codec is mimi_micro with 5 codebooks of 67 entries, the width and vocabulary of marvis-micro.
As in test_mimi_encode_gpu.py the equality of codes is claimed only after the oracle's own smallest gap has been checked against 8x its
float32 distance noise."""
import numpy as np
import pytest

import _marvis_cases as MC
import _mimi_encode_cases as ec

pytestmark = pytest.mark.gpu

CODEC, N_SAMPLES = "mimi_micro_nq5", 12 * 9 + 5


@pytest.fixture(scope="module")
def codec(ctx):
    from mlx_swift_audio_amd.mimi import MimiCodec
    c = MimiCodec.load(ctx, ec.config(CODEC), ec.weights(CODEC))
    yield c
    c.close()


def _oracle_codes(pcm):
    codes, gap, noise = ec._quant(CODEC, ec.oracle(CODEC).encode_latent(pcm))
    assert gap.min() > 8.0 * noise, (gap.min(), noise)
    return codes


@pytest.mark.parametrize("add_eos", [True, False])
def test_tokenize_audio_equals_the_rows_of_the_oracle_codes(codec, add_eos):
    from mlx_swift_audio_amd import marvis
    pcm = ec.pcm(CODEC, N_SAMPLES)
    codes = _oracle_codes(pcm)
    for k in (MC.N_CODEBOOKS, 2):
        rows, mask = marvis.tokenize_audio(codec, pcm, k, add_eos=add_eos)
        ref_rows, ref_mask = marvis.tokenize_audio_rows(codes[:k], add_eos=add_eos)
        assert rows.shape == (codes.shape[1] + int(add_eos), k + 1)
        assert np.array_equal(rows, ref_rows) and np.array_equal(mask, ref_mask)
    seg = marvis.tokenize_segment(MC.TEXT_IDS, codec, pcm, MC.N_CODEBOOKS, add_eos=add_eos)
    tr, tm = marvis.tokenize_text_rows(MC.TEXT_IDS, MC.N_CODEBOOKS)
    ar, am = marvis.tokenize_audio_rows(codes, add_eos=add_eos)
    assert np.array_equal(seg[0], np.concatenate([tr, ar])) and np.array_equal(seg[1], np.concatenate([tm, am]))
    if not add_eos:
        for got in (marvis.tokenize_start(MC.TEXT_IDS, codec, pcm, MC.N_CODEBOOKS), marvis.tokenize_start(MC.TEXT_IDS, codec, pcm)):
            ref = marvis.tokenize_start(MC.TEXT_IDS, codes)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


@pytest.mark.parametrize("rate", [24000, 16000])
def test_reference_prompt_drives_the_same_generation(ctx, codec, rate):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import audio_io, marvis
    model = marvis.MarvisModel.load(ctx, MC.config("marvis-micro"), MC.weights("marvis-micro", "f16"), m.F16)
    try:
        tts = marvis.MarvisTTS(model, codec)
        clip = ec.pcm(CODEC, 12 * 6 + 1)
        at_codec_rate = audio_io.resample(ctx, clip, rate, 24000)                 # the device resampler's own output feeds the oracle
        assert (at_codec_rate.size == clip.size) == (rate == 24000)
        ref = marvis.tokenize_start(MC.TEXT_IDS, _oracle_codes(at_codec_rate))
        rows, mask = tts.reference_prompt(MC.TEXT_IDS, clip, rate)
        assert np.array_equal(rows, ref[0]) and np.array_equal(mask, ref[1])
        uni = np.random.default_rng(5).random((6, MC.N_CODEBOOKS), dtype=np.float32)
        model.reset()
        frames = model.generate(rows, mask, 8, uni)
        model.reset()
        assert frames.shape[0] > 0 and np.array_equal(frames, model.generate(ref[0], ref[1], 8, uni))
        pcm = tts.generate(rows, mask, "low", uni)
        assert pcm.size == frames.shape[0] * ec.config(CODEC).samples_per_frame
        assert np.array_equal(pcm, tts.generate(ref[0], ref[1], "low", uni)) and np.array_equal(pcm, codec.decode(np.ascontiguousarray(frames.T)))
    finally:
        model.close()
