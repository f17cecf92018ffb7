"""The two places the trimmer is wired in: CosyVoice2Model.prepare_speaker (prepareSpeakerFromSamples, CosyVoice2Engine.swift:397-526)
and outetts.create_speaker_profile(trim=...) (OuteTTSEngine.swift:245-297).  Wiring only: recording stubs stand in for the Whisper
`stt` and, for CosyVoice2, for prepare_conditionals; the trimming itself runs on the device.

The long clip: 0.5 s of zeros, 31.5 s of noise at 0.1, 0.25 s of zeros at 24 kHz (frames 600 / 300).  Frame 38 = [11400, 12000) is all
zeros (-200 dB) and frame 39 = [11700, 12300) holds 300 noise samples (3 dB under the loudest frame), so the clip starts at 11700; the
last frame that holds noise is 2559 = [767700, 768300), so it ends at 2560 * 300 = 768000: 756300 samples, 31.5125 s, are left."""
import dataclasses

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: DACCodec.encode(SpeakerAudio) shares the device with torch)

import _outetts_speaker_ref as SR_
import _trim_cases as TC
import _trim_ref as R
from mlx_swift_audio_amd import cosyvoice2 as CV
from mlx_swift_audio_amd import outetts as O
from mlx_swift_audio_amd import synthetic as S
from mlx_swift_audio_amd import trim as T
from mlx_swift_audio_amd.timing import Word

pytestmark = pytest.mark.gpu

SR = 24000
# times in the TRIMMED clip.  " fine" ends at 29.369999 s: Float(29.369999) = 29.36999893 and the fp32 product with 24000 is 704879.974,
# which rounds to 704880.0 (fp32 spacing 0.0625 there) -- the double product 704879.976 would truncate to 704879.  " more" ends above
# 30 - 0.1; " beyond" is the safety-margin word; " low" has probability 0.1; " ghost" ends 0.39 s after the audio does.
STUB_WORDS = [(" Hello", 0.30, 0.80, 0.9), (" there", 0.80, 1.40, 0.9), (" this", 12.0, 12.5, 0.9), (" is", 19.0, 19.4, 0.9),
              (" fine", 28.6, 29.369999, 0.9), (" more", 29.5, 29.95, 0.9), (" beyond", 29.95, 30.4, 0.9), (" low", 30.5, 31.0, 0.1),
              (" ghost", 31.2, 31.9, 0.8)]


class _Seg:
    def __init__(self, words):
        self.words = words


class _Result:
    def __init__(self, text, segments):
        self.text, self.segments = text, segments


class _Stt:
    """Records every call; answers with the stub words, split over two segments, and a text of its own."""

    def __init__(self, words=STUB_WORDS, text="  the stub's text \n"):
        self.calls, self.words, self.text = [], [Word(*w) for w in words], text

    def transcribe(self, clips, word_timestamps=False, **kw):
        self.calls.append((clips, word_timestamps, kw))
        segs = [_Seg(self.words[:3]), _Seg(None), _Seg(self.words[3:])] if word_timestamps else [_Seg(None)]
        return [_Result(self.text, segs)]


def _len_16k(ctx, n):
    """Length of an n-sample 24 kHz clip after the engine's linear resampler to 16 kHz."""
    return int(ctx.lib.mia_resample_linear_len(n, float(np.float32(16000) / np.float32(24000))))


@pytest.fixture(scope="module")
def long_clip():
    x = np.concatenate([TC.zeros(12000), TC.noise(31, 756000, 0.1), TC.zeros(6000)])
    b64, margin = R.bounds_f64(x, 600, 300, 60.0)
    assert b64 == (11700, 768000) == R.bounds_literal(x, 600, 300, 60.0) and margin >= TC.MARGIN_DB
    return x


@pytest.fixture()
def model(ctx):
    m = CV.CosyVoice2Model(ctx, None, None, None)
    m.got = []

    def prepare_conditionals(ref_wav, speaker_embedding=None, prompt_text=()):
        m.got.append((ref_wav, speaker_embedding, prompt_text))
        return "conditionals"
    m.prepare_conditionals = prepare_conditionals
    return m


def test_prepare_speaker_clips_at_a_word_boundary(model, long_clip):
    stt = _Stt()
    encode = lambda text: [len(text), 7]
    emb = np.ones(192, np.float32)
    sp = model.prepare_speaker(long_clip, SR, stt=stt, encode_text=encode, speaker_embedding=emb)
    (clips, word_timestamps, _), = stt.calls                  # one call: the words' text is the transcription, nothing is transcribed again
    assert word_timestamps is True and len(clips) == 1
    assert clips[0].size == _len_16k(model.ctx, 756300) and abs(clips[0].size - 504200) <= 1      # the TRIMMED clip at 16 kHz
    assert sp.sample_count == 704880 and sp.sample_rate == 24000 and sp.clipped_at_word_boundary
    assert sp.transcription == "Hello there this is fine"
    (wav, got_emb, prompt), = model.got
    assert wav.tobytes() == long_clip[11700:11700 + 704880].tobytes()
    assert got_emb is emb and prompt == [len("Hello there this is fine"), 7] and sp.conditionals == "conditionals"


def test_prepare_speaker_without_stt_cuts_at_30_s(model, long_clip):
    sp = model.prepare_speaker(long_clip, SR)
    assert sp.sample_count == 720000 and not sp.clipped_at_word_boundary and sp.transcription is None
    (wav, _, prompt), = model.got
    assert wav.tobytes() == long_clip[11700:11700 + 720000].tobytes() and tuple(prompt) == ()


def test_prepare_speaker_falls_back_when_no_word_fits(model, long_clip):
    stt = _Stt(words=[(" endless", 0.0, 30.5, 0.9), (" tail", 30.5, 31.0, 0.9), (" end", 31.0, 31.4, 0.9)])
    sp = model.prepare_speaker(long_clip, SR, stt=stt)
    assert sp.sample_count == 720000 and not sp.clipped_at_word_boundary
    assert [c[1] for c in stt.calls] == [True, False]         # no clip point: cut, then the final audio is transcribed
    assert stt.calls[1][0][0].size == _len_16k(model.ctx, 720000) and sp.transcription == "the stub's text"
    assert tuple(model.got[0][2]) == ()                       # no encode_text: an empty prompt


def test_prepare_speaker_short_clip_with_a_transcription(model):
    stt = _Stt()
    x = TC.case("lead_trail")[1]
    sp = model.prepare_speaker(x, SR, transcription="  Given text. \n", stt=stt, encode_text=lambda t: [1, 2, 3])
    assert stt.calls == []                                    # never called
    assert sp.sample_count == 36000 - 11700 and sp.transcription == "Given text." and not sp.clipped_at_word_boundary
    assert model.got[0][0].tobytes() == x[11700:36000].tobytes() and model.got[0][2] == [1, 2, 3]
    sp = model.prepare_speaker(x, SR, transcription=" \n ")
    assert sp.transcription is None and tuple(model.got[1][2]) == ()


def test_prepare_speaker_short_clip_transcribes_after_trimming(model):
    stt = _Stt()
    x = TC.case("lead_trail")[1]
    sp = model.prepare_speaker(x, SR, stt=stt, encode_text=lambda t: [len(t)])
    (clips, word_timestamps, _), = stt.calls
    assert word_timestamps is False and clips[0].size == _len_16k(model.ctx, 36000 - 11700)        # the trimmed clip, at 16 kHz
    assert sp.transcription == "the stub's text" and model.got[0][2] == [len("the stub's text")]
    assert sp.sample_count == 24300


def test_prepare_speaker_resamples_first(model):
    x16 = np.concatenate([TC.zeros(8000), TC.tone(16000, sr=16000), TC.zeros(8000)])
    sp = model.prepare_speaker(x16, 16000)
    from mlx_swift_audio_amd import audio as A
    x24 = A.resample_audio(model.ctx, x16, 16000, 24000)
    want = T.trim_silence(model.ctx, x24, 24000, T.COSYVOICE2)
    assert sp.sample_count == want.size < x24.size and model.got[0][0].tobytes() == want.tobytes()


# ---- OuteTTS ------------------------------------------------------------------------------------------------------------------------------------
WORDS = [("The", 0.05, 0.31), (" snow", 0.31, 0.62), ("-", 0.70, 0.70), ("fell ", 0.76, 1.30), ("last", 1.40, 2.0), ("night.", 2.06, 2.28)]
LEAD, TRAIL = 7000, 9000


def test_create_speaker_profile_with_trim(ctx):
    """zeros [7000] + the 55199-sample test signal + zeros [9000].  The signal carries noise at 0.02 throughout, so every frame that holds
    at least 99 of its samples is within 60 dB of the loudest: frame 22 = [6600, 7200) is the first, frame 207 = [62100, 62700) the
    last, the bounds are (6600, 62400) and the leading trim is Float(6600) / Float(24000) = 0.275 s."""
    from mlx_swift_audio_amd import codec as HC
    raw = np.concatenate([TC.zeros(LEAD), SR_.test_signal(), TC.zeros(TRAIL)])
    b64, margin = R.bounds_f64(raw, 600, 300, 60.0)
    assert b64 == (6600, 62400) == R.bounds_literal(raw, 600, 300, 60.0) and margin >= TC.MARGIN_DB
    lead_s = LEAD / SR
    words = [(w, a + lead_s, b + lead_s, 0.9) for w, a, b in WORDS]                     # times in the untrimmed clip
    dcfg = dataclasses.replace(S.DAC_CONFIGS["dac_micro"], latent_dim=512, encoder_dim=32, encoder_rates=(2, 4, 5, 8), codebook_size=1024)
    dac = HC.DACCodec.load(ctx, dcfg, S.dac_weights(dcfg, seed=4))
    try:
        proc = O.OuteTTSAudioProcessor(ctx, dac)
        stt, stt2 = _Stt(words), _Stt(words)
        got = O.create_speaker_profile(raw, SR, stt, processor=proc, trim=T.DEFAULT, transcribe_sample_rate=SR)
        want = O.create_speaker_profile(raw[6600:62400], SR, stt2, leading_trim_seconds=float(np.float32(6600) / np.float32(SR)),
                                        transcribe_samples=raw, processor=proc, transcribe_sample_rate=SR)
        assert got == want and [w.word for w in got.words] == ["The", "snow", "-", "fell", "last", "night."]
        assert sum(len(w.c1) for w in got.words) > 100
        (clips, word_timestamps, _), = stt.calls
        assert word_timestamps is True and clips[0].tobytes() == raw.tobytes()          # the UNTRIMMED clip is transcribed
        # nothing found (top_db < 0): the whole clip with a trim of 0
        none = O.create_speaker_profile(raw, SR, _Stt(words), processor=proc, trim=T.AudioTrimConfig(top_db=-1.0), transcribe_sample_rate=SR)
        whole = O.create_speaker_profile(raw, SR, _Stt(words), processor=proc, transcribe_sample_rate=SR)
        assert none == whole != got
        with pytest.raises(ValueError, match="trim"):
            O.create_speaker_profile(raw, SR, stt, processor=proc, trim=T.DEFAULT, leading_trim_seconds=0.25)
        with pytest.raises(ValueError, match="trim"):
            O.create_speaker_profile(raw, SR, stt, processor=proc, trim=T.DEFAULT, transcribe_samples=raw)
        assert len(stt.calls) == 1                                                      # refused before anything ran
    finally:
        dac.close()


def test_trim_at_word_boundary(ctx, long_clip):
    stt = _Stt()
    r = T.trim_at_word_boundary(ctx, long_clip, SR, 30.0, stt, T.COSYVOICE2)
    assert r.clipped_at_word_boundary and r.audio.tobytes() == long_clip[11700:11700 + 704880].tobytes()
    assert r.transcription == " Hello there this is fine" and [w.word for w in r.words] == [" Hello", " there", " this", " is", " fine"]
    assert r.original_duration == float(np.float32(774000) / np.float32(SR)) and r.trimmed_duration == float(np.float32(704880) / np.float32(SR))
    assert len(stt.calls) == 1 and stt.calls[0][1] is True and abs(stt.calls[0][0][0].size - 756300 * 2 // 3) <= 1      # 16 kHz, sinc resampler
    # both fall-backs to plain truncation report max_duration, as the reference does
    for words, kept in (([], None), ([(" endless", 0.0, 30.5, 0.9), (" a", 30.5, 31.0, 0.9), (" b", 31.0, 31.4, 0.9)], [" endless", " a"])):
        r = T.trim_at_word_boundary(ctx, long_clip, SR, 30.0, _Stt(words=words))
        assert not r.clipped_at_word_boundary and r.audio.size == 720000 and r.trimmed_duration == 30.0 and r.transcription == "  the stub's text \n"
        assert (r.words if kept is None else [w.word for w in r.words]) == kept
    # already short enough after the silence trim: no transcription
    stt = _Stt()
    r = T.trim_at_word_boundary(ctx, TC.case("lead_trail")[1], SR, 30.0, stt)
    assert stt.calls == [] and r.audio.size == 24300 and r.transcription is None and r.words is None and not r.clipped_at_word_boundary
