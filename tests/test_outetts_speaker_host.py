"""Host half of OuteTTS speaker-profile creation (no GPU): the proof that the reference's forward + inverse vDSP round trip is the
closed form the pitch kernel computes, the word / code slicing rule, the trim adjustment, the JSON round trip and the engine glue."""
import json
import os

import numpy as np
import pytest

import _outetts_speaker_ref as R
from mlx_swift_audio_amd import outetts as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outetts_default_speaker.json")


def test_round_trip_is_the_closed_form():
    """calculatePitch :61-95 never multiplies the spectrum by its conjugate: autocorr[j] = C (w x)[2j] for j < 200, exactly 0 above."""
    rng = np.random.default_rng(5)
    w = R.hann_norm()
    for _ in range(20):
        fr = rng.standard_normal(R.FRAME) * rng.uniform(0.01, 1.0) * w
        lit, closed = R.autocorr_literal(fr), R.autocorr_closed(fr)
        scale = np.abs(closed).max()
        assert np.abs(lit - closed).max() <= 1e-9 * scale
        assert np.all(closed[200:] == 0.0)
        assert np.abs(lit[200:]).max() <= 1e-9 * scale          # the literal form's entries there are rounding noise of the round trip
        assert closed[0] == 0.0                                   # w[0] = 0: the voicing denominator is the bare 1e-8


def test_frame_count_rule():
    assert [R.n_frames(n) for n in (50, 80, 81, 240, 241, 399, 400, 401, 560, 561, 55199)] == [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 344]


W = [("a", 0.05, 0.31), ("b", 0.31, 0.62), ("c", 0.70, 0.70), ("d", 0.76, 1.30), ("e", 1.40, 2.0), ("f", 2.06, 2.28)]


def test_slice_words_chain():
    s = O.slice_words(W, 173, 55199, 24000)
    # first start: Int(0.05 * 75) - 20 clamps to 0; ends are Int(t * 75); the last one extends by 20 and clamps to n_codes
    assert [(x.c_start, x.c_end) for x in s] == [(0, 23), (23, 46), (46, 52), (52, 97), (97, 150), (150, 173)]
    assert [(x.a_start, x.a_end) for x in s] == [(1200, 7440), (7440, 14880), (0, 0), (18240, 31200), (33600, 48000), (49440, 54719)]      # Int(2.28 * 24000.0) = 54719: truncation of 54719.99...
    assert [x.duration for x in s] == [0.31, 0.31, 0.08, 0.6, 0.71, 0.31]


def test_slice_words_edges():
    # a zero-duration word after its predecessor's end: empty codes, default features
    s = O.slice_words([("a", 0.5, 1.0), ("b", 1.0, 1.0), ("c", 1.0, 1.2)], 200, 48000, 24000)
    assert (s[1].c_start, s[1].c_end, s[1].duration) == (75, 75, 0.0) and s[1].a_start == s[1].a_end
    assert (s[0].c_start, s[0].c_end) == (17, 75) and (s[2].c_start, s[2].c_end) == (75, 110)
    # a word whose end * sr exceeds the sample count keeps its codes and gets the default features
    s = O.slice_words([("a", 0.5, 1.0), ("b", 1.0, 2.01)], 150, 48000, 24000)
    assert s[1].a_start == s[1].a_end == 0 and (s[1].c_start, s[1].c_end) == (75, 150)
    # the last word's extension: Int(1.0 * 75) + 20 = 95 below n_codes, clamped when above
    assert O.slice_words([("a", 0.5, 1.0)], 200, 48000, 24000)[0].c_end == 95
    assert O.slice_words([("a", 0.5, 1.0)], 80, 48000, 24000)[0].c_end == 80
    # end < start chain: a word that ends before the running start is empty and does not move it
    s = O.slice_words([("a", 0.0, 1.0), ("b", 0.2, 0.4), ("c", 1.0, 1.2)], 200, 48000, 24000)
    assert [(x.c_start, x.c_end) for x in s] == [(0, 75), (75, 75), (75, 110)]
    assert (s[1].a_start, s[1].a_end) == (4800, 9600)             # its audio is still its own
    # duration at a .xx5 tie: 3 codes / 75 * 100 = 4.000 (no tie); 21 / 75 * 100 = 28.000; ties need (c * 4 / 3) = k + 0.5, i.e. none
    # for integers -- so pin the rule itself: half away from zero, where Python's round() goes to even
    assert O._round_half_away(0.5) == 1 and O._round_half_away(2.5) == 3 and O._round_half_away(-2.5) == -3 and round(2.5) == 2
    assert O._round_half_away(28.499999) == 28


def test_adjust_words_after_trim():
    words = [("gone", 0.1, 0.4), ("cut", 0.3, 0.9), ("in", 1.0, 1.5), ("clip", 2.2, 2.9), ("late", 2.6, 3.0)]
    got = O.adjust_words_after_trim(words, 0.5, 2.0)
    assert [w for w, _, _ in got] == ["cut", "in", "clip"]
    assert got[0][1] == 0.0 and got[0][2] == pytest.approx(0.4)               # start clipped at 0
    assert got[1][1:] == (pytest.approx(0.5), pytest.approx(1.0))
    assert got[2][1] == pytest.approx(1.7) and got[2][2] == 2.0                # end clipped at the trimmed duration
    assert O.adjust_words_after_trim([("edge", 0.2, 0.5)], 0.5, 2.0) == []     # ends exactly at 0: dropped (guard adjustedEnd > 0)
    assert O.adjust_words_after_trim([("edge", 2.5, 2.8)], 0.5, 2.0) == []     # starts exactly at the end: dropped


def test_json_round_trip():
    d = json.load(open(GOLDEN, encoding="utf-8"))
    p = O.SpeakerProfile.from_dict(d)
    out = p.to_dict()
    assert set(out) == set(d) and set(out["words"][0]) == set(d["words"][0]) and set(out["global_features"]) == set(d["global_features"])
    assert O.SpeakerProfile.from_dict(out) == p
    assert out["words"] == [dict(w, duration=float(w["duration"])) for w in d["words"]]
    assert out["text"] == d["text"] and out["global_features"] == d["global_features"]


def test_save_and_load(tmp_path):
    p = O.SpeakerProfile.load(GOLDEN)
    path = str(tmp_path / "speaker.json")
    p.save(path)
    assert O.SpeakerProfile.load(path) == p


class _Word:
    def __init__(self, word, start, end):
        self.word, self.start, self.end = word, start, end


class _Seg:
    def __init__(self, words):
        self.words = words


class _Result:
    def __init__(self, segments):
        self.segments = segments


class _Stt:
    def __init__(self):
        self.calls = []

    def transcribe(self, clips, word_timestamps=False, **kw):
        self.calls.append((clips, word_timestamps, kw))
        return [_Result([_Seg([_Word(" Hello", 0.2, 0.6), _Word("  ", 0.6, 0.7), _Word(" world ", 0.8, 1.4)]), _Seg(None),
                         _Seg([_Word(" late", 3.5, 3.9)])])]


class _Processor:
    sample_rate = 24000
    ctx = None

    def create_speaker_from_transcription(self, audio, text, words):
        self.got = (audio, text, words)
        return "profile"


def test_create_speaker_profile_glue():
    stt, proc = _Stt(), _Processor()
    samples = np.zeros(48000, np.float32)                        # 2 s at 24 kHz: the trimmed clip; equal rates, so no device resampling
    full = np.zeros(54000, np.float32)                           # the untrimmed clip the transcription sees
    assert O.create_speaker_profile(samples, 24000, stt, leading_trim_seconds=0.25, transcribe_samples=full, processor=proc,
                                    transcribe_sample_rate=24000) == "profile"
    (clips, wt, _), = stt.calls
    assert wt is True and len(clips) == 1 and clips[0].shape == full.shape and np.shares_memory(clips[0], full)
    audio, text, words = proc.got
    assert np.shares_memory(audio, samples) and text == "Hello world"
    assert [w for w, _, _ in words] == ["Hello", "world"]        # stripped, the blank word and the one past the end dropped
    assert words[0][1] == 0.0 and words[0][2] == pytest.approx(0.35) and words[1][1:] == (pytest.approx(0.55), pytest.approx(1.15))


def test_create_speaker_profile_errors():
    class Empty(_Stt):
        def transcribe(self, clips, word_timestamps=False, **kw):
            return [_Result([])]
    with pytest.raises(ValueError, match="no words detected"):
        O.create_speaker_profile(np.zeros(24000, np.float32), 24000, Empty(), processor=_Processor(), transcribe_sample_rate=24000)
    with pytest.raises(ValueError, match="No words remain"):
        O.create_speaker_profile(np.zeros(2400, np.float32), 24000, _Stt(), leading_trim_seconds=5.0, processor=_Processor(),
                                 transcribe_sample_rate=24000)
