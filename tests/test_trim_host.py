"""Host side of the AudioTrimmer mirror (mlx_swift_audio_amd/trim.py): the frame arithmetic, the word functions against the cases of the
reference's Tests/AudioTrimmerTests.swift (restated as data in tests/golden/audio_trimmer_cases.json), and the margin certificate the
exact comparison of tests/test_trim_gpu.py rests on.

Margin certificate.  The GPU test demands bounds EQUAL to the literal fp32 restatement's, while the device sums in double.  That is a
fair demand only where no frame sits close to the threshold.  The reference's own noise: an fp32 sequential sum of `frame` non-negative
terms is off by at most frame * 2^-24 relative, i.e. 10 log10(1 + 600 * 2^-24) = 1.6e-4 dB at 600 samples, and log10f adds about 1e-5 dB
at |dB| <= 200.  Every case keeps every frame at least 0.01 dB from the threshold in float64 -- more than 50 times that noise -- and on
every case the literal restatement and the float64 evaluation agree."""
import json
import os

import numpy as np
import pytest

import _trim_cases as TC
import _trim_ref as R
from mlx_swift_audio_amd import trim as T
from mlx_swift_audio_amd.timing import Word

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_trimmer_cases.json")))


def _words(rows):
    return [Word(*r) for r in rows]


def _config(over):
    return T.AudioTrimConfig(**over)


# ---- frame sizes and counts --------------------------------------------------------------------------------------------------------------
def test_frame_sizes():
    want = {8000: (200, 100), 16000: (400, 200), 22050: (551, 275), 24000: (600, 300), 44100: (1102, 551), 48000: (1200, 600)}
    for sr, (frame, hop) in want.items():
        assert (T.DEFAULT.frame_samples(sr), T.DEFAULT.hop_samples(sr)) == (frame, hop), sr
    assert T.AudioTrimConfig(frame_length=0.0).frame_samples(24000) == 0
    assert T.AudioTrimConfig(hop_length=1e-6).hop_samples(24000) == 0         # 0.024 truncates to 0: trim_silence returns its input


def test_frame_counts():
    assert T.num_frames(100, 600, 300) == 1                                    # n < frame: (-500) / 300 = -1 truncated, + 1 = 0, max 1
    assert T.num_frames(600, 600, 300) == 1 and T.num_frames(899, 600, 300) == 1 and T.num_frames(900, 600, 300) == 2
    assert T.num_frames(700000, 600, 300) == 2332 and T.num_frames(21000, 200, 330) == 64
    # the division truncates toward zero: (500 - 600) / 300 is 0 in Swift, -1 with Python's //.  Behind the max(1, .) both give one
    # frame for every n < frame; the restatement and trim.py still divide as the Swift does
    assert (500 - 600) // 300 == -1 and T.num_frames(500, 600, 300) == 1 and T.num_frames(10, 1000, 7) == 1
    for n, frame, hop in ((1, 1, 1), (5, 2, 3), (1000, 7, 1000), (12400, 600, 300), (48332, 600, 300)):
        assert T.num_frames(n, frame, hop) == R.num_frames(n, frame, hop)
        nf = T.num_frames(n, frame, hop)
        assert nf == 1 or (nf - 1) * hop + frame <= n < nf * hop + frame       # the last whole frame fits, one more would not


# ---- presets and word functions against the reference's own test cases ------------------------------------------------------------------
def test_presets():
    for name, want in GOLD["presets"].items():
        cfg = getattr(T, name)
        for k, v in want.items():
            assert getattr(cfg, k) == v, (name, k)
    assert T.DEFAULT == T.AudioTrimConfig() and T.COSYVOICE2 == T.DEFAULT and T.CHATTERBOX.top_db == 20.0


@pytest.mark.parametrize("case", GOLD["anomaly"], ids=lambda c: c["name"])
def test_word_anomaly_score(case):
    score = T.word_anomaly_score(Word(*case["word"]))
    if "equals" in case:
        assert abs(score - case["equals"]) <= case["accuracy"]
    else:
        assert score > case["greater_than"]


def test_word_anomaly_score_is_the_trimmers_own():
    from mlx_swift_audio_amd import timing
    # Float(end - start): 10.2 - 10.067 is subtracted in double and rounded once to 0.13300000131 > Float(0.133), so the score is 0;
    # timing.word_anomaly_score rounds both ends to fp32 first, gets a duration just below 0.133 and a score of 8.7e-6
    w = Word("x", 10.067, 10.2, 0.9)
    assert T.word_anomaly_score(w) == 0.0 and timing.word_anomaly_score(w) > 0.0
    w = Word("x", 100.01, 100.1, 0.9)
    assert T.word_anomaly_score(w) == float((np.float32(0.133) - np.float32(100.1 - 100.01)) * np.float32(15)) != timing.word_anomaly_score(w)
    assert T.word_anomaly_score(Word("y", 0.0, 3.0, 0.1)) == 2.0               # 1 for the probability, 3 - 2 for the duration
    assert T.word_anomaly_score(Word("z", 0.0, 0.05, 0.9)) == float((np.float32(0.133) - np.float32(0.05)) * np.float32(15))


@pytest.mark.parametrize("case", GOLD["drop"], ids=lambda c: c["name"])
def test_drop_unreliable_trailing_words(case):
    words = _words(case["words"])
    kept = T.drop_unreliable_trailing_words(words, case["audio_duration"], _config(case["config"]))
    if "count_less_than" in case:
        assert len(kept) < case["count_less_than"]
    if "count" in case:
        assert len(kept) == case["count"]
    if "max_end" in case:
        assert all(np.float32(w.end) <= np.float32(case["max_end"]) for w in kept)
    assert [w.word for w in kept] == case["added_kept"]
    assert kept == words[:len(kept)] and len(words) == len(case["words"])      # a prefix; the input list is not modified


@pytest.mark.parametrize("case", GOLD["clip_point"], ids=lambda c: c["name"])
def test_find_word_boundary_clip_point(case):
    got = T.find_word_boundary_clip_point(_words(case["words"]), case["max_duration"], GOLD["sample_rate"])
    if case.get("nil"):
        assert got is None
        return
    clip_sample, valid = got
    assert len(valid) == case["count"] and valid[-1].word == case["last"]
    assert abs(float(np.float32(clip_sample) / np.float32(GOLD["sample_rate"])) - case["clip_time"]) <= case["accuracy"]
    assert clip_sample == case["added_clip_sample"]


def test_clip_sample_is_the_fp32_product():
    # Int(Float(end) * Float(sr)), not Int(end * sr): Float(19.227) lies below 19.227 and the fp32 product 461447.97 truncates to
    # 461447 where the double product is 461448.0; Float(9.312) lies above and gives 223488 where the double is 223487.99999999997
    for end, want, in_double in ((19.227, 461447, 461448), (9.312, 223488, 223487), (1.1, 26400, 26400)):
        assert T.find_word_boundary_clip_point([Word("w", 0.0, end, 0.9)], 30.0, 24000)[0] == want
        assert int(end * 24000) == in_double


# ---- the margin certificate ----------------------------------------------------------------------------------------------------------------
def test_reference_noise_is_far_below_the_margin():
    noise_db = 10 * np.log10(1 + 600 * 2.0 ** -24) + 1e-5
    assert noise_db < 1.7e-4 and TC.MARGIN_DB > 50 * noise_db


@pytest.mark.parametrize("case", TC.cases(), ids=lambda c: c[0])
def test_margin_certificate(case):
    name, x, frame, hop, top_db, want = case
    lit = R.bounds_literal(x, frame, hop, top_db)
    b64, margin = R.bounds_f64(x, frame, hop, top_db)
    print(f"{name}: literal {lit} float64 {b64} margin {margin:.4f} dB")
    assert margin >= TC.MARGIN_DB
    assert lit == b64
    if want is not None:
        assert lit == want


def test_case_table():
    names = [c[0] for c in TC.cases()]
    assert len(names) == len(set(names)) == 13
    assert R.num_frames(TC.case("long")[1].size, 600, 300) == 2332 and R.num_frames(TC.case("hop_gt_frame")[1].size, 200, 330) == 64
    assert R.bounds_literal(TC.case("decaying_20")[1], 600, 300, 20.0)[1] != R.bounds_literal(TC.case("decaying_60")[1], 600, 300, 60.0)[1]
    x = TC.case("tail_click")[1]
    assert x[-1] == 1.0 and x.size - 1 >= (R.num_frames(x.size, 600, 300) - 1) * 300 + 600       # the click is behind the last whole frame
