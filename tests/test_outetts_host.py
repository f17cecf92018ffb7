"""The OuteTTS host side (mlx_swift_audio_amd/outetts.py) on the CPU: prompt builder (string form against id form), text rules, code
extraction and the bundled speaker profile (tests/golden/outetts_default_speaker.json, the reference's default_speaker.json).

Two places where this file follows the reference rather than a shorter statement of it:
  * per speaker word the id form holds word_start, features, time, three feature tokens, code, word_end AND the newline that follows
    every word (OuteTTSPromptProcessor.swift:313-338): 9 fixed ids per word, so the length is
    3 + |encode(merged)| + 4 + sum_words (9 + |encode(word)| + 2 pairs) + 1;
  * without a speaker the reference's string form ends after "<|audio_start|>\\n" (:242-251) while its id form still appends word_start
    (:342): the two differ by exactly that trailing id, and the test states so."""
import os

import _outetts_ref as R
from mlx_swift_audio_amd import outetts as OT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "outetts_default_speaker.json")
S = R.SPECIALS
NL = R.CHARS.index("\n")


def _golden():
    return OT.SpeakerProfile.load(GOLDEN)


def test_golden_profile_parses():
    spk = _golden()
    assert len(spk.words) == 26 and sum(min(len(w.c1), len(w.c2)) for w in spk.words) == 759
    assert spk.interface_version == 3 and spk.text.startswith("The cat watched") and spk.words[0].word == "The"
    assert (spk.global_features.energy, spk.global_features.spectral_centroid, spk.global_features.pitch) == (13, 20, 28)
    assert all(0 <= c <= 1023 for w in spk.words for c in w.c1 + w.c2)


def test_string_form_equals_id_form():
    p = R.processor()
    text = "  Hello “world” – again… "
    spk = _golden()
    assert p.get_completion_prompt_tokens(text, spk) == R.encode(p.get_completion_prompt(text, spk))
    # no speaker: the reference's id form appends word_start, its string form does not (module docstring)
    assert p.get_completion_prompt_tokens(text, None) == R.encode(p.get_completion_prompt(text, None)) + [S[OT.WORD_START]]
    assert p.get_completion_prompt(text, None) == '<|im_start|>\n<|text_start|>Hello "world" - again...<|text_end|>\n<|audio_start|>\n'


def test_two_word_speaker_spelled_out():
    p = R.processor()
    spk = OT.SpeakerProfile("hi yo", [OT.WordData("hi", 0.2, [3, 4], [5, 6], OT.AudioFeatures(1, 2, 3)),
                                      OT.WordData("yo", 0.31, [7], [8, 9], OT.AudioFeatures(4, 5, 6))])
    ch = lambda s: [R.CHARS.index(c) for c in s]
    want = ([S[OT.BOS], NL, S[OT.TEXT_START]] + ch("hi yo. ok") + [S[OT.TEXT_END], NL, S[OT.AUDIO_START], NL]
            + [S[OT.WORD_START]] + ch("hi") + [S[OT.FEATURES], S["<|t_0.20|>"], S["<|energy_1|>"], S["<|spectral_centroid_2|>"], S["<|pitch_3|>"], S[OT.CODE],
                                               R.C1_BASE + 3, R.C2_BASE + 5, R.C1_BASE + 4, R.C2_BASE + 6, S[OT.WORD_END], NL]
            + [S[OT.WORD_START]] + ch("yo.") + [S[OT.FEATURES], S["<|t_0.31|>"], S["<|energy_4|>"], S["<|spectral_centroid_5|>"], S["<|pitch_6|>"], S[OT.CODE],
                                                R.C1_BASE + 7, R.C2_BASE + 8, S[OT.WORD_END], NL]            # the shorter codebook: one pair
            + [S[OT.WORD_START]])
    assert p.get_completion_prompt_tokens(" ok ", spk) == want
    assert R.encode(p.get_completion_prompt(" ok ", spk)) == want


def test_id_form_length_and_codes():
    p = R.processor()
    spk = _golden()
    text = "It is snowing."
    ids = p.get_completion_prompt_tokens(text, spk)
    merged, sep = OT.merge_speaker_text(OT.normalize_text(text), spk.text)
    assert sep == ""                                                   # the profile's text ends in "."
    words = [w.word for w in spk.words]
    words[-1] += sep
    pairs = [min(len(w.c1), len(w.c2)) for w in spk.words]
    assert len(ids) == 3 + len(R.encode(merged)) + 4 + sum(9 + len(R.encode(w)) + 2 * n for w, n in zip(words, pairs)) + 1
    codes = [t for t in ids if t >= R.C1_BASE]
    want = [b + c for w in spk.words for a, d in zip(w.c1, w.c2) for b, c in ((R.C1_BASE, a), (R.C2_BASE, d))]
    assert codes == want
    # a speaker text that ends in a letter: the separator goes onto the last word
    spk2 = OT.SpeakerProfile("one two", [OT.WordData("one", 0.1, [1], [2]), OT.WordData("two", 0.1, [3], [4])])
    ids2 = p.get_completion_prompt_tokens("x", spk2)
    assert len(ids2) == 3 + len("one two. x") + 4 + (9 + 3 + 2) + (9 + len("two.") + 2) + 1


def test_missing_special_token_is_dropped():
    full = R.processor().get_completion_prompt_tokens("hey", _golden())
    p = R.processor(drop=(OT.FEATURES, "<|t_0.20|>"))
    gone = {S[OT.FEATURES], S["<|t_0.20|>"]}
    assert any(t in gone for t in full)
    assert p.get_completion_prompt_tokens("hey", _golden()) == [t for t in full if t not in gone]


def test_merge_speaker_text():
    assert OT.merge_speaker_text("Next one.", " It ends. ") == ("It ends. Next one.", "")
    assert OT.merge_speaker_text(" Next ", "no stop") == ("no stop. Next", ".")
    assert OT.merge_speaker_text("Next", "really?") == ("really? Next", "")
    assert OT.merge_speaker_text("次", "こんにちは") == ("こんにちは。次", "。")      # kana: no space
    assert OT.merge_speaker_text("次", "你好！") == ("你好！次", "")                                      # Han ending in a full-width "!"
    assert OT.merge_speaker_text("다음", "안녕") == ("안녕. 다음", ".")                                  # Hangul: ". "
    assert OT.merge_speaker_text("Next", "") == ("Next", "")


def test_normalize_text():
    assert OT.normalize_text("“Hi” ‘there’") == "\"Hi\" 'there'"
    assert OT.normalize_text("a–b—c") == "a-b-c"
    assert OT.normalize_text("wait…") == "wait..."
    assert OT.normalize_text("  a \t\n  b 　c  ") == "a b c"
    assert OT.normalize_text("a\x00b\x07c\x1fd\x7fe\x85f\x9fg") == "abcdefg"
    assert OT.normalize_text("a\x0bb") == "ab"            # a vertical tab is a control character, not white space, in the reference's regex


def test_extract_audio_from_tokens():
    p = R.processor()
    spk = _golden()
    toks = R.encode(p.create_codes(spk.words))
    c = p.extract_audio_from_tokens(toks)
    assert c == [[v for w in spk.words for v in w.c1[:min(len(w.c1), len(w.c2))]], [v for w in spk.words for v in w.c2[:min(len(w.c1), len(w.c2))]]]
    assert len(c[0]) == 759
    mixed = [S[OT.WORD_START], R.C1_BASE + 5, 3, R.C2_BASE + 6, R.VOCAB + 7, R.C1_BASE + 9, S[OT.EOS], R.C1_BASE + 1023]
    assert p.extract_audio_from_tokens(mixed) == [[5], [6]]            # non-code ids ignored, truncated to the shorter codebook
    assert p.extract_audio_from_tokens([1, 2, 3]) == [[], []]
