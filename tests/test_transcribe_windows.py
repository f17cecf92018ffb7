"""CPU tests of the window-reference form of the host transcribe loop (transcribe_batch(..., window_refs=True)) and of
DecodingOptions.task through WhisperSTT, with scripted decoders / a stub model standing in for the device path.

In the window-reference form the loop never sees a mel: the callbacks get WindowRef(clip, seek, n_valid) rows.  A fake provider that
slices numpy mels with those rows must reproduce the array form exactly (results and what the callbacks are shown)."""
import zlib

import numpy as np
import pytest

from mlx_swift_audio_amd import transcribe as T
from mlx_swift_audio_amd.timing import WordTiming
from mlx_swift_audio_amd.whisper import DecodingResult, SpecialTokens


class FakeTok:
    def decode(self, toks):
        return "".join(" w%d" % t for t in toks)


ST = SpecialTokens.for_vocab(51864)
TSB = ST.timestamp_begin
N_MELS = 80


def _mels(n_samples, seed=0):
    """A distinct, recognisable mel per clip: [n // 160 + 3000, 80]."""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n // 160 + 3000, N_MELS)).astype(np.float32) for n in n_samples]


def _key(window):
    return zlib.crc32(np.ascontiguousarray(window, np.float32).tobytes())


class Script:
    """A decoder / aligner / detector whose answers depend only on the CONTENT of the window, the prompt, the temperature and the
    uniforms, so that it can be driven by either form of the loop.  Records what it is shown."""

    def __init__(self, mels, refs):
        self.mels, self.refs, self.seen = mels, refs, []

    def _windows(self, arg):
        if not self.refs:
            assert isinstance(arg, np.ndarray) and arg.shape[1:] == (3000, N_MELS)
            return arg
        assert isinstance(arg, list) and all(isinstance(w, T.WindowRef) for w in arg)
        self.seen.append([tuple(w) for w in arg])
        return np.stack([T.pad_or_trim_mel(self.mels[c][s:s + n], 3000) for c, s, n in arg])

    def decode(self, arg, prompts, temps, uniforms, langs=None):
        out = []
        for b, w in enumerate(self._windows(arg)):
            k = _key(w)
            u = 0.0 if uniforms is None else float(uniforms[b, 0])
            # low confidence at temperature 0 for windows with an odd key: those climb the fallback ladder until T >= 0.4
            bad = (k & 1) == 1 and temps[b] < 0.4
            end = 400 + (k >> 3) % 900                    # closing timestamp: 8 .. 26 s
            toks = [TSB, 10 + k % 7, 11 + len(prompts[b]) % 5, TSB + end // 2, TSB + end // 2, 12 + int(u * 5), TSB + end, TSB + end]
            out.append(DecodingResult(toks, -1.6 if bad else -0.3, 0.01))
        self.calls = getattr(self, "calls", []) + [(len(out), list(temps), [list(p) for p in prompts], None if langs is None else list(langs))]
        return out

    def align(self, arg, text_tokens, num_frames, langs=None):
        out = []
        for w, text, nf in zip(self._windows(arg), text_tokens, num_frames):
            k = _key(w)
            t0 = 0.2 + (k % 10) / 10.0
            out.append([WordTiming(" w%d" % t, [t], t0 + 1.5 * i, t0 + 1.5 * i + 1.0, 0.9) for i, t in enumerate(text)])
        return out

    def detect(self, arg):
        return [(int(_key(w) % 50), 0.5) for w in self._windows(arg)]


def _both(n_samples, **kw):
    mels = _mels(n_samples)
    word = kw.get("word_timestamps", False)
    detect = kw.get("language", 0) is None
    res, scripts = [], []
    for refs in (False, True):
        s = Script(mels, refs)
        extra = dict(align_fn=s.align if word else None, detect_fn=s.detect if detect else None)
        if refs:
            extra["window_refs"] = True
        res.append(T.transcribe_batch(None if refs else mels, n_samples, s.decode, FakeTok(), ST, rng=np.random.default_rng(5), **extra, **kw))
        scripts.append(s)
    return res[0], res[1], scripts[0], scripts[1]


def _assert_equal(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x.text, x.language, x.duration, x.passes) == (y.text, y.language, y.duration, y.passes)
        assert x.segments == y.segments                   # dataclass equality: text, start, end, tokens, probabilities, words


N3 = [480000 * 2 + 16000 * 7, 16000 * 9, 480000]


def test_window_refs_reproduce_the_array_form_with_fallback_sub_batches():
    arr, ref, s_arr, s_ref = _both(N3)
    _assert_equal(arr, ref)
    assert s_arr.calls == s_ref.calls                      # same batch sizes, temperatures, prompts at every decode call
    assert any(len(c[1]) < len(N3) and any(t > 0 for t in c[1]) for c in s_ref.calls), "no fallback sub-batch in the scenario"
    assert any(r.passes > 1 for r in ref)
    # every decode call saw one row per pending clip: (clip, that clip's seek, min(3000, content - seek)); the first call is every clip at 0
    assert s_ref.seen[0] == [(0, 0, 3000), (1, 0, 900), (2, 0, 3000)]
    for rows in s_ref.seen:
        assert [c for c, _, _ in rows] == sorted({c for c, _, _ in rows})
        for c, seek, n in rows:
            assert 0 <= seek < N3[c] // 160 and n == min(3000, N3[c] // 160 - seek)
    # a fallback level re-decodes a sub-selection of the rows of the level before, unchanged
    for prev, cur, call in zip(s_ref.seen, s_ref.seen[1:], s_ref.calls[1:]):
        if any(t > 0 for t in call[1]):
            assert set(cur) <= set(prev)
    assert max(seek for rows in s_ref.seen for _, seek, _ in rows) > 0        # later windows are addressed by seek


def test_window_refs_with_word_timestamps_and_detection():
    arr, ref, s_arr, s_ref = _both(N3, word_timestamps=True, language=None)
    _assert_equal(arr, ref)
    assert s_arr.calls == s_ref.calls
    assert s_ref.seen[0] == [(0, 0, 3000), (1, 0, 3000), (2, 0, 3000)]        # detection: mel[:3000] of every clip, padding frames included
    assert [r.language for r in ref] == [int(_key(m[:3000]) % 50) for m in _mels(N3)]
    assert all(c[3] is not None for c in s_ref.calls)                         # per-clip languages reach decode_fn
    assert any(s.words for r in ref for s in r.segments)
    # without conditioning and without thresholds the loop is one decode per window
    arr, ref, _, s_ref = _both([480000 * 3], condition_on_previous_text=False, logprob_threshold=None, compression_ratio_threshold=None)
    _assert_equal(arr, ref)
    assert all(c[1] == [0.0] and c[2] == [[]] for c in s_ref.calls) and ref[0].passes == len(s_ref.calls)


def test_array_form_is_unchanged_and_refs_need_no_mels():
    with pytest.raises(TypeError):
        T.transcribe_batch(None, [16000], lambda *a: [], FakeTok(), ST)       # the array form still needs its mels
    res = T.transcribe_batch(None, [16000], lambda m, p, t, u: [DecodingResult([TSB, 10, TSB + 50], -0.3, 0.01)], FakeTok(), ST, window_refs=True)
    assert len(res[0].segments) == 1 and res[0].passes == 1


# ---- DecodingOptions.task through WhisperSTT (WhisperSTT.swift:120,203,449) ----------------------------------------------------------
class StubModel:
    """Records what WhisperSTT asks of the model; no device."""

    def __init__(self, n_vocab):
        self.special = SpecialTokens.for_vocab(n_vocab)
        self.last_audio_windows = None
        self.inits, self.encodes = [], 0

    def encode(self, mels):
        self.encodes += 1
        self.B = len(mels)

    def decode_ragged(self, o, inits, sot_index, temps, uniforms=None):
        self.inits.append(([list(t) for t in inits], list(sot_index), o.task))
        return [DecodingResult([], 0.0, 0.0) for _ in inits]


def _stt(n_vocab):
    model = StubModel(n_vocab)
    return T.WhisperSTT(None, model, FakeTok(), [], [], alignment_heads=[(0, 0)], split_to_word_tokens=lambda t: ([], [])), model


def test_task_reaches_the_sot_sequence_of_decode_and_align(monkeypatch):
    from mlx_swift_audio_amd import timing
    mel = np.zeros((2, 3000, 128), np.float32)
    stt, model = _stt(51866)
    st = model.special
    for task, tok in (("transcribe", st.transcribe), ("translate", st.translate)):
        stt._decode_fn(3, True, 448, task)(mel, [[], [7, 8]], [0.0, 0.0], None)
        inits, sot_idx, o_task = model.inits[-1]
        assert inits == [[st.sot, st.sot + 4, tok], [st.sot_prev, 7, 8, st.sot, st.sot + 4, tok]] and sot_idx == [0, 3] and o_task == task
        stt._decode_fn(None, False, 448, task)(mel, [[], []], [0.0, 0.0], None, [5, 9])      # per-clip languages, no timestamps
        assert model.inits[-1][0] == [[st.sot, st.sot + 6, tok, st.no_timestamps], [st.sot, st.sot + 10, tok, st.no_timestamps]]
    assert [i[0][0][2] for i in model.inits[::2]] == [st.transcribe, st.translate]
    stt._decode_fn(3, True, 448)(mel, [[], []], [0.0, 0.0], None)                            # the default stays "transcribe"
    assert model.inits[-1][0][0] == [st.sot, st.sot + 4, st.transcribe]
    # _align_fn: the teacher-forced prefix handed to find_alignment
    seen = []
    monkeypatch.setattr(timing, "find_alignment", lambda model, text, frames, sot_seq, *a: seen.append(list(sot_seq)) or [[] for _ in text])
    stt._align_fn(3, "translate")(mel, [[1], [2]], [3000, 3000])
    stt._align_fn(3, "transcribe")(mel, [[1], [2]], [3000, 3000])
    stt._align_fn(None, "translate")(mel, [[1], [2]], [3000, 3000], [4, 6])                  # two languages: one call per language
    assert seen == [[st.sot, st.sot + 4, st.translate], [st.sot, st.sot + 4, st.transcribe],
                    [st.sot, st.sot + 5, st.translate], [st.sot, st.sot + 7, st.translate]]
    for make in (lambda: stt._decode_fn(3, True, 448, "summarise"), lambda: stt._align_fn(3, "Translate"),
                 lambda: stt.transcribe([np.zeros(16000, np.float32)], task="")):
        with pytest.raises(ValueError):
            make()


def test_task_leaves_english_only_vocabularies_alone(monkeypatch):
    from mlx_swift_audio_amd import timing
    mel = np.zeros((1, 3000, 80), np.float32)
    stt, model = _stt(51864)
    st = model.special
    seen = []
    monkeypatch.setattr(timing, "find_alignment", lambda model, text, frames, sot_seq, *a: seen.append(list(sot_seq)) or [[] for _ in text])
    for task in ("transcribe", "translate"):
        stt._decode_fn(0, True, 448, task)(mel, [[]], [0.0], None)
        assert model.inits[-1][0] == [[st.sot]]
        stt._align_fn(0, task)(mel, [[1]], [3000])
    assert seen == [[st.sot], [st.sot]]
