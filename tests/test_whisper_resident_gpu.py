"""GPU: the device-resident log-mel of WhisperSTT.transcribe's seek loop (mia_whisper_audio_*, mia_whisper_encode_audio_windows).

The resident path replaces host work (per-clip log-mel into numpy, numpy slicing / zero-padding / 16-bit rounding, one upload per
window) with the same arithmetic on the device, so every comparison here is EXACT: the batched mel against the single-call mel, the
window encode against model.encode of the host-sliced window, and the whole transcribe loop against resident=False.  Micro-size models.
"""
import math

import numpy as np
import pytest

from oracle import logmel as OL
from oracle import whisper as OW

pytestmark = pytest.mark.gpu


def _dt(name):
    import mlx_swift_audio_amd as m
    return m.BF16 if name == "bf16" else m.F16


def _model(ctx, dims_name, dtype_name, seed, **kw):
    from mlx_swift_audio_amd import whisper as HW
    dims = OW.DIMS[dims_name]
    weights = OW.synthetic_weights(dims, seed=seed, round_to=dtype_name, **kw)
    return dims, HW.WhisperModel.load(ctx, dims, weights, _dt(dtype_name))


def _ragged_clips(dims):
    win = dims.n_audio_ctx * 2 * 160
    return [OL.synth_clip(0, int(win * 2.3)), OL.synth_clip(1, int(win * 0.6)), OL.synth_clip(2, win), OL.synth_clip(3, 700)]


class Tok:
    def decode(self, toks):
        return "".join(" w%d" % t for t in toks)


def _split(tokens):                                      # synthetic tokenizer: every text token is a word, the eot its own group
    return [" w%d" % t for t in tokens[:-1]] + [""], [[t] for t in tokens]


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _assert_same_results(got, ref):
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.passes == r.passes and g.language == r.language and g.text == r.text
        assert len(g.segments) == len(r.segments)
        for sg, sr in zip(g.segments, r.segments):
            assert sg.tokens == sr.tokens and sg.start == sr.start and sg.end == sr.end
            assert _same_float(sg.avg_logprob, sr.avg_logprob) and _same_float(sg.no_speech_prob, sr.no_speech_prob)
            assert sg.words == sr.words                  # timing.Word dataclasses (None without word timestamps)


@pytest.mark.parametrize("dims_name", ["micro.en", "micro"])
def test_resident_mel_equals_single_call_mel(ctx, dims_name):
    """A clip's features do not depend on the batch it is computed in: every clip of a ragged batch (2.3, 0.6 and exactly 1.0
    windows, and a 700-sample clip) equals whisperLogMelSpectrogram(audio, padding: nSamples) of that clip alone, bit for bit, and the
    frames past a clip's own count are 0.0."""
    from mlx_swift_audio_amd import audio as A
    from mlx_swift_audio_amd import whisper as HW
    dims, model = _model(ctx, dims_name, "f16", seed=5)
    clips = _ragged_clips(dims)
    audio = HW.WhisperAudio(model, clips)
    F = audio.frames
    assert F == max((c.shape[0] + A.N_SAMPLES) // 160 for c in clips)
    for b, c in enumerate(clips):
        n_b = (c.shape[0] + A.N_SAMPLES) // 160
        want = A.whisper_log_mel_spectrogram(ctx, c, dims.n_mels, padding=A.N_SAMPLES)
        assert want.shape == (n_b, dims.n_mels)
        assert np.array_equal(audio.read(b, 0, n_b), want), b
        tail = audio.read(b, n_b, F - n_b)
        assert tail.shape == (F - n_b, dims.n_mels) and not tail.any(), b
    # a slice in the middle is the same slice of the whole
    assert np.array_equal(audio.read(0, 137, 50), audio.read(0, 0, F)[137:187])
    audio.close()
    model.close()


@pytest.mark.parametrize("dtype_name", ["f16", "bf16"])
def test_window_encode_equals_host_path_encode(ctx, dtype_name):
    """encode_audio_windows (slice + zero-pad + round + layout in one device kernel) against model.encode of the window sliced with numpy,
    padded with pad_or_trim_mel and rounded by to_compute_dtype: identical audio features.  Covers seek 0, a seek in the middle,
    n_valid < 2*n_audio_ctx, n_valid = 0, a repeated clip index, and stale rows (large n_valid, then small, on the same handle)."""
    from mlx_swift_audio_amd import audio as A
    from mlx_swift_audio_amd import transcribe as HT
    from mlx_swift_audio_amd import whisper as HW
    dims, model = _model(ctx, "micro", dtype_name, seed=5)
    N = 2 * dims.n_audio_ctx
    clips = _ragged_clips(dims)
    audio = HW.WhisperAudio(model, clips)
    mels = [A.whisper_log_mel_spectrogram(ctx, c, dims.n_mels, padding=A.N_SAMPLES) for c in clips]

    def both(wins):
        model.encode_audio_windows(audio, [w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
        got = model.audio_features()
        assert model.last_audio_windows == (audio, tuple(wins))
        host = np.stack([HT.pad_or_trim_mel(mels[c][s:s + n], N) for c, s, n in wins])
        model.encode(host)
        assert model.last_audio_windows is None
        want = model.audio_features()
        assert got.shape == want.shape == (len(wins), dims.n_audio_ctx, dims.n_audio_state)
        assert np.array_equal(got, want), wins
        return got

    full = both([(0, 0, N), (0, 137, N), (1, 0, N), (0, 2 * N, 60), (2, N - 3, N)])         # large n_valid on every row first
    small = both([(0, 0, 0), (0, 137, 17), (0, 137, N), (3, 1, 1), (1, 100, 20)])           # then small ones over the same rows
    assert np.array_equal(small[2], full[1])                                                # same window, other batch row
    assert np.array_equal(both([(3, 0, 0)])[0], small[0])                                   # an all-zero window is an all-zero window
    audio.close()
    model.close()


def _stt(ctx, model, dims):
    """A WhisperSTT on synthetic text rules.  A random-init model aligns at random with near-zero word probabilities, which the anomaly
    rules would discard wholesale (tests/test_timing_gpu.py): the align wrapper records the device alignment as it is, for an exact
    comparison between the two paths, and hands the loop the same words with probability 0.9."""
    import dataclasses
    from mlx_swift_audio_amd import transcribe as HT
    heads = [(dims.n_text_layer - 1, 0), (dims.n_text_layer - 1, 1)]
    stt = HT.WhisperSTT(ctx, model, Tok(), OW.synthetic_suppress_list(model.special), [220], alignment_heads=heads, split_to_word_tokens=_split)
    stt.aligned = []
    make = stt._align_fn

    def recording(*a, **k):
        fn = make(*a, **k)

        def align(*x):
            out = fn(*x)
            stt.aligned.append([[dataclasses.replace(w) for w in wt] for wt in out])
            return [[dataclasses.replace(w, probability=0.9) for w in wt] for wt in out]
        return align

    stt._align_fn = recording
    return stt


def _transcribe_both(stt, clips, seed, **kw):
    got = stt.transcribe(clips, rng=np.random.default_rng(seed), resident=True, **kw)
    aligned, stt.aligned = stt.aligned, []
    ref = stt.transcribe(clips, rng=np.random.default_rng(seed), resident=False, **kw)
    assert aligned == stt.aligned                        # every alignment call returned the same words, times and probabilities
    stt.aligned = aligned
    return got, ref


# thresholds of the loop tests.  Chosen on the CPU by driving transcribe_batch with the fp32 oracle decoder (as
# test_transcribe_loop_hip_vs_oracle does) on these clips and weights (micro, seed 157, peaky, f16; max_tokens 24, language 0): the
# level-0 avg_logprob of the four clips' first windows is -0.358, -0.673, -0.684, -0.552 and of clip 0's later windows -0.533, -0.808,
# so with logprob_threshold -0.6 clips 1 and 2 and clip 0's last window climb the temperature ladder (oracle passes [5, 3, 6, 1]) while
# clip 3 decodes once.  With the detected languages (78, 78, 78, 30) the values are -0.799, -0.526, -0.729, -0.489 and -0.655, -0.750:
# clips 0 and 2 climb, clips 1 and 3 decode once.  The nearest value is 0.048 from the threshold; the f16 build's avg_logprob differs
# from the oracle's by ~1e-3.
LOOP_KW = dict(logprob_threshold=-0.6, compression_ratio_threshold=50.0, no_speech_threshold=0.6, max_tokens=24)


@pytest.mark.parametrize("mode", ["segments", "words", "detect"])
def test_transcribe_resident_equals_host_path(ctx, mode):
    """WhisperSTT.transcribe(resident=True) against resident=False: same clips, same uniforms -> per clip the same passes, language
    and segments (tokens, start, end, avg_logprob, no_speech_prob, words), exactly -- with segment timestamps, with word timestamps,
    and with per-clip language detection.  The temperature fallback runs for a strict subset of the clips, so T > 0 passes on
    sub-batches with re-encoded windows are part of what is compared."""
    dims, model = _model(ctx, "micro", "f16", seed=157, style="peaky")
    clips = _ragged_clips(dims)
    kw = dict(LOOP_KW, language_index=None if mode == "detect" else 0, word_timestamps=mode == "words")
    # count the windows of every clip (rows decoded at temperature 0) during the resident run
    windows = [0] * len(clips)
    ragged = model.decode_ragged

    def counting(o, inits, sot_index, temperatures, *a, **k):
        if model.last_audio_windows is not None:
            for (c, _, _), t in zip(model.last_audio_windows[1], temperatures):
                windows[c] += t == 0.0
        return ragged(o, inits, sot_index, temperatures, *a, **k)

    model.decode_ragged = counting
    stt = _stt(ctx, model, dims)
    got, ref = _transcribe_both(stt, clips, 3, **kw)
    print(mode, "passes", [r.passes for r in got], "windows", windows, "segments", [len(r.segments) for r in got],
          "words", sum(len(s.words or []) for r in got for s in r.segments))
    _assert_same_results(got, ref)
    assert all(w >= 1 for w in windows)
    assert any(r.passes > w for r, w in zip(got, windows)), ([r.passes for r in got], windows)       # the fallback ran ...
    assert any(r.passes == w for r, w in zip(got, windows)), ([r.passes for r in got], windows)      # ... but not for every clip
    if mode == "words":
        assert sum(len(wt) for call in stt.aligned for wt in call) >= 4
    else:
        assert sum(len(r.segments) for r in got) >= 1
    model.close()


def test_encode_reuse_happens_and_is_invisible(ctx):
    """The .word alignment right after a level-0 decode of the same rows reuses the handle's encode: fewer encode_audio_windows calls
    than the host path's model.encode calls for the same run, identical results."""
    dims, model = _model(ctx, "micro.en", "f16", seed=77, style="peaky")
    clips = _ragged_clips(dims)
    n = {"resident": 0, "host": 0}
    enc_w, enc_h = model.encode_audio_windows, model.encode

    def count_w(*a, **k):
        n["resident"] += 1
        return enc_w(*a, **k)

    def count_h(*a, **k):
        n["host"] += 1
        return enc_h(*a, **k)

    model.encode_audio_windows, model.encode = count_w, count_h
    kw = dict(logprob_threshold=-20.0, compression_ratio_threshold=50.0, no_speech_threshold=0.6, max_tokens=24, word_timestamps=True)
    stt = _stt(ctx, model, dims)
    got, ref = _transcribe_both(stt, clips, 3, **kw)
    print("encodes", n, "passes", [r.passes for r in got], "alignment calls", len(stt.aligned))
    _assert_same_results(got, ref)
    assert stt.aligned and 0 < n["resident"] < n["host"], n
    model.close()


def test_window_argument_errors_leave_the_handle_usable(ctx):
    """Every argument error is MIA_ERR_INVALID_ARGUMENT, raised before anything is launched; the handle encodes correctly afterwards."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import whisper as HW
    dims, model = _model(ctx, "micro", "f16", seed=5)
    dims_en, model_en = _model(ctx, "micro.en", "f16", seed=5)           # 80 mels: an audio made for it does not fit the 128-mel model
    N = 2 * dims.n_audio_ctx
    clips = _ragged_clips(dims)[:2]
    audio = HW.WhisperAudio(model, clips)
    audio_en = HW.WhisperAudio(model_en, clips)
    F = audio.frames
    model.encode_audio_windows(audio, [0, 1], [10, 0], [N, 50])
    want = model.audio_features()
    bad = [
        ([2], [0], [N]),             # clip index out of range
        ([-1], [0], [N]),
        ([0], [-1], [N]),            # negative seek
        ([0], [0], [-1]),            # n_valid outside [0, 2 * n_audio_ctx]
        ([0], [0], [N + 1]),
        ([0], [F - N + 1], [N]),     # the window ends past the frames held
        ([0], [F + 5], [0]),
        ([], [], []),                # B <= 0
    ]
    for c, s, n in bad:
        with pytest.raises(m.MiaError) as e:
            model.encode_audio_windows(audio, c, s, n)
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, (c, s, n, str(e.value))
    with pytest.raises(m.MiaError) as e:
        model.encode_audio_windows(audio_en, [0], [0], [N])
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT and "mels" in str(e.value)
    with pytest.raises(m.MiaError) as e:
        model.encode_audio_windows(audio, [0, 1], [0], [N])               # arrays of different length (caught by the mirror)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    for args in ((2, 0, 1), (0, -1, 1), (0, F, 1), (0, 0, -1)):
        with pytest.raises(m.MiaError) as e:
            audio.read(*args)
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.encode_audio_windows(audio, [0, 1], [10, 0], [N, 50])
    assert np.array_equal(model.audio_features(), want)
    model.encode_audio_windows(audio, [0], [F - N], [N])                  # the last window that fits is accepted
    for x in (audio, audio_en, model, model_en):
        x.close()


def test_translate_task_on_the_gpu(ctx):
    """task="translate" reaches the sot sequence (WhisperSTT.swift:120,203): the forced prefix holds <|translate|>, and the decode equals
    decode_ragged called directly with that prefix on the same window."""
    from mlx_swift_audio_amd import transcribe as HT
    from mlx_swift_audio_amd import whisper as HW
    dims, model = _model(ctx, "micro", "f16", seed=157, style="peaky")
    st = model.special
    sup = OW.synthetic_suppress_list(st)
    clips = [OL.synth_clip(4, dims.n_audio_ctx * 2 * 160)]
    seen = []
    ragged = model.decode_ragged

    def spy(o, inits, *a, **k):
        out = ragged(o, inits, *a, **k)
        seen.append(([list(t) for t in inits], out))
        return out

    model.decode_ragged = spy
    stt = HT.WhisperSTT(ctx, model, Tok(), sup, [220])
    kw = dict(language_index=7, max_tokens=24, logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None)
    res = {task: stt.transcribe(clips, task=task, **kw)[0] for task in ("translate", "transcribe")}
    model.decode_ragged = ragged
    assert seen[0][0] == [[st.sot, st.sot + 8, st.translate]] and seen[1][0] == [[st.sot, st.sot + 8, st.transcribe]]
    assert st.translate in seen[0][0][0]
    assert (seen[0][1][0].tokens, seen[0][1][0].avg_logprob) != (seen[1][1][0].tokens, seen[1][1][0].avg_logprob)    # the task token is decoded on
    assert res["translate"].passes == 1
    audio = HW.WhisperAudio(model, clips)
    model.encode_audio_windows(audio, [0], [0], [2 * dims.n_audio_ctx])
    o = HW.DecodingOptions(task="translate", language_index=7, suppress_ids=sup, blank_ids=[220], max_tokens=24)
    direct = model.decode_ragged(o, [[st.sot, st.sot + 8, st.translate]], [0], [0.0])[0]
    audio.close()
    loop = seen[0][1][0]
    assert loop.tokens and loop.tokens == direct.tokens
    assert _same_float(loop.avg_logprob, direct.avg_logprob) and _same_float(loop.no_speech_prob, direct.no_speech_prob)
    with pytest.raises(ValueError):
        stt.transcribe(clips, task="summarise", **kw)
    with pytest.raises(ValueError):
        stt.transcribe(clips, task="summarise", resident=False, **kw)
    host = stt.transcribe(clips, task="translate", resident=False, **kw)[0]
    _assert_same_results([res["translate"]], [host])
    model.close()
