"""The context's one device-table cache (csrc/mia_internal.h: mia_tables_find / mia_tables_build) seen from outside: sets under different
keys stay apart, a cache hit computes what the first call computed, and tables are per context.  A 0.5 s clip at 16 kHz and one at
24 kHz, every front end that caches tables, two contexts.  Only equality of ordinary results is asserted."""
import numpy as np
import pytest

import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import audio as A
from mlx_swift_audio_amd import audio_io, funasr, outetts
from oracle import logmel as OL

pytestmark = pytest.mark.gpu


def front_end_calls(ctx, y16, y24):
    """Every call that builds or hits a table set, repeats checked bit for bit against their first call; {name: first result}."""
    r = {}

    def call(name, fn):
        got = np.asarray(fn())
        assert got.size > 0 and np.isfinite(got).all(), name
        if name in r:
            assert np.array_equal(got, r[name]), f"{name}: a repeat differs from its first call"
        r.setdefault(name, got)

    # log-mel: key (n_mels, window kind)
    for n_mels in (80, 128, 80):
        call(f"whisper{n_mels}", lambda: A.whisper_log_mel_spectrogram(ctx, y16, n_mels))
    call("s3_128", lambda: A.s3_log_mel_spectrogram(ctx, y16, 128))
    call("whisper128", lambda: A.whisper_log_mel_spectrogram(ctx, y16, 128))
    call("s3_128", lambda: A.s3_log_mel_spectrogram(ctx, y16, 128))
    assert not np.array_equal(r["s3_128"].T, r["whisper128"])          # the two windows of one n_mels are two sets
    # sinc resampler: key (from, to)
    for a, b, y in ((24000, 16000, y24), (16000, 24000, y16), (24000, 16000, y24)):
        call(f"sinc{a}to{b}", lambda: audio_io.resample(ctx, y, a, b))
    assert r["sinc24000to16000"].size == y16.size and r["sinc16000to24000"].size == y24.size
    # the singletons, twice each
    sa = outetts.SpeakerAudio(ctx, y24, 24000)
    for _ in range(2):
        call("s3gen_mel", lambda: A.s3gen_mel_spectrogram(ctx, y24))
        call("funasr", lambda: funasr.features(ctx, [y16])[0])
        call("speaker", lambda: sa.raw_features([(0, len(sa)), (1000, 5000)]))
    sa.close()
    return r


def test_keys_hits_and_two_contexts():
    y16, y24 = OL.synth_clip(0, 8000), OL.synth_clip(1, 12000)
    c1 = m.Context(0)
    r1 = front_end_calls(c1, y16, y24)
    c2 = m.Context(0)                      # created afterwards: it builds its own tables
    r2 = front_end_calls(c2, y16, y24)
    c1.close()
    c2.close()
    assert r1.keys() == r2.keys() and len(r1) == 8
    for name in r1:
        assert np.array_equal(r1[name], r2[name]), f"{name}: the two contexts differ"
