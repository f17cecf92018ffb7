"""Several Mimi streams in one pass (MimiCodec.decode_streams, mia_mimi_stream_decode_batch) against the float64 streaming restatement
(tests/_mimi_ref.py, the literal per-frame step loop), on mimi_micro (context 6, 2 positions per frame).

Bound: test_mimi_gpu.TOL["mimi_micro"] = 6.32e-06 = 8 x the restatement's own float32-vs-float64 gap, as for every streamed decode there.

Stream states (frames already decoded by single one-frame calls).  cap = context + max(P, context + 2) = 6 + max(2, 8) = 14 rows (and 14
for P = 6, n = 3, too), so a stream fed frame by frame holds fill = 2 f rows after f <= 7 frames:
  0  fresh                       3  past `context` positions (6 rows >= context: the window's low end is clipped from here on)
  2  fewer than `context` rows   7  fill = 14 = cap: the next call of any n compacts the history
"""
import ctypes as C
import functools

import numpy as np
import pytest

import _mimi_cases as mc
from test_mimi_gpu import TOL

pytestmark = pytest.mark.gpu

NAME = "mimi_micro"
PRIOR = {1: [3], 2: [0, 3], 3: [0, 2, 7], 5: [7, 0, 3, 2, 5]}          # frames each stream of an S-stream call has behind it


@pytest.fixture(scope="module")
def codec(ctx):
    from mlx_swift_audio_amd.mimi import MimiCodec
    c = MimiCodec.load(ctx, mc.config(NAME), mc.weights(NAME))
    yield c
    c.close()


def _codes(u, frames, n_q):
    return mc.codes(NAME, 40 + u, 4)[:n_q, :frames]          # stream u's own ids; the n_q = 1 stream is row 0 of the n_q = 4 one


def _prepare(codec, prior, n_q):
    """Streams brought to their states by single one-frame calls."""
    streams = [codec.new_stream() for _ in prior]
    for u, (s, f) in enumerate(zip(streams, prior)):
        for t in range(f):
            s.decode_frames(_codes(u, f, n_q)[:, t:t + 1])
    return streams


@functools.lru_cache(None)
def _ref(u, prior, n, n_q):
    m = mc.oracle(NAME)
    m.reset()
    ref = m.decode_frames(_codes(u, prior + n, n_q))[prior * mc.config(NAME).samples_per_frame:]
    ref.setflags(write=False)
    return ref


def _close(streams):
    for s in streams:
        s.close()


@pytest.mark.parametrize("n_q", [1, 4])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_batch_matches_float64(codec, S, n, n_q):
    prior = PRIOR[S]
    streams = _prepare(codec, prior, n_q)
    try:
        got = codec.decode_streams(streams, np.stack([_codes(u, f + n, n_q)[:, f:] for u, f in enumerate(prior)]))
        assert got.shape == (S, n * mc.config(NAME).samples_per_frame) and np.isfinite(got).all()
        for u, f in enumerate(prior):
            gap = mc.rel_gap(got[u], _ref(u, f, n, n_q))
            print(f"S={S} n={n} n_q={n_q} stream {u} ({f} frames behind it): rel gap {gap:.3e} ({gap / TOL[NAME] * 8:.2f} x the float32 noise)")
            assert gap <= TOL[NAME], (u, f, gap)
    finally:
        _close(streams)


@pytest.mark.parametrize("n", [1, 3])
def test_stacking_changes_nothing(codec, n):
    prior, n_q = PRIOR[5], 4
    now = [_codes(u, f + n + 1, n_q)[:, f:f + n] for u, f in enumerate(prior)]
    after = [_codes(u, f + n + 1, n_q)[:, f + n:] for u, f in enumerate(prior)]
    perm = [3, 0, 4, 2, 1]
    results = []
    for how in ("one call", "one stream per call", "permuted"):
        streams = _prepare(codec, prior, n_q)
        try:
            if how == "one call":
                a, b = codec.decode_streams(streams, np.stack(now)), codec.decode_streams(streams, np.stack(after))
            elif how == "permuted":
                pa = codec.decode_streams([streams[u] for u in perm], np.stack([now[u] for u in perm]))
                pb = codec.decode_streams([streams[u] for u in perm], np.stack([after[u] for u in perm]))
                a, b = np.empty_like(pa), np.empty_like(pb)
                a[perm], b[perm] = pa, pb
            else:
                a = np.concatenate([codec.decode_streams([s], now[u][None]) for u, s in enumerate(streams)])
                b = np.concatenate([codec.decode_streams([s], after[u][None]) for u, s in enumerate(streams)])
            results.append((a.copy(), b.copy()))
        finally:
            _close(streams)
    for a, b in results[1:]:
        assert np.array_equal(a, results[0][0]) and np.array_equal(b, results[0][1])


def test_mixing_entries_and_reset(codec):
    n_q, frames = 4, 16                                       # 16 one-frame calls: the history compacts after frame 7 and again after 14
    s = codec.new_stream()
    try:
        codes = _codes(0, frames, n_q)
        out = [s.decode_frames(codes[:, t:t + 1]).copy() if t % 2 else codec.decode_streams([s], codes[None, :, t:t + 1])[0] for t in range(frames)]
        gap = mc.rel_gap(np.concatenate(out), _ref(0, 0, frames, n_q))
        print(f"alternating entries over {frames} frames: rel gap {gap:.3e}")
        assert gap <= TOL[NAME]
        s.reset()
        again = codec.decode_streams([s], codes[None, :, :3])
        fresh = codec.new_stream()
        try:
            assert np.array_equal(again, codec.decode_streams([fresh], codes[None, :, :3]))
        finally:
            fresh.close()
    finally:
        s.close()


BAD_CALLS = ["duplicate", "two codecs", "code out of range", "capacity", "no streams", "33 streams"]


@pytest.mark.parametrize("bad", BAD_CALLS)
def test_argument_errors_leave_the_state_untouched(codec, ctx, bad):
    from mlx_swift_audio_amd import _lib
    from mlx_swift_audio_amd.mimi import MimiCodec
    prior, n_q, n = PRIOR[3], 4, 2
    spf = mc.config(NAME).samples_per_frame
    codes = np.stack([_codes(u, f + n, n_q)[:, f:] for u, f in enumerate(prior)])
    other = MimiCodec.load(ctx, mc.config(NAME), mc.weights(NAME)) if bad == "two codecs" else None
    streams, clean = _prepare(codec, prior, n_q), _prepare(codec, prior, n_q)
    try:
        hs, c, cap, S = [s.h for s in streams], codes.copy(), n * spf, len(streams)
        if bad == "duplicate":
            hs[2] = hs[0]
        elif bad == "two codecs":
            foreign = other.new_stream()
            hs[1] = foreign.h
        elif bad == "code out of range":
            c[-1, -1, -1] = mc.config(NAME).quantizer_bins
        elif bad == "capacity":
            cap -= 1
        else:
            S = 0 if bad == "no streams" else 33
        arr = (C.c_void_p * 33)(*(hs + [hs[0]] * (33 - len(hs))))
        pcm, ns = np.empty((33, n * spf), np.float32), C.c_int64(0)
        rc = ctx.lib.mia_mimi_stream_decode_batch(arr, S, c.ctypes.data, n_q, n, pcm.ctypes.data, cap, C.byref(ns), _lib.MEM_HOST)
        assert rc == _lib.ERR_INVALID_ARGUMENT, (bad, rc, ctx.lib.mia_last_error(ctx.h))
        assert np.array_equal(codec.decode_streams(streams, codes), codec.decode_streams(clean, codes))
    finally:
        _close(streams + clean)
        if other is not None:
            other.close()
