"""Restatements of the frame search of Utils/AudioTrimmer.swift (findSpeechBounds :218-274, trimSilence :142-207) for the tests.

`bounds_literal` is the Swift as written: an fp32 sum over each frame in index order, one division, a square root,
20 * log10(max(rms, 1e-10)) in fp32, the maximum, and the two scans.  The sum runs over all frames at once (one NumPy vector per
position in the frame), which keeps every frame's own order of additions.
`bounds_f64` evaluates the same rule in float64 and also returns how far, in dB, the closest frame is from the threshold: the margin
the certificate of tests/test_trim_host.py is about."""
import math

import numpy as np

f32 = np.float32


def num_frames(n: int, frame: int, hop: int) -> int:
    d = n - frame
    return max(1, (abs(d) // hop) * (1 if d >= 0 else -1) + 1)       # Swift's / truncates toward zero


def _frames(x, frame, hop):
    """(start of every frame, common length): only the single frame of a clip shorter than `frame` is short."""
    n = x.size
    nf = num_frames(n, frame, hop)
    starts = np.arange(nf, dtype=np.int64) * hop
    length = min(frame, n) if nf == 1 else frame
    assert starts[-1] + length <= n
    return starts, length


def rms_db_literal(x, frame, hop):
    x = np.ascontiguousarray(x, f32)
    starts, length = _frames(x, frame, hop)
    acc = np.zeros(starts.size, f32)
    for j in range(length):                                # sumSquares += audio[j] * audio[j], frame by frame in index order
        v = x[starts + j]
        acc = acc + v * v
    rms = np.sqrt(acc / f32(length))
    return (f32(20) * np.log10(np.maximum(rms, f32(1e-10)))).astype(f32)


def _scan(db, thr, hop, n):
    hit = np.nonzero(db >= thr)[0]
    if hit.size == 0:
        return None
    start, end = int(hit[0]) * hop, min((int(hit[-1]) + 1) * hop, n)
    return (start, end) if start < end else None


def bounds_literal(x, frame, hop, top_db):
    """findSpeechBounds: (start, end) or None."""
    x = np.ascontiguousarray(x, f32)
    if x.size == 0 or frame <= 0 or hop <= 0:
        return None
    db = rms_db_literal(x, frame, hop)
    return _scan(db, db.max() - f32(top_db), hop, x.size)


def trim_literal(x, frame, hop, top_db):
    """trimSilence: no qualifying frame falls back to frames 0 .. numFrames - 1."""
    x = np.ascontiguousarray(x, f32)
    if x.size == 0 or frame <= 0 or hop <= 0:
        return x
    b = bounds_literal(x, frame, hop, top_db)
    if b is None:
        b = (0, min(num_frames(x.size, frame, hop) * hop, x.size))
    return x[b[0]:b[1]] if b[0] < b[1] else x


def mean_squares_exact(x, frame, hop, first=0, count=None):
    """Correctly rounded float64 mean squares (math.fsum over the exact squares, one division)."""
    x = np.ascontiguousarray(x, f32).astype(np.float64)
    starts, length = _frames(x, frame, hop)
    starts = starts[first:None if count is None else first + count]
    return np.asarray([math.fsum((x[s:s + length] ** 2).tolist()) / length for s in starts], np.float64)


def bounds_f64(x, frame, hop, top_db):
    """((start, end) or None, margin): the rule in float64, and the smallest |dB - threshold| over the frames."""
    x = np.ascontiguousarray(x, f32).astype(np.float64)
    starts, length = _frames(x, frame, hop)
    idx = starts[:, None] + np.arange(length)[None, :]
    ms = (x[idx] ** 2).sum(axis=1) / length
    db = 10.0 * np.log10(np.maximum(ms, 1e-20))
    thr = db.max() - float(top_db)
    return _scan(db, thr, hop, x.size), float(np.abs(db - thr).min())
