"""The clips of tests/test_trim_gpu.py, shared with the margin certificate of tests/test_trim_host.py.  Every case is
(name, samples, frame, hop, top_db, expected bounds or None when the test computes them from the restatement).  Seeds are chosen so that
every frame of every case stays 0.01 dB or more from the threshold in float64 (the certificate); a case that misses gets another seed,
it is never dropped."""
import functools

import numpy as np

SR = 24000
MARGIN_DB = 0.01


def tone(n, level=0.5, sr=SR, freq=440.0):
    return (level * np.sin(2.0 * np.pi * freq * np.arange(n) / sr)).astype(np.float32)


def zeros(n):
    return np.zeros(n, np.float32)


def noise(seed, n, level):
    return (level * np.random.Generator(np.random.PCG64(seed)).standard_normal(n)).astype(np.float32)


def _tail_click():
    x = tone(12400, 0.01)
    x[-1] = 1.0                                            # frames 600 / 300: 40 frames end at sample 12300, the click sits at 12399
    return x


def _decaying():
    t = np.arange(2 * SR) / SR
    return (0.8 * np.exp(-4.0 * t) * np.random.Generator(np.random.PCG64(11)).standard_normal(t.size)).astype(np.float32)


def _long():
    """700 000 samples: a quiet floor, two bursts of 'speech' and a pause between them."""
    x = noise(21, 700000, 1e-5)
    x[150123:420000] += noise(22, 420000 - 150123, 0.1)
    x[500000:611111] += noise(23, 111111, 0.05)
    return x


def _sizes_22050():
    return np.concatenate([zeros(5000), tone(9000, sr=22050), zeros(7000)])


@functools.lru_cache(maxsize=None)
def cases():
    lead_trail = np.concatenate([zeros(12000), tone(24000), zeros(12000)])
    floor = np.concatenate([noise(1, 11987, 1e-5), tone(24000), noise(2, 12345, 1e-5)])
    dec = _decaying()
    return (
        ("lead_trail", lead_trail, 600, 300, 60.0, (11700, 36000)),
        ("noise_floor", floor, 600, 300, 60.0, None),
        ("no_silence", tone(24000), 600, 300, 60.0, (0, 23700)),
        ("zeros", zeros(24000), 600, 300, 60.0, (0, 23700)),
        ("short", tone(100), 600, 300, 60.0, (0, 100)),
        ("exact_frame", tone(600), 600, 300, 60.0, (0, 300)),
        ("frame_hop_m1", tone(899), 600, 300, 60.0, (0, 300)),
        ("sizes_22050", _sizes_22050(), 551, 275, 60.0, (4675, 14025)),
        ("hop_gt_frame", _sizes_22050(), 200, 330, 60.0, (4950, 14190)),
        ("tail_click", _tail_click(), 600, 300, 20.0, (0, 12000)),
        ("decaying_20", dec, 600, 300, 20.0, None),
        ("decaying_60", dec, 600, 300, 60.0, None),
        ("long", _long(), 600, 300, 60.0, None),
    )


def case(name):
    return next(c for c in cases() if c[0] == name)
