"""Cases, inputs and cached oracle results shared by the Mimi tests (test_mimi_ref.py, test_mimi_gpu.py).  Every reference is computed
once per process and handed out read-only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from _mimi_ref import MimiRef

WEIGHT_SEED = 1

# (config, frames, n_q) of every whole-clip and streamed comparison of test_mimi_gpu.py
WHOLE_CASES = [("mimi_micro", 9, 1), ("mimi_micro", 9, 4), ("mimi_micro", 40, 1), ("mimi_micro", 40, 4), ("mimi_202407", 6, 32)]
STREAM_CASES = [("mimi_micro", 21, 4), ("mimi_micro_ctx250", 140, 4), ("mimi_202407", 6, 32)]


@functools.lru_cache(None)
def config(name):
    from mlx_swift_audio_amd import synthetic
    return synthetic.MIMI_CONFIGS[name]


@functools.lru_cache(None)
def weights(name):
    from mlx_swift_audio_amd import synthetic
    return synthetic.mimi_weights(config(name), WEIGHT_SEED)


def codes(name, frames, n_q):
    cfg = config(name)
    rng = np.random.default_rng(1000 * frames + n_q)
    return rng.integers(0, cfg.quantizer_bins, (n_q, frames)).astype(np.int32)


@functools.lru_cache(None)
def oracle(name, dtype=np.float64):
    return MimiRef(config(name), weights(name), dtype)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def whole_ref(name, frames, n_q, dtype=np.float64):
    return _frozen(oracle(name, dtype).decode(codes(name, frames, n_q)))


@functools.lru_cache(None)
def stream_ref(name, frames, n_q, dtype=np.float64):
    m = oracle(name, dtype)
    m.reset()
    return _frozen(m.decode_frames(codes(name, frames, n_q)))


def rel_gap(got, ref):
    """max|got - ref| / max|ref|: the measure of every Mimi comparison (the waveform is not tanh-bounded)."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / np.abs(ref).max())
