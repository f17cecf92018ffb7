"""Cases, inputs and cached oracle results shared by the Mimi encode tests (test_mimi_encode_ref.py, test_mimi_encode_gpu.py,
test_marvis_prompt_gpu.py).  Every reference is computed once per process and handed out read-only."""
import dataclasses
import functools

import numpy as np

import _mimi_cases as mc
from _mimi_encode_ref import MimiEncodeRef

WEIGHT_SEED = mc.WEIGHT_SEED

# (config, n_samples) of the latent comparisons.  mimi_micro has 12 samples per frame (ratios 2, 3 reversed, stride 2): 1 sample,
# one short of a frame, a frame, one more, whole frames, and a ragged clip.  mimi_202407: 3 * 1920 gives P = 6 positions (even, no
# edge copy behind); 3 * 1920 + 777 gives P = 7 (ODD: one copy of the last row behind), T = 4.
LATENT_CASES = [("mimi_micro", n) for n in (1, 11, 12, 13, 12 * 9, 12 * 40 + 5)] + [("mimi_202407", 3 * 1920), ("mimi_202407", 3 * 1920 + 777)]
# (config, frames, seed of the latent draw) of the quantiser comparisons; 33 and 37 frames cross a 32-frame tile
# (the seeds are those of 0, 1, 2 whose smallest oracle gap is widest: test_mimi_encode_ref.py prints the table)
QUANT_CASES = [("mimi_micro", 37, 1), ("mimi_micro_bins100", 37, 2), ("mimi_202407", 1, 1), ("mimi_202407", 5, 1), ("mimi_202407", 33, 2)]
# (config, n_samples) of the end-to-end code comparisons
ENCODE_CASES = [("mimi_micro", 12 * 40 + 5), ("mimi_202407", 3 * 1920 + 777)]


@functools.lru_cache(None)
def config(name):
    if name == "mimi_micro_bins100":
        return dataclasses.replace(mc.config("mimi_micro"), quantizer_bins=100)
    if name == "mimi_micro_bins512":                 # four entry slices of 128: the tie cases
        return dataclasses.replace(mc.config("mimi_micro"), quantizer_bins=512)
    if name == "mimi_micro_nq5":                     # the codec of the marvis-micro tests: 5 codebooks of audio_vocab = 67 entries, so
        return dataclasses.replace(mc.config("mimi_micro"), quantizer_nq=5, quantizer_bins=67)      # encoded ids are model ids and back
    return mc.config(name)


@functools.lru_cache(None)
def weights(name):
    from mlx_swift_audio_amd import synthetic
    return synthetic.mimi_weights(config(name), WEIGHT_SEED, encoder=True)


@functools.lru_cache(None)
def oracle(name, dtype=np.float64):
    return MimiEncodeRef(config(name), weights(name), dtype)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(None)
def pcm(name, n_samples):
    rng = np.random.default_rng(7000 + n_samples)
    return _frozen((0.3 * rng.standard_normal(n_samples)).astype(np.float32))


@functools.lru_cache(None)
def latent_ref(name, n_samples, dtype=np.float64):
    return _frozen(oracle(name, dtype).encode_latent(pcm(name, n_samples)))


@functools.lru_cache(None)
def latent_draw(name, frames, seed):
    rng = np.random.default_rng(9000 + 131 * frames + seed)
    return _frozen(rng.standard_normal((frames, config(name).transformer.d_model)).astype(np.float32))


@functools.lru_cache(None)
def quant_ref(name, frames, seed):
    """(codes, gap) of the float64 oracle and the distance noise max|d32 - d64| of the float32 chain teacher-forced on its picks."""
    z = latent_draw(name, frames, seed)
    return _quant(name, z)


def _quant(name, z):
    codes, gap, d64 = oracle(name).quantize(z)
    _, _, d32 = oracle(name, np.float32).quantize(z, forced=codes)
    noise = max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(d32, d64))
    return _frozen(codes), _frozen(gap), noise


@functools.lru_cache(None)
def encode_ref(name, n_samples):
    """The same triple for the oracle's own latent of a clip."""
    return _quant(name, latent_ref(name, n_samples))


def rel_gap(got, ref):
    return mc.rel_gap(got, ref)
