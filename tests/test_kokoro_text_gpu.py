"""Kokoro's text half on the GPU against the NumPy restatement (tests/_kokoro_text_ref.py), under the tolerance rule of
test_kokoro_gpu.py: a GPU result must lie within 8 x the restatement's own float32-against-float64 noise.  Every test prints its
figures before it asserts; README.md ("Kokoro") lists the ratios measured on an MI355X.

The seeds of the duration cases were chosen on the CPU, with the restatement alone, as the first of 0, 1, 2, ... for which the
condition the test asserts before it compares holds: no token's float64 duration before rounding lies within 8 x its float32 noise of a
half-integer (where rint could go either way)."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library loads: the operator hook and the pipeline take torch device tensors)

import _kokoro_ref as R
import _kokoro_text_ref as TR
from _kokoro_cases import WEIGHT_SEED
from test_kokoro_gpu import _within

pytestmark = pytest.mark.gpu

# (configuration, N, speed) -> seed of _inputs
DURATION_SEEDS = {("kokoro_micro", 2, 1.0): 0, ("kokoro_micro", 3, 1.0): 0, ("kokoro_micro", 19, 1.0): 0, ("kokoro_micro", 19, 1.3): 0,
                  ("kokoro_82m", 8, 1.0): 0}


def _cfg(name):
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS
    return KOKORO_CONFIGS[name]


@functools.lru_cache(maxsize=None)
def _weights(name):
    from mlx_swift_audio_amd import synthetic
    return synthetic.kokoro_weights(_cfg(name), WEIGHT_SEED[name], text=True)


@functools.lru_cache(maxsize=None)
def _ref(name, dt):
    return TR.KokoroTextRef(_cfg(name), _weights(name), dt)


def _inputs(cfg, N, seed):
    rng = np.random.default_rng([seed, N, cfg.d_model])
    d_en = rng.standard_normal((N, cfg.d_model)).astype(np.float32)
    voice = rng.standard_normal(2 * cfg.style_dim).astype(np.float32)
    ids = rng.integers(1, cfg.n_symbols, N).astype(np.int32)
    ids[0] = ids[-1] = 0                                                            # the reference pads with 0 at both ends
    return d_en, voice, ids


@pytest.fixture(scope="module")
def models(ctx):
    from mlx_swift_audio_amd.kokoro import KokoroDecoder, KokoroText
    made = {}

    def get(name, kind=KokoroText):
        if (name, kind) not in made:
            made[name, kind] = kind.load(ctx, _cfg(name), _weights(name))
        return made[name, kind]

    get.decoder = lambda name: get(name, KokoroDecoder)
    yield get
    for m in made.values():
        m.close()


@pytest.mark.parametrize("T,In,H", [(1, 32, 32), (2, 96, 32), (17, 96, 32), (3, 640, 256), (33, 512, 256)])
def test_bilstm(ctx, T, In, H):
    from mlx_swift_audio_amd.kokoro import bilstm
    rng = np.random.default_rng([T, In, H])
    w = {k: (rng.standard_normal((4 * H, In) if k.startswith("weight_ih") else (4 * H, H) if k.startswith("weight_hh") else 4 * H) /
             np.sqrt(H)).astype(np.float32) for k in TR.LSTM_KEYS}
    x = rng.standard_normal((T, In)).astype(np.float32)
    r64 = TR.bilstm(x.astype(np.float64), {k: v.astype(np.float64) for k, v in w.items()})
    got = bilstm(ctx, x, w)
    _within(f"bilstm T={T} In={In} H={H}", got, r64, TR.bilstm(x, w), relative=False)
    assert bilstm(ctx, x, w).tobytes() == got.tobytes()


@pytest.mark.parametrize("name,N,speed", sorted(DURATION_SEEDS))
def test_durations(models, name, N, speed):
    cfg = _cfg(name)
    d_en, voice, _ = _inputs(cfg, N, DURATION_SEEDS[name, N, speed])
    s = voice[cfg.style_dim:]
    d64, dur64, raw64 = _ref(name, np.float64).durations(d_en, s, speed)
    d32, _, raw32 = _ref(name, np.float32).durations(d_en, s, speed)
    margin = (np.abs(raw64 - (np.floor(raw64) + 0.5)) / (8.0 * np.abs(raw32 - raw64))).min()
    print(f"durations {name} N={N} speed={speed}: half-integer margin {margin:.2f} (needs >= 1), durations {dur64.tolist()}")
    assert margin >= 1.0
    d, dur, raw = models(name).durations(d_en, s, speed)
    _within(f"durations {name} N={N} d", d, d64, d32, relative=False)
    _within(f"durations {name} N={N} raw", raw, raw64, raw32, relative=False)
    assert dur.dtype == np.int32 and dur.tolist() == dur64.tolist()


@pytest.mark.parametrize("name,N", [("kokoro_micro", 2), ("kokoro_micro", 19), ("kokoro_82m", 8)])
def test_encode(models, name, N):
    ids = _inputs(_cfg(name), N, 0)[2]
    _within(f"encode {name} N={N}", models(name).encode(ids), _ref(name, np.float64).encode(ids), _ref(name, np.float32).encode(ids), relative=False)


@pytest.mark.parametrize("dur", [[1, 7, 1, 3], [1, 2, 1, 1, 3, 1, 23, 1, 2, 2, 1, 1, 4, 1, 1, 2, 1, 3, 1]])
def test_align_shared_f0n(models, dur):
    name, N = "kokoro_micro", len(dur)
    cfg = _cfg(name)
    rng = np.random.default_rng(N)
    d = rng.standard_normal((N, cfg.d_model + cfg.style_dim)).astype(np.float32)
    t_en = rng.standard_normal((N, cfg.d_model)).astype(np.float32)
    s = rng.standard_normal(cfg.style_dim).astype(np.float32)
    en, asr = models(name).align(d, t_en, dur)
    want_en, want_asr = TR.align(d, t_en, np.array(dur))
    assert en.shape == (sum(dur), cfg.d_model + cfg.style_dim) and en.tobytes() == want_en.tobytes()
    assert asr.tobytes() == np.ascontiguousarray(want_asr).tobytes()
    x = models(name).shared(en)
    x64, x32 = _ref(name, np.float64).shared(en), _ref(name, np.float32).shared(en)
    _within(f"shared N={N}", x, x64, x32, relative=False)
    f0, n = models.decoder(name).f0n(x, s)
    a64, b64 = R.KokoroRef(cfg, _weights(name), np.float64).f0n(x64, s)
    a32, b32 = R.KokoroRef(cfg, _weights(name), np.float32).f0n(x32, s)
    _within(f"shared -> f0n N={N} F0", f0, a64, a32)
    _within(f"shared -> f0n N={N} N", n, b64, b32)


@pytest.mark.parametrize("forced", [None, [2, 1, 5, 1, 3]])
def test_synthesize_equals_the_parts_chained_by_hand(models, forced):
    from mlx_swift_audio_amd.kokoro import KokoroPipeline
    cfg = _cfg("kokoro_micro")
    text, dec = models("kokoro_micro"), models.decoder("kokoro_micro")
    d_en, voice, ids = _inputs(cfg, 5, 1)
    s_dec, s_pred = voice[:cfg.style_dim], voice[cfg.style_dim:]
    d, dur, _ = text.durations(d_en, s_pred, 1.1)
    dur = dur if forced is None else np.array(forced, np.int32)
    en, asr = text.align(d, text.encode(ids), dur)
    f0, n = dec.f0n(text.shared(en), s_pred)
    noise = np.random.default_rng(3).standard_normal((2 * en.shape[0] * cfg.upsample_scale, cfg.n_harmonics + 1)).astype(np.float32)
    want = dec.decode(asr, f0, n, s_dec, noise)
    pipe = KokoroPipeline(text, dec)
    got = pipe.synthesize(d_en, ids, voice, speed=1.1, noise=noise, durations=forced)
    assert pipe.last_durations.tolist() == dur.tolist() and got.shape == (600 * int(dur.sum()),) and got.tobytes() == want.tobytes()


def test_errors(ctx, models):
    from mlx_swift_audio_amd import MiaError
    from mlx_swift_audio_amd.kokoro import KokoroText, bilstm
    cfg = _cfg("kokoro_micro")
    m = models("kokoro_micro")
    w = dict(_weights("kokoro_micro"))
    del w["predictor.shared.weight_hh_l0_reverse"]
    with pytest.raises(MiaError, match="predictor.shared.weight_hh_l0_reverse"):
        KokoroText.load(ctx, cfg, w)
    W = cfg.d_model + cfg.style_dim
    with pytest.raises(MiaError, match="10000"):                                     # T beyond the decoder's limit
        m.align(np.zeros((2, W), np.float32), np.zeros((2, cfg.d_model), np.float32), [6000, 4001])
    with pytest.raises(MiaError, match="512"):                                       # N outside the supported range
        m.encode(np.zeros(513, np.int32))
    with pytest.raises(MiaError):
        m.durations(np.zeros((0, cfg.d_model), np.float32), np.zeros(cfg.style_dim, np.float32))
    for H, In in ((24, 32), (272, 32), (32, 1056)):                                  # H not a multiple of 16, H > 256, In > 1024
        bad = {k: np.zeros((4 * H, In) if k.startswith("weight_ih") else (4 * H, H) if k.startswith("weight_hh") else 4 * H, np.float32) for k in TR.LSTM_KEYS}
        with pytest.raises(MiaError, match="multiple of 16"):
            bilstm(ctx, np.zeros((2, In), np.float32), bad)
