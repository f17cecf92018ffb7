"""Pins the NumPy restatement of Kokoro's waveform half (tests/_kokoro_ref.py) and the decisions it writes down (no GPU needed)."""
import numpy as np
import pytest

import _kokoro_cases as kc
import _kokoro_ref as R


def _cfg():
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS
    return KOKORO_CONFIGS["kokoro_micro"]


@pytest.fixture(scope="module")
def ref():
    return R.KokoroRef(_cfg(), kc.weights("kokoro_micro"), np.float64)


@pytest.mark.parametrize("T", [1, 2, 3, 17])
def test_lengths(ref, T):
    cfg = _cfg()
    asr, f0, n, s, noise = kc.decode_inputs(cfg, T, 0)
    L = 2 * T
    a, b = ref.f0n(np.zeros((cfg.pred_dim, T)) + np.arange(T), s)
    assert a.shape == b.shape == (2 * T,)
    src = ref.sine_source(f0, noise)
    assert src.shape == (300 * L,)
    assert ref.har(src).shape == (60 * L + 1, 22)
    pcm, _ = ref.decode(asr, f0, n, s, noise)
    assert pcm.shape == (600 * T,)
    # the float32 size expressions of interpolate (Interpolate.swift:37-40) give L and 300 L for every L the entry points accept
    for Lq in (1, 2, 3, 34, 9999, 20000):
        assert R.interp_size(300 * Lq, np.float32(1) / np.float32(300)) == Lq and R.interp_size(Lq, 300.0) == 300 * Lq


def test_weight_norm_fold_and_orientation():
    rng = np.random.default_rng(0)
    v, g = rng.standard_normal((5, 3, 7)), rng.standard_normal((5, 1, 1))
    w = R.weight_norm(v, g)
    for i in range(5):
        assert np.allclose(w[i], g[i, 0, 0] * v[i] / (np.sqrt((v[i] ** 2).sum()) + 1e-7), rtol=1e-14, atol=0)
    assert R.oriented(w, 7) is w                                      # last axis == input channels: as stored
    assert R.oriented(w, 5).shape == (7, 3, 5)                        # ups: [Cin][K][Cout] -> [Cout][K][Cin], every axis reversed
    assert (R.oriented(w, 5)[2, 1, 4] == w[4, 1, 2])
    p = rng.standard_normal((6, 3, 1))
    assert R.oriented(p, 6, groups=6) is p                            # pool: grouped, as stored


def test_adain_equals_its_affine_form():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((23, 10)) * 3 + 1
    fw, fb, s = rng.standard_normal((20, 4)) * 0.2, rng.standard_normal(20) * 0.1, rng.standard_normal(4)
    assert np.abs(R.adain(x, fw, fb, s) - R.adain_affine(x, fw, fb, s)).max() < 1e-12
    one = rng.standard_normal((1, 10))                                # T = 1: variance 0, the output is beta
    assert np.allclose(R.adain(one, fw, fb, s)[0], (fw @ s + fb)[10:], rtol=0, atol=1e-15)
    assert np.allclose(R.instance_norm_stats(one)[1], 1 / np.sqrt(1e-5))


def test_unwrap_is_the_identity_on_sine_valued_phases():
    rng = np.random.default_rng(2)
    p = np.sin(rng.standard_normal((11, 400)) * 10)                   # every step below 2 < pi
    assert (R.unwrap(p) == p).all()
    q = p.copy(); q[:, 100] += 2 * np.pi                              # and it is not a no-op in general
    assert not (R.unwrap(q) == q).all()


def test_rand_ini_has_no_effect(ref):
    rng = np.random.default_rng(3)
    f0 = kc.f0_curve(rng, 5); f0[0] = 200.0
    noise = rng.standard_normal((1500, 9))
    base = ref.sine_source(f0, noise)
    assert (ref.sine_source(f0, noise, rand_ini=rng.standard_normal(9)) == base).all()


def test_pointwise_conv_commutes_with_nearest_upsampling():
    rng = np.random.default_rng(4)
    x, w = rng.standard_normal((9, 6)), rng.standard_normal((4, 1, 6))
    assert (R.conv1d(np.repeat(x, 2, axis=0), w) == np.repeat(R.conv1d(x, w), 2, axis=0)).all()


def test_stft_istft_pair():
    """The pair is analysis window x synthesis window over the window SUM: x sum(w^2) / sum(w) wherever sum(w) != 0, the sums running
    over the frames that cover the sample -- 0.75 x away from the ends (the reference's own normalisation, MLXSTFT.swift:155)."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal(600)
    mag, ph = R.stft_transform(x)
    assert mag.shape == (121, 11)
    assert ((ph[:, 0] == 0) | (ph[:, 0] == np.pi)).all() and ((ph[:, 10] == 0) | (ph[:, 10] == np.pi)).all() and (ph[0] >= 0).all()
    w = R.window(20, np.float64)
    assert w[0] == 0 and np.allclose(w[1:], w[1:][::-1])
    y = R.istft(mag, ph)
    assert y.shape == x.shape
    sw, sw2 = np.zeros(620), np.zeros(620)
    for f in range(121):
        sw[5 * f:5 * f + 20] += w
        sw2[5 * f:5 * f + 20] += w * w
    assert (sw[10:610] != 0).all()
    ratio = sw2[10:610] / sw[10:610]
    assert np.abs(y - x * ratio).max() < 1e-12
    assert np.allclose(ratio[20:580], 0.75)


def test_first_samples_read_the_last_phase_row(ref):
    """interpolate1d takes floor of a negative position for the first 150 samples (xLow = -1); the gather counts that from the end, so
    they blend the LAST phase row into the first."""
    L = 6
    f0 = np.full(L, 150.0, np.float32)
    a = ref.sine_source(f0)
    f0b = f0.copy(); f0b[-1] = 170.0                                  # changes the last phase row only
    b = ref.sine_source(f0b)
    assert (ref.phase_rows(f0)[:-1] == ref.phase_rows(f0b)[:-1]).all()
    assert np.abs(a[:150] - b[:150]).max() > 1e-3
    assert (a[150:300 * (L - 2) + 150] == b[150:300 * (L - 2) + 150]).all()
