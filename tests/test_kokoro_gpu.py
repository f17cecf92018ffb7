"""Kokoro's decoder, generator, source and F0 / N blocks on the GPU against the NumPy restatement (tests/_kokoro_ref.py).

Tolerance rule (the project's own, as for Mimi): a GPU result must lie within 8 x the restatement's own float32 noise, which every test
measures itself: max |float32 run - float64 run| of the same case, relative to the float64 peak where the quantity is a waveform (or a
predicted curve).  Nothing here is tuned to the kernels.  Every test prints its figures before it asserts; README.md ("Kokoro") lists
the ratios measured on an MI355X.  AdaIN exists in one form only (materialised), so there is no fused / materialised comparison."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library loads, as in test_ops_gpu.py: the instance-norm hook takes torch device tensors)

import _kokoro_cases as kc
import _kokoro_ref as R

pytestmark = pytest.mark.gpu


def _cfg(name):
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS
    return KOKORO_CONFIGS[name]


@functools.lru_cache(maxsize=None)
def _ref(name, dt):
    return R.KokoroRef(_cfg(name), kc.weights(name), dt)


@pytest.fixture(scope="module")
def models(ctx):
    from mlx_swift_audio_amd.kokoro import KokoroDecoder
    made = {}

    def get(name):
        if name not in made:
            made[name] = KokoroDecoder.load(ctx, _cfg(name), kc.weights(name))
        return made[name]

    yield get
    for m in made.values():
        m.close()


def _within(what, got, r64, r32, relative=True):
    """|got - r64| <= 8 x |r32 - r64| (maxima; relative to the float64 peak for waveforms and curves)."""
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    scale = np.abs(r64).max() if relative else 1.0
    noise = np.abs(r32.astype(np.float64) - r64).max() / scale
    err = np.abs(got.astype(np.float64) - r64).max() / scale
    print(f"{what}: err {err:.3e}, float32 noise of the restatement {noise:.3e}, ratio {err / noise if noise else float('inf') if err else 0.0:.2f} (bound 8)")
    assert np.isfinite(got).all() and err <= 8.0 * noise, (what, err, noise)


@pytest.mark.parametrize("T,C", [(1, 32), (2, 66), (63, 130), (64, 130), (65, 1090), (4801, 128)])
def test_instance_norm(ctx, T, C):
    from mlx_swift_audio_amd.kokoro import instance_norm
    rng = np.random.default_rng([T, C])
    x = rng.standard_normal((T, C)).astype(np.float32)
    x[:, 3] = (100.0 + 0.01 * rng.standard_normal(T)).astype(np.float32)          # the mean dwarfs the spread
    x[:, 5] = np.float32(-7.25)                                                    # constant
    ld = (C + 31) // 32 * 32
    m64, r64 = R.instance_norm_stats(x.astype(np.float64))
    m32, r32 = R.instance_norm_stats(x)
    mean, rstd = instance_norm(ctx, x, ld)
    _within(f"instance_norm {T}x{C} mean", mean, m64, m32, relative=False)
    _within(f"instance_norm {T}x{C} rstd", rstd, r64, r32, relative=False)
    mean2, rstd2 = instance_norm(ctx, x, ld)
    assert mean.tobytes() == mean2.tobytes() and rstd.tobytes() == rstd2.tobytes()


@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("L", [2, 3, 33])
def test_source(models, L, with_noise):
    cfg = _cfg("kokoro_micro")
    rng = np.random.default_rng([L, int(with_noise)])
    f0 = kc.f0_curve(rng, L)
    f0[0], f0[-1] = 220.0, 5.0                                                      # both kinds present at every L
    noise = rng.standard_normal((L * cfg.upsample_scale, cfg.n_harmonics + 1)).astype(np.float32) if with_noise else None
    s64 = _ref("kokoro_micro", np.float64).sine_source(f0, noise)
    s32 = _ref("kokoro_micro", np.float32).sine_source(f0, noise)
    src, har = models("kokoro_micro").source(f0, noise)
    assert har.shape == (60 * L + 1, 22)
    _within(f"source L={L} noise={with_noise}", src, s64, s32, relative=False)
    # har as complex numbers, against the transform of the restatement's own source in both precisions
    re64, im64 = R.stft_complex(s64)
    re32, im32 = R.stft_complex(s32)
    mag, ph = har[:, :11].astype(np.float64), har[:, 11:].astype(np.float64)
    _within(f"har re L={L}", (mag * np.cos(ph)).astype(np.float32), re64, re32, relative=False)
    _within(f"har im L={L}", (mag * np.sin(ph)).astype(np.float32), im64, im32, relative=False)
    for b in (0, 10):
        assert np.all((har[:, 11 + b] == 0.0) | (har[:, 11 + b] == np.float32(np.pi))), b
        assert not np.signbit(har[:, 11 + b]).any()


@pytest.mark.parametrize("name,T", [("kokoro_micro", 1), ("kokoro_micro", 2), ("kokoro_micro", 17), ("kokoro_micro", 64), ("kokoro_82m", 8)])
def test_f0n(models, name, T):
    cfg = _cfg(name)
    rng = np.random.default_rng([T, cfg.pred_dim])
    x = rng.standard_normal((cfg.pred_dim, T)).astype(np.float32)
    s = rng.standard_normal(cfg.style_dim).astype(np.float32)
    a64, b64 = _ref(name, np.float64).f0n(x, s)
    a32, b32 = _ref(name, np.float32).f0n(x, s)
    f0, n = models(name).f0n(x, s)
    _within(f"f0n {name} T={T} F0", f0, a64, a32)
    _within(f"f0n {name} T={T} N", n, b64, b32)


@pytest.mark.parametrize("name,L", [("kokoro_micro", 2), ("kokoro_micro", 3), ("kokoro_micro", 34), ("kokoro_micro", 80), ("kokoro_82m", 2), ("kokoro_82m", 16)])
def test_generate(models, name, L):
    cfg = _cfg(name)
    rng = np.random.default_rng([L, cfg.up_initial])
    x = rng.standard_normal((cfg.up_initial, L)).astype(np.float32)
    s = rng.standard_normal(cfg.style_dim).astype(np.float32)
    f0 = kc.f0_curve(rng, L)
    noise = rng.standard_normal((L * cfg.upsample_scale, cfg.n_harmonics + 1)).astype(np.float32)
    r64 = _ref(name, np.float64)
    har = r64.har(r64.sine_source(f0, noise)).astype(np.float32)                    # pinned: both runs and the GPU read these values
    assert har.shape[0] == 60 * L + 1
    p64 = r64.generate(x, s, har)
    p32 = _ref(name, np.float32).generate(x, s, har)
    pcm = models(name).generate(x, s, har)
    assert pcm.shape == (300 * L,)
    _within(f"generate {name} L={L}", pcm, p64, p32)


@pytest.mark.parametrize("name,T", sorted(kc.DECODE_SEEDS))
def test_decode(models, name, T):
    cfg = _cfg(name)
    asr, f0, n, s, noise = kc.decode_inputs(cfg, T, kc.DECODE_SEEDS[(name, T)])
    p64, s64 = _ref(name, np.float64).decode(asr, f0, n, s, noise)
    p32, s32 = _ref(name, np.float32).decode(asr, f0, n, s, noise)
    # the condition, on the restatement alone: no phase of the source STFT sits on the branch cut within the float32 noise
    re64, im64 = R.stft_complex(s64)
    _, im32 = R.stft_complex(s32)
    margin = kc.branch_cut_margin(re64, im64, im32)
    print(f"decode {name} T={T}: branch-cut margin {margin:.2f} (needs >= 1)")
    assert margin >= 1.0
    m = models(name)
    assert m.output_len(T) == 600 * T
    pcm = m.decode(asr, f0, n, s, noise)
    assert pcm.shape == (600 * T,)
    _within(f"decode {name} T={T}", pcm, p64, p32)
    assert m(asr, f0, n, s, noise).tobytes() == pcm.tobytes()


def test_errors(ctx, models):
    from mlx_swift_audio_amd import MiaError
    from mlx_swift_audio_amd.kokoro import KokoroDecoder
    cfg = _cfg("kokoro_micro")
    m = models("kokoro_micro")
    s = np.zeros(cfg.style_dim, np.float32)
    with pytest.raises(MiaError):
        m.decode(np.zeros((cfg.dim_in, 0), np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), s)
    with pytest.raises(MiaError):
        m.f0n(np.zeros((cfg.pred_dim, 0), np.float32), s)
    w = dict(kc.weights("kokoro_micro"))
    del w["decoder.generator.noise_res.1.adain2.2.fc.weight"]
    with pytest.raises(MiaError, match="decoder.generator.noise_res.1.adain2.2.fc.weight"):
        KokoroDecoder.load(ctx, cfg, w)
    bare = KokoroDecoder.load(ctx, cfg, kc.weights("kokoro_micro", predictor=False))
    try:
        with pytest.raises(MiaError, match="predictor"):
            bare.f0n(np.zeros((cfg.pred_dim, 4), np.float32), s)
    finally:
        bare.close()
