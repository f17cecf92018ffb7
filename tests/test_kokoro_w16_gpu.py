"""KokoroDecoder.use_w16 against the NumPy restatement in float64 under test_kokoro_gpu.py's own rule and bound (8 x the restatement's
float32 noise), unchanged: the path rounds no activation and the weights here are bf16 values already.  Every tap-GEMM weight of
synthetic.kokoro_weights is put on the bf16 grid; a weight-normed one gets weight_v = bf16(its fold) and weight_g = the float32 norm of
that weight_v, so the fold returns weight_v within a few fp32 ulps (asserted on the host: a condition, not a measurement -- the fold is
off by ~1e-7 relative, a bf16 half-ulp is 2^-9).  `pool`, F0_conv and N_conv are not tap GEMMs and stay as they are."""
import functools

import numpy as np
import pytest
import torch

import _kokoro_cases as kc
import _kokoro_ref as R
from test_kokoro_gpu import _cfg, _within

pytestmark = pytest.mark.gpu


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


@functools.lru_cache(maxsize=None)
def _weights(name):
    w = dict(kc.weights(name))
    for k in list(w):
        if k.endswith(".weight_v") and not k.endswith(("pool.weight_v", "F0_conv.weight_v", "N_conv.weight_v")):
            g = k[:-1] + "g"
            v = _bf16(R.weight_norm(w[k], w[g]))
            w[k], w[g] = v, np.sqrt(np.sum(v * v, axis=(1, 2), keepdims=True, dtype=np.float32))
            assert np.array_equal(_bf16(R.weight_norm(v.astype(np.float64), w[g].astype(np.float64))), v), k
        elif "noise_convs" in k and k.endswith(".weight") or k.endswith("_proj.weight"):
            w[k] = _bf16(w[k])
    return w


@functools.lru_cache(maxsize=None)
def _ref(name, dt):
    return R.KokoroRef(_cfg(name), _weights(name), dt)


@pytest.fixture(scope="module")
def models(ctx):
    from mlx_swift_audio_amd.kokoro import KokoroDecoder
    made = {}

    def get(name, on=True):
        if (name, on) not in made:
            made[name, on] = KokoroDecoder.load(ctx, _cfg(name), _weights(name))
            made[name, on].use_w16(on)
        return made[name, on]

    yield get
    for h in made.values():
        h.close()


@pytest.mark.parametrize("name,T", [("kokoro_micro", 1), ("kokoro_micro", 17), ("kokoro_82m", 8)])
def test_f0n(models, name, T):
    cfg = _cfg(name)
    rng = np.random.default_rng([T, cfg.pred_dim])
    x, s = rng.standard_normal((cfg.pred_dim, T)).astype(np.float32), rng.standard_normal(cfg.style_dim).astype(np.float32)
    got, r64, r32 = models(name).f0n(x, s), _ref(name, np.float64).f0n(x, s), _ref(name, np.float32).f0n(x, s)
    for i, curve in enumerate(("F0", "N")):
        _within(f"w16 f0n {name} T={T} {curve}", got[i], r64[i], r32[i])


@pytest.mark.parametrize("name,L", [("kokoro_micro", 2), ("kokoro_micro", 34), ("kokoro_82m", 2)])
def test_generate(models, name, L):
    cfg = _cfg(name)
    rng = np.random.default_rng([L, cfg.up_initial])
    x, s = rng.standard_normal((cfg.up_initial, L)).astype(np.float32), rng.standard_normal(cfg.style_dim).astype(np.float32)
    noise = rng.standard_normal((L * cfg.upsample_scale, cfg.n_harmonics + 1)).astype(np.float32)
    r64 = _ref(name, np.float64)
    har = r64.har(r64.sine_source(kc.f0_curve(rng, L), noise)).astype(np.float32)
    _within(f"w16 generate {name} L={L}", models(name).generate(x, s, har), r64.generate(x, s, har), _ref(name, np.float32).generate(x, s, har))


@pytest.mark.parametrize("name,T", [("kokoro_micro", 2), ("kokoro_micro", 17), ("kokoro_82m", 8)])
def test_decode(models, name, T):
    args = kc.decode_inputs(_cfg(name), T, kc.DECODE_SEEDS[(name, T)])
    (p64, s64), (p32, s32) = _ref(name, np.float64).decode(*args), _ref(name, np.float32).decode(*args)
    assert kc.branch_cut_margin(*R.stft_complex(s64), R.stft_complex(s32)[1]) >= 1.0     # test_kokoro_gpu.py's condition; the source has no tap GEMM
    _within(f"w16 decode {name} T={T}", models(name).decode(*args), p64, p32)


def test_switch(models):
    args = kc.decode_inputs(_cfg("kokoro_micro"), 17, kc.DECODE_SEEDS[("kokoro_micro", 17)])
    never, h = models("kokoro_micro", on=False), models("kokoro_micro")
    fp32, on = never.decode(*args).tobytes(), h.decode(*args).tobytes()
    h.use_w16(True)
    assert h.decode(*args).tobytes() == on                       # twice equals once
    h.use_w16(False)
    assert h.decode(*args).tobytes() == fp32                     # off: the fp32 launches, byte for byte
    h.use_w16(True)
