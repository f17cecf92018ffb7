"""The CPU restatement of Fun-ASR's audio half (tests/_sensevoice_ref.py) pinned on the CPU, and the bounds of the GPU tests shown to be
satisfiable and able to fail before anything runs on a GPU.

Rounded reference (every GEMM operand and the stored q | k | v / attention output rounded to the 16-bit type, nothing else changed)
against the fp32 reference, worst over both micro configs, T in {1, 7, 64, 65, 201} and feature amplitudes 1 and 1e-3:
    enc_out   max / mean |d|        bf16 0.0225 / 0.0037   (bound 0.06 / 0.008)     f16 0.0032 / 0.0005   (bound 0.01 / 0.0015)
    adaptor   the same over std     bf16 0.0213 / 0.0051                            f16 0.0029 / 0.0007
so the Whisper encoder's bounds carry over unchanged; no bound had to be widened to twice the rounded reference's error.

Discriminating checks (modified fp32 reference against the unmodified one; the bf16 bound is the widest, 0.06 / 0.008):
    FSMN taps zeroed                      max / mean 2.6 .. 3.9 / 0.60 .. 0.70 at either amplitude
    layer 0 given a residual              4.8 .. 6.5 / 1.0 on unit-variance features; on features of amplitude 1e-3 only 0.04 / 0.008, the
                                          residual itself being that small
    sqrt(encoder_dim) input scale dropped on unit-variance features EXACTLY as large as LayerNorm's eps lets it be, 0.000 / 0.0000 (< 1e-4): layer 0
                                          has no residual, so the scaled input meets nothing but norm1, which divides the scale out again.
                                          The scale is observable only where eps = 1e-5 competes with the row variance: on features of
                                          amplitude 1e-3 (variance 1e-6 unscaled, 2.6e-4 scaled) dropping it moves enc_out by 2.3 .. 2.8 / 0.45.
That is why the GPU tests of tests/test_sensevoice_gpu.py run every length at BOTH amplitudes: unit variance is what CMVN delivers and
shows a wrong layer-0 residual, 1e-3 shows a missing input scale."""
import os

import numpy as np
import pytest
import torch

import _sensevoice_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "funasr_fbank.npz")


def _cfg(name):
    from mlx_swift_audio_amd import funasr
    return funasr.SENSEVOICE_CONFIGS[name]


def _weights(name, kind=None, seed=1):
    from mlx_swift_audio_amd import synthetic
    return synthetic.sensevoice_weights(_cfg(name), seed=seed, round_to=kind)


# ---- the restatement against torch's own operators ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sensevoice-micro", "sensevoice-micro-shift2"])
def test_sanm_attention_against_sdpa_and_grouped_conv(name):
    cfg, w = _cfg(name), _weights(name)
    ref = R.SenseVoiceRef(cfg, w)
    D, H, K = cfg.encoder_dim, cfg.n_heads, cfg.kernel_size
    p = "audio_encoder.encoders.0.self_attn"
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((37, D)).astype(np.float32))
    got = ref.sanm_attention(x, p)
    wt = {k: torch.from_numpy(v) for k, v in w.items()}
    qkv = torch.nn.functional.linear(x, wt[p + ".linear_q_k_v.weight"], wt[p + ".linear_q_k_v.bias"])
    q, k, v = (t.reshape(37, H, D // H).transpose(0, 1)[None] for t in qkv.split(D, dim=-1))
    att = torch.nn.functional.scaled_dot_product_attention(q, k, v)[0].transpose(0, 1).reshape(37, D)
    left = (K - 1) // 2 + cfg.sanm_shift
    assert (left, K - 1 - left) == ((5, 5) if cfg.sanm_shift == 0 else (7, 3))
    vv = qkv[:, 2 * D:].t()[None]                                               # [1, D, T]
    mem = torch.nn.functional.conv1d(torch.nn.functional.pad(vv, (left, K - 1 - left)), wt[p + ".fsmn_block.weight"], groups=D)[0].t()
    want = torch.nn.functional.linear(att, wt[p + ".linear_out.weight"], wt[p + ".linear_out.bias"]) + mem + qkv[:, 2 * D:]
    assert torch.allclose(got, want, atol=2e-5, rtol=1e-5)


def test_fsmn_taps_accepts_both_layouts():
    w = np.random.default_rng(1).standard_normal((8, 1, 11)).astype(np.float32)
    a = R.fsmn_taps(w, 8)
    b = R.fsmn_taps(np.ascontiguousarray(w.transpose(0, 2, 1)), 8)
    assert a.shape == (11, 8) and np.array_equal(a, b) and a[3, 5] == w[5, 0, 3]


def test_layer_norm_against_torch():
    x = torch.from_numpy(np.random.default_rng(2).standard_normal((9, 560)).astype(np.float32)) * 3 + 1
    ln = torch.nn.LayerNorm(560, eps=1e-5)
    with torch.no_grad():
        ln.weight.copy_(torch.linspace(0.5, 1.5, 560)); ln.bias.copy_(torch.linspace(-1, 1, 560))
        assert torch.allclose(R.layer_norm(x, ln.weight, ln.bias), ln(x), atol=2e-6, rtol=1e-6)


@pytest.mark.parametrize("T", [1, 5, 6, 7, 13, 100])
def test_lfr_rows_are_clamped_stacks(T):
    f = np.random.default_rng(T).standard_normal((T, 80))
    got = R.apply_lfr(f)
    assert got.shape == (-(-T // 6), 560)
    for i in range(got.shape[0]):
        want = np.concatenate([f[min(max(6 * i - 3 + m, 0), T - 1)] for m in range(7)])
        assert np.array_equal(got[i], want)


@pytest.mark.parametrize("L,frames,rows", [(160, 2, 1), (959, 6, 1), (960, 7, 2), (16000, 101, 17), (16001, 101, 17)])
def test_feature_lengths(L, frames, rows):
    assert R.n_frames_of(L) == frames and R.t_lfr_of(L) == rows
    if L > 200:
        assert R.features(np.random.default_rng(L).standard_normal(L) * 0.1).shape == (rows, 560)


def test_cmvn_is_population_variance():
    f = np.random.default_rng(3).standard_normal((11, 4)) * 2 + 5
    got = R.apply_cmvn(f)
    assert np.allclose(got, (f - f.mean(0)) / (f.std(0, ddof=0) + 1e-6), atol=1e-12)
    assert abs(got.std(0, ddof=0) - 1).max() < 1e-5


def test_filterbank_frozen():
    """Shape, each filter's first / last non-zero bin (weights above 1e-9: an edge that lands on a bin within rounding is not counted) and
    the weights themselves against tests/golden/funasr_fbank.npz, frozen from this restatement; the grid quirk is pinned separately."""
    fb = R.mel_filters()
    g = np.load(GOLDEN)
    assert fb.shape == (80, 200) == tuple(g["shape"])
    nz = fb > 1e-9
    first = nz.argmax(axis=1)
    last = 199 - nz[:, ::-1].argmax(axis=1)
    assert np.array_equal(first, g["first"]) and np.array_equal(last, g["last"])
    assert np.allclose(fb, g["weights"], rtol=1e-9, atol=1e-15)
    # the reference's grid is linspace(0, 8000, 200), not k * 40 Hz (FunASRAudio.swift:363-364): its bin 199 sits at 8000 Hz, the last
    # filter's upper edge, and carries no weight; on a 40 Hz grid bin 199 = 7960 Hz would lie inside that filter
    f_pts = 700.0 * (10 ** (np.linspace(0, 2595 * np.log10(1 + 8000 / 700), 82) / 2595) - 1)
    assert last[79] == 198 and f_pts[80] < 199 * 40.0 < f_pts[81]


# ---- the GPU tests' bounds: satisfiable, and able to fail ---------------------------------------------------------------------------
LENGTHS = (1, 7, 64, 65, 201)


def _feats(T, amp):
    return (amp * np.random.default_rng(T).standard_normal((T, 560))).astype(np.float32)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["sensevoice-micro", "sensevoice-micro-shift2"])
def test_rounded_reference_fits_the_bounds(name, kind):
    cfg, w = _cfg(name), _weights(name, kind)
    ref, rnd = R.SenseVoiceRef(cfg, w), R.SenseVoiceRef(cfg, w, round_kind=kind)
    b_max, b_mean = R.BOUNDS[kind]
    for T in LENGTHS:
        for amp in (1.0, 1e-3):
            e0, a0 = ref.encode_audio(_feats(T, amp))
            e1, a1 = rnd.encode_audio(_feats(T, amp))
            de, da = np.abs(e1 - e0), np.abs(a1 - a0) / a0.std()
            assert de.max() <= b_max and de.mean() <= b_mean, (T, amp, de.max(), de.mean())
            assert da.max() <= b_max and da.mean() <= b_mean, (T, amp, da.max(), da.mean())


@pytest.mark.parametrize("mutate,amp", [("zero_fsmn", 1.0), ("zero_fsmn", 1e-3), ("layer0_residual", 1.0), ("no_input_scale", 1e-3)])
@pytest.mark.parametrize("name", ["sensevoice-micro", "sensevoice-micro-shift2"])
def test_bounds_can_fail(name, mutate, amp):
    """Each modification moves enc_out by 5x the widest (bf16) bound or more, in the maximum and in the mean (module docstring for the
    amplitude each one needs)."""
    cfg, w = _cfg(name), _weights(name)
    b_max, b_mean = R.BOUNDS["bf16"]
    for T in (7, 65):
        e0, _ = R.SenseVoiceRef(cfg, w).encode_audio(_feats(T, amp))
        e1, _ = R.SenseVoiceRef(cfg, w, mutate=mutate).encode_audio(_feats(T, amp))
        d = np.abs(e1 - e0)
        assert d.max() >= 5 * b_max and d.mean() >= 5 * b_mean, (T, d.max(), d.mean())


def test_input_scale_is_invisible_on_unit_variance_features():
    """The other half of the docstring's statement: after CMVN-like features the dropped scale changes nothing a test could see."""
    cfg, w = _cfg("sensevoice-micro"), _weights("sensevoice-micro")
    e0, _ = R.SenseVoiceRef(cfg, w).encode_audio(_feats(65, 1.0))
    e1, _ = R.SenseVoiceRef(cfg, w, mutate="no_input_scale").encode_audio(_feats(65, 1.0))
    assert np.abs(e1 - e0).max() < 1e-3
