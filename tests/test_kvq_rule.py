"""The quantised KV cache's rule (tests/_kvq_rule.py) against the project's MLX-affine restatement (oracle/quant.py), on the CPU: the
helper's packed codes de-quantise through oracle.quant.dequantize_affine to the helper's own values bit for bit, and a value read back
sits within half a step of what went in."""
import numpy as np
import pytest

import _kvq_rule as R
from mlx_swift_audio_amd.synthetic import round_array
from oracle import quant as OQ


def _rows(kind, seed=0):
    """[rows, 128] of 16-bit values: seeded O(1) rows, rows with an outlier channel per group, a constant group (hi == lo), a group
    whose range is so small that its scale rounds to zero in f16 (and to a denormal-sized bf16 value), zeros, and a huge-bias group."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((40, 128)).astype(np.float32)
    x[8:16, 5] = 20.0; x[8:16, 64 + 9] = -17.0                     # planted outlier channels
    x[16, :64] = 0.75                                              # constant group
    x[17, 64:] = -3.0
    x[18, :] = 0.0
    tiny = np.float32(2.0 ** -24 if kind == "f16" else 2.0 ** -126)   # adjacent representable values: (hi - lo) / n rounds to zero (f16) / flushes nowhere (bf16)
    x[19, :64] = 0.0; x[19, 3] = tiny
    x[20, 64:] = 1024.0 + 8.0 * rng.integers(0, 3, 64)            # large bias, few distinct levels
    x[21, :64] = np.float32(3e4 if kind == "f16" else 1.5e38) * rng.choice([-1.0, 1.0], 64)      # widest range the type holds
    return round_array(x, kind)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("bits", [4, 8])
def test_packed_codes_dequantise_through_the_affine_oracle(kind, bits):
    x = _rows(kind)
    codes, s, b = R.quantise(x, bits, kind)
    assert codes.max() <= (1 << bits) - 1
    np.testing.assert_array_equal(round_array(s, kind), s)        # the pair is stored in the 16-bit type
    np.testing.assert_array_equal(round_array(b, kind), b)
    mine = R.dequantise(codes, s, b)
    theirs = OQ.dequantize_affine(R.pack(codes, bits), s, b, 64, bits)
    assert np.array_equal(mine.view(np.uint32), theirs.view(np.uint32))
    # the edge groups did what the rule says
    assert np.all(s[16, 0] == 1.0) and np.all(codes[16, :64] == 0) and np.all(mine[16, :64] == 0.75)      # hi == lo: scale 1, value = bias
    assert np.all(mine[18] == 0.0)
    if kind == "f16":
        assert s[19, 0] == 0.0 and np.all(mine[19, :64] == 0.0)   # zero range after rounding: every code reads back as the bias
    assert np.isfinite(mine).all()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("bits", [4, 8])
def test_read_back_within_half_a_step(kind, bits):
    """|x - dq(x)| <= 0.5 * scale + n * |scale - unrounded scale| (a rounded-down scale clamps the top codes) + the fp32 rounding of
    scale * code + bias; the pair's bias is exact (the minimum is a value of the type)."""
    rng = np.random.default_rng(7)
    x = round_array(rng.standard_normal((200, 128)).astype(np.float32) * rng.choice([0.3, 1.0, 4.0], (200, 1)).astype(np.float32), kind)
    x[::7, 11] += np.float32(12.0)
    x = round_array(x, kind)
    codes, s, b = R.quantise(x, bits, kind)
    dq = R.dequantise(codes, s, b)
    g = x.reshape(200, 2, 64)
    n = np.float32((1 << bits) - 1)
    s_exact = ((g.max(-1) - g.min(-1)).astype(np.float64) / float(n))
    np.testing.assert_array_equal(b, g.min(-1))
    bound = 0.5 * s.astype(np.float64) + float(n) * np.abs(s.astype(np.float64) - s_exact) + 2.0 ** -22 * np.abs(g).max(-1)
    err = np.abs(dq.reshape(200, 2, 64).astype(np.float64) - g)
    assert (err <= bound[..., None]).all(), float((err - bound[..., None]).max())
    assert err.max() > 0.25 * s.max()                              # (the bound is not vacuous: errors do reach a good part of it)
