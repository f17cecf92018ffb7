"""Operator-level parity of the power-of-two real FFT of speaker_features.hip (mia_op_rfft_pow2) against numpy.fft.rfft in float64.

Tolerance (per case, computed here, not fixed): e_cpu = max|dX| / ||x||_2 of torch.fft.rfft in fp32 on the CPU against the float64
result on the same input; the GPU gets 4 x e_cpu, because two fp32 FFTs with different factorisations differ by a small constant in
the log N error term, with a floor of 2^-22.  Both errors are printed (run with -s); LABNOTES.md has the table."""
import numpy as np
import pytest
import torch

import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import ops

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -22


def _sizes(L):
    return [2, 4, 8, 64, 128, L, 2 * L, 4 * L, 1 << 19]      # 2L, 4L: the first four-step sizes, one not a square and one square


def _input(kind, n, N):
    if kind == "impulse":                                     # analytic: every bin has modulus 1
        x = np.zeros(n, np.float32)
        x[n - 1] = 1.0
        return x
    if kind == "cosine":                                      # exactly on bin N / 4 (bin 0 at N = 2)
        return np.cos(2 * np.pi * (N // 4) * np.arange(n) / N).astype(np.float32)
    return (0.1 * np.random.default_rng(11).standard_normal(n)).astype(np.float32)


@pytest.mark.parametrize("kind", ["impulse", "cosine", "noise"])
@pytest.mark.parametrize("which_n", ["N", "N/2+1", "1"])
@pytest.mark.parametrize("size", range(9))
def test_rfft_against_float64(ctx, size, which_n, kind):
    N = _sizes(ops.rfft_block(ctx))[size]
    n = {"N": N, "N/2+1": N // 2 + 1, "1": 1}[which_n]
    x = _input(kind, n, N)
    ref = np.fft.rfft(np.concatenate([x.astype(np.float64), np.zeros(N - n)]))
    if kind == "impulse":
        assert np.abs(np.abs(ref) - 1.0).max() < 1e-12
    norm = float(np.linalg.norm(x.astype(np.float64)))
    xp = torch.zeros(N, dtype=torch.float32)
    xp[:n] = torch.from_numpy(x)
    e_cpu = float(np.abs(torch.fft.rfft(xp).numpy().astype(np.complex128) - ref).max()) / norm
    got = ops.rfft_pow2(ctx, x, N)
    assert got.shape == (N // 2 + 1,)
    e_gpu = float(np.abs(got.astype(np.complex128) - ref).max()) / norm
    tol = max(4 * e_cpu, FLOOR)
    print(f"rfft N={N} n={n} {kind}: cpu fp32 {e_cpu:.3e}  gpu {e_gpu:.3e}  tol {tol:.3e}")
    assert e_gpu <= tol


def test_block_size_is_a_power_of_two_within_lds(ctx):
    L = ops.rfft_block(ctx)
    assert L >= 256 and L & (L - 1) == 0 and L * 8 <= 160 * 1024


def test_refusals(ctx):
    lib = ctx.lib
    x = np.ones(8, np.float32)
    out = np.zeros((1 << 10, 2), np.float32)
    bad = m._lib.ERR_INVALID_ARGUMENT
    assert lib.mia_op_rfft_pow2(ctx.h, x.ctypes.data, 3, 3, out.ctypes.data) == bad            # N = 3
    assert lib.mia_op_rfft_pow2(ctx.h, x.ctypes.data, 8, 1 << 25, out.ctypes.data) == bad      # N = 2^25
    assert lib.mia_op_rfft_pow2(ctx.h, x.ctypes.data, 8, 4, out.ctypes.data) == bad            # n > N
    assert lib.mia_op_rfft_pow2(ctx.h, x.ctypes.data, 8, 8, None) == bad                       # null out
    assert lib.mia_op_rfft_pow2(ctx.h, None, 8, 8, out.ctypes.data) == bad
    assert lib.mia_op_rfft_pow2(ctx.h, x.ctypes.data, 0, 8, out.ctypes.data) == bad
    assert np.all(out == 0)
    got = ops.rfft_pow2(ctx, x, 8)                                                            # and the context still works
    assert abs(got[0] - 8) < 1e-6 and np.abs(got[1:]).max() < 1e-6
