"""The SANM memory kernel (fsmn.hip) against the restated forwardFSMN, and the GEMM's ReLU epilogue against relu(x W^T + b).

FSMN: exact up to fp32 rounding, <= 1e-5 of the largest reference value (13 fp32 additions per output; the reference runs in fp64 on the
same 16-bit-rounded values).  Measured on the MI355X: 1.6e-7 at the most."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K, D = 11, 256


def _ref(x, v, taps, left, kind):
    import _sensevoice_ref as R
    from mlx_swift_audio_amd.synthetic import round_array
    v64 = torch.from_numpy(round_array(v, kind).astype(np.float64))
    return x.astype(np.float64) + R.fsmn_memory(v64, torch.from_numpy(taps.astype(np.float64)), left).numpy()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("T", [1, 5, 10, 11, 12, 300])
def test_fsmn_add_matches_reference(ctx, T, shift, kind):
    import _sensevoice_ref as R
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    rng = np.random.default_rng(T * 10 + shift)
    x = rng.standard_normal((T, D)).astype(np.float32)
    v = rng.standard_normal((T, D)).astype(np.float32)
    taps = (0.3 * rng.standard_normal((K, D))).astype(np.float32)
    left, right = R.fsmn_pads(K, shift)
    assert (left, right) == ((5, 5) if shift == 0 else (7, 3))
    got = ops.fsmn_add(ctx, x, v, taps, left, dtype=m.BF16 if kind == "bf16" else m.F16)
    ref = _ref(x, v, taps, left, kind)
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"fsmn_add {kind} T={T} shift={shift}: relative error {err:.2e}")
    assert err <= 1e-5


@pytest.mark.parametrize("shift", [0, 2])
def test_fsmn_add_ragged_stack(ctx, shift):
    """No tap crosses a sequence's end, rows beyond it are untouched, and a sequence's rows are those of its own call bit for bit."""
    import _sensevoice_ref as R
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    lens = (12, 1, 7)
    B, T = len(lens), max(lens)
    rng = np.random.default_rng(5 + shift)
    x = rng.standard_normal((B * T, D)).astype(np.float32)
    v = rng.standard_normal((B * T, D)).astype(np.float32)
    taps = (0.3 * rng.standard_normal((K, D))).astype(np.float32)
    left, _ = R.fsmn_pads(K, shift)
    got = ops.fsmn_add(ctx, x, v, taps, left, B=B, seq_len=lens, dtype=m.BF16)
    for b, n in enumerate(lens):
        rows = slice(b * T, b * T + n)
        single = ops.fsmn_add(ctx, x[rows], v[rows], taps, left, dtype=m.BF16)
        assert np.array_equal(got[rows], single)
        ref = _ref(x[rows], v[rows], taps, left, "bf16")
        assert np.abs(single - ref).max() <= 1e-5 * np.abs(ref).max()
        assert np.array_equal(got[b * T + n:(b + 1) * T], x[b * T + n:(b + 1) * T])


def test_fsmn_add_refuses_negative_right_context(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    z = np.zeros((4, D), np.float32)
    with pytest.raises(m.MiaError, match="left context"):
        ops.fsmn_add(ctx, z, z, np.zeros((K, D), np.float32), K)          # left = K: right = -1


def _relu_ref(x, w, b, kind):
    from mlx_swift_audio_amd.synthetic import round_array
    return torch.relu(torch.from_numpy(round_array(x, kind)) @ torch.from_numpy(round_array(w, kind)).t() + torch.from_numpy(b)).numpy()


@pytest.mark.parametrize("variant", [0, 1])
def test_linear_relu(ctx, variant):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    M, N, Kd = 70, 128, 64
    rng = np.random.default_rng(variant)
    x = rng.standard_normal((M, Kd)).astype(np.float32)
    w = (rng.standard_normal((N, Kd)) / 8.0).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    got = ops.linear(ctx, x, w, b, None, act="relu", dtype=m.BF16, out_f32=True, variant=variant)
    ref = _relu_ref(x, w, b, "bf16")
    np.testing.assert_allclose(got, ref, atol=2e-4, rtol=1e-4)           # test_ops_gpu's fp32-output tolerance
    assert (got >= 0).all() and (got == 0).mean() > 0.2                    # the clamp is doing something
    got16 = ops.linear(ctx, x, w, b, None, act="relu", dtype=m.F16, out_f32=False, variant=variant)
    np.testing.assert_allclose(got16, _relu_ref(x, w, b, "f16"), atol=4e-3, rtol=2e-3)


def test_linear_relu_auto_variant_takes_the_128_tile(ctx):
    """The 8-phase kernel has no ReLU form: at a shape that fills the chip (where auto would pick it) and under variant 4 the launch runs
    the 128^2 LDS-DMA kernel instead, so the three results are the same bits."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    M, N, Kd = 4096, 4096, 128
    rng = np.random.default_rng(9)
    x = rng.standard_normal((M, Kd)).astype(np.float32)
    w = (rng.standard_normal((N, Kd)) / 11.0).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    v1 = ops.linear(ctx, x, w, b, None, act="relu", dtype=m.BF16, out_f32=False, variant=1)
    np.testing.assert_allclose(v1, _relu_ref(x, w, b, "bf16"), atol=2e-2, rtol=8e-3)    # one bf16 rounding of the output
    assert np.array_equal(v1, ops.linear(ctx, x, w, b, None, act="relu", dtype=m.BF16, out_f32=False, variant=3))
    assert np.array_equal(v1, ops.linear(ctx, x, w, b, None, act="relu", dtype=m.BF16, out_f32=False, variant=4))
