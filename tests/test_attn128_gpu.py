"""mia_op_attention_h128 (attn128.hip) against an fp64 softmax(q k^T d_k^-0.5) v of the same 16-bit-rounded inputs.

The kernel's tiles: a workgroup owns a query tile of 128 rows (four waves of 32), and walks the keys in tiles of 64.  T covers 1, 2 and one
below, at and one above 32 (a wave's queries), 64 (the key tile) and 128 (the query tile), plus 193 (three full key tiles and a one-key tail).

Bound, per element: 1 ulp of the output type at the output's magnitude (the output's own rounding) + 2^-8 (bf16) | 2^-11 (f16) of the
largest |v| (P is rounded to the 16-bit type before P V: sum_j p_j d_j v_j / sum_j p_j with |d_j| <= half an ulp).  Measured on the
MI355X (worst error / bound over all cases): bf16 0.25, f16 0.28 (both at T = 2); T >= 31: 0.09 .. 0.18; the spiked case 0.41 / 0.40."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193]


def _kinds():
    import mlx_swift_audio_amd as m
    return {"bf16": (m.BF16, 2.0 ** -8, 7), "f16": (m.F16, 2.0 ** -11, 10)}


def _ref(qkv, B, T, H, kind, seq_len=None):
    from mlx_swift_audio_amd.synthetic import round_array
    x = round_array(qkv, kind).astype(np.float64)
    D = H * 128
    out = np.zeros((B * T, D))
    for b in range(B):
        n = T if seq_len is None else int(seq_len[b])
        r = x[b * T:b * T + n]
        for h in range(H):
            q, k, v = (r[:, i * D + h * 128:i * D + (h + 1) * 128] for i in range(3))
            s = q @ k.T * 128 ** -0.5
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[b * T:b * T + n, h * 128:(h + 1) * 128] = (p / p.sum(axis=1, keepdims=True)) @ v
    return out, float(np.abs(x[:, 2 * D:]).max())


def _bound(ref, got, vmax, rel, mant_bits):
    mag = np.maximum(np.abs(ref), np.abs(got))
    expo = np.floor(np.log2(np.maximum(mag, 2.0 ** -14)))          # (f16 subnormals share the ulp of 2^-14)
    return 2.0 ** (expo - mant_bits) + rel * vmax


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("T", EDGES)
def test_attention_h128_matches_reference(ctx, T, H, kind):
    from mlx_swift_audio_amd import ops
    dtype, rel, mant = _kinds()[kind]
    rng = np.random.default_rng(1000 * T + H)
    qkv = rng.standard_normal((T, 3 * H * 128)).astype(np.float32)
    got = ops.attention_h128(ctx, qkv, 1, T, H, dtype=dtype)
    ref, vmax = _ref(qkv, 1, T, H, kind)
    err, bound = np.abs(got - ref), _bound(ref, got, vmax, rel, mant)
    print(f"attn128 {kind} T={T} H={H}: max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(got, ops.attention_h128(ctx, qkv, 1, T, H, dtype=dtype))           # deterministic


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_attention_h128_rescale_branch(ctx, kind):
    """The running maximum has to move after the first tile: key 150 (third tile) is 8 x query 5, a raw score about 60 x 128^0.5 above
    the rest, far past the lazy-rescale threshold; key 70 does the same for query 100 one tile earlier."""
    from mlx_swift_audio_amd import ops
    dtype, rel, mant = _kinds()[kind]
    T, H = 193, 2
    rng = np.random.default_rng(7)
    qkv = rng.standard_normal((T, 3 * H * 128)).astype(np.float32)
    D = H * 128
    qkv[150, D:2 * D] = 8.0 * qkv[5, :D]
    qkv[70, D:2 * D] = 8.0 * qkv[100, :D]
    got = ops.attention_h128(ctx, qkv, 1, T, H, dtype=dtype)
    ref, vmax = _ref(qkv, 1, T, H, kind)
    err, bound = np.abs(got - ref), _bound(ref, got, vmax, rel, mant)
    print(f"attn128 {kind} spiked: worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_attention_h128_ragged_stack_equals_single_calls(ctx, kind):
    from mlx_swift_audio_amd import ops
    dtype, rel, mant = _kinds()[kind]
    lens, H = (129, 1, 70), 3
    B, T = len(lens), max(lens)
    rng = np.random.default_rng(11)
    qkv = (100.0 * rng.standard_normal((B * T, 3 * H * 128))).astype(np.float32)          # the padding rows: large, finite, unused
    for b, n in enumerate(lens):
        qkv[b * T:b * T + n] = rng.standard_normal((n, 3 * H * 128)).astype(np.float32)
    got = ops.attention_h128(ctx, qkv, B, T, H, seq_len=lens, dtype=dtype, fill=-3.0)
    ref, vmax = _ref(qkv, B, T, H, kind, seq_len=lens)
    for b, n in enumerate(lens):
        single = ops.attention_h128(ctx, qkv[b * T:b * T + n], 1, n, H, dtype=dtype)
        assert np.array_equal(got[b * T:b * T + n], single), f"sequence {b}"
        assert (got[b * T + n:(b + 1) * T] == -3.0).all()                                   # rows beyond a sequence are left alone
        r = ref[b * T:b * T + n]
        assert (np.abs(single - r) <= _bound(r, single, 1.0 * np.abs(qkv[b * T:b * T + n]).max(), rel, mant)).all()


def test_attention_h128_rejects_bad_arguments(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    x = np.zeros((4, 3 * 128), np.uint16)
    with pytest.raises(m.MiaError):          # row stride not a multiple of 8 elements
        ctx.check(ctx.lib.mia_op_attention_h128(ctx.h, x.ctypes.data, 380, x.ctypes.data, 380, x.ctypes.data, 380, x.ctypes.data, 128, 1, 4, 1,
                                                0.088, None, m.BF16, m._lib.MEM_HOST))
    with pytest.raises(m.MiaError):          # fp32 is not a type of this kernel
        ctx.check(ctx.lib.mia_op_attention_h128(ctx.h, x.ctypes.data, 384, x.ctypes.data, 384, x.ctypes.data, 384, x.ctypes.data, 128, 1, 4, 1,
                                                0.088, None, m.F32, m._lib.MEM_HOST))
