"""Packed 6-bit weights, the parts that need no GPU: the storage rule (tests/_quant6.py) pinned on a worked example and by round trips, the
Python quantiser and packer against it, the host repack at 6 bits (mia_quant_repack: both planes decoded by the layout documented in
csrc/skinny_quant.hip, and the (scale, offset) pairs), and what still refuses odd widths."""
import numpy as np
import pytest

import _quant6 as Q6


def test_packing_rule_worked_example():
    # 1 | 2 << 6 | 3 << 12 | 4 << 18 = 0x103081: three bytes, little end first
    w = Q6.pack6(np.array([[1, 2, 3, 4] * 4]))
    assert w.dtype == np.uint32 and w.shape == (1, 3)
    assert w.view(np.uint8)[0, :3].tobytes().hex() == "813010"
    assert w.view(np.uint8).tobytes().hex() == "813010" * 4


def test_pack_unpack_round_trip_and_straddling():
    rng = np.random.default_rng(0)
    for K in (16, 64, 192, 1024):
        q = rng.integers(0, 64, (5, K))
        w = Q6.pack6(q)
        assert w.shape == (5, K * 6 // 32)
        np.testing.assert_array_equal(Q6.unpack6(w), q)
    # code 5 occupies bits [30, 36): two bits in word 0, four in word 1
    q = np.zeros((1, 16), np.int64)
    q[0, 5] = 0b101101
    w = Q6.pack6(q)
    assert int(w[0, 0]) == (0b01 << 30) and int(w[0, 1]) == 0b1011 and int(w[0, 2]) == 0


def test_checkpoint_packer_and_quantiser_follow_the_rule():
    from mlx_swift_audio_amd import checkpoint as CK
    rng = np.random.default_rng(1)
    q = rng.integers(0, 64, (7, 192))
    np.testing.assert_array_equal(CK.pack_codes(q, 6), Q6.pack6(q))
    w = rng.standard_normal((6, 256)).astype(np.float32)
    codes, s, b = CK.quantize_affine(w, 64, 6, np.float32)
    assert codes.dtype == np.uint32 and codes.shape == (6, 256 * 6 // 32) and s.shape == b.shape == (6, 4)
    assert Q6.unpack6(codes).max() == 63 and Q6.unpack6(codes).min() == 0
    back = Q6.dequant6(codes, s, b)
    step = (w.reshape(6, 4, 64).max(-1) - w.reshape(6, 4, 64).min(-1)) / 63
    assert np.abs(back - w).max() <= 0.5 * step.max() + 1e-6
    # the 4- and 8-bit words are what they were
    from oracle import quant as OQ
    for bits in (4, 8):
        np.testing.assert_array_equal(CK.quantize_affine(w, 64, bits, np.float32)[0], OQ.quantize_affine(w, 64, bits)[0])
    for bits in (3, 5, 7):
        import mlx_swift_audio_amd as m
        with pytest.raises(m.MiaError):
            CK.pack_codes(q, bits)


def _store(x, sdt):
    from mlx_swift_audio_amd import audio
    if sdt == "bf16":
        a = audio.f32_to_bf16(x.astype(np.float32))
        return a, audio.bf16_to_f32(a).astype(np.float64)
    a = x.astype(np.float16 if sdt == "f16" else np.float32)
    return a, a.astype(np.float64)


@pytest.mark.parametrize("N,K", [(20, 128), (33, 128), (20, 384), (33, 384)])
@pytest.mark.parametrize("compute", ["f16", "bf16"])
@pytest.mark.parametrize("sdt", ["f16", "bf16", "f32"])
def test_repack_6bit_layout(N, K, compute, sdt):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    rng = np.random.default_rng(N * K)
    q = rng.integers(0, 64, (N, K))
    assert len(np.unique(q & 15)) == 16 and len(np.unique(q >> 4)) == 4
    s, s64 = _store(rng.uniform(0.01, 0.1, (N, K // 64)), sdt)
    b, b64 = _store(rng.uniform(-2.0, 2.0, (N, K // 64)), sdt)
    tags = {"f16": m._lib.F16, "bf16": m._lib.BF16, "f32": m._lib.F32}
    wf, st = ops.quant_repack(Q6.pack6(q), s, b, 6, tags[sdt], tags[compute])
    tiles = (N + 15) // 16
    assert wf.size == tiles * (K // 128) * 384 and st.shape == (tiles, K // 128, 16, 4)
    got = Q6.decode_wfrag6(wf, N, K)
    np.testing.assert_array_equal(got[:N], q)
    np.testing.assert_array_equal(got[N:], np.repeat(q[-1:], tiles * 16 - N, 0))          # the last tile repeats its final row
    mag = 17.0 * (1024.0 if compute == "f16" else 128.0)
    nn, g = np.meshgrid(np.arange(N), np.arange(K // 64), indexing="ij")
    np.testing.assert_array_equal(st[nn // 16, g // 2, nn % 16, 2 * (g % 2)], s64.astype(np.float32))
    np.testing.assert_array_equal(st[nn // 16, g // 2, nn % 16, 2 * (g % 2) + 1], (b64 - mag * s64).astype(np.float32))


def test_odd_widths_are_still_refused():
    import mlx_swift_audio_amd as m
    lib = m._lib.load()
    codes, s, b = np.zeros((16, 128), np.uint32), np.ones((16, 2), np.float16), np.ones((16, 2), np.float16)
    wf, st = np.zeros(16 * 1024, np.uint32), np.zeros(64, np.float32)
    for bits in (3, 5, 7):
        assert lib.mia_quant_repack(codes.ctypes.data, s.ctypes.data, b.ctypes.data, 16, 128, bits, m._lib.F16, m._lib.F16, wf.ctypes.data,
                                    st.ctypes.data) == m._lib.ERR_INVALID_ARGUMENT
    assert lib.mia_quant_repack(codes.ctypes.data, s.ctypes.data, b.ctypes.data, 16, 128, 6, m._lib.F16, m._lib.F16, wf.ctypes.data, st.ctypes.data) == 0
    # null handles are reported, not dereferenced
    assert lib.mia_marvis_attach_quantized(None, None, 0, 64, 6) == m._lib.ERR_MODEL_NOT_LOADED
    assert lib.mia_marvis_use_packed(None, 1) == m._lib.ERR_MODEL_NOT_LOADED
