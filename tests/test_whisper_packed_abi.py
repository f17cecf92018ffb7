"""Packed-weight Whisper step, the parts that need no GPU: the two entry points are exported with the declared signatures, and the host
repack shared by the LM and Whisper loaders (csrc/quant_repack.hip, reached through the test hook mia_quant_repack) puts every code and
every (scale, offset) pair where the packed kernels read them -- wfrag / stfrag indices recomputed here from the layout's definition
(csrc/skinny_quant.hip)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    text = open(os.path.join(ROOT, "include", "mia.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_symbols_exported_with_the_stated_signatures():
    import mlx_swift_audio_amd as m
    lib = m._lib.load()
    h = _header()
    assert "int mia_whisper_attach_quantized(mia_whisper* w, const mia_tensor_view* tensors, int n_tensors, int group_size, int bits);" in h
    assert "int mia_whisper_use_packed(mia_whisper* w, int on);" in h
    for name in ("mia_whisper_attach_quantized", "mia_whisper_use_packed", "mia_quant_repack"):
        assert hasattr(lib, name), name
    # a null handle is reported, not dereferenced
    assert lib.mia_whisper_attach_quantized(None, None, 0, 64, 4) == m._lib.ERR_MODEL_NOT_LOADED
    assert lib.mia_whisper_use_packed(None, 1) == m._lib.ERR_MODEL_NOT_LOADED
    # the Python surface
    from mlx_swift_audio_amd import checkpoint, whisper
    assert callable(whisper.WhisperModel.attach_quantized) and callable(whisper.WhisperModel.use_packed)
    import inspect
    assert inspect.signature(checkpoint.load_whisper_checkpoint).parameters["keep_packed"].default is False


def _repack(codes, scales, biases, bits, scale_dt, compute_dt):
    import mlx_swift_audio_amd as m
    lib = m._lib.load()
    N, K = codes.shape[0], codes.shape[1] * (32 // bits)
    tiles, nblk, planes = (N + 15) // 16, K // 128, bits // 4
    wf = np.zeros((tiles, nblk, planes, 64, 4), np.uint32)
    st = np.zeros((tiles, nblk, 16, 4), np.float32)
    rc = lib.mia_quant_repack(codes.ctypes.data, scales.ctypes.data, biases.ctypes.data, N, K, bits, scale_dt, compute_dt, wf.ctypes.data, st.ctypes.data)
    return rc, wf, st


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("compute", ["f16", "bf16"])
@pytest.mark.parametrize("scale_dtype", [np.float16, np.float32])
def test_repack_layout_32x256(bits, compute, scale_dtype):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd.checkpoint import quantize_affine
    rng = np.random.default_rng(bits)
    N, K = 32, 256
    w = rng.standard_normal((N, K)).astype(np.float32)
    codes, scales, biases = quantize_affine(w, 64, bits, scale_dtype)
    per = 32 // bits
    q = ((codes[:, :, None] >> (np.arange(per, dtype=np.uint32) * np.uint32(bits))) & np.uint32((1 << bits) - 1)).reshape(N, K)
    assert len(np.unique(q & 15)) == 16 and len(np.unique(q >> 4)) == (16 if bits == 8 else 1)      # every nibble value occurs in every plane
    rc, wf, st = _repack(codes, scales, biases, bits, m._lib.F16 if scale_dtype == np.float16 else m._lib.F32, m._lib.F16 if compute == "f16" else m._lib.BF16)
    assert rc == 0
    # wfrag [tile = n / 16][blk = k / 128][plane][lane = 16 c + r][word]: word `stp` of lane (r, c) = the plane's nibbles of
    # W[16 tile + r][128 blk + 32 stp + 8 c .. + 7]; K-value 2 i at bits [4 i, 4 i + 4), 2 i + 1 at bits [16 + 4 i, ...)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    tile, r, blk, stp, c, j = n // 16, n % 16, k // 128, (k % 128) // 32, (k % 32) // 8, k % 8
    shift = np.where(j % 2 == 0, 4 * (j // 2), 16 + 4 * (j // 2)).astype(np.uint32)
    for plane in range(bits // 4):
        got = (wf[tile, blk, plane, 16 * c + r, stp] >> shift) & np.uint32(15)
        np.testing.assert_array_equal(got, (q >> np.uint32(4 * plane)) & np.uint32(15))
    # stfrag [tile][blk][r][4] = (s, t) of the block's two groups; t = b - MAG s (x 17 with two planes), rounded once from fp64
    mag = (1024.0 if compute == "f16" else 128.0) * (17.0 if bits == 8 else 1.0)
    s32, b32 = scales.astype(np.float32), biases.astype(np.float32)
    nn, g = np.meshgrid(np.arange(N), np.arange(K // 64), indexing="ij")
    np.testing.assert_array_equal(st[nn // 16, g // 2, nn % 16, 2 * (g % 2)], s32)
    np.testing.assert_array_equal(st[nn // 16, g // 2, nn % 16, 2 * (g % 2) + 1], (b32.astype(np.float64) - mag * s32.astype(np.float64)).astype(np.float32))


def test_repack_pads_the_last_tile_and_rejects_bad_sizes():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd.checkpoint import quantize_affine
    rng = np.random.default_rng(0)
    w = rng.standard_normal((20, 128)).astype(np.float32)
    codes, scales, biases = quantize_affine(w, 64, 4, np.float16)
    rc, wf, st = _repack(codes, scales, biases, 4, m._lib.F16, m._lib.F16)
    assert rc == 0
    for r in range(4, 16):                                  # rows 20..31 of the second tile repeat row 19 (never stored by the kernels)
        np.testing.assert_array_equal(wf[1, 0, 0, r::16], wf[1, 0, 0, 3::16])
        np.testing.assert_array_equal(st[1, 0, r], st[1, 0, 3])
    bad = np.zeros((16, 12), np.uint32)                     # K = 96: not a multiple of 128
    assert _repack(bad, scales, biases, 4, m._lib.F16, m._lib.F16)[0] == m._lib.ERR_INVALID_ARGUMENT
    lib = m._lib.load()
    assert lib.mia_quant_repack(None, None, None, 16, 128, 4, m._lib.F16, m._lib.F16, None, None) == m._lib.ERR_INVALID_ARGUMENT
    assert lib.mia_quant_repack(codes.ctypes.data, scales.ctypes.data, biases.ctypes.data, 20, 128, 3, m._lib.F16, m._lib.F16, wf.ctypes.data, st.ctypes.data) == m._lib.ERR_INVALID_ARGUMENT


def test_keep_packed_returns_the_raw_triples_of_a_quantised_file(tmp_path, monkeypatch):
    """File -> load_whisper_checkpoint(keep_packed=True) -> third value: exactly the stored `<p>.weight` / `.scales` / `.biases` of the
    quantised modules, bit for bit and with their dtypes, nothing of the dense tensors; the default call still returns two values.  (The
    de-quantisation itself runs on the GPU and is checked in tests/test_checkpoint.py: here it is replaced by the numpy formula.)"""
    import json
    from safetensors.numpy import save_file
    from mlx_swift_audio_amd import checkpoint as CK
    from mlx_swift_audio_amd import synthetic as S
    dims = S.DIMS["micro.en"]
    disk, stored = {}, {}
    for k, v in S.synthetic_weights(dims, seed=5).items():
        if k.endswith(".weight") and v.ndim == 2 and v.shape[1] % 64 == 0:
            q, s, b = CK.quantize_affine(v, 64, 4, np.float16)
            for suffix, a in ((".weight", q), (".scales", s), (".biases", b)):
                disk[k[:-7] + suffix] = stored[k[:-7] + suffix] = a
        else:
            disk[k] = v.astype(np.float32)
    save_file({k: np.ascontiguousarray(v) for k, v in disk.items()}, os.path.join(str(tmp_path), "model.safetensors"))
    cfg = {k: getattr(dims, k) for k in ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "n_vocab", "n_text_ctx", "n_text_state",
                                         "n_text_head", "n_text_layer")}
    json.dump(cfg, open(os.path.join(str(tmp_path), "config.json"), "w"))

    def dequant(ctx, wq, scales, biases, group_size=64, bits=4):
        per = 32 // bits
        q = ((np.asarray(wq)[:, :, None] >> (np.arange(per, dtype=np.uint32) * np.uint32(bits))) & np.uint32((1 << bits) - 1)).reshape(wq.shape[0], -1, group_size)
        return (np.asarray(scales, np.float32)[..., None] * q.astype(np.float32) + np.asarray(biases, np.float32)[..., None]).reshape(wq.shape[0], -1)

    monkeypatch.setattr(CK, "dequantize_affine", dequant)
    two = CK.load_whisper_checkpoint(None, str(tmp_path))
    assert len(two) == 2
    d3, dense, packed = CK.load_whisper_checkpoint(None, str(tmp_path), keep_packed=True)
    assert d3 == dims and set(dense) == set(two[1])
    assert set(packed) == set(stored) and "decoder.token_embedding.scales" in packed and "encoder.blocks.0.mlp1.weight" in packed
    for k, a in stored.items():
        assert packed[k].dtype == a.dtype and packed[k].shape == a.shape, k
        np.testing.assert_array_equal(np.asarray(packed[k]), a)
    assert not any(k.endswith((".scales", ".biases")) for k in dense)
    assert dense["decoder.blocks.0.mlp1.weight"].shape == (4 * dims.n_text_state, dims.n_text_state)
    # what attach_quantized would pass on: the decoder triples only
    assert CK.packed_tensors({"x.weight": np.zeros((2, 2), np.float32)}) == {}
