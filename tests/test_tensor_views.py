"""_abi.tensor_views / _abi.dtype_tag: the one place a name -> array dict becomes the mia_tensor_view array of a load or attach call.
Pure ctypes: no library is loaded and no GPU is needed."""
import ctypes as C

import numpy as np
import pytest

from mlx_swift_audio_amd import _abi, _lib, checkpoint

DENSE = (_lib.F32, _lib.F16, _lib.BF16)
PACKED = (_lib.U32, _lib.F16, _lib.BF16)
REFUSE = "attach_q4: '{name}' must be uint32 codes or 16-bit scales / biases (got {dtype})"


def _tagged(a, tag):
    t = a.view(checkpoint.Tensor)
    t.st_dtype = tag
    return t


def _data(view, dtype, count):
    return np.frombuffer(C.string_at(view.data, count * np.dtype(dtype).itemsize), dtype)


def test_tag_per_dtype():
    u16 = np.arange(6, dtype=np.uint16)
    assert _abi.dtype_tag(np.zeros(2, np.float32)) == _lib.F32
    assert _abi.dtype_tag(np.zeros(2, np.float16)) == _lib.F16
    assert _abi.dtype_tag(np.zeros(2, np.uint32)) == _lib.U32
    assert _abi.dtype_tag(_tagged(u16, "BF16")) == _lib.BF16
    assert _abi.dtype_tag(u16) == _lib.BF16                      # untagged uint16: a bf16 payload (the docstring's rule)
    assert _abi.dtype_tag(_tagged(u16, "U16")) is None
    for other in (np.float64, np.int32, np.int64, np.uint8, np.int16):
        assert _abi.dtype_tag(np.zeros(2, other)) is None
    assert (_lib.F32, _lib.F16, _lib.BF16, _lib.U32) == (0, 1, 2, 3)


def test_checkpoint_uses_the_same_rule():
    u16 = np.arange(6, dtype=np.uint16)
    assert checkpoint._mia_dtype(_tagged(u16, "BF16")) == _lib.BF16
    assert checkpoint._mia_dtype(u16) == _lib.BF16
    assert checkpoint._mia_dtype(np.zeros(2, np.float16)) == _lib.F16
    assert checkpoint._mia_dtype(np.zeros(2, np.float32)) == _lib.F32
    for bad in (np.zeros(2, np.uint32), np.zeros(2, np.float64), _tagged(u16, "U16")):
        with pytest.raises(_lib.MiaError, match="scales / biases must be f32, f16 or bf16"):
            checkpoint._mia_dtype(bad)


def test_views_names_tags_and_padded_shapes():
    tensors = {"a.weight": np.arange(24, dtype=np.float32).reshape(2, 3, 4), "b": np.arange(5, dtype=np.float16),
               "c": _tagged(np.arange(6, dtype=np.uint16).reshape(3, 2), "BF16"), "d": np.float32(7).reshape(()),
               "e": np.arange(16, dtype=np.float32).reshape(1, 2, 2, 4)}
    views, n, keep = _abi.tensor_views(tensors, DENSE)
    assert n == 5 and len(views) == 5 and len(keep) == 5
    want = [(b"a.weight", _lib.F32, 3, [2, 3, 4, 0]), (b"b", _lib.F16, 1, [5, 0, 0, 0]), (b"c", _lib.BF16, 2, [3, 2, 0, 0]),
            (b"d", _lib.F32, 1, [1, 0, 0, 0]), (b"e", _lib.F32, 4, [1, 2, 2, 4])]
    for v, a, (name, tag, ndim, shape) in zip(views, keep, want):                 # ("d": a scalar is handed over as [1])
        assert (v.name, v.dtype, v.ndim, list(v.shape)) == (name, tag, ndim, shape)
        assert v.data == a.ctypes.data
    np.testing.assert_array_equal(_data(views[2], np.uint16, 6), np.arange(6, dtype=np.uint16))      # the bf16 bit patterns, untouched
    np.testing.assert_array_equal(_data(views[1], np.float16, 5), np.arange(5, dtype=np.float16))


def test_non_contiguous_input_is_copied_and_kept_alive():
    base = np.arange(12, dtype=np.float32).reshape(3, 4)
    views, n, keep = _abi.tensor_views({"t": base.T, "s": base[:, ::2].astype(np.float16)[:, ::-1]}, DENSE)
    assert n == 2 and all(a.flags["C_CONTIGUOUS"] for a in keep)
    assert list(views[0].shape) == [4, 3, 0, 0] and views[0].data == keep[0].ctypes.data != base.ctypes.data
    np.testing.assert_array_equal(_data(views[0], np.float32, 12), base.T.reshape(-1))
    np.testing.assert_array_equal(_data(views[1], np.float16, 6), np.asarray([[2, 0], [6, 4], [10, 8]], np.float16).reshape(-1))
    del base
    np.testing.assert_array_equal(keep[0], np.arange(12, dtype=np.float32).reshape(3, 4).T)


def test_fp32_only_forces_float32():
    tensors = {"h": np.asarray([1.5, -2.0], np.float16), "d": np.asarray([3.0, 4.0], np.float64), "i": np.asarray([5, 6], np.int64),
               "f": np.asarray([7.0, 8.0], np.float32)}
    views, n, keep = _abi.tensor_views(tensors)
    assert n == 4 and all(v.dtype == _lib.F32 for v in views) and all(a.dtype == np.float32 for a in keep)
    np.testing.assert_array_equal(np.concatenate([_data(v, np.float32, 2) for v in views]), np.asarray([1.5, -2, 3, 4, 5, 6, 7, 8], np.float32))
    assert keep[3] is tensors["f"] or keep[3].ctypes.data == tensors["f"].ctypes.data          # already float32 and contiguous: no copy


def test_dense_converts_what_has_no_16_bit_tag():
    views, n, keep = _abi.tensor_views({"d": np.asarray([1.0, 2.0], np.float64), "u": np.asarray([3, 4], np.uint32)}, DENSE)
    assert [v.dtype for v in views] == [_lib.F32, _lib.F32]
    np.testing.assert_array_equal(np.concatenate(keep), np.asarray([1, 2, 3, 4], np.float32))


def test_refused_kind_keeps_the_attach_texts():
    ok = {"p.weight": np.zeros((2, 8), np.uint32), "p.scales": np.zeros((2, 1), np.float16), "p.biases": _tagged(np.zeros((2, 1), np.uint16), "BF16")}
    views, n, _keep = _abi.tensor_views(ok, PACKED, REFUSE)
    assert n == 3 and [v.dtype for v in views] == [_lib.U32, _lib.F16, _lib.BF16]
    with pytest.raises(_lib.MiaError) as e:
        _abi.tensor_views({**ok, "p.scales": np.zeros((2, 1), np.float32)}, PACKED, REFUSE)
    assert "attach_q4: 'p.scales' must be uint32 codes or 16-bit scales / biases (got float32)" in str(e.value)
    with pytest.raises(_lib.MiaError) as e:
        _abi.tensor_views({**ok, "p.biases": np.zeros((2, 1), np.int8)}, PACKED + (_lib.F32,),
                          "attach_quantized: '{name}' must be uint32 codes or f16 / bf16 / f32 scales / biases (got {dtype})")
    assert "attach_quantized: 'p.biases' must be uint32 codes or f16 / bf16 / f32 scales / biases (got int8)" in str(e.value)


def test_empty_dict_still_gives_an_array():
    views, n, keep = _abi.tensor_views({})
    assert n == 0 and len(views) == 1 and keep == []
