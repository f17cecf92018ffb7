"""The stacked codec decode entries (mia_snac_decode_batch / mia_dac_decode_batch) are exported, their ctypes declarations load, and a null
handle is refused with MIA_ERR_MODEL_NOT_LOADED before anything touches a GPU (so this runs on a machine without one)."""
import numpy as np


def _lib():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import codec as HC
    lib = m._lib.load()
    return m, lib


def test_batch_entries_are_declared():
    _, lib = _lib()
    assert len(lib.mia_snac_decode_batch.argtypes) == 11
    assert len(lib.mia_dac_decode_batch.argtypes) == 9


def test_null_handle_is_refused_without_a_gpu():
    m, lib = _lib()
    codes = np.zeros(6, np.int32)
    n = np.asarray([2, 4], np.int32)
    T = np.asarray([3], np.int64)
    off = np.asarray([0, 64], np.int64)
    pcm = np.zeros(64, np.float32)
    ns = np.zeros(1, np.int64)
    assert lib.mia_snac_decode_batch(None, 1, codes.ctypes.data, n.ctypes.data, 2, None, 0, pcm.ctypes.data, off.ctypes.data, ns.ctypes.data,
                                     m._lib.MEM_HOST) == m._lib.ERR_MODEL_NOT_LOADED
    assert lib.mia_dac_decode_batch(None, 1, codes.ctypes.data, 2, T.ctypes.data, pcm.ctypes.data, off.ctypes.data, ns.ctypes.data,
                                    m._lib.MEM_HOST) == m._lib.ERR_MODEL_NOT_LOADED
