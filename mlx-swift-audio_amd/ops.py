"""Operator-level host wrappers (include/mia.h "operator level"): used by kernel-level parity tests and micro-benchmarks."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import audio as _audio


def _declare(lib):
    if getattr(lib, "_ops_declared", False):
        return
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    lib.mia_op_linear.restype = i32
    lib.mia_op_linear.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, i32, i32]
    lib.mia_op_attention_h128.restype = i32
    lib.mia_op_attention_h128.argtypes = [vp, vp, i64, vp, i64, vp, i64, vp, i64, i32, i32, i32, C.c_float, vp, i32, i32]
    lib.mia_op_fsmn_add.restype = i32
    lib.mia_op_fsmn_add.argtypes = [vp, vp, i64, vp, i64, vp, i32, i32, i32, i32, i32, vp, i32, i32]
    lib._ops_declared = True


def to16(a: np.ndarray, dtype: int) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).astype(np.float16) if dtype == _lib.F16 else _audio.f32_to_bf16(a)


def from16(a: np.ndarray, dtype: int) -> np.ndarray:
    return a.astype(np.float32) if dtype == _lib.F16 else _audio.bf16_to_f32(a)


def linear(ctx: _lib.Context, x: np.ndarray, w: np.ndarray, bias=None, residual=None, act: str | None = None,
           dtype: int = _lib.BF16, out_f32: bool = False, variant: int = 1) -> np.ndarray:
    """y = act(x @ w.T + bias) + residual on the GPU; x [M,K], w [N,K] fp32 (rounded to `dtype` here)."""
    _declare(ctx.lib)
    M, K = x.shape
    N = w.shape[0]
    x16, w16 = to16(x, dtype), to16(w, dtype)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    r = None if residual is None else np.ascontiguousarray(residual, np.float32)
    y = np.empty((M, N), np.float32 if out_f32 else (np.float16 if dtype == _lib.F16 else np.uint16))
    ctx.check(ctx.lib.mia_op_linear(ctx.h, x16.ctypes.data, K, w16.ctypes.data, None if b is None else b.ctypes.data,
                                    None if r is None else r.ctypes.data, N, y.ctypes.data, N, M, N, K,
                                    {None: 0, "gelu": 1, "relu": 2}[act], dtype, 1 if out_f32 else 0, variant, _lib.MEM_HOST))
    return y if out_f32 else from16(y, dtype)


def attention_h128(ctx: _lib.Context, qkv: np.ndarray, B: int, T: int, H: int, scale: float | None = None, seq_len=None,
                   dtype: int = _lib.BF16, fill: float = 0.0) -> np.ndarray:
    """mia_op_attention_h128 on a fused q | k | v buffer [B*T, 3*H*128] (fp32 here, rounded to `dtype`): full softmax(q k^T scale) v per
    head, head dim 128.  seq_len [B] masks keys at or beyond a sequence's length; rows beyond it keep `fill`.  Returns fp32 [B*T, H*128]."""
    _declare(ctx.lib)
    D = H * 128
    assert qkv.shape == (B * T, 3 * D)
    x16 = to16(qkv, dtype)
    out = to16(np.full((B * T, D), fill, np.float32), dtype)
    sl = None if seq_len is None else np.ascontiguousarray(seq_len, np.int32)
    base, es = x16.ctypes.data, x16.itemsize
    ctx.check(ctx.lib.mia_op_attention_h128(ctx.h, base, 3 * D, base + D * es, 3 * D, base + 2 * D * es, 3 * D, out.ctypes.data, D, B, T, H,
                                            float(128 ** -0.5 if scale is None else scale), None if sl is None else sl.ctypes.data,
                                            dtype, _lib.MEM_HOST))
    return from16(out, dtype)


def fsmn_add(ctx: _lib.Context, x: np.ndarray, v: np.ndarray, w: np.ndarray, left: int, B: int = 1, seq_len=None,
             dtype: int = _lib.BF16) -> np.ndarray:
    """mia_op_fsmn_add: x [B*T, D] fp32 + the SANM memory of v [B*T, D] (rounded to `dtype`) under taps w [K, D]; returns the new x."""
    _declare(ctx.lib)
    rows, D = x.shape
    T = rows // B
    xo = np.array(x, np.float32, order="C")
    v16 = to16(v, dtype)
    w32 = np.ascontiguousarray(w, np.float32)
    sl = None if seq_len is None else np.ascontiguousarray(seq_len, np.int32)
    ctx.check(ctx.lib.mia_op_fsmn_add(ctx.h, xo.ctypes.data, D, v16.ctypes.data, D, w32.ctypes.data, B, T, D, w32.shape[0], int(left),
                                      None if sl is None else sl.ctypes.data, dtype, _lib.MEM_HOST))
    return xo


def kvq_attention(ctx: _lib.Context, q: np.ndarray, k: np.ndarray, v: np.ndarray, bits: int = 4, dtype: int = _lib.BF16) -> np.ndarray:
    """mia_op_kvq_attention: the LM's single-token GQA attention for the last of T positions over a cache the op fills from k / v
    [Hkv, T, dh] (fp32 here, rounded to `dtype`): bits 0 = the 16-bit cache, 4 | 8 = the quantised one.  q [Hq, dh]; returns fp32 [Hq, dh]."""
    lib = ctx.lib
    lib.mia_op_kvq_attention.restype = C.c_int
    lib.mia_op_kvq_attention.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6
    Hq, dh = q.shape
    Hkv, T, _ = k.shape
    q16, k16, v16 = to16(q, dtype), to16(k, dtype), to16(v, dtype)
    out = np.empty((Hq, dh), np.float32)
    ctx.check(lib.mia_op_kvq_attention(ctx.h, q16.ctypes.data, k16.ctypes.data, v16.ctypes.data, out.ctypes.data, Hq, Hkv, T, dh, int(bits), dtype))
    return out
