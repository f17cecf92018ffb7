"""Operator-level host wrappers (include/mia.h "operator level"): used by kernel-level parity tests and micro-benchmarks."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import ConvGemmDesc, SkinnyDesc
from . import audio as _audio


def to16(a: np.ndarray, dtype: int) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).astype(np.float16) if dtype == _lib.F16 else _audio.f32_to_bf16(a)


def from16(a: np.ndarray, dtype: int) -> np.ndarray:
    return a.astype(np.float32) if dtype == _lib.F16 else _audio.bf16_to_f32(a)


def linear(ctx: _lib.Context, x: np.ndarray, w: np.ndarray, bias=None, residual=None, act: str | None = None,
           dtype: int = _lib.BF16, out_f32: bool = False, variant: int = 1) -> np.ndarray:
    """y = act(x @ w.T + bias) + residual on the GPU; x [M,K], w [N,K] fp32 (rounded to `dtype` here)."""
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


EPI_QKV_VT, EPI_HEADMAJOR = 1, 2


def bits16(a: np.ndarray, dtype: int) -> np.ndarray:
    """fp32 values rounded to `dtype`, as uint16 bit patterns."""
    return to16(a, dtype).view(np.uint16)


def from_bits16(a: np.ndarray, dtype: int) -> np.ndarray:
    return from16(a.view(np.float16) if dtype == _lib.F16 else a, dtype)


def enc_attention_buffers(q: np.ndarray, k: np.ndarray, v: np.ndarray, B: int, T: int, H: int, Tpad: int, ld_qk: int, pad_fill: float, dtype: int):
    """The encoder attention's native operands from q / k / v [B*T, H*64] fp32 (rounded to `dtype`), as uint16 bit patterns:
    qk [B*T, ld_qk] = q | k | padding columns holding `pad_fill`; vt [B, H, 64, Tpad] with columns [T, align_up(T, 64)) zero (the model's
    contract) and columns at or beyond align_up(T, 64) holding `pad_fill`."""
    D = H * 64
    assert q.shape == k.shape == v.shape == (B * T, D)
    qk = bits16(np.full((B * T, ld_qk), pad_fill, np.float32), dtype)
    qk[:, :D], qk[:, D:2 * D] = bits16(q, dtype), bits16(k, dtype)
    vt = bits16(np.full((B, H, 64, Tpad), pad_fill, np.float32), dtype)
    vt[..., T:min(Tpad, (T + 63) // 64 * 64)] = 0
    vt[..., :T] = bits16(v, dtype).reshape(B, T, H, 64).transpose(0, 2, 3, 1)
    return qk, vt


def attention_h64(ctx: _lib.Context, q: np.ndarray, k: np.ndarray, v: np.ndarray, B: int, T: int, H: int, *, Tpad: int | None = None,
                  ld_qk: int | None = None, ld_out: int | None = None, fill: float = 0.0, pad_fill: float = 0.0,
                  dtype: int = _lib.BF16) -> np.ndarray:
    """mia_op_attention_h64 (the Whisper encoder's attention, head dim 64) on q / k / v [B*T, H*64] fp32, rounded to `dtype` and laid out
    by enc_attention_buffers; Tpad defaults to align_up(T, 64), ld_qk to 2*H*64, ld_out to H*64.  out starts as `fill` everywhere.
    Returns fp32 [B*T, ld_out], the whole buffer."""
    D = H * 64
    Tpad = (T + 63) // 64 * 64 if Tpad is None else Tpad
    ld_qk = 2 * D if ld_qk is None else ld_qk
    ld_out = D if ld_out is None else ld_out
    qk, vt = enc_attention_buffers(q, k, v, B, T, H, Tpad, ld_qk, pad_fill, dtype)
    out = bits16(np.full((B * T, ld_out), fill, np.float32), dtype)
    ctx.check(ctx.lib.mia_op_attention_h64(ctx.h, qk.ctypes.data, ld_qk, vt.ctypes.data, out.ctypes.data, ld_out, B, T, H, Tpad, dtype, _lib.MEM_HOST))
    return from_bits16(out, dtype)


ATT_REG128, ATT_DMA128, ATT_DMA256 = 0, 1, 2      # csrc/ops.h MIA_ATT_*: queries per workgroup x K / V^T staging
ATT_VARIANTS = {"reg128": ATT_REG128, "dma128": ATT_DMA128, "dma256": ATT_DMA256}


def attention_h64_bits(ctx: _lib.Context, q: np.ndarray, k: np.ndarray, v: np.ndarray, B: int, T: int, H: int, *, variant: int = -1,
                       Tpad: int | None = None, ld_qk: int | None = None, ld_out: int | None = None, fill: float = 0.0,
                       pad_fill: float = 0.0, dtype: int = _lib.BF16) -> np.ndarray:
    """attention_h64 through mia_op_attention_h64_variant: the kernel form is the caller's choice (-1 = the one the encoder launches at
    this T).  Returns the raw 16-bit output buffer, uint16 [B*T, ld_out]; from_bits16 widens it."""
    D = H * 64
    Tpad = (T + 63) // 64 * 64 if Tpad is None else Tpad
    ld_qk = 2 * D if ld_qk is None else ld_qk
    ld_out = D if ld_out is None else ld_out
    qk, vt = enc_attention_buffers(q, k, v, B, T, H, Tpad, ld_qk, pad_fill, dtype)
    out = bits16(np.full((B * T, ld_out), fill, np.float32), dtype)
    ctx.check(ctx.lib.mia_op_attention_h64_variant(ctx.h, qk.ctypes.data, ld_qk, vt.ctypes.data, out.ctypes.data, ld_out, B, T, H, Tpad, dtype,
                                                   variant, _lib.MEM_HOST))
    return out


def attention_h64_device(ctx: _lib.Context, qk, vt, out, B: int, T: int, H: int, Tpad: int, ld_qk: int, ld_out: int, dtype: int) -> None:
    """mia_op_attention_h64 on torch device tensors (16-bit elements), in place."""
    assert qk.is_cuda and vt.is_cuda and out.is_cuda
    _run(ctx, lambda: ctx.lib.mia_op_attention_h64(ctx.h, _ptr(qk), ld_qk, _ptr(vt), _ptr(out), ld_out, B, T, H, Tpad, dtype, _lib.MEM_DEVICE))


def attention_h64_device_variant(ctx: _lib.Context, qk, vt, out, B: int, T: int, H: int, Tpad: int, ld_qk: int, ld_out: int, dtype: int,
                                 variant: int) -> None:
    """mia_op_attention_h64_variant on torch device tensors (16-bit elements), in place."""
    assert qk.is_cuda and vt.is_cuda and out.is_cuda
    _run(ctx, lambda: ctx.lib.mia_op_attention_h64_variant(ctx.h, _ptr(qk), ld_qk, _ptr(vt), _ptr(out), ld_out, B, T, H, Tpad, dtype, variant,
                                                           _lib.MEM_DEVICE))


def linear_epi(ctx: _lib.Context, x: np.ndarray, w: np.ndarray, bias, y: np.ndarray, vt, *, epi: int, T: int, H: int, Tpad: int = 0,
               ldy: int | None = None, dtype: int = _lib.BF16, variant: int = 3, out_f32: bool = False, batch: int = 1, N: int | None = None):
    """mia_op_linear_epi: x [M, K], w [N, K] fp32 (rounded to `dtype` here), bias fp32 [N] or None; y and vt are uint16 arrays holding the
    destinations' initial bit patterns (QKV_VT: y [M, ldy], vt [B, H, 64, Tpad]; HEADMAJOR: y [B, H, T, 64], vt None) and are not
    modified.  Returns (y_bits, vt_bits, y_f32, vt_f32): the destinations after the GEMM as bit patterns and widened (vt: None, None for
    HEADMAJOR)."""
    M, K = x.shape
    x16, w16 = to16(x, dtype), to16(w, dtype)
    b = None if bias is None else np.ascontiguousarray(bias, np.float32)
    yo = np.array(y, np.uint16, order="C")
    vo = None if vt is None else np.array(vt, np.uint16, order="C")
    ldy = int(ldy if ldy is not None else (yo.shape[1] if yo.ndim == 2 else H * 64))
    ctx.check(ctx.lib.mia_op_linear_epi(ctx.h, x16.ctypes.data, K, w16.ctypes.data, None if b is None else b.ctypes.data, yo.ctypes.data, ldy,
                                        None if vo is None else vo.ctypes.data, M, int(w.shape[0] if N is None else N), K, int(epi), int(T), int(H),
                                        int(Tpad), int(batch), dtype, 1 if out_f32 else 0, int(variant), _lib.MEM_HOST))
    return yo, vo, from_bits16(yo, dtype), None if vo is None else from_bits16(vo, dtype)


def linear_epi_device(ctx: _lib.Context, x, w, bias, y, vt, *, M: int, N: int, K: int, epi: int, T: int, H: int, Tpad: int, ldy: int,
                      dtype: int, variant: int = 3) -> None:
    """mia_op_linear_epi on torch device tensors (x, w, y, vt 16-bit elements, bias fp32), in place."""
    _run(ctx, lambda: ctx.lib.mia_op_linear_epi(ctx.h, _ptr(x), K, _ptr(w), _ptr(bias), _ptr(y), ldy, _ptr(vt), M, N, K, int(epi), T, H, Tpad, 1,
                                                dtype, 0, int(variant), _lib.MEM_DEVICE))


def fsmn_add(ctx: _lib.Context, x: np.ndarray, v: np.ndarray, w: np.ndarray, left: int, B: int = 1, seq_len=None,
             dtype: int = _lib.BF16) -> np.ndarray:
    """mia_op_fsmn_add: x [B*T, D] fp32 + the SANM memory of v [B*T, D] (rounded to `dtype`) under taps w [K, D]; returns the new x."""
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
    Hq, dh = q.shape
    Hkv, T, _ = k.shape
    q16, k16, v16 = to16(q, dtype), to16(k, dtype), to16(v, dtype)
    out = np.empty((Hq, dh), np.float32)
    ctx.check(lib.mia_op_kvq_attention(ctx.h, q16.ctypes.data, k16.ctypes.data, v16.ctypes.data, out.ctypes.data, Hq, Hkv, T, dh, int(bits), dtype))
    return out


def lm_prompt_attention(ctx: _lib.Context, q: np.ndarray, k: np.ndarray, v: np.ndarray, dtype: int = _lib.BF16) -> np.ndarray:
    """mia_op_lm_prompt_attention: the prompt pass's tiled causal GQA attention (lm_prefill_attn.hip) over a 16-bit cache the op fills
    from k / v [Hkv, T, dh] (fp32 here, rounded to `dtype`).  q [n, Hq, dh]: the rows at positions T - n .. T - 1, the row at p sees
    keys [0, p]; returns fp32 [n, Hq, dh]."""
    lib = ctx.lib
    n, Hq, dh = q.shape
    Hkv, T, _ = k.shape
    q16, k16, v16 = to16(q, dtype), to16(k, dtype), to16(v, dtype)
    out = np.empty((n, Hq, dh), np.float32)
    ctx.check(lib.mia_op_lm_prompt_attention(ctx.h, q16.ctypes.data, k16.ctypes.data, v16.ctypes.data, out.ctypes.data, Hq, Hkv, T, n, dh, dtype))
    return out


def rfft_block(ctx: _lib.Context) -> int:
    """mia_op_rfft_block: the largest power-of-two transform one workgroup runs in LDS; larger ones take the four-step split."""
    return int(ctx.lib.mia_op_rfft_block())


def rfft_pow2(ctx: _lib.Context, x: np.ndarray, N: int) -> np.ndarray:
    """mia_op_rfft_pow2: the unscaled DFT of x [n] zero-padded to N (a power of two), complex64 [N/2 + 1]."""
    a = np.ascontiguousarray(x, np.float32).reshape(-1)
    out = np.empty((max(int(N) // 2 + 1, 1), 2), np.float32)
    ctx.check(ctx.lib.mia_op_rfft_pow2(ctx.h, a.ctypes.data, a.size, int(N), out.ctypes.data))
    return out.view(np.complex64).reshape(-1)


# ---- fp32 tap GEMM and fp32 attention (device pointers; the test hooks expose every launch argument) -------------------------------


_DESC_F32 = ("X", "W", "bias", "alpha", "ralpha", "Y", "R", "R2", "noise")
_DESC_I32 = ("phase_len", "seq_len", "noise_seq_off")
_DESC_DEFAULTS = dict(y_row_mul=1, dil=1, taps=1, x_row_mul=1, n_seq=1)


def _dev(a, np_dtype=np.float32):
    """A torch CUDA tensor as it is (views included: its data_ptr and row stride are what the op sees), a numpy array uploaded."""
    import torch
    if a is None:
        return None
    if isinstance(a, torch.Tensor):
        assert a.is_cuda, "device tensors only"
        return a
    return torch.from_numpy(np.ascontiguousarray(a, np_dtype)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ld(t, ld):
    return int(ld) if ld is not None else (int(t.stride(0)) if t is not None and t.dim() == 2 else 0)


def _run(ctx, call):
    """torch's uploads are complete before the op is enqueued on the context's stream, and the op before the result is read."""
    import torch
    torch.cuda.synchronize()
    try:
        ctx.check(call())
    finally:
        ctx.synchronize()


def conv1d_f32(ctx: _lib.Context, x, w, y, *, Cin: int, taps: int = 1, stride: int = 1, dil: int = 1, pad: int = 0, act: int = 0, bias=None,
               r=None, T_in: int | None = None, T_out: int | None = None, N: int | None = None, ldx: int | None = None,
               ldy: int | None = None) -> np.ndarray:
    """mia_op_conv1d_f32: x [T_in, ldx], w [N, taps*Cin], y [rows, ldy] (its contents are what unwritten elements keep; a device tensor is written in place), r in
    y's layout.  Returns y's whole buffer."""
    dx, dw, dy, db, dr = _dev(x), _dev(w), _dev(y), _dev(bias), _dev(r)
    _run(ctx, lambda: ctx.lib.mia_op_conv1d_f32(ctx.h, _ptr(dx), _ld(dx, ldx), int(dx.shape[0] if T_in is None else T_in), _ptr(dw), _ptr(db),
                                                 _ptr(dr), _ptr(dy), _ld(dy, ldy), int(dy.shape[0] if T_out is None else T_out),
                                                 int(dw.shape[0] if N is None else N), int(Cin), int(taps), int(stride), int(dil), int(pad), int(act)))
    return dy.cpu().numpy()


def conv_gemm_f32(ctx: _lib.Context, phases: int = 1, **d) -> np.ndarray:
    """mia_op_conv_gemm_f32: keyword arguments are the fields of mia_conv_gemm_desc, arrays for its pointers (X, Y, R, R2 two-dimensional:
    ldx / ldy / ldr default to their row strides; Y's contents are what unwritten elements keep, a device tensor is written in place).
    Returns Y's whole buffer."""
    unknown = set(d) - {n for n, _ in ConvGemmDesc._fields_}
    assert not unknown, f"not a mia_conv_gemm_desc field: {sorted(unknown)}"
    t = {k: _dev(d.get(k)) for k in _DESC_F32}
    t.update({k: _dev(d.get(k), np.int32) for k in _DESC_I32})
    desc = ConvGemmDesc()
    for name, _ in ConvGemmDesc._fields_:
        if name in t:
            setattr(desc, name, _ptr(t[name]))
        elif name in ("ldx", "ldy", "ldr"):
            setattr(desc, name, _ld(t[{"ldx": "X", "ldy": "Y", "ldr": "R"}[name]] if name != "ldr" or t["R"] is not None else t["R2"], d.get(name)))
        else:
            setattr(desc, name, d.get(name, _DESC_DEFAULTS.get(name, 0)))
    _run(ctx, lambda: ctx.lib.mia_op_conv_gemm_f32(ctx.h, C.byref(desc), int(phases)))
    return None if t["Y"] is None else t["Y"].cpu().numpy()


def attention_f32_ex(ctx: _lib.Context, q, k, v, out, B: int, T: int, H: int, scale: float = 0.125, p=None, bias_u=None, bias_v=None,
                     seq_len=None, chunk: int = 0, ldq=None, ldk=None, ldv=None, ldp=None, ldo=None, plain: bool = False) -> np.ndarray:
    """mia_op_attention_f32_ex (plain: mia_op_attention_f32): q / k / v [B*T, ld] (three views of one fused device buffer are fine), head h
    in columns h*64..; out [B*T, ldo], its contents are what unwritten elements keep (a device tensor is written in place).  Returns out's whole buffer."""
    dq, dk, dv, do, dp, du, dbv = _dev(q), _dev(k), _dev(v), _dev(out), _dev(p), _dev(bias_u), _dev(bias_v)
    ds = _dev(seq_len, np.int32)
    head = (ctx.h, _ptr(dq), _ld(dq, ldq), _ptr(dk), _ld(dk, ldk), _ptr(dv), _ld(dv, ldv))
    if plain:
        assert p is None and seq_len is None and not chunk
        _run(ctx, lambda: ctx.lib.mia_op_attention_f32(*head, _ptr(do), _ld(do, ldo), int(B), int(T), int(H), float(scale)))
    else:
        _run(ctx, lambda: ctx.lib.mia_op_attention_f32_ex(*head, _ptr(dp), _ld(dp, ldp), _ptr(du), _ptr(dbv), _ptr(do), _ld(do, ldo), int(B), int(T),
                                                           int(H), float(scale), _ptr(ds), int(chunk)))
    return do.cpu().numpy()


def attention_f32(ctx: _lib.Context, q, k, v, out, B: int, T: int, H: int, scale: float = 0.125, **ld) -> np.ndarray:
    """mia_op_attention_f32: full softmax(q k^T scale) v per head, head dim 64; see attention_f32_ex."""
    return attention_f32_ex(ctx, q, k, v, out, B, T, H, scale, plain=True, **ld)


# ---- the LM step's skinny GEMMs (device tensors; the test hook exposes every launch argument) ---------------------------------------


SK_OUT16, SK_OUTF32, SK_PARTIAL, SK_QKV, SK_SWIGLU, SK_RESID = range(6)
_SKINNY_PTRS = ("A", "W", "wfrag", "stfrag", "bias", "out", "xres", "nw", "ss_out", "ss_in")


def quant_repack(codes: np.ndarray, scales: np.ndarray, biases: np.ndarray, bits: int, scale_dtype: int, compute_dtype: int):
    """mia_quant_repack (host): one packed Linear (quantize_affine's three arrays; bf16 scales as uint16 bit patterns) -> (wfrag, stfrag)."""
    lib = _lib.load()
    codes, scales, biases = np.ascontiguousarray(codes, np.uint32), np.ascontiguousarray(scales), np.ascontiguousarray(biases)
    N, K = codes.shape[0], codes.shape[1] * 32 // bits
    tiles = (N + 15) // 16
    # 6 bit: [64][4] low-nibble words then [64][2] words of 2-bit high parts per (tile, block) (csrc/skinny_quant.hip)
    wf = np.zeros((tiles, K // 128, 384) if bits == 6 else (tiles, K // 128, bits // 4, 64, 4), np.uint32)
    st = np.zeros((tiles, K // 128, 16, 4), np.float32)
    rc = lib.mia_quant_repack(codes.ctypes.data, scales.ctypes.data, biases.ctypes.data, N, K, int(bits), int(scale_dtype), int(compute_dtype),
                              wf.ctypes.data, st.ctypes.data)
    if rc != 0:
        raise _lib.MiaError(rc, "quant_repack: bad argument")
    return wf, st


def skinny_gemm(ctx: _lib.Context, **d) -> None:
    """mia_op_skinny_gemm: keyword arguments are the fields of mia_skinny_desc, torch device tensors (views included) or None for its
    pointers; lda / ldo default to the row strides of two-dimensional A / out, S to 1, rs_scale to 1.  Outputs are written in place."""
    lib = ctx.lib
    unknown = set(d) - {n for n, _ in SkinnyDesc._fields_}
    assert not unknown, f"not a mia_skinny_desc field: {sorted(unknown)}"
    desc = SkinnyDesc()
    for name, _ in SkinnyDesc._fields_:
        v = d.get(name)
        if name in _SKINNY_PTRS:
            assert v is None or v.is_cuda, "device tensors only"
            setattr(desc, name, _ptr(v))
        elif name == "lda":
            desc.lda = _ld(d.get("A"), v)
        elif name == "ldo":
            desc.ldo = _ld(d.get("out"), v)
        else:
            setattr(desc, name, {"S": 1, "rs_scale": 1.0}.get(name, 0) if v is None else v)
    _run(ctx, lambda: lib.mia_op_skinny_gemm(ctx.h, C.byref(desc)))


def gemm_quant(ctx: _lib.Context, A, wfrag, stfrag, bits: int, C_out, M: int, N: int, K: int, dtype: int, R=None, lda=None, ldc=None, ldr=None) -> None:
    """mia_op_gemm_quant: C_out fp32 [M][ldc] = A [M][lda] . Wq^T (+ R), the packed prompt pass's GEMM (csrc/gemm_quant.hip) on torch
    device tensors; wfrag / stfrag as quant_repack builds them.  Strides default to the row strides of two-dimensional tensors; R may be
    C_out itself.  Written in place."""
    from ._abi import GemmQuantDesc
    for t in (A, wfrag, stfrag, C_out, R):
        assert t is None or t.is_cuda, "device tensors only"
    desc = GemmQuantDesc(_ptr(A), _ld(A, lda), _ptr(wfrag), _ptr(stfrag), int(bits), _ptr(C_out), _ld(C_out, ldc), _ptr(R),
                         _ld(R, ldr) if R is not None else 0, int(M), int(N), int(K), int(dtype))
    _run(ctx, lambda: ctx.lib.mia_op_gemm_quant(ctx.h, C.byref(desc)))
