"""float64 references of the LM step's skinny GEMMs (csrc/skinny.h: skinny_gemm_launch, skinny_gemm_q_launch), written from the formulas
in skinny.h and skinny_quant.hip over the 16-bit-rounded operands, with the error bound each comparison is entitled to.

Bounds are derived per element, none is tuned (u = 2^-24, one fp32 rounding):
 * 16-bit kernels: the products of two 16-bit values are exact in fp32 and are accumulated in fp32, so for ANY summation order (K-steps
   inside a wave, waves through LDS, tails) the accumulator is within (K + 2) u sum |a w| of the exact sum.
 * packed kernels do not sum w a.  Per 64-input group g they form P_g = sum (MAG + q) a on the matrix cores (MAG = 128 for bf16, 1024
   for f16; 8 bit: two nibble planes, P = P_lo + 16 P_hi by one fma), A_g = sum a, and y += s_g P_g + t_g A_g by two fmas, t = b - MAG s
   (x 17 for 8 bit) built in double and rounded to fp32 once.  What is accumulated has the magnitude
       Q = sum_g (|s_g| sum (MAG + q_lo) |a| (+ 16 sum (MAG + q_hi) |a|) + |t_g| sum |a|),
   and the roundings are: 64 inside a group's MFMA sums, 1 for the plane fma, 2 fmas per group over G = K / 64 groups, at most 15
   cross-wave adds: (64 + 1 + 2 G + 16) u Q, plus u sum_g |t_g| |A_g| for the rounding of t.
 * carried norm (consumer side): rstd = rsqrt(sum_t ss[t] / dim + eps) * rs_scale in fp32: T + 1 roundings on the positive sum (half of
   them survive the square root), one each for the rsqrt result and the scale, plus the caller's allowance for rsqrtf; the accumulator
   times rstd, plus the bias, adds one rounding each.
 * SiLU: v / (1 + exp(-v)) is 1.1-Lipschitz; its fp32 evaluation (__expf, the division) gets the caller's allowance; the product with
   the up value adds one rounding.
 * SK_RESID: x += fl(acc + bias) is two roundings; x * nw one; the tile's sum of squares 16 squares and 15 adds.
 * 16-bit outputs: the kernel's fp32 value v is within the fp32 bound b of the reference, and the stored value within half an ulp of the
   type at v: b + ulp16(|ref| + b) / 2, with f16's subnormal spacing 2^-24 as the floor.
The callers measure the two intrinsic allowances on the CPU (tests/test_skinny_gpu.py says how)."""
from __future__ import annotations

import numpy as np

from mlx_swift_audio_amd import _lib
from mlx_swift_audio_amd import audio as _audio

U = 2.0 ** -24
SK_OUTF32, SK_PARTIAL, SK_SWIGLU, SK_RESID = 1, 2, 4, 5
EXACT_LIMIT = 2 ** 24


def mag_of(dtype: int) -> float:
    return 1024.0 if dtype == _lib.F16 else 128.0


def store16(x, dtype: int) -> np.ndarray:
    """float -> the 16-bit storage array of `dtype` (np.float16, or uint16 bit patterns for bf16), round to nearest even"""
    x = np.asarray(x, np.float64)
    if dtype == _lib.F16:
        return x.astype(np.float16)
    return _audio.f32_to_bf16(x.astype(np.float32))


def load16(a: np.ndarray, dtype: int) -> np.ndarray:
    return (a.astype(np.float32) if dtype == _lib.F16 else _audio.bf16_to_f32(a)).astype(np.float64)


def round16(x, dtype: int) -> np.ndarray:
    return load16(store16(x, dtype), dtype)


def half_ulp16(x, dtype: int) -> np.ndarray:
    """half the spacing of the 16-bit type at magnitude |x| (f16: subnormal floor)"""
    a = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(a, 1e-300)))
    if dtype == _lib.F16:
        return 2.0 ** (np.maximum(e, -14.0) - 11.0)
    return 2.0 ** (np.maximum(e, -126.0) - 8.0)


def bound16(ref, b32, dtype: int) -> np.ndarray:
    return b32 + half_ulp16(np.abs(ref) + b32, dtype)


def silu64(v):
    return v / (1.0 + np.exp(-v))


def rstd_ref(ss_in, ss_tiles: int, ss_dim: int, eps: float, rs_scale: float, rsqrt_allow: float = 0.0, wrong: str | None = None):
    """rstd[m] (float64) and its relative fp32 error bound.  ss_in [tiles][M]."""
    ss = np.asarray(ss_in, np.float64)[:ss_tiles]
    eps, rs = float(np.float32(eps)), float(np.float32(rs_scale))
    mean = ss.sum(0) / ss_dim
    r = 1.0 / np.sqrt(mean + eps) * rs
    if wrong == "eps-outside":
        r = 1.0 / (np.sqrt(mean) + eps) * rs
    if wrong == "no-rs-scale":
        r = 1.0 / np.sqrt(mean + eps)
    rel = (0.5 * (ss_tiles + 3) + 2.0) * U + rsqrt_allow
    return r, rel


# ---- the accumulator and the bound of its fp32 evaluation ---------------------------------------------------------------------------
def acc16(A, W, k0: int, k1: int):
    """16-bit family: exact sum over [k0, k1) and (K + 2) u sum |a w|"""
    a, w = A[:, k0:k1], W[:, k0:k1]
    return a @ w.T, (k1 - k0 + 2) * U * (np.abs(a) @ np.abs(w).T)


def unpack_codes(codes: np.ndarray, bits: int) -> np.ndarray:
    """MLX packing, little end first: uint32 [N][K bits / 32] -> codes uint8 [N][K]"""
    per = 32 // bits
    sh = (np.arange(per, dtype=np.uint32) * bits)[None, None, :]
    return ((codes[:, :, None] >> sh) & np.uint32((1 << bits) - 1)).astype(np.uint8).reshape(codes.shape[0], -1)


def t_offset(s64, b64, bits: int, dtype: int, wrong: str | None = None):
    """the fp32 offset the repack stores: fl32(b - MAG s) (8 bit: 17 MAG s), built in double"""
    mag = mag_of(dtype)
    if wrong == "wrong-mag":
        mag = 128.0 if mag == 1024.0 else 1024.0
    return (b64 - mag * (17.0 if bits == 8 else 1.0) * s64).astype(np.float32).astype(np.float64)


def _gdot(a3, q3):
    """[M][G][64] x [N][G][64] -> [M][N][G]"""
    out = np.empty((a3.shape[0], q3.shape[0], a3.shape[1]))
    for g in range(a3.shape[1]):          # one BLAS call per group on strided views (a batched matmul of the transposes copies both)
        out[:, :, g] = a3[:, g, :] @ q3[:, g, :].T
    return out


def accq(A, q, s64, b64, bits: int, dtype: int, k0: int, k1: int, wrong: str | None = None):
    """packed family over [k0, k1) (multiples of 64): sum_g (s_g sum q a + b_g sum a), the bound described at the top, and the largest
    magnitude any intermediate of the kernel can reach (for the exact-integer cases)"""
    M, N = A.shape[0], q.shape[0]
    g0, g1 = k0 // 64, k1 // 64
    G = g1 - g0
    a3 = A[:, k0:k1].reshape(M, G, 64)
    q3 = q[:, k0:k1].reshape(N, G, 64).astype(np.float64)
    s, b = s64[:, g0:g1], b64[:, g0:g1]
    mag = mag_of(dtype)
    t = t_offset(s, b, bits, dtype)
    Asum, Aabs = a3.sum(-1), np.abs(a3).sum(-1)                               # [M][G]
    if wrong == "no-hi-weight" and bits == 8:
        q3 = np.floor(q3 / 16) + np.mod(q3, 16)                               # P_lo + P_hi: the plane weight 16 missing
    P = _gdot(a3, q3)                                     # sum q a per group
    contrib = s[None] * P + b[None] * Asum[:, None, :]
    y = contrib.sum(-1)
    if bits == 8:
        lo, hi = np.mod(q3, 16), np.floor(q3 / 16)
        Pmag = _gdot(np.abs(a3), mag + lo) + 16.0 * _gdot(np.abs(a3), mag + hi)
    else:
        Pmag = _gdot(np.abs(a3), mag + q3)
    Qg = np.abs(s)[None] * Pmag + np.abs(t)[None] * Aabs[:, None, :]
    bound = (64 + 1 + 2 * G + 16) * U * Qg.sum(-1) + U * (np.abs(t)[None] * np.abs(Asum)[:, None, :]).sum(-1)
    peak = np.abs(contrib).sum(-1) + Qg.max(-1)                              # any partial sum of groups + one group's uncancelled terms
    if wrong == "wrong-mag":                                                  # the offset built with the other type's MAG does not cancel
        y = y + ((t_offset(s, b, bits, dtype, wrong) - t)[None] * Asum[:, None, :]).sum(-1)
    return y, bound, max(float(peak.max()), float(Pmag.max()))


# ---- the four modes ------------------------------------------------------------------------------------------------------------------
def skinny_ref(*, mode: int, dtype: int, A, W=None, q=None, scales=None, biases=None, bits: int = 0, bias=None, S: int = 1, ss_in=None, ss_tiles: int = 0,
               ss_dim: int = 0, eps: float = 0.0, rs_scale: float = 1.0, xres=None, nw=None, silu_allow: float = 0.0, rsqrt_allow: float = 0.0,
               wrong: str | None = None) -> dict:
    """A [M][K] float64 (16-bit values); W [N][K] float64 (16-bit values) or q integer codes [N][K] with scales / biases float64 [N][K/64]
    (values of their stored type).  Returns float64 arrays: out + out_tol (SK_PARTIAL: [S][M][N]), for SK_RESID also xres / xres_tol and
    ss_out / ss_tol [N/16][M]; `peak`: the largest magnitude an intermediate can reach (exact-integer cases).
    wrong: a deliberately wrong formula (tests/test_skinny_ref.py shows each leaves the bound)."""
    A = np.asarray(A, np.float64)
    M, K = A.shape
    N = (W if q is None else q).shape[0]
    peak = 0.0

    def acc(k0, k1):
        nonlocal peak
        if q is None:
            y, b = acc16(A, W, k0, k1)
            peak = max(peak, float((np.abs(A[:, k0:k1]) @ np.abs(W[:, k0:k1]).T).max()))
            return y, b
        y, b, pk = accq(A, q, scales, biases, bits, dtype, k0, k1, wrong)
        peak = max(peak, pk)
        return y, b

    rstd, rrel = (np.ones(M), 0.0) if ss_in is None else rstd_ref(ss_in, ss_tiles, ss_dim, eps, rs_scale, rsqrt_allow, wrong)
    bs = np.zeros(N) if bias is None else np.asarray(bias, np.float64)

    def scaled(y, b):                      # the accumulator times rstd: (value, bound)
        if ss_in is None:
            return y, b
        v = y * rstd[:, None]
        return v, b * np.abs(rstd)[:, None] + np.abs(v) * (rrel + U)

    if mode == SK_PARTIAL:
        Kc = K // S
        outs, tols = [], []
        for s in range(S):
            k0 = s * Kc + ((32 if q is None else 64) if wrong == "k-slice-shift" else 0)      # one K-step (one group) late
            y, b = acc(k0, min(k0 + Kc, K))
            v, b = scaled(y, b)
            outs.append(v); tols.append(b)
        return dict(out=np.stack(outs), out_tol=np.stack(tols), peak=peak)

    y, b = acc(0, K)
    if wrong == "rstd-after-bias" and ss_in is not None:
        v, vb = (y + bs[None]) * rstd[:, None], b
    else:
        v, vb = scaled(y, b)
        v = v + bs[None]
        vb = vb + U * np.abs(v) * (bias is not None)
    if mode == SK_OUTF32:
        return dict(out=v, out_tol=vb, peak=peak)
    if mode == SK_SWIGLU:
        g, up = (v[:, 0::2], v[:, 1::2]) if wrong != "gate-up-swapped" else (v[:, 1::2], v[:, 0::2])
        gb, ub = vb[:, 0::2], vb[:, 1::2]
        sg = silu64(g)
        o = sg * up
        ob = (1.1 * gb + silu_allow) * np.abs(up) + np.abs(sg) * ub + gb * ub * 1.1 + U * np.abs(o)
        return dict(out=round16(o, dtype), out_tol=bound16(o, ob, dtype), out_f64=o, gate=g, peak=peak)
    assert mode == SK_RESID and N % 16 == 0
    x0 = np.asarray(xres, np.float64)
    xn = x0 + v
    xb = vb + U * np.abs(v) + U * np.abs(xn)                         # fl(acc + bias), then fl(x + .)
    o = xn * np.asarray(nw, np.float64)[None]
    ob = xb * np.abs(nw)[None] + U * np.abs(o)
    sq = (xn * xn).reshape(M, N // 16, 16)
    ss = sq.sum(-1).T                                                # [tile][m]
    ssb = ((2 * np.abs(xn) * xb + xb * xb).reshape(M, N // 16, 16).sum(-1) + 17 * U * sq.sum(-1)).T
    if wrong == "ss-tile-shift":
        ss = np.roll(ss, 1, axis=0)
    return dict(out=round16(o, dtype), out_tol=bound16(o, ob, dtype), xres=xn, xres_tol=xb, ss_out=ss, ss_tol=ssb, peak=max(peak, float(sq.sum(-1).max())))


def norm_linear_ref(x, gain, W, eps: float):
    """float64 RMSNorm then Linear of a residual x [M][D]: the function a producer -> consumer chain computes"""
    x = np.asarray(x, np.float64)
    h = x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * np.asarray(gain, np.float64)[None]
    return h @ np.asarray(W, np.float64).T
