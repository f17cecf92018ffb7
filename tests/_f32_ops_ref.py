"""float64 references of the two fp32 operators (the tap-structured GEMM of codec_kernels.hip and the attention of attn_f32.hip), with
the error bound each comparison is entitled to.

The bounds are derived, not tuned.  Both kernels form exact fp32 products and accumulate them in fp32, so for ANY summation order the
error of a length-K dot product is at most (K + 2) * 2^-24 * A, A = sum |x w| + |bias| of that output (computed here in float64).
Every later fp32 operation of the epilogue adds one rounding of its own result and scales the error carried so far by its Lipschitz
constant; device intrinsics get an allowance the caller measures on the CPU (tests/test_f32_ops_gpu.py says how)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

EPS32 = 2.0 ** -24
SIN_CW_ABS = 2e-7                 # absolute error codec_kernels.hip documents for its sin
ACT_LIPSCHITZ = {0: 1.0, 1: 1.13, 2: 1.0, 3: 1.0, 4: 1.1, 5: 1.0, 6: 1.0}


def act_f64(v: np.ndarray, act: int) -> np.ndarray:
    if act == 0:
        return v
    if act == 1:
        return 0.5 * v * (1.0 + torch.erf(torch.from_numpy(v / np.sqrt(2.0))).numpy())
    if act == 2:
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    if act == 3:
        return np.abs(v)
    if act == 4:
        return v / (1.0 + np.exp(-v))
    if act == 5:
        return np.where(v > 0, v, 0.01 * v)
    if act == 6:
        return np.maximum(v, 0.0)
    raise ValueError(act)


def act_f32_torch(v32: np.ndarray, act: int) -> np.ndarray:
    """The same activation evaluated in float32 by torch (the yardstick the device intrinsics are held against)."""
    import torch.nn.functional as F
    t = torch.from_numpy(np.ascontiguousarray(v32, np.float32))
    f = {0: lambda x: x, 1: F.gelu, 2: F.elu, 3: torch.abs, 4: F.silu, 5: lambda x: F.leaky_relu(x, 0.01), 6: F.relu}[act]
    return f(t).numpy()


def prologue_f64(x: np.ndarray, alpha=None, ralpha=None, lrelu_slope: float = 0.0) -> np.ndarray:
    if alpha is not None:
        a = np.asarray(alpha, np.float64)
        ra = 1.0 / (a + 1e-9) if ralpha is None else np.asarray(ralpha, np.float64)
        return x + np.sin(a * x) ** 2 * ra
    if lrelu_slope > 0:
        return np.where(x > 0, x, x * float(np.float32(lrelu_slope)))
    return x


class TapGemm(NamedTuple):
    Y: np.ndarray          # float64, Y's whole buffer (unwritten elements keep the given contents)
    written: np.ndarray    # bool, same shape
    tol: np.ndarray        # per-element bound on |kernel - Y| (0 where nothing is written)
    pre: np.ndarray        # acc + bias of the written elements


def tap_gemm_ref(phases: int = 1, *, X, W, Y=None, T_in, T_out, M, N, Cin, taps=1, dil=1, pad=0, x_row_mul=1, ldx=None, ldw=0, w_phase_stride=0,
                 bias=None, alpha=None, ralpha=None, lrelu_slope=0.0, ldy=None, y_row_mul=1, y_row_off=0, y_phase_step=0, R=None, R2=None,
                 ldr=None, noise=None, out_scale=0.0, act=0, tanh_out=0, phase_len=None, x_phase_step=0, n_seq=1, x_seq_step=0, y_seq_step=0,
                 seq_len=None, noise_seq_off=None, allow_pre=None, wrong=None) -> TapGemm:
    """codec.h's formula, one loop per grid phase z, stacked sequence u and tap:
        Y[u*y_seq_step + row(m)][n] = epi(sum_{tap,c} pre(X[u*x_seq_step + z*x_phase_step + m*x_row_mul + tap*dil - pad][c]) W_z[n][tap*Cin + c] + bias[n])
        row(m) = m*y_row_mul + y_row_off + z*y_phase_step, dropped outside [0, T_out); X rows outside [0, T_valid) are zero.
    allow_pre [Cin]: bound on the device's error in pre() per input channel (snake_allowance / lrelu_allowance); the allowances of the
    activation and of the final tanh are measured here, per (u, z) block, over the block's own values (act_allowance, tanh_allowance).
    wrong = "order" applies out_scale after R2 (a deliberately wrong epilogue for the can-it-fail checks)."""
    X = np.asarray(X, np.float64)
    Wf = np.asarray(W, np.float64).reshape(-1)
    K = taps * Cin
    ldw = int(ldw) if ldw else K
    rows_y = (n_seq - 1) * int(y_seq_step) + T_out
    Yo = np.zeros((rows_y, N)) if Y is None else np.array(Y, np.float64)
    written = np.zeros(Yo.shape, bool)
    tol = np.zeros(Yo.shape)
    pre_o = np.zeros(Yo.shape)
    Rf = None if R is None else np.asarray(R, np.float64)
    R2f = None if R2 is None else np.asarray(R2, np.float64)
    nzf = None if noise is None else np.asarray(noise, np.float64).reshape(-1)
    b = np.zeros(N) if bias is None else np.asarray(bias, np.float64)
    dpre = None if allow_pre is None else np.asarray(allow_pre, np.float64)
    m = np.arange(M)
    for u in range(n_seq):
        for z in range(phases):
            Xb = X[u * int(x_seq_step) + z * int(x_phase_step):]
            T_valid = min(T_in, int(seq_len[u])) if seq_len is not None else min(T_in, int(phase_len[z])) if phase_len is not None else T_in
            Wz = Wf[z * int(w_phase_stride):][:(N - 1) * ldw + K]
            Wz = np.stack([Wz[n * ldw:n * ldw + K] for n in range(N)])
            acc = np.zeros((M, N))
            A = np.zeros((M, N))
            E = np.zeros((M, N))
            for tap in range(taps):
                r = m * x_row_mul + tap * dil - pad
                ok = (r >= 0) & (r < T_valid)
                xa = np.zeros((M, Cin))
                xa[ok] = prologue_f64(Xb[r[ok], :Cin], alpha, ralpha, lrelu_slope)
                wt = Wz[:, tap * Cin:(tap + 1) * Cin]
                acc += xa @ wt.T
                A += np.abs(xa) @ np.abs(wt).T
                if dpre is not None:
                    E += ok[:, None] * (np.abs(wt) @ dpre)[None, :]
            v = acc + b
            e = (K + 2) * EPS32 * (A + np.abs(b)) + E
            pre = v
            yr = m * y_row_mul + y_row_off + z * y_phase_step
            T_lim = min(T_out, T_valid) if (noise is not None and noise_seq_off is not None) else T_out
            keep = (yr >= 0) & (yr < T_lim)
            yk = yr[keep]
            rows = u * int(y_seq_step) + yk
            v, e, pre = v[keep], e[keep], pre[keep]
            if act:
                v = act_f64(v, act)
                e = ACT_LIPSCHITZ[act] * e + act_allowance(pre, act) + EPS32 * np.abs(v)
            if nzf is not None:
                nz = nzf[(int(noise_seq_off[u]) if noise_seq_off is not None else 0) + yk][:, None]
                e = np.abs(nz) * e + EPS32 * np.abs(nz * v)
                v = Rf[rows, :N] + nz * v
                e = e + EPS32 * np.abs(v)
            elif Rf is not None:
                v = v + Rf[rows, :N]
                e = e + EPS32 * np.abs(v)
            if wrong == "order":
                if R2f is not None:
                    v = v + R2f[rows, :N]
                if out_scale != 0.0:
                    v = v * float(np.float32(out_scale))
            else:
                if out_scale != 0.0:
                    v = v * float(np.float32(out_scale))
                    e = abs(out_scale) * e + EPS32 * np.abs(v)
                if R2f is not None:
                    v = v + R2f[rows, :N]
                    e = e + EPS32 * np.abs(v)
            if tanh_out:
                e = e + tanh_allowance(v) + EPS32
                v = np.tanh(v)
            Yo[rows, :N] = v
            written[rows, :N] = True
            tol[rows, :N] = e
            pre_o[rows, :N] = pre
    return TapGemm(Yo, written, tol, pre_o)


def snake_allowance(x32: np.ndarray, alpha32: np.ndarray, ralpha32=None) -> np.ndarray:
    """Per input channel: 4 x the largest error of the snake prologue evaluated in float32 by torch against float64 over the values x32
    [rows, Cin], plus the documented absolute error of the kernel's sin carried through d(ralpha s^2) = ralpha 2 |s| ds, |s| <= 1."""
    x = torch.from_numpy(np.ascontiguousarray(x32, np.float32))
    a = torch.from_numpy(np.ascontiguousarray(alpha32, np.float32))
    ra = 1.0 / (a + 1e-9) if ralpha32 is None else torch.from_numpy(np.ascontiguousarray(ralpha32, np.float32))
    s = torch.sin(a * x)
    y32 = (x + ra * (s * s)).numpy().astype(np.float64)
    y64 = prologue_f64(x32.astype(np.float64), alpha32.astype(np.float64), None if ralpha32 is None else ralpha32.astype(np.float64))
    return 4.0 * np.abs(y32 - y64).max(axis=0) + ra.numpy().astype(np.float64) * 2.0 * SIN_CW_ABS


def lrelu_allowance(x32: np.ndarray, slope: float) -> np.ndarray:
    """Per input channel: the one rounding of x * slope."""
    return EPS32 * abs(slope) * np.abs(x32).max(axis=0).astype(np.float64)


def act_allowance(pre: np.ndarray, act: int) -> float:
    """4 x the largest error of the activation evaluated in float32 by torch against float64 over these pre-activation values."""
    p32 = np.ascontiguousarray(pre, np.float32).reshape(-1)
    return 4.0 * float(np.abs(act_f32_torch(p32, act).astype(np.float64) - act_f64(p32.astype(np.float64), act)).max()) if p32.size else 0.0


def tanh_allowance(v: np.ndarray) -> float:
    v32 = np.ascontiguousarray(v, np.float32).reshape(-1)
    return 4.0 * float(np.abs(np.tanh(v32).astype(np.float64) - np.tanh(v32.astype(np.float64))).max()) if v32.size else 0.0


# ---- attention ------------------------------------------------------------------------------------------------------------------
def _attn_mask(T: int, Tb: int, chunk: int, wrong=None) -> np.ndarray:
    i = np.arange(T)[:, None]
    j = np.arange(T)[None, :]
    lim = np.full((T, 1), Tb)
    if chunk > 0:
        lim = np.minimum(Tb, ((i + (1 if wrong == "chunk" else 0)) // chunk + 1) * chunk)
    if wrong == "last_key":
        lim = lim - 1
    return j < lim


def attention_ref(q, k, v, scale, p=None, bias_u=None, bias_v=None, seq_len=None, chunk=0, *, B, T, H, dtype=np.float64, wrong=None):
    """softmax(((q + u) k^T + (q + v) p^T) scale) v per (batch, head), head dim 64, in `dtype` (float64: the reference; float32: the
    naive evaluation whose error sets the bound).  q / k / v [B*T, H*64], p [T, H*64], bias_u / bias_v [H, 64]; keys at or beyond
    max(1, seq_len[b]) and, with chunk > 0, at or beyond (i / chunk + 1) * chunk are masked.  Returns [B*T, H*64] (rows at or beyond
    seq_len[b] are computed like the others and mean nothing).  wrong: "last_key" | "chunk" | "bias" (deliberately wrong variants)."""
    q, k, v = (np.asarray(a, dtype) for a in (q, k, v))
    out = np.zeros((B * T, H * 64), dtype)
    sc = dtype(scale)
    for b in range(B):
        Tb = T if seq_len is None else min(T, max(1, int(seq_len[b])))
        mask = _attn_mask(T, Tb, chunk, wrong)
        for h in range(H):
            cs = slice(h * 64, h * 64 + 64)
            rs = slice(b * T, (b + 1) * T)
            qh, kh, vh = q[rs, cs], k[rs, cs], v[rs, cs]
            if p is not None:
                bu = np.asarray(bias_u, dtype)[h]
                bv = np.asarray(bias_u if wrong == "bias" else bias_v, dtype)[h]
                s = ((qh + bu) @ kh.T + (qh + bv) @ np.asarray(p, dtype)[:, cs].T) * sc
            else:
                s = (qh @ kh.T) * sc
            s = np.where(mask, s, -np.inf)
            s = s - s.max(axis=1, keepdims=True)
            e = np.exp(s)
            out[rs, cs] = (e @ vh) / e.sum(axis=1, keepdims=True)
    return out


def attention_tol(ref64: np.ndarray, naive32: np.ndarray, valid=None) -> float:
    """8 x the largest error of the naive float32 evaluation on the same inputs (over the rows that mean something)."""
    d = np.abs(naive32.astype(np.float64) - ref64)
    return 8.0 * float((d if valid is None else d[valid]).max())
