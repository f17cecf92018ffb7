"""Cases of the packed skinny GEMM at 6 bits (tests/test_skinny6_gpu.py), in the style of _skinny_cases._q.  The 6-bit instantiation of
skinny_gemm_qi takes the 8-bit form rule unchanged (csrc/skinny_quant.hip: skinny_qi_launch_t) and the 8-bit arithmetic behind its unpack
(two planes, P = P_lo + 16 P_hi, t = b - 17 MAG s), so the restated dispatch is _skinny_cases.dispatch_q(..., bits=8) and the float64
reference with its derived bound is _skinny_ref.accq(..., bits=8) on the unpacked codes: as_8(case) is the case those two are asked about.
The bound needs no change: a high part of 0..3 is a special case of the 0..15 it was derived for."""
from __future__ import annotations

import zlib
from dataclasses import replace

import numpy as np

import _quant6 as Q6
import _skinny_cases as sc
import _skinny_ref as ref
from _skinny_ref import SK_OUTF32, SK_PARTIAL, SK_RESID, SK_SWIGLU
from mlx_swift_audio_amd import _lib
from mlx_swift_audio_amd import checkpoint

ROWS = (1, 16, 17, 33)


def _q6(mode, N, K, S=1, dtypes=(_lib.BF16, _lib.F16), **kw):
    return [sc.Case(id=f"q6-{sc.MODE_NAME[mode]}-N{N}-K{K}-S{S}-{sc._dt(dt)}-s{kw.get('sdt', 'f16')}" + (f"-{kw['note']}" if kw.get("note") else ""), fam="q", mode=mode,
                    N=N, K=K, S=S, dtype=dt, bits=6, **kw) for dt in dtypes]


def _build() -> list[sc.Case]:
    c: list[sc.Case] = []
    # one wave: 1, 3, 5, 7 blocks (7 wraps the ring of three); 2, 3, 4 waves; S = 2
    for K, sdt in ((128, "f16"), (384, "bf16"), (640, "f16"), (896, "f32"), (768, "f16"), (1024, "bf16"), (1536, "f16"), (2048, "f16")):
        c += _q6(SK_PARTIAL, 41, K, Ms=ROWS, sdt=sdt, lda_extra=8 if K == 896 else 0)
    c += _q6(SK_PARTIAL, 41, 1536, 2, Ms=ROWS)
    for K in (128, 896):
        c += _q6(SK_SWIGLU, 36, K, Ms=ROWS, ldo_extra=1)
    for K in (256, 768):
        c += _q6(SK_OUTF32, 37, K, Ms=ROWS)                                   # ldo 37: scalar stores
    c += _q6(SK_RESID, 48, 1024, Ms=ROWS) + _q6(SK_RESID, 16, 8192, Ms=ROWS, bias=False) + _q6(SK_RESID, 16, 896, Ms=ROWS)
    # four tiles per wave: above 16 rows (one wave, four waves), by workgroup count at <= 16 rows, the one-wave vocabulary head (1, 4, 7 blocks)
    c += _q6(SK_PARTIAL, 3072, 512, 4, Ms=(1, 16, 17, 40), note="nt4") + _q6(SK_PARTIAL, 3072, 2048, 4, dtypes=(_lib.F16,), Ms=(1, 16, 17, 40), note="nt4")
    c += _q6(SK_PARTIAL, 65536, 512, 4, dtypes=(_lib.BF16,), Ms=(1, 16), note="nt4-by-count")
    c += _q6(SK_OUTF32, 65560, 128, Ms=(1, 17), note="head41") + _q6(SK_OUTF32, 65560, 512, dtypes=(_lib.F16,), Ms=(1, 17), note="head41")
    c += _q6(SK_OUTF32, 65560, 896, dtypes=(_lib.BF16,), Ms=(1, 17), note="head41")
    # the consumer side of the carried norm
    for t, rs, i in ((1, 0.125, 0), (65, 3.0, 1)):
        kw = dict(carry=t, rs_scale=rs, note=f"carry{t}", Ms=sc.FEW_M)
        c += _q6(SK_PARTIAL, 37, 768, **kw)[i:i + 1] + _q6(SK_OUTF32, 33, 256, **kw)[1 - i:2 - i]
    return c


CASES = _build()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case id"


def ids(pred=None):
    return [c.id for c in CASES if pred is None or pred(c)]


def as_8(c: sc.Case) -> sc.Case:
    """the case the 8-bit dispatch rule and the 8-bit reference are asked about"""
    return replace(c, bits=8)


def make_data(c: sc.Case, kind: str) -> sc.Data:
    """_skinny_cases.make_data for 6-bit codes (same operand rules): "real": quantize_affine(bits=6) of weights scaled to unit-size outputs;
    "int": a in {-1, 0, 1}, any code 0..63, scales 1 or 2, biases multiples of the scale"""
    rng = np.random.default_rng(zlib.crc32(f"{c.id}/{kind}".encode()))
    rows, N, K = max(c.Ms), c.N, c.K
    real = kind == "real"
    a = rng.standard_normal((rows, K)) if real else rng.integers(-1, 2, (rows, K))
    A16 = ref.store16(a, c.dtype)
    if real:
        codes, s, b = checkpoint.quantize_affine((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), 64, 6, np.float32)
        q = Q6.unpack6(codes)
    else:
        q = rng.integers(0, 64, (N, K))
        codes = Q6.pack6(q)
        s = rng.integers(1, 3, (N, K // 64)).astype(np.float64)
        b = s * rng.integers(-8, 9, (N, K // 64))
    sc_, s64 = sc._store_sdt(np.asarray(s, np.float64), c.sdt)
    bi, b64 = sc._store_sdt(np.asarray(b, np.float64), c.sdt)
    d = sc.Data(rows, A16, ref.load16(A16, c.dtype), codes=codes, scales=sc_, biases=bi, s64=s64, b64=b64, q=q)
    if c.bias and c.mode != SK_PARTIAL:
        d.bias = (rng.standard_normal(N) if real else rng.integers(-50, 51, N)).astype(np.float32)
    if c.mode == SK_RESID:
        d.nw = (1.0 + 0.1 * rng.standard_normal(N) if real else 2.0 ** rng.integers(-1, 2, N)).astype(np.float32)
        if real:
            d.xres = (3.0 * rng.standard_normal((rows, N))).astype(np.float32)
        else:      # the updated residual is a small integer r: x0 = r - (acc + bias), itself an integer below 2^24
            y = ref.accq(d.A, d.q, d.s64, d.b64, 8, c.dtype, 0, K)[0] + (0.0 if d.bias is None else d.bias.astype(np.float64)[None])
            x0 = rng.integers(-200, 201, (rows, N)) - y
            d.xres = x0.astype(np.float32)
            assert np.array_equal(d.xres.astype(np.float64), x0) and np.abs(x0).max() < ref.EXACT_LIMIT
    if c.carry and real:
        d.ss_in = rng.uniform(4.0, 40.0, (c.carry, rows)).astype(np.float32)
        d.ss_dim = 16 * c.carry
    return d


def reference(c: sc.Case, d: sc.Data, cols=None, **kw) -> dict:
    return sc.reference(as_8(c), d, cols, **kw)
