"""Operator-level parity of the many-row packed GEMM (csrc/gemm_quant.hip through mia_op_gemm_quant) -- the kernel behind
mia_lm_set_prompt_weights(lm, 1) -- against the float64 reference of the packed family, tests/_skinny_ref.py: accq, with that reference's
own per-element bound.  The bound counts 64 roundings inside a group's MFMA sums, one for the plane fma, two fmas per group and 16
cross-wave adds over the magnitude of what is really accumulated; it is per output element and does not depend on M, and this kernel has
no cross-wave add at all, so it applies unchanged (6 bits go through the 8-bit reference on the unpacked codes, _skinny6_cases.as_8).
Weights are packed by the existing packers (checkpoint.quantize_affine, _quant6) and repacked by the attach-side repack
(ops.quant_repack = mia_quant_repack).

 * bounded parity: M in {1, 31, 33, 127, 129, 200} (below, at and across the 16 / 32 / 64-row forms, two, three and four workgroups in M),
   N in {16, 41, 272} (one tile, a ragged tile, nine column blocks with a ragged last one), K in {128, 384, 896, 2048} (1, 3, 7 and 16
   blocks: the two-group register ring wraps), bits 4 / 6 / 8, both activation types, f16 and bf16 scales; per bit width one case with
   lda = K + 8, one with ldc = N + 1, one with the residual aliased to C and one with a separate R.  Every output sits between sentinel
   guards (columns past N, rows past M).
 * exact parity: scales 1, biases 0, activations small integers -- the result is the integer product, bit for bit.
 * tile independence: rows of an M = 200 call equal the same rows computed in an M = 33 call bit for bit (the K order is fixed and a
   row's result depends on its own A row alone).
Observed on an MI355X 2026-10-21, worst error / bound over the bounded cases: 0.0044 (q8-M129-N41-K128-f16)."""
import zlib

import numpy as np
import pytest
import torch

import _skinny6_cases as s6
import _skinny_cases as sc
import _skinny_ref as ref
import mlx_swift_audio_amd as m
from _skinny_ref import SK_OUTF32
from mlx_swift_audio_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 8
SENT = np.float32(-1234.5)
MS, NS, KS = (1, 31, 33, 127, 129, 200), (16, 41, 272), (128, 384, 896, 2048)
DTS, SDTS = (m._lib.BF16, m._lib.F16), ("f16", "bf16")


def _cases():
    """twelve per bit width: every M twice, every N four times, every K three times, both types and both scale types; four of them carry
    one of the stride / residual variants"""
    out = []
    for bi, bits in enumerate((4, 6, 8)):
        for i in range(12):
            M, N, K = MS[i % 6], NS[(i + i // 6 + bi) % 3], KS[(i + bi) % 4]
            dt, sdt = DTS[(i // 2 + bi) % 2], SDTS[(i + i // 4) % 2]
            extra = {1: "lda", 2: "ldc", 3: "alias", 4: "resid"}.get(i, "")
            out.append(pytest.param(bits, M, N, K, dt, sdt, extra, id=f"q{bits}-M{M}-N{N}-K{K}-{sc._dt(dt)}-s{sdt}" + (f"-{extra}" if extra else "")))
    return out


def _data(bits, M, N, K, dt, sdt, kind):
    c = sc.Case(id=f"gq{bits}-M{M}-N{N}-K{K}-{dt}-{sdt}", fam="q", mode=SK_OUTF32, N=N, K=K, dtype=dt, bits=bits, sdt=sdt, Ms=(M,), bias=False)
    d = (s6.make_data if bits == 6 else sc.make_data)(c, kind)
    wf, st = ops.quant_repack(d.codes, d.scales, d.biases, bits, sc.SDT[sdt], dt)
    return c, d, torch.from_numpy(wf.view(np.int32)).cuda(), torch.from_numpy(st).cuda()


def _t16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _run(ctx, A16, wf, st, bits, M, N, K, dt, extra="", R=None):
    """one call on rows A16 [M][K]; returns C [M][N] after checking the guards around it"""
    if extra == "lda":          # a view into a larger buffer: two rows and 8 columns in
        buf = torch.zeros((M + 4, K + 8), dtype=torch.int16, device="cuda")
        buf[2:2 + M, 8:8 + K] = _t16(A16)
        A = buf[2:2 + M, 8:8 + K]
    else:
        A = _t16(A16)
    ldc = N + 1 if extra == "ldc" else N + GUARD
    full = torch.full((M + 2, ldc), float(SENT), dtype=torch.float32, device="cuda")
    Cv = full[1:1 + M, :N]
    Rt = None
    if extra == "alias":
        Cv.copy_(torch.from_numpy(R))
        Rt = Cv
    elif extra == "resid":
        Rt = torch.from_numpy(R).cuda()
    ops.gemm_quant(ctx, A, wf, st, bits, Cv, M, N, K, dt, R=Rt, lda=A.stride(0), ldc=ldc, ldr=None if Rt is None else Rt.stride(0))
    got = full.cpu().numpy()
    assert (got[0] == SENT).all() and (got[-1] == SENT).all() and (got[:, N:] == SENT).all(), "wrote outside C"
    return got[1:1 + M, :N].copy()


@pytest.mark.parametrize("bits,M,N,K,dt,sdt,extra", _cases())
def test_bounded_parity(ctx, bits, M, N, K, dt, sdt, extra):
    c, d, wf, st = _data(bits, M, N, K, dt, sdt, "real")
    y, bound, _ = ref.accq(d.A, d.q, d.s64, d.b64, s6.as_8(c).bits if bits == 6 else bits, dt, 0, K)
    R = None
    if extra in ("alias", "resid"):
        R = np.random.default_rng(zlib.crc32(c.id.encode())).standard_normal((M, N)).astype(np.float32)
        y = y + R.astype(np.float64)
        bound = bound + ref.U * np.abs(y)                 # one more rounding: fl(acc + r)
    got = _run(ctx, d.A16, wf, st, bits, M, N, K, dt, extra, R)
    err = np.abs(got.astype(np.float64) - y)
    print(f"{c.id}: worst error / bound {float((err / bound).max()):.4f}, worst error {float(err.max()):.3e}")
    assert np.isfinite(got).all() and (err <= bound).all(), f"{float((err / bound).max())} x the bound"
    # and a second launch agrees bit for bit
    assert np.array_equal(got, _run(ctx, d.A16, wf, st, bits, M, N, K, dt, extra, R))


@pytest.mark.parametrize("bits,dt", [(4, m._lib.BF16), (6, m._lib.F16), (8, m._lib.BF16)])
def test_exact_integer_product(ctx, bits, dt):
    M, N, K = 129, 41, 896
    rng = np.random.default_rng(bits)
    a = rng.integers(-3, 4, (M, K))
    q = rng.integers(0, 1 << bits, (N, K))
    codes = s6.Q6.pack6(q) if bits == 6 else sc._pack(q, bits)
    s, b = np.ones((N, K // 64), np.float16), np.zeros((N, K // 64), np.float16)
    want = a @ q.T
    # every intermediate the kernel forms is an integer below 2^24: a plane's group sum, the 8-bit plane fma, t A and the running sum
    mag = ref.mag_of(dt)
    assert 17 * (mag + 15) * 3 * 64 + np.abs(want).max() + 64 * 255 * 3 * (K // 64) < ref.EXACT_LIMIT
    wf, st = ops.quant_repack(codes, s, b, bits, m._lib.F16, dt)
    got = _run(ctx, ref.store16(a, dt), torch.from_numpy(wf.view(np.int32)).cuda(), torch.from_numpy(st).cuda(), bits, M, N, K, dt)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


@pytest.mark.parametrize("bits,dt", [(4, m._lib.F16), (6, m._lib.BF16), (8, m._lib.F16)])
def test_rows_do_not_depend_on_the_row_tile(ctx, bits, dt):
    N, K = 41, 896
    c, d, wf, st = _data(bits, 200, N, K, dt, "f16", "real")
    big = _run(ctx, d.A16, wf, st, bits, 200, N, K, dt)
    for r0 in (0, 100, 167):
        part = _run(ctx, d.A16[r0:r0 + 33], wf, st, bits, 33, N, K, dt)
        assert np.array_equal(part, big[r0:r0 + 33]), r0
    # the 16- and 32-row forms too: one row alone, and 17 rows
    assert np.array_equal(_run(ctx, d.A16[199:200], wf, st, bits, 1, N, K, dt), big[199:200])
    assert np.array_equal(_run(ctx, d.A16[64:81], wf, st, bits, 17, N, K, dt), big[64:81])


def test_refusals(ctx):
    c, d, wf, st = _data(4, 33, 16, 128, m._lib.BF16, "f16", "real")
    A, Cv = _t16(d.A16), torch.zeros((33, 16), dtype=torch.float32, device="cuda")
    for kw in (dict(bits=5), dict(K=64), dict(lda=132), dict(ldc=8), dict(M=0), dict(dtype=m._lib.F32)):
        args = dict(bits=4, M=33, N=16, K=128, dtype=m._lib.BF16, lda=128, ldc=16)
        args.update(kw)
        with pytest.raises(m._lib.MiaError) as e:
            ops.gemm_quant(ctx, A, wf, st, args["bits"], Cv, args["M"], args["N"], args["K"], args["dtype"], lda=args["lda"], ldc=args["ldc"])
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, kw
    assert not Cv.any()
