"""Operator-level parity of the LM step's skinny GEMMs: every kernel form skinny_gemm_launch (16-bit weights, csrc/skinny_rowmajor.hip) and
skinny_gemm_q_launch (packed 4- / 8-bit weights, csrc/skinny_quant.hip) choose from the shape, through the mia_op_skinny_gemm hook, against
the float64 references of tests/_skinny_ref.py (pinned against torch and shown able to fail in tests/test_skinny_ref.py).  The cases and
the restated dispatch rules are in tests/_skinny_cases.py.

Per case:
 * bounded parity on random real operands: |got - ref| <= bound at every element, the bound derived per element in _skinny_ref.py
   ((K + 2) 2^-24 sum |a w| for the 16-bit family; the magnitude of what the packed kernels really accumulate, sum_g |s| sum (MAG + q)|a|
   + |t| sum |a|, for the packed family; one rounding per epilogue operation; half an ulp of the 16-bit type for 16-bit outputs);
 * exact parity on small integers (every intermediate below 2^24, asserted on the CPU): SK_OUTF32, every SK_PARTIAL slice, xres, ss_out
   and the 16-bit SK_RESID output equal the reference bit for bit;
 * untouched memory: every output sits between sentinel guards (columns past N, rows past M, ss_out past its tiles, xres rows past M);
 * contracts, bit for bit: two launches agree; fragment-order weights agree with row-major; row r of an M-row call is the one-row call
   on that row (16-bit: every M; packed: wherever the restated rule gives both M the same split of K -- always within M <= 16 and within
   M > 16 -- and for every M once M_cap carries the capacity; where the split of K depends on M the bound is asserted instead, those
   shapes are listed at skinny_gemm_q_launch in csrc/skinny.h).

Intrinsic allowances (4 x the error of the same function in float32 torch against float64, over the case's own values), measured on the
CPU 2026-10-19, already times 4, largest over the cases: SiLU (for __expf and the division) 1.7e-6 absolute at gates up to |v| ~ 5
(q4-swiglu-N40-K128-S1-bf16); rsqrt 3.4e-7 relative (the Qwen2-0.5B fused q|k|v tuple).
Observed on an MI355X the same day, worst error / bound: 16-bit family 0.67 (h-resid-N48-K2048-S1-f16, a 16-bit output: half an ulp of
f16 dominates; fp32 outputs 0.022), packed family 0.39 (q4-swiglu-N36-K896-S1-bf16-carry64, a 16-bit output; fp32 outputs 0.006), producer -> consumer chain 0.13.
The fp32 bounds are worst-case bounds over every summation order, so random operands sit far inside them; what a tolerance cannot
see -- a dropped, doubled or misplaced K-step or tile -- is what the exact-integer cases are for.  No bound was widened."""
import numpy as np
import pytest
import torch

import _skinny_cases as sc
import _skinny_ref as ref
import mlx_swift_audio_amd as m
from _skinny_ref import SK_OUTF32, SK_PARTIAL, SK_RESID, SK_SWIGLU
from mlx_swift_audio_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 16
SENT32 = np.float32(-1234.5)
SENT16 = np.int16(-15206)         # 0xC49A: a finite value in both 16-bit types


def _t16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


class Dev:
    """the operands of a case on the device (weights once; activations per call)"""

    def __init__(self, c: sc.Case, d: sc.Data):
        self.c, self.d = c, d
        if c.fam == "h":
            self.W = _t16(d.W16)
        else:
            wf, st = ops.quant_repack(d.codes, d.scales, d.biases, c.bits, sc.SDT[c.sdt], c.dtype)
            self.wfrag, self.stfrag = torch.from_numpy(wf.view(np.int32)).cuda(), torch.from_numpy(st).cuda()
        self.A = _t16(d.A16)
        self.bias = None if d.bias is None else torch.from_numpy(d.bias).cuda()
        self.nw = None if d.nw is None else torch.from_numpy(d.nw).cuda()


def run(ctx, dev: Dev, M: int, r0: int = 0, w_frag: int = 0, M_cap: int = 0, **over) -> dict:
    """rows [r0, r0 + M) of the case as one call; checks the guards; returns the outputs as numpy arrays (16-bit ones as bit patterns)"""
    c, d = dev.c, dev.d
    N, K, tiles = c.N, c.K, (c.N + 15) // 16
    if c.lda_extra:               # a view into a larger buffer: two rows and 8 columns in
        buf = torch.zeros((M + 4, K + c.lda_extra), dtype=torch.int16, device="cuda")
        buf[2:2 + M, 8:8 + K] = dev.A[r0:r0 + M]
        A = buf[2:2 + M, 8:8 + K]
    else:
        A = dev.A[r0:r0 + M]
    kw = dict(A=A, M=M, N=N, K=K, S=c.S, mode=c.mode, dtype=c.dtype, bias=dev.bias, w_frag=w_frag, M_cap=M_cap)
    if c.fam == "h":
        kw.update(W=dev.W)
    else:
        kw.update(wfrag=dev.wfrag, stfrag=dev.stfrag, bits=c.bits)
    if c.mode == SK_PARTIAL:
        big = torch.full((64 + c.S * M * N + 64,), float(SENT32), dtype=torch.float32, device="cuda")
        kw.update(out=big[64:64 + c.S * M * N], ldo=0)
    else:
        ldo = c.ncols + c.ldo_extra
        f32 = c.mode == SK_OUTF32
        big = torch.full((GUARD + M + GUARD, ldo), float(SENT32) if f32 else int(SENT16), dtype=torch.float32 if f32 else torch.int16, device="cuda")
        kw.update(out=big[GUARD:GUARD + M], ldo=ldo)
    xbig = sbig = None
    if c.mode == SK_RESID:
        xbig = torch.full((M + GUARD, N), float(SENT32), dtype=torch.float32, device="cuda")
        xbig[:M] = torch.from_numpy(d.xres[r0:r0 + M]).cuda()
        sbig = torch.full(((tiles + GUARD) * M,), float(SENT32), dtype=torch.float32, device="cuda")
        kw.update(xres=xbig, nw=dev.nw, ss_out=sbig)
    if d.ss_in is not None:
        kw.update(ss_in=torch.from_numpy(np.ascontiguousarray(d.ss_in[:, r0:r0 + M])).cuda(), ss_tiles=c.carry, ss_dim=d.ss_dim, eps=d.eps, rs_scale=c.rs_scale)
    kw.update(over)
    ops.skinny_gemm(ctx, **kw)
    o = big.cpu().numpy()
    res = {}
    if c.mode == SK_PARTIAL:
        assert (o[:64] == SENT32).all() and (o[-64:] == SENT32).all(), f"{c.id}: wrote outside out"
        res["out"] = o[64:-64].reshape(c.S, M, N)
    else:
        sent = SENT32 if c.mode == SK_OUTF32 else SENT16
        assert (o[:GUARD] == sent).all() and (o[-GUARD:] == sent).all(), f"{c.id}: wrote rows outside out"
        assert (o[GUARD:-GUARD, c.ncols:] == sent).all(), f"{c.id}: wrote columns past the row"
        res["out"] = o[GUARD:-GUARD, :c.ncols]
    if c.mode == SK_RESID:
        x, s = xbig.cpu().numpy(), sbig.cpu().numpy()
        assert (x[M:] == SENT32).all(), f"{c.id}: wrote xres rows past M"
        assert (s[tiles * M:] == SENT32).all(), f"{c.id}: wrote ss_out past its tiles"
        res["xres"], res["ss_out"] = x[:M], s[:tiles * M].reshape(tiles, M)
    return res


def _same(a: dict, b: dict, rows=slice(None)) -> bool:
    """bit for bit (outputs hold no NaN); rows: the rows of `a` that `b` holds"""
    for k in a:
        x = a[k][:, rows] if k == "ss_out" or (k == "out" and a[k].ndim == 3) else a[k][rows]
        if not np.array_equal(x, b[k]):
            return False
    return True


def _values(c: sc.Case, res: dict) -> dict:
    """float64 values of the outputs"""
    out = dict(res)
    if c.mode in (SK_SWIGLU, SK_RESID):
        out["out"] = ref.load16(res["out"].view(np.float16) if c.dtype == m._lib.F16 else res["out"].view(np.uint16), c.dtype)
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def _allowances(c: sc.Case, d: sc.Data, cols) -> tuple[float, float]:
    """4 x the float32 torch error against float64 of SiLU over this case's gate values and of rsqrt over its mean squares"""
    silu = rsq = 0.0
    if d.ss_in is not None:
        x32 = (d.ss_in.astype(np.float64).sum(0) / d.ss_dim + d.eps).astype(np.float32)
        r32 = torch.rsqrt(torch.from_numpy(x32)).numpy().astype(np.float64)
        rsq = 4.0 * float(np.abs(r32 * np.sqrt(x32.astype(np.float64)) - 1.0).max())
    if c.mode == SK_SWIGLU:
        g32 = sc.reference(c, d, cols)["gate"].astype(np.float32)
        s32 = torch.nn.functional.silu(torch.from_numpy(g32)).numpy().astype(np.float64)
        silu = 4.0 * float(np.abs(s32 - ref.silu64(g32.astype(np.float64))).max())
    return silu, rsq


def _sel(c: sc.Case, vals: dict, M: int, tiles: np.ndarray, cols: np.ndarray) -> dict:
    """the evaluated columns of a call's outputs"""
    oc = cols[0::2] // 2 if c.mode == SK_SWIGLU else cols
    out = {"out": vals["out"][..., oc]}
    if c.mode == SK_RESID:
        out["xres"], out["ss_out"] = vals["xres"][:, cols], vals["ss_out"][tiles]
    return out


def _rows(r: dict, key: str, M: int) -> tuple:
    v, t = r[key], r[key + "_tol" if key != "ss_out" else "ss_tol"]
    if key == "ss_out" or v.ndim == 3:
        return v[:, :M], t[:, :M]
    return v[:M], t[:M]


def _bounded(c, got: dict, r: dict, M: int, what: str) -> float:
    worst = 0.0
    for k, g in got.items():
        want, tol = _rows(r, k, M)
        assert np.isfinite(g).all(), f"{c.id} {what}: {k} not finite"
        err = np.abs(g - want)
        ratio = float((err / np.maximum(tol, 1e-300)).max())
        i = np.unravel_index(int(np.argmax(err / np.maximum(tol, 1e-300))), err.shape)
        print(f"RATIO {c.fam} {c.id} {what} {k}: max err {err.max():.3e}, worst err / bound {ratio:.3f} (bound {tol[i]:.3e})")
        assert (err <= tol).all(), f"{c.id} {what}: {k} err {err[i]:.3e} > bound {tol[i]:.3e} at {i}"
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize("cid", sc.ids())
def test_bounded_parity_and_contracts(ctx, cid):
    c = sc.BY_ID[cid]
    d = sc.make_data(c, "real")
    dev = Dev(c, d)
    tiles = sc.ref_tiles(c)
    cols = sc.tile_cols(c, tiles)
    silu, rsq = _allowances(c, d, cols)
    print(f"ALLOW {cid}: silu {silu:.3e} rsqrt {rsq:.3e}")
    r = sc.reference(c, d, cols, silu_allow=silu, rsqrt_allow=rsq)
    res = {M: run(ctx, dev, M) for M in c.Ms}
    for M in c.Ms:
        _bounded(c, _sel(c, _values(c, res[M]), M, tiles, cols), r, M, f"M={M}")
    top = max(c.Ms)
    assert _same(res[top], run(ctx, dev, top)), f"{cid}: two launches differ"
    if c.fam == "h":
        for M in (min(c.Ms), top):
            assert _same(res[M], run(ctx, dev, M, w_frag=1)), f"{cid}: fragment-order weights differ from row-major at M = {M}"
    # a row's result does not depend on the other rows of the call
    for M in c.Ms:
        if c.fam == "h" or c.ksplit(M) == c.ksplit(top):
            assert _same(res[top], res[M], slice(0, M)), f"{cid}: rows of the M = {M} call differ from the same rows of the M = {top} call"
    low = [M for M in c.Ms if M <= 16]
    for M in low:              # (packed: the calls of at most 16 rows agree among themselves whatever the calls above 16 do)
        assert _same(res[low[-1]], res[M], slice(0, M)), f"{cid}: rows of the M = {M} call differ from the same rows of the M = {low[-1]} call"
    last = run(ctx, dev, 1, r0=top - 1)
    if c.fam == "h" or c.ksplit(1) == c.ksplit(top):
        assert _same(res[top], last, slice(top - 1, top)), f"{cid}: row {top - 1} alone differs from the M = {top} call"
    else:     # the split of K follows the rows of the call unless the caller passes its capacity: then every M agrees bit for bit
        assert c.fam == "q" and (top > 16) != (min(c.Ms) > 16)
        cap = {M: run(ctx, dev, M, M_cap=top) for M in c.Ms}
        for M in c.Ms:
            assert _same(cap[top], cap[M], slice(0, M)), f"{cid}: with M_cap = {top}, rows of the M = {M} call differ from the M = {top} call"
        assert _same(cap[top], res[top])
        assert _same(cap[top], run(ctx, dev, 1, r0=top - 1, M_cap=top), slice(top - 1, top))


@pytest.mark.parametrize("cid", sc.ids(pred=lambda c: not c.carry and c.mode != SK_SWIGLU))
def test_exact_integer_parity(ctx, cid):
    c = sc.BY_ID[cid]
    d = sc.make_data(c, "int")
    tiles = sc.ref_tiles(c)
    cols = sc.tile_cols(c, tiles)
    r = sc.reference(c, d, cols)
    assert r["peak"] < ref.EXACT_LIMIT, f"{cid}: an intermediate can reach {r['peak']:.0f} >= 2^24"
    dev = Dev(c, d)
    for M in {min(c.Ms), max(c.Ms)}:
        got = _sel(c, _values(c, run(ctx, dev, M)), M, tiles, cols)
        for k, g in got.items():
            want = _rows(r, k, M)[0]
            assert np.array_equal(g, want), f"{cid} M={M}: {k} differs from the integer reference at {int((g != want).sum())} of {g.size} elements"


# ---- producer -> consumer chain ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,dtype,bits", [("h", m._lib.BF16, 0), ("h", m._lib.F16, 0), ("q", m._lib.BF16, 4), ("q", m._lib.F16, 8)])
def test_chain_producer_feeds_consumer(ctx, fam, dtype, bits):
    """SK_RESID (down projection) -> SK_OUTF32 consumer fed the producer kernel's own out and ss_out, against float64
    RMSNorm + Linear of the updated residual.  The consumer's operand is the 16-bit x * gain * p (p = 1/8: the carried pre-scale), so the
    bound is: the consumer's own bound on that operand and the kernel's sums of squares, plus what the operand's rounding (half an ulp
    per element, through |W|) and the producer's fp32 bound move the result."""
    D, K1, N2, M = 256, 512, 40, 4
    eps, p = float(np.float32(1e-5)), 0.125
    prod = sc.Case(f"chain-prod-{fam}-{dtype}", fam, SK_RESID, D, K1, dtype=dtype, bits=bits, Ms=(M,), bias=True)
    cons = sc.Case(f"chain-cons-{fam}-{dtype}", fam, SK_OUTF32, N2, D, dtype=dtype, bits=bits, Ms=(M,), bias=True, carry=D // 16, rs_scale=1.0 / p)
    dp, dc = sc.make_data(prod, "real"), sc.make_data(cons, "real")
    gain = dp.nw.astype(np.float64)
    dp.nw = (dp.nw * np.float32(p)).astype(np.float32)
    rp = sc.reference(prod, dp)
    got_p = run(ctx, Dev(prod, dp), M)
    h16 = got_p["out"].view(np.float16) if dtype == m._lib.F16 else got_p["out"].view(np.uint16)
    dc.A16, dc.A = h16, ref.load16(h16, dtype)
    dc.ss_in, dc.ss_dim, dc.eps = got_p["ss_out"], D, eps
    silu, rsq = _allowances(cons, dc, None)
    rc = sc.reference(cons, dc, rsqrt_allow=rsq)
    got_c = run(ctx, Dev(cons, dc), M)["out"].astype(np.float64)
    assert (np.abs(got_c - rc["out"]) <= rc["out_tol"]).all()              # the consumer on the operands it was really given
    W = dc.W if fam == "h" else (dc.s64[:, :, None] * dc.q.reshape(N2, D // 64, 64) + dc.b64[:, :, None]).reshape(N2, D)
    want = ref.norm_linear_ref(rp["xres"], gain, W, eps) + dc.bias.astype(np.float64)[None]
    # consumer - bias = r_k (h16 W^T) with the kernel's r_k; want - bias = r (h W^T), h = x gain p.  The difference is
    # r_k ((h16 - h) W^T) + (r_k - r)(h W^T), and with the sums of squares within D of the exact sum X, r_k / r = (X' / X'_k)^(1/2) lies
    # within drel = (1 - D / X')^(-1/2) - 1 of 1 (X' = X + dim eps): no linearisation, nothing dropped
    rstd = 1.0 / np.sqrt((rp["xres"] ** 2).mean(-1) + eps) / p
    dh = rp["out_tol"]                                                     # |h16 - x gain p|: producer bound + half an ulp
    drel = (1.0 - rp["ss_tol"].sum(0) / (rp["ss_out"].sum(0) + D * eps)) ** -0.5 - 1.0
    tol = rc["out_tol"] + (rstd * (1.0 + drel))[:, None] * (dh @ np.abs(W).T) + drel[:, None] * np.abs(want - dc.bias[None])
    err = np.abs(got_c - want)
    print(f"RATIO {fam} chain-{fam}-{dtype}: worst err / bound {(err / tol).max():.3f}")
    assert (err <= tol).all()


# ---- error paths: refused on the host, nothing is launched -----------------------------------------------------------------------------
def _small(mode=SK_PARTIAL, fam="h", **kw):
    M, N, K = kw.pop("M", 2), kw.pop("N", 32), kw.pop("K", 256)
    i16 = lambda *s: torch.zeros(s, dtype=torch.int16, device="cuda")
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    # (operands of zeros, an output of sevens: any launch would change it)
    d = dict(A=i16(M, K), M=M, N=N, K=K, S=1, mode=mode, dtype=m._lib.BF16, out=(f32(M, N) if mode in (SK_PARTIAL, SK_OUTF32) else i16(M, N)) + 7)
    if fam == "h":
        d.update(W=i16(N, K))
    else:
        d.update(wfrag=torch.zeros(((N + 15) // 16) * (K // 128) * 256 * 2, dtype=torch.int32, device="cuda"), stfrag=f32(((N + 15) // 16) * (K // 128) * 64), bits=4)
    if mode == SK_RESID:
        d.update(xres=f32(M, N), nw=f32(N), ss_out=f32(N // 16 + 1, M))
    d.update(kw)
    return d


def _refused(ctx, **d):
    out = d["out"]
    before = None if out is None else out.clone()
    with pytest.raises(m.MiaError) as e:
        ops.skinny_gemm(ctx, **d)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, e.value
    assert before is None or torch.equal(out, before)
    ops.skinny_gemm(ctx, **_small())       # the context stays usable


@pytest.mark.parametrize("fam", ["h", "q"])
def test_rejects_bad_shapes(ctx, fam):
    unit = 32 if fam == "h" else 128
    _refused(ctx, **_small(fam=fam, K=unit * 3, S=2))                                     # K not a multiple of unit * S
    _refused(ctx, **_small(fam=fam, K=256 + unit // 2))
    a = torch.zeros((2, 260), dtype=torch.int16, device="cuda")
    _refused(ctx, **_small(fam=fam, A=a[:, :256]))                                        # lda % 8
    _refused(ctx, **_small(fam=fam, lda=128))                                             # lda < K
    _refused(ctx, **_small(SK_SWIGLU, fam, N=30))                                         # SK_SWIGLU with N % 4
    _refused(ctx, **_small(SK_RESID, fam, S=2, K=512))
    _refused(ctx, **_small(SK_RESID, fam, N=40))
    for missing in ("xres", "nw", "ss_out"):
        _refused(ctx, **_small(SK_RESID, fam, **{missing: None}))
    ss = torch.ones((513, 2), dtype=torch.float32, device="cuda")
    _refused(ctx, **_small(fam=fam, ss_in=ss, ss_tiles=0, ss_dim=16))
    _refused(ctx, **_small(fam=fam, ss_in=ss, ss_tiles=513, ss_dim=16))
    for mode in (0, 3, 6):                                                                # SK_OUT16, SK_QKV, unknown
        _refused(ctx, **_small(fam=fam, mode=mode))
    for null in ("A", "out") + (("W",) if fam == "h" else ("stfrag",)):
        _refused(ctx, **_small(fam=fam, **{null: None}))
    o = torch.ones((2, 32), dtype=torch.float32, device="cuda")
    _refused(ctx, **_small(SK_OUTF32, fam, out=o, ldo=31))                                # ldo < N
    _refused(ctx, **_small(SK_SWIGLU, fam, ldo=15))
    _refused(ctx, **_small(fam=fam, M=0))
    _refused(ctx, **_small(SK_OUTF32, fam, S=2, K=512))                                   # only SK_PARTIAL splits K over workgroups


@pytest.mark.parametrize("fam", ["h", "q"])
def test_launchers_refuse_non_positive_sizes_and_4_gib_operands(ctx, fam):
    """the hook leaves these to the launchers' own checks; nothing is launched, so the small buffers are never addressed"""
    for name in ("M", "N", "K", "S"):
        for v in (0, -1):
            d = _small(fam=fam)
            d[name] = v
            _refused(ctx, **d)
    # a 262144 x 8192 head is exactly 4 GiB at 16 bit; 524288 x 8192 is 4 GiB of 8-bit codes
    d = _small(SK_OUTF32, fam)
    d.update(A=torch.zeros((2, 8192), dtype=torch.int16, device="cuda"), K=8192)
    if fam == "h":
        d.update(N=262144, ldo=262144)
        _refused(ctx, **d)
        _refused(ctx, **dict(d, w_frag=1))
        _refused(ctx, **dict(_small(fam="h"), lda=1 << 30))             # M * lda * 2 bytes = 4 GiB of activations
    else:
        d.update(N=524288, ldo=524288, bits=8)
        _refused(ctx, **d)


def test_rejects_bits_3_and_missing_packed_arrays(ctx):
    _refused(ctx, **_small(fam="q", bits=3))
    d = _small(fam="q")
    d.pop("wfrag")
    _refused(ctx, **d)                                                                    # neither W nor wfrag
