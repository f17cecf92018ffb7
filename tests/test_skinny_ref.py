"""CPU checks of the skinny-GEMM references and case table (tests/_skinny_ref.py, tests/_skinny_cases.py) that tests/test_skinny_gpu.py
relies on: the references agree with independent torch float64 compositions, the derived bounds are reachable by honest fp32 arithmetic
in several summation orders (ratio below 1), every check can fail (deliberately wrong formulas leave the bound by a factor of at least
WIDE = 50 and differ exactly on the integer operands), and the case table reaches every kernel form the two launchers can select."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _skinny_cases as sc
import _skinny_ref as ref
from _skinny_ref import SK_OUTF32, SK_PARTIAL, SK_RESID, SK_SWIGLU
from mlx_swift_audio_amd import _lib

WIDE = 50.0
BF16, F16 = _lib.BF16, _lib.F16


def _case(fam, mode, N, K, S=1, dtype=BF16, bits=0, **kw):
    return sc.Case(f"cpu-{fam}-{mode}-{N}-{K}-{S}-{dtype}-{bits}-{kw.get('carry', 0)}", fam, mode, N, K, S, dtype=dtype, bits=bits, Ms=(5,), **kw)


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _dequant_torch(d: sc.Data, bits: int) -> torch.Tensor:
    """MLX affine de-quantisation written independently of _skinny_ref.unpack_codes: shifts on int64 tensors"""
    w = torch.from_numpy(d.codes.astype(np.int64))
    per = 32 // bits
    q = torch.stack([(w >> (bits * j)) & ((1 << bits) - 1) for j in range(per)], dim=-1).reshape(w.shape[0], -1).to(torch.float64)
    s, b = _t(d.s64).repeat_interleave(64, dim=1), _t(d.b64).repeat_interleave(64, dim=1)
    return s * q + b


# ---- the references against torch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_outf32_and_partial_are_matmul(dtype):
    c = _case("h", SK_OUTF32, 37, 224, dtype=dtype)
    d = sc.make_data(c, "real")
    r = sc.reference(c, d)
    want = _t(d.A) @ _t(d.W).T + _t(d.bias)[None]
    assert np.abs(r["out"] - want.numpy()).max() < 1e-12
    assert np.array_equal(ref.load16(d.A16, dtype), d.A) and np.array_equal(ref.round16(d.A, dtype), d.A)      # operands are 16-bit values
    c = _case("h", SK_PARTIAL, 22, 384, 3, dtype=dtype)
    d = sc.make_data(c, "real")
    r = sc.reference(c, d)
    for s in range(3):
        want = _t(d.A[:, 128 * s:128 * (s + 1)]) @ _t(d.W[:, 128 * s:128 * (s + 1)]).T
        assert np.abs(r["out"][s] - want.numpy()).max() < 1e-12
    assert np.abs(r["out"].sum(0) - (_t(d.A) @ _t(d.W).T).numpy()).max() < 1e-12


def test_swiglu_is_silu_gate_times_up():
    c = _case("h", SK_SWIGLU, 36, 256)
    d = sc.make_data(c, "real")
    r = sc.reference(c, d)
    v = _t(d.A) @ _t(d.W).T + _t(d.bias)[None]
    want = F.silu(v[:, 0::2]) * v[:, 1::2]
    assert r["out_f64"].shape == (5, 18) and np.abs(r["out_f64"] - want.numpy()).max() < 1e-12
    assert np.array_equal(r["out"], ref.round16(r["out_f64"], BF16))


def test_resid_and_consumer_are_rmsnorm_then_linear():
    D, K1, N2 = 64, 128, 24
    prod = _case("h", SK_RESID, D, K1)
    dp = sc.make_data(prod, "real")
    rp = sc.reference(prod, dp)
    x = _t(dp.xres) + _t(dp.A) @ _t(dp.W).T + _t(dp.bias)[None]
    assert np.abs(rp["xres"] - x.numpy()).max() < 1e-12
    assert np.abs(rp["ss_out"] - (x * x).reshape(5, D // 16, 16).sum(-1).T.numpy()).max() < 1e-10
    assert np.array_equal(rp["out"], ref.round16((x * _t(dp.nw)[None]).numpy(), BF16))
    # the consumer on the exact (unrounded) operand x * gain and the exact tile sums is RMSNorm then Linear
    cons = _case("h", SK_OUTF32, N2, D, carry=D // 16, rs_scale=4.0)
    dc = sc.make_data(cons, "real")
    dc.A, dc.ss_in, dc.ss_dim, dc.eps = (x * _t(dp.nw)[None] * 0.25).numpy(), rp["ss_out"], D, float(np.float32(1e-5))
    rc = sc.reference(cons, dc)
    h = x / torch.sqrt((x * x).mean(-1, keepdim=True) + dc.eps) * _t(dp.nw)[None]
    want = h @ _t(dc.W).T + _t(dc.bias)[None]
    assert np.abs(rc["out"] - want.numpy()).max() < 1e-10
    assert np.abs(ref.norm_linear_ref(x.numpy(), dp.nw, dc.W, dc.eps) + dc.bias[None] - want.numpy()).max() < 1e-10


@pytest.mark.parametrize("bits,sdt", [(4, "f16"), (8, "bf16"), (8, "f32")])
def test_packed_is_dequantize_then_matmul(bits, sdt):
    c = _case("q", SK_OUTF32, 21, 256, bits=bits, sdt=sdt)
    for kind in ("real", "int"):
        d = sc.make_data(c, kind)
        r = sc.reference(c, d)
        want = _t(d.A) @ _dequant_torch(d, bits).T + _t(d.bias)[None]
        assert np.abs(r["out"] - want.numpy()).max() < 1e-9 * max(1.0, float(want.abs().max()))


# ---- the bounds are reachable by honest fp32 arithmetic ----------------------------------------------------------------------------------
def _sum32(terms: np.ndarray, order: str) -> np.ndarray:
    """fp32 sum over the last axis of exact fp32 terms in a given order"""
    t = terms.astype(np.float32)
    if order == "pairwise":
        return t.sum(-1, dtype=np.float32)
    if order == "reverse":
        t = t[..., ::-1]
    if order == "waves4":          # four K slices summed on their own, then added in wave order
        parts = [_sum32(p, "forward") for p in np.split(t, 4, axis=-1)]
        out = parts[0]
        for p in parts[1:]:
            out = (out + p).astype(np.float32)
        return out
    out = np.zeros(t.shape[:-1], np.float32)
    for k in range(t.shape[-1]):
        out = (out + t[..., k]).astype(np.float32)
    return out


@pytest.mark.parametrize("order", ["forward", "reverse", "pairwise", "waves4"])
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_bound_16bit_holds_for_fp32_in_any_order(order, dtype):
    c = _case("h", SK_OUTF32, 24, 512, dtype=dtype)
    d = sc.make_data(c, "real")
    r = sc.reference(c, d)
    prod = d.A[:, None, :] * d.W[None, :, :]
    assert np.array_equal(prod.astype(np.float32).astype(np.float64), prod)       # products of 16-bit values are exact in fp32
    got = (_sum32(prod, order) + d.bias[None]).astype(np.float32)
    ratio = (np.abs(got - r["out"]) / r["out_tol"]).max()
    assert 0 < ratio < 1, ratio


def _fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


@pytest.mark.parametrize("order", ["forward", "reverse", "pairwise"])
@pytest.mark.parametrize("bits,dtype", [(4, BF16), (4, F16), (8, BF16), (8, F16)])
def test_bound_packed_holds_for_the_offset_trick_in_fp32(order, bits, dtype):
    """the kernel's arithmetic in numpy: per group P = sum (MAG + q) a per nibble plane, A = sum a, P = fma(16, P_hi, P_lo),
    y = fma(s, P, fma(t, A, y)), t = fl32(b - MAG s (x 17))"""
    c = _case("q", SK_OUTF32, 20, 512, dtype=dtype, bits=bits, bias=False)
    d = sc.make_data(c, "real")
    r = sc.reference(c, d)
    mag = ref.mag_of(dtype)
    G = c.K // 64
    a3 = d.A.reshape(5, 1, G, 64)
    q3 = d.q.reshape(c.N, G, 64).astype(np.float64)[None]
    t = ref.t_offset(d.s64, d.b64, bits, dtype)
    Asum = _sum32(np.broadcast_to(a3, (5, 1, G, 64)), order)[:, 0]
    planes = [q3 % 16, q3 // 16] if bits == 8 else [q3]
    P = [_sum32((mag + p) * a3, order) for p in planes]
    Pg = _fma32(16.0, P[1], P[0]) if bits == 8 else P[0]
    y = np.zeros((5, c.N), np.float32)
    for g in (range(G) if order != "reverse" else range(G - 1, -1, -1)):
        y = _fma32(d.s64[None, :, g], Pg[:, :, g], _fma32(t[None, :, g], Asum[:, None, g], y))
    ratio = (np.abs(y - r["out"]) / r["out_tol"]).max()
    assert 0 < ratio < 1, ratio


# ---- every check can fail ----------------------------------------------------------------------------------------------------------------
def _margin(good: dict, bad: dict, key="out", tol="out_tol") -> float:
    return float((np.abs(bad[key] - good[key]) / good[tol]).max())


WRONG = [   # wrong formula, case, the output it shows in
    ("k-slice-shift", _case("h", SK_PARTIAL, 20, 256, 2), "out"),
    ("k-slice-shift", _case("q", SK_PARTIAL, 20, 512, 2, bits=4), "out"),
    ("gate-up-swapped", _case("h", SK_SWIGLU, 20, 128), "out"),
    ("rstd-after-bias", _case("h", SK_OUTF32, 20, 128, carry=8, rs_scale=0.125), "out"),
    ("no-rs-scale", _case("h", SK_PARTIAL, 20, 128, carry=8, rs_scale=0.125), "out"),
    ("eps-outside", _case("q", SK_OUTF32, 20, 128, bits=4, carry=8, rs_scale=0.125), "out"),
    ("no-hi-weight", _case("q", SK_OUTF32, 20, 128, bits=8, dtype=F16), "out"),
    ("wrong-mag", _case("q", SK_OUTF32, 20, 128, bits=4), "out"),
    ("wrong-mag", _case("q", SK_OUTF32, 20, 128, bits=8, dtype=F16), "out"),
    ("ss-tile-shift", _case("h", SK_RESID, 48, 128), "ss_out"),
]


@pytest.mark.parametrize("wrong,c,key", WRONG, ids=[f"{w}-{c.fam}{c.bits}" for w, c, _ in WRONG])
def test_a_wrong_formula_leaves_the_bound(wrong, c, key):
    d = sc.make_data(c, "real")
    if wrong == "eps-outside":
        d.ss_in, d.eps = d.ss_in * np.float32(1e-3), 1e-2          # a residual small enough for eps to matter
    good, bad = sc.reference(c, d), sc.reference(c, d, wrong=wrong)
    m = _margin(good, bad, key, "ss_tol" if key == "ss_out" else "out_tol")
    assert m > WIDE, f"{wrong}: the wrong formula moves the result by only {m:.1f} bounds"
    if not c.carry and c.mode != SK_SWIGLU:                        # the exact cases tell the two apart as well
        di = sc.make_data(c, "int")
        gi, bi = sc.reference(c, di), sc.reference(c, di, wrong=wrong)
        assert gi["peak"] < ref.EXACT_LIMIT and not np.array_equal(gi[key], bi[key])


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
def test_every_form_is_selected():
    forms16 = {(f["kernel"], f["tail"], f["nb"]) for c in sc.CASES if c.fam == "h" for M in c.Ms for f in [c.form(M)]}
    for kernel, tail, nb in sc.REQUIRED_16:
        assert any(k == kernel and t == tail and (nb is None or n == nb) for k, t, n in forms16), f"no case selects {kernel} tail {tail} nb {nb}"
    formsq = [dict(c.form(M), bits=c.bits, dtype=c.dtype) for c in sc.CASES if c.fam == "q" for M in c.Ms]
    for want in sc.REQUIRED_Q:
        for bits, dtype in ((4, BF16), (8, F16)) if not want.get("head41") and not (want.get("nt4") and want.get("M16")) else ((4, BF16),):
            assert any(all(f[k] == v for k, v in want.items()) and f["bits"] == bits and f["dtype"] == dtype for f in formsq), f"no case selects {want} at {bits} bit"
    for M16 in (True, False):
        for NP in (1, 2):
            assert any(f["M16"] == M16 and f["NP"] == NP for f in formsq)
    # both families: every listed row count on one shape per mode, a view with lda > K, the carried norm at 1, 64, 65 and 512 tiles
    for fam in ("h", "q"):
        for mode in (SK_OUTF32, SK_PARTIAL, SK_RESID) if fam == "h" else (SK_PARTIAL, SK_RESID):
            assert any(c.fam == fam and c.mode == mode and c.Ms == sc.ALL_M for c in sc.CASES), (fam, mode)
        assert any(c.fam == fam and c.lda_extra for c in sc.CASES)
        assert {c.carry for c in sc.CASES if c.fam == fam and c.carry} >= {1, 64, 65, 512}
    assert {c.sdt for c in sc.CASES if c.fam == "q"} == {"f16", "bf16", "f32"}


def test_model_tuples_keep_their_form_when_cut():
    """the real models' (N, K, S, mode) run at an N cut to a few tiles only where both sides of the 16 / 17 boundary keep the full form"""
    n = 0
    for name in sc.MODELS:
        for fam in ("h", "q"):
            for role, mode, N, K, S, carry in sc.model_tuples(name, fam):
                cut = min(N, 48) if mode == SK_RESID else sc.cut_N(fam, mode, N, K, S, 4)
                full = sc.Case("full", fam, mode, N, K, S, bits=4 if fam == "q" else 0)
                small = sc.Case("cut", fam, mode, cut, K, S, bits=4 if fam == "q" else 0)
                if not (fam == "q" and mode == SK_OUTF32):
                    assert all(full.form(M) == small.form(M) for M in (1, 16, 17, 32)), (name, role)
                assert any(c.fam == fam and c.mode == mode and c.N == cut and c.K == K and c.S == S and c.carry == carry for c in sc.CASES), (name, fam, role)
                n += 1
    assert n == 80
    assert sc.pick_split(896, 4, 32) == 4 and sc.pick_split(896, 4, 128) == 1 and sc.pick_split(4864, 8, 128) == 2 and sc.pick_split(8192, 8, 32) == 8


def test_packed_forms_that_depend_on_the_rows_follow_the_capacity():
    """where the packed split of K differs across the 16 / 17 boundary (Qwen3-0.6B q|k|v, the wide vocabulary heads), a capacity passed
    as M_cap makes the form the same for every row count"""
    differing = [c for c in sc.CASES if c.fam == "q" and c.ksplit(1) != c.ksplit(17)]
    assert any("qwen3-0.6b-qkv" in c.id for c in differing) and any("head41" in c.id and c.K == 512 for c in differing)
    for c in differing:
        assert len({c.ksplit(M, 32) for M in (1, 4, 16, 17, 32)}) == 1, c.id
    for c in sc.CASES:
        if c.fam == "h":
            assert len({c.ksplit(M) for M in sc.ALL_M}) == 1, c.id
