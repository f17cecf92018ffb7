"""Operator-level parity of the packed skinny GEMM at 6 bits (csrc/skinny_quant.hip: the HB = 2 instantiation of skinny_gemm_qi) through the
mia_op_skinny_gemm hook: the comparisons of tests/test_skinny_gpu.py (whose runner, guards and comparison functions are used as they
are) on the cases of tests/_skinny6_cases.py.  The reference and its derived error bound are _skinny_ref's 8-bit ones on the unpacked
6-bit codes -- the kernel's arithmetic behind the unpack is the 8-bit kernel's -- and the restated dispatch is the 8-bit rule; no
tolerance is new.  Bounded parity on real operands, bit-exact parity on small integers, untouched memory around every output, and the
row-independence contracts."""
import numpy as np
import pytest

import _skinny6_cases as s6
import _skinny_cases as sc
import _skinny_ref as ref
import mlx_swift_audio_amd as m
import test_skinny_gpu as T
from _skinny_ref import SK_SWIGLU
from mlx_swift_audio_amd import ops

pytestmark = pytest.mark.gpu


def test_table_reaches_every_form():
    """every form of REQUIRED_Q (each exists with two planes), both compute types, the three scale types, both row variants"""
    forms = [dict(s6.as_8(c).form(M), dtype=c.dtype) for c in s6.CASES for M in c.Ms]
    for want in sc.REQUIRED_Q:
        assert any(all(f[k] == v for k, v in want.items()) for f in forms), f"no 6-bit case selects {want}"
    assert all(f["NP"] == 2 for f in forms)
    for M16 in (True, False):
        for dt in (m._lib.BF16, m._lib.F16):
            assert any(f["M16"] == M16 and f["dtype"] == dt for f in forms)
    assert {c.sdt for c in s6.CASES} == {"f16", "bf16", "f32"}
    assert {c.carry for c in s6.CASES if c.carry} == {1, 65}
    assert any(c.lda_extra for c in s6.CASES)


@pytest.mark.parametrize("cid", s6.ids())
def test_bounded_parity_and_contracts(ctx, cid):
    c = s6.BY_ID[cid]
    d = s6.make_data(c, "real")
    dev = T.Dev(c, d)
    tiles = sc.ref_tiles(c)
    cols = sc.tile_cols(c, tiles)
    silu, rsq = T._allowances(s6.as_8(c), d, cols)
    r = s6.reference(c, d, cols, silu_allow=silu, rsqrt_allow=rsq)
    res = {M: T.run(ctx, dev, M) for M in c.Ms}
    for M in c.Ms:
        T._bounded(c, T._sel(c, T._values(c, res[M]), M, tiles, cols), r, M, f"M={M}")
    top = max(c.Ms)
    assert T._same(res[top], T.run(ctx, dev, top)), f"{cid}: two launches differ"
    for M in c.Ms:             # a row's result does not depend on the other rows of the call, wherever both calls split K alike
        if c.ksplit(M) == c.ksplit(top):
            assert T._same(res[top], res[M], slice(0, M)), f"{cid}: rows of the M = {M} call differ from the same rows of the M = {top} call"
    low = [M for M in c.Ms if M <= 16]
    for M in low:
        assert T._same(res[low[-1]], res[M], slice(0, M)), f"{cid}: rows of the M = {M} call differ from the same rows of the M = {low[-1]} call"
    last = T.run(ctx, dev, 1, r0=top - 1)
    if c.ksplit(1) == c.ksplit(top):
        assert T._same(res[top], last, slice(top - 1, top)), f"{cid}: row {top - 1} alone differs from the M = {top} call"
    else:                      # with the capacity passed, every M splits K alike
        cap = {M: T.run(ctx, dev, M, M_cap=top) for M in c.Ms}
        for M in c.Ms:
            assert T._same(cap[top], cap[M], slice(0, M)), f"{cid}: with M_cap = {top}, rows of the M = {M} call differ from the M = {top} call"
        assert T._same(cap[top], res[top])
        assert T._same(cap[top], T.run(ctx, dev, 1, r0=top - 1, M_cap=top), slice(top - 1, top))


@pytest.mark.parametrize("cid", s6.ids(pred=lambda c: not c.carry and c.mode != SK_SWIGLU))
def test_exact_integer_parity(ctx, cid):
    c = s6.BY_ID[cid]
    d = s6.make_data(c, "int")
    tiles = sc.ref_tiles(c)
    cols = sc.tile_cols(c, tiles)
    r = s6.reference(c, d, cols)
    assert r["peak"] < ref.EXACT_LIMIT, f"{cid}: an intermediate can reach {r['peak']:.0f} >= 2^24"
    dev = T.Dev(c, d)
    for M in {min(c.Ms), max(c.Ms)}:
        got = T._sel(c, T._values(c, T.run(ctx, dev, M)), M, tiles, cols)
        for k, g in got.items():
            want = T._rows(r, k, M)[0]
            assert np.array_equal(g, want), f"{cid} M={M}: {k} differs from the integer reference at {int((g != want).sum())} of {g.size} elements"


def test_rejects_bits_5_7_and_4_gib_of_6_bit_codes(ctx):
    for bits in (3, 5, 7):
        T._refused(ctx, **T._small(fam="q", bits=bits))
    ops.skinny_gemm(ctx, **dict(T._small(fam="q", K=256), bits=6))                  # zeros in, zeros out: the width itself is accepted
    # 43691 tiles x 64 blocks x 1536 B is just above 4 GiB; nothing is launched, so the small buffers are never addressed
    import torch
    d = T._small(1, "q")
    d.update(A=torch.zeros((2, 8192), dtype=torch.int16, device="cuda"), K=8192, N=43691 * 16, ldo=43691 * 16, bits=6)
    T._refused(ctx, **d)
