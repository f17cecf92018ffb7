"""CPU pins of the float64 references behind tests/test_f32_ops_gpu.py, and the proof that those GPU comparisons can fail.

 * tap_gemm_ref against torch's conv1d and conv_transpose1d, attention_ref against scaled_dot_product_attention: float64 on both sides,
   bounded at the float64 level -- 256 ulp (2^-45) of the accumulated magnitude sum |x w| + |b| of each output (the two sides only
   differ in summation order, (K + 2) 2^-53 of it; 256 ulp leaves room for K up to a few hundred and nothing else).  For the transposed
   convolutions the per-phase weight layouts of codec_load.hip (convt_phases) and hift.hip (Loader::convt) are restated in
   _f32_ops_cases.py, so the phase decomposition itself is what torch checks.
 * the launch rule of codec_conv_gemm_launch as the tests restate it, with its constants read from the source, selects the instantiation
   every tile case is meant for.
 * every case of every GPU family: a deliberately wrong reference (pad off by one, last tap dropped, rows past seq_len not zeroed, output
   phase shifted by one, out_scale applied after R2, last key masked, chunk boundary off by one, bias_v replaced by bias_u) leaves the
   case's own tolerance by more than 100 x on at least one element."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _f32_ops_cases as cases
import _f32_ops_ref as ref

ULP64 = 2.0 ** -53


def _magnitude(r: ref.TapGemm, K: int) -> np.ndarray:
    """sum |x w| + |b| per output, recovered from the plain case's bound (K + 2) 2^-24 (sum |x w| + |b|)."""
    return r.tol / ((K + 2) * ref.EPS32)


def _assert_f64(got, want, mag):
    err = np.abs(got - want)
    assert (err <= 256 * ULP64 * mag).all(), float((err / (ULP64 * np.maximum(mag, 1e-300))).max())


@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("dil", [1, 3, 9])
@pytest.mark.parametrize("pad", [0, 1, 4, 27])
def test_tap_gemm_ref_is_conv1d(stride, dil, pad):
    rng = np.random.default_rng(stride * 100 + dil * 10 + pad)
    T_in, Cin, N, taps = 61, 32, 5, 3
    T_out = (T_in + 2 * pad - dil * (taps - 1) - 1) // stride + 1
    x, w, b = rng.standard_normal((T_in, Cin)), rng.standard_normal((N, taps, Cin)), rng.standard_normal(N)
    r = ref.tap_gemm_ref(X=x, W=w.reshape(N, -1), bias=b, T_in=T_in, T_out=T_out, M=T_out, N=N, Cin=Cin, taps=taps, dil=dil, pad=pad, x_row_mul=stride)
    want = F.conv1d(torch.from_numpy(x.T[None]), torch.from_numpy(w.transpose(0, 2, 1).copy()), torch.from_numpy(b), stride=stride, padding=pad, dilation=dil)[0].T.numpy()
    assert r.written.all() and want.shape == r.Y.shape
    _assert_f64(r.Y, want, _magnitude(r, taps * Cin))


def _convt_torch(x, wm, b, s, p):
    # MLX weight [Cout][K][Cin] -> torch's [Cin][Cout][K]
    return F.conv_transpose1d(torch.from_numpy(x.T[None].astype(np.float64)), torch.from_numpy(wm.transpose(2, 0, 1).astype(np.float64).copy()),
                              torch.from_numpy(b.astype(np.float64)), stride=s, padding=p)[0].T.numpy()


@pytest.mark.parametrize("s", [2, 4, 8])
@pytest.mark.parametrize("T", [1, 2, 37])
def test_snac_phase_decomposition_is_conv_transpose1d(s, T):
    rng = np.random.default_rng(s * 100 + T)
    Cin, N = 32, 5
    x, wm, b = cases.f32(rng.standard_normal((T, Cin))), cases.f32(rng.standard_normal((N, 2 * s, Cin))), cases.f32(rng.standard_normal(N))
    d, T_out = cases.snac_convt_desc(x, wm, b, s, T)
    r = ref.tap_gemm_ref(s, **d)
    want = _convt_torch(x, wm, b, s, (s + 1) // 2)
    assert want.shape[0] == T_out and r.written[:T_out, :N].all() and not r.written[T_out:].any() and not r.written[:, N:].any()
    _assert_f64(r.Y[:T_out, :N], want, _magnitude(r, 2 * Cin)[:T_out, :N])


@pytest.mark.parametrize("s,K", [(8, 16), (5, 11), (3, 7), (4, 10), (2, 6)])
@pytest.mark.parametrize("T,shift", [(1, 0), (2, 0), (37, 0), (37, 1)])
def test_hift_phase_decomposition_is_conv_transpose1d(s, K, T, shift):
    rng = np.random.default_rng(s * 1000 + K * 10 + T + shift)
    Cin, N = 32, 5
    x, wm, b = cases.f32(rng.standard_normal((T, Cin))), cases.f32(rng.standard_normal((N, K, Cin))), cases.f32(rng.standard_normal(N))
    d, T_out = cases.hift_convt_desc(x, wm, b, s, T, shift)
    d["Y"] = d["Y"][shift:]
    r = ref.tap_gemm_ref(s, **d)
    want = _convt_torch(x, wm, b, s, (K - s) // 2)
    assert want.shape[0] == T * s and T_out == T * s - shift and r.written[:T_out, :N].all() and not r.written[T_out:].any()
    nt = (K + s - 1) // s
    _assert_f64(r.Y[:T_out, :N], want[:T_out], _magnitude(r, nt * Cin)[:T_out, :N])


def _sdpa(c: cases.AttnCase, mask=None):
    q, k, v = (torch.from_numpy(a.astype(np.float64).reshape(c.B, c.T, c.H, 64).transpose(0, 2, 1, 3).copy()) for a in c.parts())
    o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, scale=c.scale)
    return o.numpy().transpose(0, 2, 1, 3).reshape(c.B * c.T, c.H * 64)


def test_attention_ref_is_sdpa():
    for cid in ("attn-T33-B2H3", "attn-T129-B1H1"):
        c = cases.attn_case("attn-plain", cid)
        assert np.abs(cases.attn_reference("attn-plain", cid)[0] - _sdpa(c)).max() <= 256 * ULP64 * np.abs(c.parts()[2]).max()


@pytest.mark.parametrize("cid", ["attn-chunk7", "attn-chunk50", "attn-seqlen", "attn-seqlen-chunk32"])
def test_attention_ref_is_sdpa_under_an_explicit_mask(cid):
    c = cases.attn_case("attn-ex", cid)
    i, j = np.arange(c.T)[:, None], np.arange(c.T)[None, :]
    mask = np.ones((c.B, 1, c.T, c.T), bool)
    if c.chunk:
        mask &= (j < (i // c.chunk + 1) * c.chunk)[None, None]
    if c.seq_len is not None:
        mask &= j[None, None] < np.asarray(c.seq_len)[:, None, None, None]
    got, want = cases.attn_reference("attn-ex", cid)[0], _sdpa(c, torch.from_numpy(mask))
    valid = c.valid_rows()
    assert np.abs(got - want)[valid].max() <= 256 * ULP64 * np.abs(c.parts()[2][valid]).max()


def test_tile_cases_select_their_instantiation():
    seen = set()
    for c in cases.family("tiles"):
        d = c.d
        assert cases.instantiation(d["M"], d["N"], d["taps"] * d["Cin"]) == c.expect, c.id
        seen.add(c.expect)
        if d["M"] > 1:
            assert d["M"] % 64 == 1 and (d["N"] % 32 == 1 or c.id == "tile-111-wg330"), c.id
        assert d["X"].shape[1] == d["Cin"] + 4 and d["Y"].shape[1] == d["N"] + 3
    assert seen == {"<1,1,4>", "<1,1,1>", "<2,2,1>", "<2,1,1>"}
    # every other family stays on the 64 x 64 tiles
    for fam in ("geometry", "activations", "rowmap", "epilogue", "stacked"):
        for c in cases.family(fam):
            assert cases.instantiation(c.d["M"], c.d["N"], c.d["taps"] * c.d["Cin"], c.phases * c.d.get("n_seq", 1)) in ("<1,1,4>", "<1,1,1>"), c.id


def test_geometry_cases_meet_the_ends_of_x():
    for c in cases.family("geometry"):
        d = c.d
        first = -d["pad"]
        last = (d["M"] - 1) * d["x_row_mul"] + (d["taps"] - 1) * d["dil"] - d["pad"]
        assert first < 0, c.id
        if c.id.endswith("last-in"):
            assert last == d["T_in"] - 1
        elif c.id.endswith("last-at"):
            assert last == d["T_in"]
        elif c.id.endswith("last-past"):
            assert last > d["T_in"]
        else:
            assert (d["taps"] - 1) * d["dil"] - d["pad"] < 0       # row 0's last tap is still before row 0


def test_activation_cases_span_both_signs_up_to_ten():
    for c in cases.family("activations"):
        r = cases.reference("activations", c.id)
        pre = r.pre[r.written]
        assert pre.min() < -8 and pre.max() > 8, (c.id, pre.min(), pre.max())


def test_snake_cases_reach_large_arguments():
    c = cases.case("epilogue", "snake-default")
    ax = np.abs(c.d["alpha"][None] * c.d["X"][:, :c.d["Cin"]])
    assert c.d["alpha"].min() <= 0.05001 and c.d["alpha"].max() >= 19.99 and 200 < ax.max() < 1000


def _visible(right: ref.TapGemm, wrong: ref.TapGemm) -> float:
    """Largest |wrong - right| / tolerance over the elements either of them writes (an element only one writes is compared with the sentinel
    the other leaves)."""
    where = right.written | wrong.written
    diff = np.abs(wrong.Y - right.Y)[where]
    tol = np.maximum(right.tol, wrong.tol)[where]
    return float((diff / np.maximum(tol, 1e-30)).max())


@pytest.mark.parametrize("fam", list(cases.FAMILIES))
def test_tap_gemm_cases_can_fail(fam):
    used = set()
    for c in cases.family(fam):
        right = cases.reference(fam, c.id)
        assert right.written.any() and np.isfinite(right.Y).all()
        for w in c.wrongs:
            assert _visible(right, cases.mutate(c, w)) > 100, (c.id, w)
            used.add(w)
    need = {"tiles": {"pad", "tap"}, "geometry": {"pad", "tap"}, "activations": {"pad", "tap"}, "rowmap": {"phase", "tap", "pad"},
            "epilogue": {"pad", "tap", "order"}, "stacked": {"seq", "pad", "phase"}}[fam]
    assert need <= used


@pytest.mark.parametrize("fam", list(cases.ATTN_FAMILIES))
def test_attention_cases_can_fail(fam):
    used = set()
    for c in cases.attn_family(fam):
        r64, tol = cases.attn_reference(fam, c.id)
        valid = c.valid_rows()
        assert np.isfinite(r64[valid]).all() and tol > 0
        for w in c.wrongs:
            with np.errstate(invalid="ignore"):
                diff = np.abs(cases.attn_eval(c, wrong=w) - r64)[valid]
            assert np.nan_to_num(diff, nan=np.inf).max() > 100 * tol, (c.id, w)
            used.add(w)
    assert used >= {"attn-plain": {"last_key"}, "attn-ex": {"last_key", "chunk", "bias"}}[fam]


def test_onehot_case_puts_all_mass_on_one_key():
    c = cases.attn_case("attn-plain", "attn-onehot")
    q, k, v = (a.astype(np.float64) for a in c.parts())
    r64, tol = cases.attn_reference("attn-plain", "attn-onehot")
    for b in range(c.B):
        for h in range(c.H):
            cs, rs = slice(h * 64, h * 64 + 64), slice(b * c.T, (b + 1) * c.T)
            s = q[rs, cs] @ k[rs, cs].T * c.scale
            assert (s.argmax(axis=1) == c.one_hot[rs]).all() and s.max() > 150 and s.min() < -150
            top2 = np.sort(s, axis=1)[:, -2:]
            assert (top2[:, 1] - top2[:, 0]).min() > 60          # e^-60: every other key's mass is below any float32 rounding
    assert np.array_equal(r64.astype(np.float32), np.concatenate([v[b * c.T + c.one_hot[b * c.T:(b + 1) * c.T]] for b in range(c.B)]).astype(np.float32))
    assert tol < 1e-6
