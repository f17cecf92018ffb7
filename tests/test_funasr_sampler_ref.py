"""Pins tests/_funasr_sampler_ref.py (the CPU restatement of Fun-ASR's temperature > 0 sampler) on hand-worked rows: the reference's own
arithmetic written out literally for a row without ties (STT/FunASR/FunASRModel.swift:165-198), the tie rule, the clamp of n, top_k = 0
meaning 50, and a row shorter than k.  No GPU."""
import numpy as np

import _funasr_sampler_ref as F


def _softmax(v):
    e = np.exp(v - v.max())
    return e / e.sum()


def _swift_literal(logits, temperature, top_p, top_k):
    """sampleNextToken's second branch line by line, in float64: returns (finalIndices, categorical weights probs + 1e-10)."""
    last = np.asarray(logits, np.float64) / temperature
    eff = top_k if top_k > 0 else 50
    topk_idx = np.argpartition(-last, eff - 1)[:eff]
    topk_logits = last[topk_idx]
    final_logits, final_idx = topk_logits, topk_idx
    if top_p < 1.0:
        probs = _softmax(topk_logits)
        sorted_idx = np.argsort(-probs)
        cums = np.cumsum(probs[sorted_idx])
        n_tokens = max(1, int((cums < top_p).sum()) + 1)
        sel = sorted_idx[:n_tokens]
        final_idx = topk_idx[sel]
        final_logits = last[final_idx]
    return final_idx, _softmax(final_logits) + 1e-10


def test_reference_arithmetic_on_a_row_without_ties():
    rng = np.random.default_rng(0)
    x = rng.permutation(np.linspace(-4.0, 6.0, 400)).astype(np.float32)        # 400 distinct values
    for temperature, top_p, top_k in [(0.7, 0.9, 0), (1.3, 0.5, 7), (0.3, 0.95, 64)]:
        idx, w = _swift_literal(x, float(np.float32(temperature)), float(np.float32(top_p)), top_k)
        d = F.sample(x, 0.4, temperature, top_p, top_k)
        assert d.kept == idx.tolist()                                          # argSort(-probs) order = value descending
        np.testing.assert_allclose(np.diff(np.concatenate([[0.0], d.cw])), w, rtol=1e-12)
        cdf = np.cumsum(w)
        assert d.pick == int(idx[np.flatnonzero(cdf > np.float32(0.4) * cdf[-1])[0]])
    # top_p >= 1: the reference's set (argPartition leaves its order open; here it is value descending)
    idx, w = _swift_literal(x, 0.5, 1.0, 9)
    d = F.sample(x, 0.99, 0.5, 1.0, 9)
    assert sorted(d.kept) == sorted(idx.tolist()) and d.kept == np.argsort(-x.astype(np.float64))[:9].tolist()
    np.testing.assert_allclose(np.sort(np.diff(np.concatenate([[0.0], d.cw]))), np.sort(w), rtol=1e-12)


def test_hand_worked_row():
    # logits ln 8, ln 4, ln 2, ln 1, ln 1 at T = 1: p = 8/16, 4/16, 2/16, 1/16, 1/16 over k = 5
    x = np.log(np.array([1, 8, 2, 1, 4], np.float64)).astype(np.float32)
    d = F.sample(x, 0.0, 1.0, 0.8, 5)
    assert d.kept == [1, 4, 2] and d.k == 5                  # cumsum 0.5, 0.75 < 0.8; 0.875 crosses: n = 3
    np.testing.assert_allclose(d.cum, [0.5, 0.75, 0.875, 0.9375, 1.0], rtol=1e-6)
    np.testing.assert_allclose(d.cw, np.cumsum(np.array([8, 4, 2]) / 14 + 1e-10), rtol=1e-6)
    assert [F.sample(x, u, 1.0, 0.8, 5).pick for u in (0.0, 0.5, 0.58, 0.85, 0.86, 0.999)] == [1, 1, 4, 4, 2, 2]     # edges at 8/14, 12/14
    assert F.sample(x, 0.999, 1.0, 0.8, 1).kept == [1]       # top_k = 1: the argmax whatever u
    d_p, d_u = F.boundary_distance(x, 0.5, 1.0, 0.8, 5)
    assert abs(d_p - 0.05) < 1e-6 and abs(d_u - (8 / 14 - 0.5)) < 1e-6


def test_ties_go_to_the_lowest_index():
    x = np.array([1, 3, 2, 3, 2, 2, 0, 2], np.float32)
    assert F.kept_order(x, 4).tolist() == [1, 3, 2, 4]        # two 3s, then the lowest two of the four 2s
    assert F.kept_order(x, 6).tolist() == [1, 3, 2, 4, 5, 7]
    assert F.kept_order(np.full(9, 0.5, np.float32), 3).tolist() == [0, 1, 2]
    z = np.array([-0.0, 0.0, -1.0, 0.0], np.float32)          # -0 and +0 are one value
    assert F.kept_order(z, 3).tolist() == [0, 1, 3]
    y = np.array([np.nan, -np.inf, 2.0, np.nan, np.inf, -np.inf], np.float32)
    assert F.kept_order(y, 6).tolist() == [4, 2, 1, 5, 0, 3]  # NaN below -inf, lowest index first
    d = F.sample(y, 0.7, 1.0, 1.0, 6)
    assert d.pick == 4 and d.kept == [4, 2, 1, 5, 0, 3]       # +inf is the maximum: e = 1 there, 0 elsewhere (w = 1e-10 each)
    assert F.sample(y, 0.7, 1.0, 1.0, 2).kept == [4, 2]
    nan = F.sample(np.full(7, np.nan, np.float32), 0.3, 1.0, 0.9, 3)
    assert nan.pick == 0 and nan.kept == [0, 1, 2]


def test_n_is_clamped_to_k():
    # top_p one ulp below 1: three cumulative values lie below it, and the last one (1 up to rounding) may or may not -- the count is
    # 3 or 4, and n is 4 = k either way, never the reference's out-of-range k + 1
    x = np.array([0.3, 0.1, 0.2, 0.0], np.float32)
    p = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    d = F.sample(x, 0.5, 1.0, p, 4)
    assert d.cum.size == 4 and int((d.cum < p).sum()) in (3, 4) and d.kept == [0, 2, 1, 3]
    assert F.sample(x, 0.5, 1.0, p, 2).kept == [0, 2]
    tiny = F.sample(x, 0.5, 1.0, 1e-6, 4)
    assert tiny.kept == [0]                                    # count 0 -> n = 1


def test_top_k_zero_means_fifty_and_short_rows():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(300).astype(np.float32)
    assert F.effective_k(0, 300) == 50 and F.sample(x, 0.2, 1.0, 1.0, 0).kept == np.argsort(-x, kind="stable")[:50].tolist()
    short = x[:33]
    d = F.sample(short, 0.2, 1.0, 1.0, 0)
    assert d.k == 33 and d.kept == np.argsort(-short, kind="stable").tolist()     # V < k: the whole row, sorted
    one = F.sample(x[:1], 0.9, 0.5, 0.5, 0)
    assert one.pick == 0 and one.kept == [0] and one.k == 1
