"""GPU parity of Fun-ASR's temperature > 0 sampler at operator level (mia_sample_top_k_top_p: radix-select top-k over the vocabulary
slices, nucleus cut, inverse-CDF draw) against the CPU restatement tests/_funasr_sampler_ref.py.

The kept set and its order are integer-exact: no tolerance.  The nucleus size and the pick are exact under the project's boundary rule
(tests/test_lm_gpu.py): a case counts only if every cumulative probability is >= 1e-4 from top_p and u * sum(w) is >= 1e-4 (of sum(w))
from the edges of its interval -- and the seeds below were chosen on the CPU so that EVERY case counts; the test asserts that on the
restatement alone before it looks at the GPU."""
import functools

import numpy as np
import pytest

import _funasr_sampler_ref as F

pytestmark = pytest.mark.gpu

V_QWEN3 = 151936
SIZES = [1, 33, 49, 50, 51, 3000, V_QWEN3]          # 33: 32 slices of 2, most of them empty; 49 / 50 / 51 around the default k; 3000: slices of 94
KS = [1, 2, 50, 64, 65, 1024]


def _kept(ctx, x, top_k, temperature=1.0, top_p=1.0, u=0.5):
    from mlx_swift_audio_amd import lm as HL
    return HL.sample_top_k_top_p(ctx, x, u, temperature, top_p, top_k, want_kept=True)


@functools.lru_cache(maxsize=None)
def _rows(V):
    """Two rows per size, shared and never written to: continuous values, and values rounded to 1/8 (ties at every rank, the k-th included)."""
    rng = np.random.default_rng(V)
    a = (rng.standard_normal(V) * 3).astype(np.float32)
    b = (np.round(rng.standard_normal(V) * 8) / 8).astype(np.float32)
    for r in (a, b):
        r.setflags(write=False)
    return a, b


@pytest.mark.parametrize("V", SIZES)
def test_kept_set_and_order_are_exact(ctx, V):
    for x in _rows(V):
        for k in KS + [0]:
            pick, kept = _kept(ctx, x, k)
            ref = F.sample(x, 0.5, 1.0, 1.0, k)
            assert len(ref.kept) == min(k or 50, V)
            assert kept == ref.kept, (V, k)
            assert pick in kept


def test_engineered_ties_straddle_the_cut(ctx):
    """V = 3000: slices of 94.  Seven larger values, then the k-th value five times: at 90, 92, 93 (slice 0) and 94, 100 (slice 1)."""
    x = np.linspace(-3.0, -1.0, 3000).astype(np.float32)
    big = [5, 93 + 94, 600, 1234, 2000, 2998, 2999]
    x[big] = np.arange(10, 17, dtype=np.float32)
    ties = [90, 92, 93, 94, 100]
    x[ties] = 2.5
    order_big = sorted(big, key=lambda i: -x[i])
    for k in range(7, 14):
        want = order_big + ties[:max(0, k - 7)] if k <= 12 else None
        pick, kept = _kept(ctx, x, k)
        assert kept == F.sample(x, 0.5, 1.0, 1.0, k).kept, k
        if want is not None:
            assert kept == want, k                             # the lowest indices win, across the slice boundary


@pytest.mark.parametrize("V", [3000, V_QWEN3])
def test_constant_row(ctx, V):
    x = np.full(V, -1.25, np.float32)
    for k in (1, 50, 95, 1024):
        pick, kept = _kept(ctx, x, k, u=0.9995)
        assert kept == list(range(k)) and pick == k - 1, k    # equal weights: u = 0.9995 sits inside the last of k <= 1024 intervals
    pick, kept = _kept(ctx, x, 1024, u=0.0)
    assert pick == 0


def test_inf_and_nan_entries(ctx):
    rng = np.random.default_rng(3)
    x = rng.standard_normal(3000).astype(np.float32)
    x[rng.choice(3000, 2900, replace=False)] = np.nan          # 100 numbers left: k = 1024 must take NaNs, k = 64 none
    num = np.flatnonzero(~np.isnan(x))
    x[num[:5]] = -np.inf
    x[num[5]] = -0.0
    x[num[6]] = 0.0
    for k in (1, 64, 100, 101, 1024):
        pick, kept = _kept(ctx, x, k)
        ref = F.sample(x, 0.5, 1.0, 1.0, k)
        assert kept == ref.kept and pick == ref.pick, k
        assert not np.isnan(x[pick])
    y = x.copy()
    y[num[7]] = np.inf                                          # +inf is the maximum: it takes all the mass
    assert _kept(ctx, y, 50, temperature=0.7, top_p=0.9, u=0.3) == (int(num[7]), [int(num[7])])


@pytest.mark.parametrize("V", [1, 33, 3000])
def test_all_nan_row_gives_id_zero(ctx, V):
    pick, kept = _kept(ctx, np.full(V, np.nan, np.float32), 0, temperature=0.5, top_p=0.9)
    assert pick == 0 and kept == list(range(min(50, V)))


# (V, top_k): the default k on Qwen3's vocabulary, the largest k on a small row, a row shorter than k
DRAW_ROWS = [(V_QWEN3, 0), (3000, 1024), (51, 64)]
# (seed, logit spread), chosen on the CPU (restatement alone) so that all 3 x 3 cases of a row clear the boundary rule.  Smallest distance
# to top_p / to a CDF edge: 9.5e-4 / 4.2e-4, 1.6e-4 (either), 5.7e-4 / 1.3e-3; kept-set sizes 1 .. 50, 1 .. 144 and 1024, 1 .. 51.  (With
# k = 1024 the cumulative values are dense: at spread 2 no seed of 400 keeps all 1024 of them 1e-4 away from 0.95 at temperature 1.5.)
DRAW_SEEDS = {(V_QWEN3, 0): (0, 2.0), (3000, 1024): (1, 5.0), (51, 64): (1, 2.0)}
TEMPERATURES = [0.3, 0.8, 1.5]
TOP_PS = [0.5, 0.95, 1.0]


@functools.lru_cache(maxsize=None)
def _draw_case(V, top_k):
    seed, spread = DRAW_SEEDS[(V, top_k)]
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(V) * spread).astype(np.float32)
    x.setflags(write=False)
    us = rng.random(9).astype(np.float32)
    return x, us


@pytest.mark.parametrize("V,top_k", DRAW_ROWS)
def test_nucleus_and_draw(ctx, V, top_k):
    x, us = _draw_case(V, top_k)
    cases = [(t, p, float(us[3 * i + j])) for i, t in enumerate(TEMPERATURES) for j, p in enumerate(TOP_PS)]
    dist = [F.boundary_distance(x, u, t, p, top_k) for t, p, u in cases]
    print("smallest distances to top_p / to a CDF edge:", min(d[0] for d in dist), min(d[1] for d in dist))
    assert all(d_p >= 1e-4 and d_u >= 1e-4 for d_p, d_u in dist), dist       # precondition, on the restatement alone: no case is excused
    sizes = set()
    for t, p, u in cases:
        ref = F.sample(x, u, t, p, top_k)
        pick, kept = _kept(ctx, x, top_k, t, p, u)
        assert kept == ref.kept, (t, p, u, len(kept), len(ref.kept))
        assert pick == ref.pick, (t, p, u)
        sizes.add(len(kept))
    assert len(sizes) >= 3                                                     # the nucleus really cuts at different places


def test_top_k_one_is_the_argmax(ctx):
    x, us = _draw_case(V_QWEN3, 0)
    for t in (0.05, 1.0, 30.0):
        for u in (0.0, 0.5, 0.99999):
            assert _kept(ctx, x, 1, t, 0.95, u) == (int(np.argmax(x)), [int(np.argmax(x))])


def test_error_table(ctx):
    import mlx_swift_audio_amd as m
    INV, UNS = m._lib.ERR_INVALID_ARGUMENT, m._lib.ERR_UNSUPPORTED
    x, us = _draw_case(3000, 1024)
    assert min(F.boundary_distance(x, 0.37, 0.8, 0.9, 40)) >= 1e-4
    good = _kept(ctx, x, 40, 0.8, 0.9, 0.37)
    ref = F.sample(x, 0.37, 0.8, 0.9, 40)
    assert good == (ref.pick, ref.kept)
    lib, out, nk = ctx.lib, np.zeros(1, np.int32), np.zeros(1, np.int32)

    def call(logits=x.ctypes.data, V=3000, t=0.8, k=40, p=0.9, o=out.ctypes.data):
        return lib.mia_sample_top_k_top_p(ctx.h, logits, V, t, k, p, 0.37, o, None, nk.ctypes.data)

    bad = [(dict(logits=None), INV), (dict(o=None), INV), (dict(V=0), INV), (dict(t=0.0), INV), (dict(t=-1.0), INV), (dict(t=float("nan")), INV),
           (dict(t=float("inf")), INV), (dict(p=0.0), INV), (dict(p=-0.5), INV), (dict(p=float("nan")), INV), (dict(p=float("inf")), INV),
           (dict(k=-1), INV), (dict(k=1025), UNS), (dict(k=3000), UNS)]
    for kw, code in bad:
        assert call(**kw) == code, kw
        assert _kept(ctx, x, 40, 0.8, 0.9, 0.37) == good
    assert call(k=1024) == 0 and nk[0] >= 1
    assert call(V=1000, k=1025) == 0 and nk[0] <= 1000                      # the bound is on the effective k = min(k, V)
    assert call(V=40, k=5000) == 0 and nk[0] <= 40
