"""Shared cases of the Marvis tests (CPU and GPU): prompts, checkpoints, the logit bound and its derivation, the sampler's constructed rows,
and the oracle-side choice of uniforms whose draws no admissible logit error can change."""
import functools

import numpy as np

import _marvis_ref as R

AUDIO_VOCAB, N_CODEBOOKS = 67, 5
TEXT_IDS = [5, 17, 256]

# The step chain's per-dtype bound on max |logit error| / std(logits) (tests/test_lm_qwen3_gpu.py: TOL) is the bound of every case here.
TOL = {"bf16": 0.08, "f16": 0.015}
# What the rule for a wider bound would allow, had the second stack chained behind the first needed one -- derived on the CPU from the
# oracle alone (derived_bound below): its float64 run against its own run with the activations rounded to the storage type where the GPU
# rounds them, times 4 for the summation orders the oracle does not model; the worst head over the six teacher-forced frames of the logits
# test.  test_marvis_ref.py recomputes the table.  It is on record only: the chain's own bound is the one asserted.
DERIVED = {("marvis-micro", "f16"): 0.0194, ("marvis-micro", "bf16"): 0.1754, ("marvis-micro128", "f16"): 0.0139, ("marvis-micro128", "bf16"): 0.1383}


def bound(name, dtype):
    return TOL[dtype]


def config(name):
    from mlx_swift_audio_amd import synthetic
    return synthetic.MARVIS_CONFIGS[name]


LOUD = 4.0      # the peaked checkpoints: the head rows of every 11th id (0 among them) are this much louder, so the top logits stand apart


@functools.lru_cache(maxsize=None)
def weights(name, dtype, seed=3, peaked=False):
    """Synthetic checkpoint; peaked: the same with the rows of ids 0, 11, 22, ... of every head scaled by LOUD (synthetic heads only)."""
    from mlx_swift_audio_amd import synthetic
    w = synthetic.marvis_weights(config(name), seed=seed, round_to=dtype)
    if peaked:
        w = dict(w)
        c0, ah = w["codebook0_head.weight"].copy(), w["audio_head"].copy()
        c0[::11] *= LOUD
        ah[:, :, ::11] *= LOUD
        w["codebook0_head.weight"], w["audio_head"] = R.round_to(c0, dtype).astype(np.float32), R.round_to(ah, dtype).astype(np.float32)
    return w


def voice_codes(T, salt=0):
    return np.array([[(3 * c + 7 * t + 1 + salt) % AUDIO_VOCAB for t in range(T)] for c in range(N_CODEBOOKS)], np.int32)


def prompt(n_audio=9, salt=0):
    """3 text rows + n_audio audio rows (12 rows; 37 audio rows give the 40-row prompt)."""
    from mlx_swift_audio_amd import marvis
    return marvis.tokenize_start(TEXT_IDS, voice_codes(n_audio, salt))


def feedback(ids):
    """A drawn frame as the next call's row of full width: [ids | 0 ...] with mask [1 .. 1 | 0 ...]."""
    row, mask = np.zeros((1, N_CODEBOOKS + 1), np.int32), np.zeros((1, N_CODEBOOKS + 1), np.int32)
    row[0, :len(ids)] = ids
    mask[0, :len(ids)] = 1
    return row, mask


FORCED = np.random.default_rng(0).integers(0, AUDIO_VOCAB, (6, N_CODEBOOKS))


@functools.lru_cache(maxsize=None)
def forced_run(name, dtype, codebooks, rnd=None, n_audio=9, seed=3, peaked=False):
    """The oracle's logits [6][codebooks][V] over six teacher-forced frames behind the prompt (computed once, shared)."""
    ref = R.MarvisRef(config(name), weights(name, dtype, seed, peaked), rnd=rnd)
    tk, mk = prompt(n_audio)
    out = []
    for f in range(6):
        _, lg = ref.generate_frame(codebooks, tk, mk, lambda x, i: 0, FORCED[f])
        out.append(lg)
        tk, mk = feedback(FORCED[f][:codebooks])
    out = np.stack(out)
    out.setflags(write=False)
    return out


def derived_bound(name, dtype, seed=3, peaked=False):
    a, b = forced_run(name, dtype, N_CODEBOOKS, None, 9, seed, peaked), forced_run(name, dtype, N_CODEBOOKS, dtype, 9, seed, peaked)
    return 4.0 * float((np.abs(a - b).max(-1) / a.std(-1)).max())


# ---- the sampler's constructed rows: every probability is a power of two or zero, so fp32 and float64 agree exactly ---------------------
NEG = -np.inf


def sampler_rows():
    """(label, logits, temperature, top_p, u)"""
    four = np.zeros(4, np.float32)
    eight = np.array([0, NEG, 0, 0, NEG, 0, NEG, NEG, 0, 0, 0, 0], np.float32)      # eight entries of 1/8 and four zeros
    nan = np.array([0, np.nan, 0, 0, 0], np.float32)
    rows = [("ties, half kept", four, 1.0, 0.5, 0.3), ("ties, half kept, other pick", four, 1.0, 0.5, 0.75),
            ("cumulative exactly at 1 - top_p", four, 0.5, 0.75, 0.1),                # c = .25 == threshold: not kept
            ("top_p = 1", eight, 1.0, 1.0, 0.55), ("top_p = 1 keeps no zero", eight, 2.0, 1.0, 0.0),
            ("tiny top_p keeps the largest", four, 1.0, 1e-6, 0.5),
            ("NaN ranks lowest", nan, 1.0, 1.0, 0.2), ("NaN, half kept", nan, 1.0, 0.5, 0.9),
            ("u just below 1", eight, 1.0, 0.5, float(np.nextafter(np.float32(1), np.float32(0)))), ("u = 0", eight, 1.0, 0.5, 0.0)]
    big = np.full(2051, NEG, np.float32)
    big[[7, 900, 2050, 33]] = 0                                                       # more than one thread's share, odd V
    rows += [("V 2051", big, 1.0, 0.5, 0.6), ("V 8192", np.zeros(8192, np.float32), 0.7, 2.0 ** -10, 0.3)]
    return rows


SAMPLER_SLACK = 1e-5      # fp32 cumulative sums: at most ~40 roundings of 2^-24 on sums <= 1, plus expf and the division at a few ulp per term


def random_sampler_rows(n=200, seed=11):
    """Random rows the oracle's margins clear by SAMPLER_SLACK (kept threshold, order of the kept entries, pick)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        V = int(rng.choice([67, 300, 2051]))
        x = (rng.standard_normal(V) * rng.uniform(1, 4)).astype(np.float32)
        t, p, u = float(rng.uniform(0.3, 1.2)), float(rng.uniform(0.05, 1.0)), float(rng.uniform(0, 1))
        _, _, mg = R.sample_top_p_ascending(x, t, p, u)
        if min(mg["keep"], mg["pick"]) > SAMPLER_SLACK and mg["order"] > 1e-4:
            out.append((x, t, p, u))
    return out


# ---- draws that no admissible logit error can change -------------------------------------------------------------------------------------
def safe_intervals(logits, temperature, top_p, delta):
    """With every logit anywhere within +- delta: None if the kept set could change (a cumulative sum crossing the threshold, or the last
    dropped entry overtaking the first kept one); else [(id, lo, hi)]: for each kept entry whose place among its two neighbours cannot
    change, the open interval of u that picks it whatever the error (a swap among other kept entries moves neither the sum below the
    pick nor the pick).  With r = exp(2 delta / T): the ratio
    of two probabilities moves by a factor within r^+-1 (the softmax denominator cancels), and a fraction A / (A + B) of two disjoint
    sums of exponentials lies between A / (A + B r) and A r / (A r + B) (A and B move by exp(+-delta / T) in opposite directions)."""
    x = np.asarray(logits, np.float64)
    z = x / np.float64(np.float32(temperature))
    e = np.exp(z - z.max())
    p = e / e.sum()
    order = np.lexsort((np.arange(x.size), p))
    ps, c = p[order], np.cumsum(p[order])
    thr = float(np.float32(1.0) - np.float32(top_p))
    r = float(np.exp(2.0 * delta / temperature))
    lo_of = lambda f: f / (f + (1.0 - f) * r) - SAMPLER_SLACK
    hi_of = lambda f: f * r / (f * r + (1.0 - f)) + SAMPLER_SLACK
    above = np.nonzero(c > thr)[0]
    if not above.size:
        return None
    j0 = int(above[0])
    if lo_of(min(c[j0], 1.0)) <= thr or (j0 > 0 and hi_of(c[j0 - 1]) >= thr):
        return None
    if j0 > 0 and ps[j0 - 1] * r >= ps[j0]:
        return None
    cum = np.minimum(np.cumsum(ps[j0:]) / ps[j0:].sum(), 1.0)
    out = []
    for k in range(cum.size):
        j = j0 + k
        if (j > 0 and ps[j - 1] * r >= ps[j]) or (j + 1 < x.size and ps[j] * r >= ps[j + 1]):
            continue
        lo = hi_of(cum[k - 1]) if k else 0.0
        hi = lo_of(cum[k]) if k < cum.size - 1 else 1.0
        out.append((int(order[j0 + k]), lo, hi))
    return out


def choose_uniforms(name, dtype, codebooks, n_frames, temperature, top_p, choice_seed, weight_seed=3, peaked=True, want=None, tokens=None, mask=None, tol=None):
    """Walk the oracle frame by frame and draw by draw behind the 12-row prompt; at each draw take, among the kept entries whose safe
    interval is not empty, one by the seeded choice (want(frame, i, ids) may name it) and the middle of its interval as the uniform.
    -> (uniforms [n][codebooks], frames [n][codebooks] as the oracle draws them (the all-zero frame included), smallest margin) or None when
    some draw cannot be made safe."""
    cfg, rng = config(name), np.random.default_rng(choice_seed)
    ref = R.MarvisRef(cfg, weights(name, dtype, weight_seed, peaked))
    tol = tol if tol is not None else TOL[dtype]      # the logits test's bound
    tk, mk = (tokens, mask) if tokens is not None else prompt()
    uniforms, frames, margin = [], [], np.inf
    for f in range(n_frames):
        us = []

        def sampler(lg, i):
            nonlocal margin
            iv = safe_intervals(lg, temperature, top_p, tol * lg.std())
            ok = [(t, lo, hi) for t, lo, hi in (iv or []) if hi - lo > 4 * SAMPLER_SLACK]
            if not ok:
                raise LookupError
            ids = [t for t, _, _ in ok]
            pickd = want(f, i, ids) if want else None
            t, lo, hi = ok[ids.index(pickd)] if pickd in ids else ok[int(rng.integers(len(ok)))]
            u = np.float32((lo + hi) / 2)
            margin = min(margin, float(u) - lo, hi - float(u))
            got, _, _ = R.sample_top_p_ascending(lg, temperature, top_p, u)
            assert got == t
            us.append(u)
            return t
        try:
            ids, _ = ref.generate_frame(codebooks, tk, mk, sampler)
        except LookupError:
            return None
        uniforms.append(us)
        frames.append(ids)
        if ids.sum() == 0:
            break
        tk, mk = np.concatenate([ids, [0]])[None, :], np.concatenate([np.ones(ids.size, np.int64), [0]])[None, :]
    return np.array(uniforms, np.float32), np.array(frames, np.int64), margin
