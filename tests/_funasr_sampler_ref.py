"""CPU restatement (numpy; selection on the fp32 bits, probabilities in float64) of Fun-ASR's sampler for temperature > 0 as this project
builds it: FunASRModel.sampleNextToken, STT/FunASR/FunASRModel.swift:165-198, with the three things the reference leaves open fixed by
the project's convention (explicit uniform, lowest index on ties, inverse CDF).  The rule, as include/mia.h states it at
mia_lm_generate_topk, for a row x[0..V) of fp32 logits and one uniform u in [0, 1):

  1. k = min(top_k > 0 ? top_k : 50, V)
  2. kept = the first k entries under "higher value first, then lower index" on the raw logits; -0 counts as +0, a NaN ranks below
     every number; a row whose best entry is NaN gives id 0
  3. the kept entries stay in that order
  4. top_p < 1: p = softmax((x - x_max) / temperature) over the kept entries (a kept NaN has p = 0),
     n = clamp(count(cumsum(p) < top_p) + 1, 1, k); else n = k
  5. q = softmax over the first n, w = q + 1e-10, pick = first j with cumsum(w)_j > u * sum(w), else the last

tests/test_funasr_sampler_ref.py pins this file on hand-worked rows and on the reference's arithmetic written out literally."""
from __future__ import annotations

import dataclasses

import numpy as np

MAX_K = 1024
EPS_W = float(np.float32(1e-10))


def order_keys(x: np.ndarray) -> np.ndarray:
    """uint32 keys with key(a) > key(b) <=> a > b as floats; -0 -> the key of +0; NaN -> 0 (below -inf)."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    b = x.view(np.uint32).copy()
    nan = (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 0
    return key


def effective_k(top_k: int, V: int) -> int:
    return min(top_k if top_k > 0 else 50, V)


def kept_order(x: np.ndarray, k: int) -> np.ndarray:
    """Indices of the first k entries under (value descending, index ascending), in that order."""
    key = order_keys(x).astype(np.uint64)
    idx = np.arange(key.size, dtype=np.uint64)
    comp = (key << np.uint64(32)) | (np.uint64(0xffffffff) - idx)         # unique: descending comp = the order
    if k < key.size:
        part = np.argpartition(comp, key.size - k)[key.size - k:]
    else:
        part = np.arange(key.size)
    return part[np.argsort(comp[part])[::-1]].astype(np.int64)


@dataclasses.dataclass
class Draw:
    pick: int
    kept: list            # the n kept ids in kept order
    k: int
    cum: np.ndarray       # float64 cumsum of p over the k kept entries (empty when top_p >= 1 or the row has no ordered value)
    cw: np.ndarray        # float64 cumsum of w over the n kept entries
    goal: float           # u * sum(w)
    slot: int             # position of the pick in `kept`


def sample(x, u: float, temperature: float, top_p: float = 0.95, top_k: int = 0) -> Draw:
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    k = effective_k(top_k, x.size)
    assert 1 <= k <= MAX_K
    T, P, U = float(np.float32(temperature)), float(np.float32(top_p)), float(np.float32(u))
    order = kept_order(x, k)
    xk = x[order].astype(np.float64)
    if np.isnan(xk[0]):
        return Draw(0, order.tolist(), k, np.zeros(0), np.zeros(0), 0.0, 0)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((xk - xk[0]) / T)
    e[xk == xk[0]] = 1.0
    e[np.isnan(xk)] = 0.0
    n, cum = k, np.zeros(0)
    if P < 1.0:
        cum = np.cumsum(e / e.sum())
        n = max(1, min(int((cum < P).sum()) + 1, k))
    w = e[:n] / e[:n].sum() + EPS_W
    cw = np.cumsum(w)
    goal = U * cw[-1]
    hit = np.flatnonzero(cw > goal)
    slot = int(hit[0]) if hit.size else n - 1
    return Draw(int(order[slot]), order[:n].tolist(), k, cum, cw, goal, slot)


def boundary_distance(x, u: float, temperature: float, top_p: float = 0.95, top_k: int = 0) -> tuple[float, float]:
    """(smallest |cumsum(p)_j - top_p| over the k kept entries -- inf when top_p >= 1 --, distance of u * sum(w) to the nearer edge of the
    chosen interval over sum(w)).  A draw whose two distances are both large cannot be moved by fp32 rounding of the sums: the same idea
    as oracle/lm.py:sample_boundary_distance."""
    d = sample(x, u, temperature, top_p, top_k)
    if d.cw.size == 0:
        return float("inf"), float("inf")
    d_p = float(np.abs(d.cum - float(np.float32(top_p))).min()) if d.cum.size else float("inf")
    lo = d.cw[d.slot - 1] if d.slot > 0 else 0.0
    d_u = min(d.goal - lo, d.cw[d.slot] - d.goal) / d.cw[-1]
    return d_p, float(d_u)


def generate(logits_of_rows, embed: np.ndarray, prompt: np.ndarray, uniforms, stop_ids, max_new_tokens: int, temperature: float, top_p: float = 0.95,
             top_k: int = 0, trace: list | None = None) -> list[int]:
    """FunASRSTT.swift:132-156 with the sampler above: logits_of_rows(rows) appends embedding rows to the model's cache and returns the
    last row's logits.  A stop id ends the loop and is not emitted; draw i takes uniforms[i].  `trace` receives (logits, Draw) per draw."""
    logits = logits_of_rows(prompt)
    out: list[int] = []
    for i in range(max_new_tokens):
        d = sample(logits, float(uniforms[i]), temperature, top_p, top_k)
        if trace is not None:
            trace.append((np.array(logits, np.float32), d))
        if d.pick in stop_ids:
            break
        out.append(d.pick)
        if len(out) < max_new_tokens:
            logits = logits_of_rows(embed[d.pick][None])
    return out
