"""Pins of the text-half restatement itself (tests/_kokoro_text_ref.py), no GPU: the BiLSTM against a scalar step-by-step loop at
float64, and the alignment gather against the dense matmul with pred_aln_trg, to 0."""
import math

import numpy as np
import pytest

import _kokoro_text_ref as TR


@pytest.mark.parametrize("T,In,H", [(1, 3, 2), (2, 3, 2), (5, 4, 3)])
def test_bilstm_equals_the_scalar_loop(T, In, H):
    rng = np.random.default_rng([T, In, H])
    w = {k: rng.standard_normal((4 * H, In) if "ih" in k and "weight" in k else (4 * H, H) if "weight" in k else 4 * H) for k in TR.LSTM_KEYS}
    x = rng.standard_normal((T, In))
    want = np.zeros((T, 2 * H))
    for d, sfx in enumerate(("", "_reverse")):
        h, c = [0.0] * H, [0.0] * H
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            g = [w["bias_ih_l0" + sfx][r] + w["bias_hh_l0" + sfx][r] + sum(w["weight_ih_l0" + sfx][r][k] * x[t][k] for k in range(In)) +
                 sum(w["weight_hh_l0" + sfx][r][k] * h[k] for k in range(H)) for r in range(4 * H)]
            sg = lambda v: 1.0 / (1.0 + math.exp(-v))
            c = [sg(g[H + j]) * c[j] + sg(g[j]) * math.tanh(g[2 * H + j]) for j in range(H)]
            h = [sg(g[3 * H + j]) * math.tanh(c[j]) for j in range(H)]
            want[t, d * H:(d + 1) * H] = h
    np.testing.assert_allclose(TR.bilstm(x, w), want, rtol=0, atol=1e-14)


def test_gather_equals_the_dense_matmul():
    rng = np.random.default_rng(5)
    dur = np.array([1, 7, 1, 3, 2])
    d, t_en = rng.standard_normal((5, 12)), rng.standard_normal((5, 8))
    m = TR.alignment_matrix(dur)
    assert m.shape == (5, 14) and (m.sum(axis=0) == 1).all() and (m.sum(axis=1) == dur).all()
    en, asr = TR.align(d, t_en, dur)
    assert (en == (d.T @ m).T).all() and (asr == t_en.T @ m).all()
