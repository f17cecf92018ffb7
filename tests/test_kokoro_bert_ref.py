"""The restatement of Kokoro's ALBERT (tests/_kokoro_bert_ref.py) against what it claims to restate, and voice_row (no GPU needed)."""
import math

import numpy as np
import pytest

import _kokoro_bert_ref as BR


def test_gelu_is_the_erf_form():
    x = np.array([-6.0, -1.5, -0.1, 0.0, 0.3, 2.0, 7.5])
    assert np.abs(BR.gelu(x) - [0.5 * v * (1 + math.erf(v / math.sqrt(2))) for v in x]).max() < 1e-15
    assert BR.gelu(x.astype(np.float32)).dtype == np.float32


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_the_all_ones_mask_adds_exactly_zero(dt):
    m, s = BR.mask_term(5, dt), np.random.default_rng(0).standard_normal((2, 5, 5)).astype(dt)
    assert m.dtype == dt and (m == 0).all() and (s + m).tobytes() == s.tobytes()


def test_n_layers_is_that_many_applications_of_the_one_layer():
    from mlx_swift_audio_amd import synthetic
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS
    cfg = KOKORO_CONFIGS["kokoro_micro"]
    ref, ids = BR.KokoroBertRef(cfg, synthetic.kokoro_weights(cfg, 1, bert=True)), np.array([0, 3, 9, 1, 0])
    x = ref.linear("bert.encoder.embedding_hidden_mapping_in", ref.embeddings(ids))
    for k in range(1, cfg.bert_layers + 1):
        x = ref.layer(x)
        assert (ref.encode(ids, k)[0] == x).all()
    assert (ref.encode(ids)[0] == x).all() and ref.encode(ids)[1].shape == (5, cfg.d_model)


def test_voice_row_clamps_at_the_last_row():
    from mlx_swift_audio_amd import MiaError
    from mlx_swift_audio_amd.kokoro import voice_row
    pack = np.arange(4 * 6, dtype=np.float32).reshape(4, 1, 6)
    for n, row in ((1, 0), (4, 3), (5, 3), (500, 3)):
        assert (voice_row(pack, n) == pack[row, 0]).all() and (voice_row(pack[:, 0], n) == pack[row, 0]).all()
    with pytest.raises(MiaError):
        voice_row(pack, 0)
