"""Kokoro's ALBERT and bert_encoder on the GPU against the NumPy restatement (tests/_kokoro_bert_ref.py), under the tolerance rule of
test_kokoro_gpu.py: a GPU result must lie within 8 x the restatement's own float32-against-float64 noise.  Every test prints its
figures before it asserts; README.md ("Kokoro") lists the ratios measured on an MI355X."""
import functools

import numpy as np
import pytest
import torch  # noqa: F401  (before the HIP library loads: the pipeline takes torch device tensors)

import _kokoro_bert_ref as BR
from _kokoro_cases import WEIGHT_SEED
from test_kokoro_gpu import _cfg, _within

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _weights(name):
    from mlx_swift_audio_amd import synthetic
    return synthetic.kokoro_weights(_cfg(name), WEIGHT_SEED[name], text=True, bert=True)


def _ids(cfg, N):
    ids = np.random.default_rng([N, cfg.n_symbols]).integers(1, cfg.n_symbols, N).astype(np.int32)
    ids[0] = ids[-1] = 0                                                            # the reference pads with 0 at both ends
    return ids


@pytest.fixture(scope="module")
def models(ctx):
    from mlx_swift_audio_amd import kokoro
    made = {}

    def get(name, kind="KokoroBert"):
        if (name, kind) not in made:
            made[name, kind] = getattr(kokoro, kind).load(ctx, _cfg(name), _weights(name))
        return made[name, kind]

    yield get
    for m in made.values():
        m.close()


# N = 1: softmax over one key; 33 / 65 cross the 32-query workgroup and the 32-key tile; 130: more than one key tile per wave of the
# split-KV; 160: the position table's limit.  kokoro_82m: three float4 per lane in the LayerNorm, K = 2048.
@pytest.mark.parametrize("name,N,layers", [("kokoro_micro", N, L) for N in (1, 2, 33, 65, 130, 160) for L in (1, 3)] +
                         [("kokoro_82m", 8, 1), ("kokoro_82m", 8, 12)])
def test_encode(models, name, N, layers):
    ids = _ids(_cfg(name), N)
    r64, r32 = (BR.KokoroBertRef(_cfg(name), _weights(name), dt).encode(ids, layers) for dt in (np.float64, np.float32))
    got = models(name).encode(ids, n_layers=layers, return_hidden=True)
    for i, what in enumerate(("hidden", "d_en")):
        _within(f"bert {name} N={N} layers={layers} {what}", got[i], r64[i], r32[i], relative=False)


def test_constant_embedding_row_gives_beta_exactly(ctx):
    """Tables constant across E make word + position + type a constant row: x - mean is exactly 0, rstd = 1e6 multiplies that zero and
    the embedding LayerNorm returns beta, exactly what all-zero tables give -- so the two models must agree byte for byte."""
    from mlx_swift_audio_amd.kokoro import KokoroBert
    cfg, ids, out = _cfg("kokoro_micro"), np.array([0, 7], np.int32), []
    for scale in (0.0, 1.0):
        w = dict(_weights("kokoro_micro"))
        for k in (f"bert.embeddings.{t}_embeddings.weight" for t in ("word", "position", "token_type")):
            w[k] = np.ascontiguousarray(np.broadcast_to(np.float32(scale) * w[k][:, :1], w[k].shape))
        m = KokoroBert.load(ctx, cfg, w)
        out.append(m.encode(ids, return_hidden=True))
        m.close()
    ref = BR.KokoroBertRef(cfg, w)                                                  # the constant, non-zero tables
    assert (ref.embeddings(ids) == ref.w["bert.embeddings.LayerNorm.bias"]).all()
    _within("constant row d_en", out[1][1], ref.encode(ids)[1], BR.KokoroBertRef(cfg, w, np.float32).encode(ids)[1], relative=False)
    assert out[0][0].tobytes() == out[1][0].tobytes() and out[0][1].tobytes() == out[1][1].tobytes()


def test_seam(models):
    m, ids = models("kokoro_micro"), _ids(_cfg("kokoro_micro"), 19)
    first = m.encode(ids)
    assert m.encode(ids).tobytes() == first.tobytes() and m.encode(ids, n_layers=_cfg("kokoro_micro").bert_layers).tobytes() == first.tobytes()
    assert m.encode(ids, n_layers=1).tobytes() != first.tobytes()


def test_synthesize_ids_equals_the_stages_chained_by_hand(models):
    from mlx_swift_audio_amd.kokoro import KokoroPipeline, voice_row
    cfg, rng = _cfg("kokoro_micro"), np.random.default_rng(5)
    bert, text, dec = (models("kokoro_micro", k) for k in ("KokoroBert", "KokoroText", "KokoroDecoder"))
    ids = rng.integers(1, cfg.n_symbols, 6).astype(np.int32)
    pack = rng.standard_normal((4, 1, 2 * cfg.style_dim)).astype(np.float32)          # 6 ids clamp to the last row
    padded = np.concatenate([[0], ids, [0]]).astype(np.int32)
    want = KokoroPipeline(text, dec).synthesize(bert.encode(padded), padded, voice_row(pack, len(ids)))
    pipe = KokoroPipeline(text, dec, bert)
    got = pipe.synthesize_ids(ids, pack)
    assert got.shape == (600 * int(pipe.last_durations.sum()),) and got.tobytes() == want.tobytes()
    assert pipe.synthesize(None, padded, pack[3, 0]).tobytes() == want.tobytes()


def test_errors(ctx, models):
    from mlx_swift_audio_amd import MiaError, _lib
    from mlx_swift_audio_amd.kokoro import KokoroBert
    cfg, m = _cfg("kokoro_micro"), models("kokoro_micro")
    ids, w = _ids(cfg, 5), dict(_weights("kokoro_micro"))
    want = m.encode(ids).tobytes()
    del w[BR.GROUP + "attention.key.bias"]
    with pytest.raises(MiaError, match=BR.GROUP + "attention.key.bias"):
        KokoroBert.load(ctx, cfg, w)
    bad = ids.copy()
    bad[2] = cfg.n_symbols
    for case in (np.zeros(0, np.int32), np.zeros(cfg.bert_positions + 1, np.int32), bad):
        with pytest.raises(MiaError) as e:
            m.encode(case)
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    assert ctx.lib.mia_kokoro_bert_encode(m.h, ids.ctypes.data, 5, 0, None, None, _lib.MEM_HOST) == _lib.ERR_INVALID_ARGUMENT
    assert m.encode(ids).tobytes() == want
