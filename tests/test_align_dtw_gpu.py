"""The alignment's DTW and backtrace on the device (csrc/align_dtw.hip; mia_op_dtw mode 1, mia_whisper_set_align_dtw) against
oracle.whisper.dtw: the SAME path, entry for entry -- fp32 accumulators, one add per cell and the literal tie rule leave no tolerance."""
import functools

import numpy as np
import pytest

from oracle import whisper as OW

pytestmark = pytest.mark.gpu

# the issue's shapes, then one on each side of the kernel's own partition edges: rows per lane 1 | 2 | 4 | 7 at 64 | 128 | 256 rows, and
# the 256-step LDS chunk of the backtrace (steps = M + ceil(N / R) - 1: 256 at (64, 193), 257 at (64, 194))
SHAPES = [(1, 1), (1, 5), (5, 1), (7, 9), (65, 130), (129, 257), (447, 1500)]
EDGES = {"rows64-chunk256": (64, 193), "rows64-chunk257": (64, 194), "rows128": (128, 40), "rows256": (256, 33), "rows257": (257, 31)}
CASES = [pytest.param(s, id="%dx%d" % s) for s in SHAPES] + [pytest.param(s, id=k) for k, s in EDGES.items()]


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(cost, the oracle's path), computed once per (shape, kind)."""
    rng = np.random.default_rng(shape[0] * 2003 + shape[1])
    cost = rng.standard_normal(shape).astype(np.float32) if kind == "normal" else rng.integers(-1, 2, shape).astype(np.float32)
    cost.setflags(write=False)
    return cost, OW.dtw(cost)


@pytest.mark.parametrize("kind", ["normal", "ties"])        # ties: {-1, 0, 1} costs, nearly every cell decided by a branch of the rule
@pytest.mark.parametrize("shape", CASES)
def test_path_equals_oracle(ctx, shape, kind):
    from mlx_swift_audio_amd import ops
    cost, want = _case(shape, kind)
    ld = shape[1] + (3 if kind == "normal" else 0)          # ld > M, and rows that start off a 16-byte boundary
    assert ops.dtw(ctx, cost, mode=1, ld=ld) == want
    if shape == (129, 257):
        assert ops.dtw(ctx, cost, mode=0, ld=ld) == want and {0, 1} <= set(np.diff(want[0])) and {0, 1} <= set(np.diff(want[1]))   # all three moves


def test_ragged_batch_equals_single_calls(ctx):
    from mlx_swift_audio_amd import ops
    clips = [_case(s, "normal") for s in ((129, 257), (7, 9), (65, 130))]      # the batch runs at 4 rows per lane, the singles at 4, 1, 2
    assert ops.dtw(ctx, [c for c, _ in clips], mode=1) == [w for _, w in clips]


def test_on_the_model(ctx):
    """mia_whisper_align with the DTW on the device: the same probs bits and paths as the host mode on the same encode, the exact DTW of
    the returned matrix, and the same again without the matrix (micro checkpoint and set-up of tests/test_timing_gpu.py, ragged clips)."""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import timing as HT
    from mlx_swift_audio_amd import whisper as HW
    dims = OW.DIMS["micro"]
    model = HW.WhisperModel.load(ctx, dims, OW.synthetic_weights(dims, seed=11, round_to="f16"), m.F16)
    st = OW.SpecialTokens.for_vocab(dims.n_vocab)
    rng = np.random.default_rng(3)
    mel = OW.round_array((0.5 * rng.standard_normal((3, 2 * dims.n_audio_ctx, dims.n_mels))).astype(np.float32), "f16")
    model.encode(mel)
    sot = st.sot_sequence(3, "transcribe")
    seqs = [sot + [st.no_timestamps] + rng.integers(300, 5000, n).tolist() + [st.eot] for n in (9, 5, 14)]
    frames = [2 * dims.n_audio_ctx, 2 * dims.n_audio_ctx - 10, 37]
    heads = [(0, 1), (dims.n_text_layer - 1, 0), (dims.n_text_layer - 1, dims.n_text_head - 1)]
    probs0, paths0, _ = HT.align(model, seqs, heads, frames, len(sot), st.eot, want_matrix=True)
    model.set_align_dtw(1)
    probs1, paths1, mat = HT.align(model, seqs, heads, frames, len(sot), st.eot, want_matrix=True)
    assert probs1.tobytes() == probs0.tobytes() and paths1 == paths0
    for b, seq in enumerate(seqs):
        assert OW.dtw(-mat[b, len(sot):len(seq) - 1, :frames[b] // 2]) == paths1[b]
    assert HT.align(model, seqs, heads, frames, len(sot), st.eot)[1] == paths0
    with pytest.raises(m.MiaError) as e:
        model.set_align_dtw(2)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_short_path_cap_is_refused_and_the_context_lives(ctx, mode):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    cost, want = _case((65, 130), "normal")
    with pytest.raises(m.MiaError) as e:
        ops.dtw(ctx, cost, mode=mode, path_cap=len(want[0]) - 1)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT and "path_cap" in str(e.value)
    assert ops.dtw(ctx, cost, mode=mode, path_cap=len(want[0])) == want


def test_mode_and_size_errors(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    with pytest.raises(m.MiaError) as e:
        ops.dtw(ctx, np.zeros((3, 4), np.float32), mode=2)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    for shape in ((449, 8), (8, 1501)):
        with pytest.raises(m.MiaError) as e:
            ops.dtw(ctx, np.zeros(shape, np.float32), mode=1)
        assert e.value.code == m._lib.ERR_UNSUPPORTED
