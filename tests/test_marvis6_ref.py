"""CPU side of the packed-6-bit Marvis cases (tests/_marvis6_cases.py): the table of derived bounds is recomputed, the checkpoints are what
they claim to be, and the recorded seeds give the runs the GPU tests rest on -- all from the oracle alone."""
import numpy as np

import _marvis6_cases as M6
import _marvis_cases as MC
import _quant6 as Q6


def test_derived_bounds_are_the_recorded_ones():
    for (name, dtype), want in M6.DERIVED_PROMPT_PASS.items():
        got = M6.derived_bound16(name, dtype)
        assert abs(got - want) <= 5e-4 * max(1.0, want / 0.01), (name, dtype, got, want)


def test_checkpoint_quantises_every_linear_and_nothing_else():
    from mlx_swift_audio_amd import checkpoint as CK
    stored, dense = M6.checkpoint("marvis-micro", "f16")
    base = MC.weights("marvis-micro", "f16")
    assert set(dense) == set(base)
    packed = {k[:-7] for k in stored if k.endswith(".scales")}
    assert packed == {k[:-7] for k in base if M6.is_linear(k)} and len(packed) == 2 * 2 * 7 + 2
    for k, v in base.items():
        if M6.is_linear(k):
            p = k[:-7]
            assert stored[p + ".weight"].dtype == np.uint32 and stored[p + ".weight"].shape == (v.shape[0], v.shape[1] * 6 // 32)
            assert stored[p + ".scales"].dtype == np.float16 and stored[p + ".scales"].shape == (v.shape[0], v.shape[1] // 64)
            step = stored[p + ".scales"].astype(np.float64).max()
            assert np.abs(dense[k] - v).max() <= 0.51 * step + 1e-3 and len(np.unique(Q6.unpack6(stored[p + ".weight"]))) == 64
        else:
            assert np.array_equal(stored[k], v) and dense[k] is stored[k]
    both, _ = M6.checkpoint("marvis-micro", "f16", quantise_embeddings=True)
    assert {k[:-7] for k in both if k.endswith(".scales")} == packed | {"text_embeddings", "audio_embeddings"}
    assert CK.sanitize_marvis([M6.raw_name(k) for k in both]) == list(both)


def test_recorded_seeds_give_safe_runs():
    s = M6.STOP
    u, frames, margin = M6.choose_uniforms(s["name"], s["dtype"], s["codebooks"], 8, s["temperature"], s["top_p"], 0, s["weight_seed"], M6.stop_want,
                                           tol=M6.TOL_PROMPT_PASS[s["dtype"]])
    assert margin > 4 * MC.SAMPLER_SLACK and len(frames) == 3 and frames[-1].sum() == 0 and all(f.sum() > 0 for f in frames[:-1])
    s = M6.SAMPLED
    runs = [M6.choose_uniforms(s["name"], s["dtype"], 5, 6, s["temperature"], s["top_p"], cs, s["weight_seed"], tol=M6.TOL_PROMPT_PASS[s["dtype"]]) for cs in s["choice_seeds"]]
    assert all(r is not None and r[1].shape == (6, 5) and r[2] > 4 * MC.SAMPLER_SLACK for r in runs) and runs[0][1].tolist() != runs[1][1].tolist()
    assert set(MC.weights("marvis-micro", "f16", 148, True)) == set(M6.checkpoint("marvis-micro", "f16")[1]) and MC.weights.cache_info().currsize > 0      # the oracle-side patch of MC.weights was undone
