"""Marvis with the backbone's prompt pass on the packed weights (mia_marvis_use_packed_prompt) and with the 16-bit layer Linears of both
stacks released (mia_marvis_release_dense), on the micro configs and the 6-bit checkpoints of tests/_marvis6_cases.py, against the float64
oracle on the de-quantised checkpoint.

(a) The first frame behind a 24-row prompt (23 rows through the packed prompt pass, the last through the frame): every head's logits
    within the step chain's own TOL of _marvis_cases (0.08 bf16, 0.015 f16) -- the bound of the prompt walked through the packed step,
    not the 0.08 / 0.02 "behind the default prompt pass".  The walked prompt (set_debug(2)) is held to the same bound as a control.
(b) Sampled frames equal the oracle's exactly on the cases' safe uniforms (M6.SAMPLED, chosen from the oracle alone).
(c) release_dense() followed by generate gives the same frames; the two switches back are MIA_ERR_UNSUPPORTED.
Measured on an MI355X 2026-10-21, worst head of (a): f16 0.0038 packed prompt pass / 0.0033 walked, bf16 0.0216 / 0.0381."""
import numpy as np
import pytest

import _marvis6_cases as M6
import _marvis_cases as MC
import _marvis_ref as R
from test_marvis_packed_gpu import _load, _ratio

pytestmark = pytest.mark.gpu


def _first_frame(model, tk, mk):
    ids, lg = model.frame(tk, mk, MC.N_CODEBOOKS, np.full(MC.N_CODEBOOKS, 0.5, np.float32), forced=MC.FORCED[0], return_logits=True)
    assert ids.tolist() == MC.FORCED[0].tolist()
    return lg


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", ["marvis-micro", "marvis-micro128"])
def test_first_frame_behind_a_packed_prompt_meets_the_chain_bound(ctx, name, dtype):
    tk, mk = MC.prompt(21)
    assert tk.shape[0] == 24
    _, ref = R.MarvisRef(MC.config(name), M6.checkpoint(name, dtype)[1]).generate_frame(MC.N_CODEBOOKS, tk, mk, lambda x, i: 0, MC.FORCED[0])
    ref = np.asarray(ref)
    model = _load(ctx, name, dtype)
    default = _first_frame(model, tk, mk)
    model.use_packed_prompt(True)
    model.reset()
    packed = _first_frame(model, tk, mk)
    model.set_debug(2)
    model.reset()
    walked = _first_frame(model, tk, mk)
    for what, lg in (("packed prompt pass", packed), ("walked", walked)):
        r = _ratio(lg, ref)
        print(f"{name} {dtype} {what}: max |delta| / std per head = {r.round(4).tolist()}; bound {MC.TOL[dtype]}")
        assert (r <= MC.TOL[dtype]).all(), (what, r)
    assert not np.array_equal(packed, default)                # the switch reaches the prompt pass
    model.set_debug(0)
    model.use_packed_prompt(False)
    model.reset()
    assert np.array_equal(_first_frame(model, tk, mk), default)
    model.close()


def test_sampled_frames_equal_the_oracle_and_survive_release_dense(ctx):
    import mlx_swift_audio_amd as m
    s = M6.SAMPLED
    runs = [M6.choose_uniforms(s["name"], s["dtype"], 5, 6, s["temperature"], s["top_p"], cs, s["weight_seed"], tol=M6.TOL_PROMPT_PASS[s["dtype"]]) for cs in s["choice_seeds"]]
    assert all(r is not None for r in runs)
    model = _load(ctx, s["name"], s["dtype"], s["weight_seed"], True)
    model.use_packed_prompt(True)
    tk, mk = MC.prompt()
    kw = dict(temperature=s["temperature"], top_p=s["top_p"])
    for u, frames, margin in runs:
        assert margin > 4 * MC.SAMPLER_SLACK
        model.reset()
        assert model.generate(tk, mk, 5, u, **kw).tolist() == frames.tolist()
    model.release_dense()
    for u, frames, _ in runs:
        model.reset()
        assert model.generate(tk, mk, 5, u, **kw).tolist() == frames.tolist()
    for call in (lambda: model.use_packed(False), lambda: model.use_packed_prompt(False)):
        with pytest.raises(m.MiaError) as e:
            call()
        assert e.value.code == m._lib.ERR_UNSUPPORTED
    model.use_packed(True); model.use_packed_prompt(True)
    model.close()


def test_switches_need_attached_weights(ctx):
    import mlx_swift_audio_amd as m
    model = _load(ctx, "marvis-micro", "f16", attach=False)
    for call in (lambda: model.use_packed_prompt(True), model.release_dense):
        with pytest.raises(m.MiaError) as e:
            call()
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    model.use_packed_prompt(False)
    model.close()
