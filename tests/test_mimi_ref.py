"""The Mimi oracle against itself (no GPU): the literal per-frame step loop equals the one-pass form with the explicit key range
[max(0, 2 f - context), 2 f + 2) -- the mask the kernel implements -- the streamed convolutions equal their whole-clip forms, the two
entry points are different functions, the sanitiser renames as Mimi.sanitize does, and the lengths are right."""
import numpy as np
import pytest

import _mimi_cases as mc
from _mimi_ref import MimiRef, elu

GPU_TOL = {"mimi_micro": 6.32e-06, "mimi_micro_ctx250": 5.94e-06}          # test_mimi_gpu.TOL (that module's docstring derives them)


@pytest.mark.parametrize("name,frames,n_q", [("mimi_micro", 21, 4), ("mimi_micro", 21, 1), ("mimi_micro_ctx250", 140, 4)])
def test_step_loop_equals_one_pass_with_the_pair_range(name, frames, n_q):
    m = mc.oracle(name)
    literal = mc.stream_ref(name, frames, n_q)
    onepass = m.decode_frames_onepass(mc.codes(name, frames, n_q))
    assert literal.shape == onepass.shape
    assert np.abs(literal - onepass).max() <= 1e-10


def test_window_bites_in_the_cases():
    """context 6: from frame 4 on a pair no longer sees position 0; context 250: from frame 126 on."""
    for name, frames in (("mimi_micro", 21), ("mimi_micro_ctx250", 140)):
        ctx = mc.config(name).transformer.context
        assert 2 * (frames - 1) - ctx > 0


def test_streamed_convolutions_equal_whole_clip():
    name = "mimi_micro"
    m = MimiRef(mc.config(name), mc.weights(name))
    rng = np.random.default_rng(5)
    z = rng.standard_normal((17, mc.config(name).seanet.dimension))
    whole_up = m.upsample(z)
    whole_sea = m.seanet(whole_up)
    for split in ([17], [1] * 17, [3, 1, 5, 8]):
        m.reset()
        ups, seas, at = [], [], 0
        for n in split:
            u = m.upsample.step(z[at:at + n])
            ups.append(u)
            seas.append(m.seanet_step(u))
            at += n
        assert np.abs(np.concatenate(ups) - whole_up).max() <= 1e-10
        assert np.abs(np.concatenate(seas) - whole_sea).max() <= 1e-10


@pytest.mark.parametrize("name,frames,n_q", [("mimi_micro", 21, 4), ("mimi_micro_ctx250", 140, 4)])
def test_decode_and_decode_frames_differ(name, frames, n_q):
    assert mc.rel_gap(mc.whole_ref(name, frames, n_q), mc.stream_ref(name, frames, n_q)) >= 100 * GPU_TOL[name]


def test_output_lengths_and_empty_input():
    for name, spf in (("mimi_micro", 12), ("mimi_micro_ctx250", 12), ("mimi_202407", 1920)):
        cfg = mc.config(name)
        assert cfg.samples_per_frame == spf and cfg.upsample_stride == 2
    assert mc.whole_ref("mimi_micro", 9, 4).shape == (108,) and mc.stream_ref("mimi_micro", 21, 4).shape == (252,)
    m = mc.oracle("mimi_micro")
    assert m.decode(np.zeros((4, 0), np.int32)).shape == (0,)
    m.reset()
    assert m.decode_frames(np.zeros((4, 0), np.int32)).shape == (0,)


def test_synthetic_weights_exercise_the_corners():
    w = mc.weights("mimi_micro")
    usage = w["quantizer.rvq_rest.vq.layers.1.codebook.cluster_usage"]
    assert (usage < 1e-5).any() and (usage > 1e-5).any()
    assert np.abs(w["decoder_transformer.transformer.layers.0.layer_scale_1.scale"] - 1).min() > 0.1
    assert np.abs(w["decoder_transformer.transformer.layers.1.norm2.weight"] - 1).max() > 0.05
    assert np.abs(w["decoder_transformer.transformer.layers.1.norm2.bias"]).max() > 0.01
    for name, frames, n_q in mc.WHOLE_CASES[:4]:
        assert 0.1 <= np.abs(mc.whole_ref(name, frames, n_q)).max() <= 1.0
    x = np.array([-2.0, 0.0, 3.0])
    assert np.allclose(elu(x), [np.expm1(-2.0), 0.0, 3.0])


# raw names as a PyTorch Mimi checkpoint spells them (written out here, not taken from a file) -> the keys Mimi.sanitize produces
RENAMES = {
    "decoder.model.0.conv.conv.weight": "decoder.init_conv1d.conv.conv.weight",
    "decoder.model.2.convtr.convtr.weight": "decoder.layers.0.upsample.convtr.convtr.weight",
    "decoder.model.3.block.1.conv.conv.weight": "decoder.layers.0.residuals.0.block.0.conv.conv.weight",
    "decoder.model.3.block.3.conv.conv.bias": "decoder.layers.0.residuals.0.block.1.conv.conv.bias",
    "decoder.model.11.convtr.convtr.bias": "decoder.layers.3.upsample.convtr.convtr.bias",
    "decoder.model.12.block.3.conv.conv.weight": "decoder.layers.3.residuals.0.block.1.conv.conv.weight",
    "decoder.model.14.conv.conv.weight": "decoder.final_conv1d.conv.conv.weight",
    "encoder.model.0.conv.conv.weight": "encoder.init_conv1d.conv.conv.weight",
    "encoder.model.1.block.1.conv.conv.weight": "encoder.layers.0.residuals.0.block.0.conv.conv.weight",
    "encoder.model.3.conv.conv.weight": "encoder.layers.0.downsample.conv.conv.weight",
    "encoder.model.12.conv.conv.bias": "encoder.layers.3.downsample.conv.conv.bias",
    "encoder.model.14.conv.conv.weight": "encoder.final_conv1d.conv.conv.weight",
    "decoder_transformer.transformer.layers.3.self_attn.in_proj_weight": "decoder_transformer.transformer.layers.3.self_attn.in_proj.weight",
    "decoder_transformer.transformer.layers.3.self_attn.out_proj.weight": "decoder_transformer.transformer.layers.3.self_attn.out_proj.weight",
    "decoder_transformer.transformer.layers.0.linear1.weight": "decoder_transformer.transformer.layers.0.gating.linear1.weight",
    "decoder_transformer.transformer.layers.0.linear2.weight": "decoder_transformer.transformer.layers.0.gating.linear2.weight",
    "decoder_transformer.transformer.layers.7.layer_scale_2.scale": "decoder_transformer.transformer.layers.7.layer_scale_2.scale",
    "quantizer.rvq_first.vq.layers.0._codebook.embedding_sum": "quantizer.rvq_first.vq.layers.0.codebook.embedding_sum",
    "quantizer.rvq_rest.vq.layers.30._codebook.cluster_usage": "quantizer.rvq_rest.vq.layers.30.codebook.cluster_usage",
    "quantizer.rvq_rest.vq.layers.30._codebook._initialized": "quantizer.rvq_rest.vq.layers.30.codebook.initialized",
    "quantizer.rvq_first.output_proj.weight": "quantizer.rvq_first.output_proj.weight",
    "upsample.convtr.convtr.weight": "upsample.convtr.convtr.weight",
    "downsample.conv.conv.weight": "downsample.conv.conv.weight",
}


def test_sanitiser_renames_and_swaps_axes():
    from mlx_swift_audio_amd.checkpoint import sanitize_mimi
    assert sanitize_mimi(list(RENAMES)) == list(RENAMES.values())
    rng = np.random.default_rng(0)
    raw = {"decoder.model.0.conv.conv.weight": rng.standard_normal((8, 5, 7)),            # PyTorch Conv1d [out, in, k]
           "decoder.model.2.convtr.convtr.weight": rng.standard_normal((6, 4, 3)),        # PyTorch ConvTranspose1d [in, out, k]
           "upsample.convtr.convtr.weight": rng.standard_normal((5, 1, 4)),               # depthwise [C, 1, k]
           "quantizer.rvq_first.output_proj.weight": rng.standard_normal((9, 4, 1)),
           "decoder.model.0.conv.conv.bias": rng.standard_normal(8),
           "decoder_transformer.transformer.layers.0.self_attn.in_proj_weight": rng.standard_normal((12, 4))}
    out = sanitize_mimi(raw)
    assert out["decoder.init_conv1d.conv.conv.weight"].shape == (8, 7, 5)
    assert out["decoder.init_conv1d.conv.conv.weight"][3, 2, 4] == raw["decoder.model.0.conv.conv.weight"][3, 4, 2]
    assert out["decoder.layers.0.upsample.convtr.convtr.weight"].shape == (4, 3, 6)
    assert out["decoder.layers.0.upsample.convtr.convtr.weight"][1, 2, 5] == raw["decoder.model.2.convtr.convtr.weight"][5, 1, 2]
    assert out["upsample.convtr.convtr.weight"].shape == (1, 4, 5)
    assert out["quantizer.rvq_first.output_proj.weight"].shape == (9, 1, 4)
    assert out["decoder.init_conv1d.conv.conv.bias"].shape == (8,)
    assert np.array_equal(out["decoder_transformer.transformer.layers.0.self_attn.in_proj.weight"],
                          raw["decoder_transformer.transformer.layers.0.self_attn.in_proj_weight"])
