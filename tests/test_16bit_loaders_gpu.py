"""The host plumbing the 16-bit models share (csrc/tensor_loader.h under whisper_load.hip, lm_load.hip and sensevoice.hip; the packed
lookup / upload of quant_repack.h under both attach calls): every loader reports a missing or mis-shaped tensor by name with
INVALID_ARGUMENT and leaves the context -- for an attach: the handle -- usable, and a checkpoint whose values the handle's 16-bit type
represents loads to the same bits whether its tensors arrive as float32, float16 or bf16 payloads.  Micro configurations only;
everything is compared bit for bit.

The two attach calls name the Linear, not one of its three tensors, when a shape is wrong: "'<p>' is not a 4-bit group-64 Linear of the
expected shape"; the dense loaders say "tensor '<name>' has an unexpected shape"."""
import ctypes as C

import numpy as np
import pytest

import mlx_swift_audio_amd as M
from mlx_swift_audio_amd import synthetic as S

from _whisper_packed import quantised_checkpoint

pytestmark = pytest.mark.gpu

DT = {"bf16": M.BF16, "f16": M.F16}


# ---- the models: (weights, load(ctx, weights), run(handle) -> array) ---------------------------------------------------------------------
def _whisper_run(model):
    from mlx_swift_audio_amd import whisper as HW
    d = model.dims
    mel = S.round_array((0.5 * np.random.default_rng(1).standard_normal((2, 2 * d.n_audio_ctx, d.n_mels))).astype(np.float32), "bf16")
    res = HW.GreedyDecoder(model, HW.DecodingOptions(timestamps=False, max_new_tokens=6)).decode(mel)
    feats = model.audio_features()
    assert np.isfinite(feats).all()
    return np.concatenate([feats.reshape(-1)] + [np.asarray(r.tokens + [r.avg_logprob, r.no_speech_prob], np.float32) for r in res])


def _whisper(kind="bf16", seed=3):
    from mlx_swift_audio_amd import whisper as HW
    dims = S.DIMS["micro"]
    return S.synthetic_weights(dims, seed=seed, round_to=kind), lambda c, w: HW.WhisperModel.load(c, dims, w, DT[kind]), _whisper_run


def _lm(name, kind="bf16"):
    from mlx_swift_audio_amd import lm as HL
    cfg = S.LM_CONFIGS[name]
    w = {k: S.round_array(v, kind) for k, v in S.lm_weights(cfg, seed=5).items()}          # the norm gains too
    return w, lambda c, w: HL.CausalLM.load(c, cfg, w, DT[kind]), lambda h: h.forward([7, 1, 2999, 40]).copy()


def _sensevoice():
    from mlx_swift_audio_amd import funasr
    cfg = funasr.SENSEVOICE_CONFIGS["sensevoice-micro"]
    feats = np.random.default_rng(7).standard_normal((7, 560)).astype(np.float32)
    return (S.sensevoice_weights(cfg, seed=1, round_to="bf16"), lambda c, w: funasr.SenseVoiceEncoder.load(c, cfg, w, M.BF16),
            lambda h: np.concatenate([a.reshape(-1) for a in h.encode([feats])]))


# model -> (its entry above, tensor to drop, tensor to mis-shape)
DENSE = {
    "whisper": (_whisper, "decoder.blocks.1.cross_attn.key.weight", "encoder.blocks.0.mlp1.weight"),
    "llama": (lambda: _lm("llama-micro"), "model.layers.1.mlp.up_proj.weight", "model.layers.0.self_attn.k_proj.weight"),
    "qwen3": (lambda: _lm("qwen3-micro", "f16"), "model.layers.1.self_attn.k_norm.weight", "model.layers.0.mlp.down_proj.weight"),
    "sensevoice": (_sensevoice, "audio_encoder.tp_encoders.1.self_attn.fsmn_block.weight", "audio_encoder.encoders0.0.self_attn.linear_q_k_v.weight"),
}


def _reversed(a):
    wrong = a.reshape(a.shape[::-1])               # same element count and rank, the axes' sizes reversed
    assert wrong.shape != a.shape
    return wrong


def _refused(fn, *needles):
    with pytest.raises(M.MiaError) as e:
        fn()
    assert e.value.code == M._lib.ERR_INVALID_ARGUMENT, e.value
    for n in needles:
        assert n in str(e.value), (n, str(e.value))


@pytest.mark.parametrize("model", list(DENSE))
def test_loader_names_the_bad_tensor_and_the_context_stays_usable(ctx, model):
    entry, drop, misshape = DENSE[model]
    w, load, run = entry()
    assert drop in w and misshape in w
    _refused(lambda: load(ctx, {k: v for k, v in w.items() if k != drop}), drop, "missing tensor")
    _refused(lambda: load(ctx, {**w, misshape: _reversed(w[misshape])}), misshape, "unexpected shape")
    h = load(ctx, w)                                                   # the context that saw both failures
    got = run(h)
    h.close()
    fresh = M.Context(0)
    h2 = load(fresh, w)
    want = run(h2)
    h2.close()
    fresh.close()
    assert got.size > 0
    np.testing.assert_array_equal(got, want)


# ---- the attach calls: a refused attach leaves the handle as it was, and a later good one is accepted ------------------------------------
def _whisper_attach(bits):
    from mlx_swift_audio_amd import whisper as HW
    dims = S.DIMS["micro"]
    dense, packed = quantised_checkpoint(dims, 49, bits, "bf16")
    return (lambda c: HW.WhisperModel.load(c, dims, dense, M.BF16), packed, lambda h, p: h.attach_quantized(p, bits=bits), lambda h, on: h.use_packed(on),
            _whisper_run, "decoder.blocks.1.cross_attn.out", "decoder.blocks.0.mlp2")


def _lm_attach(name, kind, bits):
    from mlx_swift_audio_amd import lm as HL
    from mlx_swift_audio_amd.checkpoint import quantize_affine
    cfg = S.LM_CONFIGS[name]
    dense, packed = S.lm_weights(cfg, seed=11), {}
    names = ["model.embed_tokens" if cfg.tie_embeddings else "lm_head"]
    for l in range(cfg.n_layers):
        names += [f"model.layers.{l}.self_attn.{n}_proj" for n in "qkvo"] + [f"model.layers.{l}.mlp.{n}_proj" for n in ("gate", "up", "down")]
    for n in names:
        packed[n + ".weight"], packed[n + ".scales"], packed[n + ".biases"] = quantize_affine(dense[n + ".weight"], 64, bits)

    def run(h):
        h.reset()
        return np.concatenate([h.forward([t]).copy() for t in (7, 1, 2999)])

    return (lambda c: HL.CausalLM.load(c, cfg, dense, DT[kind]), packed, lambda h, p: h.attach_q4(p, bits=bits), lambda h, on: h.use_q4(on), run,
            "model.layers.1.mlp.up_proj", "model.layers.0.self_attn.k_proj")


ATTACH = {"whisper-4": lambda: _whisper_attach(4), "llama-4": lambda: _lm_attach("llama-micro", "bf16", 4), "qwen3-8": lambda: _lm_attach("qwen3-micro", "f16", 8)}


@pytest.mark.parametrize("case", list(ATTACH))
def test_refused_attach_leaves_the_handle_and_a_good_one_follows(ctx, case):
    load, packed, attach, use, run, drop, misshape = ATTACH[case]()
    h = load(ctx)
    before = run(h)
    _refused(lambda: attach(h, {k: v for k, v in packed.items() if k != drop + ".biases"}), drop + ".biases", "missing tensor")
    _refused(lambda: attach(h, {**packed, misshape + ".weight": _reversed(packed[misshape + ".weight"])}), "'" + misshape + "'", "expected shape")
    _refused(lambda: use(h, True))                                     # nothing was attached
    np.testing.assert_array_equal(run(h), before)
    attach(h, packed)                                                  # the handle that refused two attaches takes a good one
    use(h, True)
    got = run(h)
    h.close()
    fresh = M.Context(0)
    h2 = load(fresh)
    attach(h2, packed)
    use(h2, True)
    want = run(h2)
    h2.close()
    fresh.close()
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(got, want)


# ---- source dtype: float32, float16 and bf16 payloads of the same values load to the same bits -------------------------------------------
def _as_source(w, kind):
    """The checkpoint as a file of that type holds it: float16 arrays, or uint16 bf16 payloads tagged as checkpoint.read_safetensors tags them."""
    from mlx_swift_audio_amd.checkpoint import Tensor
    if kind == "f16":
        out = {k: v.astype(np.float16) for k, v in w.items()}
    else:
        out = {}
        for k, v in w.items():
            out[k] = (np.ascontiguousarray(v, np.float32).view(np.uint32) >> 16).astype(np.uint16).view(Tensor)
            out[k].st_dtype = "BF16"
    for k, v in w.items():                                             # the values are representable: nothing is rounded away here
        back = out[k].astype(np.float32) if kind == "f16" else (np.asarray(out[k]).astype(np.uint32) << 16).view(np.float32)
        assert np.array_equal(back, v), k
    return out


@pytest.mark.parametrize("kind", ["f16", "bf16"])
@pytest.mark.parametrize("model", ["whisper", "llama", "qwen3"])
def test_source_dtype_does_not_change_the_handle(ctx, model, kind):
    w, load, run = {"whisper": lambda: _whisper(kind), "llama": lambda: _lm("llama-micro", kind), "qwen3": lambda: _lm("qwen3-micro", kind)}[model]()
    h = load(ctx, w)
    want = run(h)
    h.close()
    h = load(ctx, _as_source(w, kind))
    got = run(h)
    h.close()
    assert got.size > 0
    np.testing.assert_array_equal(got, want)


# ---- a uint32 view where a dense weight is expected ---------------------------------------------------------------------------------------
def _views_as_given(tensors):
    """mia_tensor_view array that tags every array by its own dtype (the package's builder converts a uint32 array of a dense load to
    float32 before the library sees it)."""
    from mlx_swift_audio_amd._abi import TensorView
    tag = {np.dtype(np.float32): M.F32, np.dtype(np.uint32): M._lib.U32}
    keep = [np.ascontiguousarray(a) for a in tensors.values()]
    views = (TensorView * len(keep))()
    for i, (name, a) in enumerate(zip(tensors, keep)):
        views[i] = TensorView(name.encode(), tag[a.dtype], a.ndim, (C.c_int64 * 4)(*(list(a.shape) + [0] * (4 - a.ndim))), a.ctypes.data)
    return views, keep


@pytest.mark.parametrize("model", ["whisper", "llama"])
def test_u32_view_is_refused_as_a_dense_weight(ctx, model):
    from mlx_swift_audio_amd import _abi
    if model == "whisper":
        w, name = _whisper()[0], "encoder.blocks.1.attn.out.weight"
        dims = S.DIMS["micro"]
        cfg = _abi.WhisperDims(*[int(getattr(dims, f[0])) for f in _abi.WhisperDims._fields_])
        call = ctx.lib.mia_whisper_load
    else:
        w, name = _lm("llama-micro")[0], "model.layers.1.self_attn.o_proj.weight"
        c = S.LM_CONFIGS["llama-micro"]
        cfg = _abi.LmConfig(c.vocab, c.hidden, c.inter, c.n_layers, c.n_heads, c.n_kv_heads, c.head_dim, c.max_ctx, c.rms_eps, c.rope_theta,
                            1 if c.rope_llama3 else 0, c.rope_factor, c.rope_low, c.rope_high, c.rope_old_ctx, 1 if c.qkv_bias else 0, 1 if c.tie_embeddings else 0)
        call = ctx.lib.mia_lm_load
    views, keep = _views_as_given({**w, name: w[name].view(np.uint32)})
    h = call(ctx.h, C.byref(cfg), views, len(keep), M.BF16)
    msg = ctx.lib.mia_last_error(ctx.h).decode()
    if h:
        (ctx.lib.mia_whisper_free if model == "whisper" else ctx.lib.mia_lm_free)(h)
    assert not h, "a uint32 view was loaded as a dense weight"
    assert "tensor '" + name + "' must be float32, float16 or bfloat16" in msg, msg
