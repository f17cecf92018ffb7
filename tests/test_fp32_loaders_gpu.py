"""The host plumbing the fp32 models share (csrc/tensor_loader.h, mia_grow): every loader reports a missing or mis-shaped tensor by
name and leaves the context usable, and a handle's grow-only buffers give the same bits after growing and when reused at a smaller
size (stale contents behind the valid rows) as a fresh handle does.  Micro configurations only; everything is compared bit for bit."""
import numpy as np
import pytest

import mlx_swift_audio_amd as M
from mlx_swift_audio_amd import synthetic as S

pytestmark = pytest.mark.gpu


# ---- one entry per loader: (weights, load(ctx, weights), run(handle) -> array, tensor to drop, tensor to mis-shape) -------------------------
def _snac():
    from mlx_swift_audio_amd import codec as HC
    cfg = S.SNAC_CONFIGS["snac_micro"]
    codes = _snac_codes(cfg, 5, 1)
    return (S.snac_weights(cfg, 3), lambda c, w: HC.SNACDecoder.load(c, cfg, w), lambda h: h.decode(codes, _snac_noise(h, cfg, 5, 2)),
            "decoder.model.layers.2.block.layers.2.linear.weight_g", "decoder.model.layers.2.block.layers.1.weight_v")


def _dac_weights(encoder):
    cfg = S.DAC_CONFIGS["dac_micro"]
    w = S.dac_weights(cfg, 4)
    return cfg, w if encoder else {k: v for k, v in w.items() if not k.startswith("encoder.")}


def _dac():
    from mlx_swift_audio_amd import codec as HC
    cfg, w = _dac_weights(False)
    codes = np.random.default_rng(1).integers(0, cfg.codebook_size, (cfg.n_codebooks, 9))
    return (w, lambda c, ww: HC.DACCodec.load(c, cfg, ww), lambda h: h.decode_from_codes(codes),
            "decoder.model.layers.2.block.layers.3.block.layers.2.alpha", "decoder.model.layers.1.block.layers.1.weight_v")


def _dac_encoder():
    from mlx_swift_audio_amd import codec as HC
    cfg, w = _dac_weights(True)
    audio = np.random.default_rng(2).standard_normal(203).astype(np.float32) * 0.3
    return (w, lambda c, ww: HC.DACCodec.load(c, cfg, ww), lambda h: h.encode(audio),
            "encoder.block.layers.1.block.layers.3.alpha", "encoder.block.layers.1.block.layers.4.weight_v")


def _hift():
    from mlx_swift_audio_amd import hift as HH
    cfg = S.HIFT_CONFIGS["hift_micro"]
    mel, noise = _hift_inputs(cfg, 3)
    return (S.hift_weights(cfg), lambda c, w: HH.HiFTGenerator.load(c, cfg, w), lambda h: np.concatenate(h(mel, noise=noise)),
            "source_resblocks.1.activations2.0.alpha", "ups.1.weight")


def _s3():
    from mlx_swift_audio_amd import s3tok as HS
    cfg = S.S3_CONFIGS["s3_micro"]
    mel = _s3_mel(cfg, 37)
    return (S.s3_weights(cfg, 2), lambda c, w: HS.S3Tokenizer.load(c, cfg, w), lambda h: _flat(h.quantize(mel, [37])),
            "encoder.blocks.1.attn.out.bias", "encoder.blocks.1.attn.fsmn_block.weight")


def _flow():
    from mlx_swift_audio_amd import flow as HF
    cfg = S.FLOW_CONFIGS["flow_micro"]
    rng = np.random.default_rng(3)
    tok, ptok = rng.integers(0, cfg.vocab_size, 5).astype(np.int32), rng.integers(0, cfg.vocab_size, 2).astype(np.int32)
    pf, emb = rng.standard_normal((3, 80)).astype(np.float32), rng.standard_normal(cfg.spk_embed_dim).astype(np.float32)
    z = rng.standard_normal((80, 14)).astype(np.float32)
    return (S.flow_weights(cfg), lambda c, w: HF.FlowModule.load(c, cfg, w), lambda h: h.inference(tok, ptok, pf, emb, z, n_timesteps=2),
            "encoder.up_encoders.0.self_attn.pos_bias_v", "decoder.estimator.down_blocks.0.resnet.mlp_linear.weight")


def _campplus():
    from mlx_swift_audio_amd import speaker as SP
    feats = (np.random.default_rng(4).standard_normal((9, 80)) * 2.0).astype(np.float32)
    return (S.campplus_weights(7), SP.CAMPlusSpeakerEncoder.load, lambda h: h.forward(feats),
            "blocks.1.layers.3.nonlinear2.0.running_var", "blocks.1.layers.3.cam_layer.linear_local.weight")


LOADERS = {"snac": _snac, "dac": _dac, "dac_encoder": _dac_encoder, "hift": _hift, "s3tok": _s3, "flow": _flow, "campplus": _campplus}


@pytest.mark.parametrize("model", list(LOADERS))
def test_loader_names_the_bad_tensor_and_the_context_stays_usable(ctx, model):
    w, load, run, drop, misshape = LOADERS[model]()
    assert drop in w and misshape in w
    with pytest.raises(M.MiaError) as e:
        load(ctx, {k: v for k, v in w.items() if k != drop})
    assert drop in str(e.value) and "missing tensor" in str(e.value)
    wrong = w[misshape].reshape(w[misshape].shape[::-1])               # same element count and rank, the axes' sizes reversed
    assert wrong.shape != w[misshape].shape
    with pytest.raises(M.MiaError) as e:
        load(ctx, {**w, misshape: wrong})
    assert misshape in str(e.value) and "unexpected shape" in str(e.value)
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


# ---- grow rule: short -> long (reallocation) -> short (the larger buffer reused, stale contents behind the valid rows) -----------------------
def _snac_codes(cfg, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, cfg.codebook_size, n * (cfg.vq_strides[0] // s)).tolist() for s in cfg.vq_strides]


def _snac_noise(dec, cfg, n, seed):
    return np.random.default_rng(seed).standard_normal(dec.noise_len(n * cfg.vq_strides[0])).astype(np.float32)


def _hift_inputs(cfg, T):
    rng = np.random.default_rng(10 + T)
    return ((rng.standard_normal((cfg.in_channels, T)) * 1.5 - 2).astype(np.float32),
            rng.standard_normal((T * 480, cfg.nb_harmonics + 1)).astype(np.float32))


def _flat(arrays):
    return np.concatenate([np.asarray(a).reshape(-1) for a in arrays])


def _s3_mel(cfg, T):
    return np.random.default_rng(20 + T).standard_normal((1, cfg.n_mels, T)).astype(np.float32)


def _assert_grow_rule(load, run, sizes):
    """run(handle, size) on ONE handle through `sizes` must give, call by call, what a fresh handle gives for that size."""
    h = load()
    got = [run(h, n) for n in sizes]
    h.close()
    for n, g in zip(sizes, got):
        f = load()
        want = run(f, n)
        f.close()
        assert g.size > 0
        np.testing.assert_array_equal(g, want, err_msg=f"size {n} in the sequence {sizes}")


def test_grow_rule_snac_decode_with_noise(ctx):
    from mlx_swift_audio_amd import codec as HC
    cfg = S.SNAC_CONFIGS["snac_micro"]
    w = S.snac_weights(cfg, 3)
    _assert_grow_rule(lambda: HC.SNACDecoder.load(ctx, cfg, w), lambda h, n: h.decode(_snac_codes(cfg, n, n), _snac_noise(h, cfg, n, n)), (3, 9, 3))


def test_grow_rule_dac_decode(ctx):
    from mlx_swift_audio_amd import codec as HC
    cfg, w = _dac_weights(False)
    codes = lambda n: np.random.default_rng(n).integers(0, cfg.codebook_size, (cfg.n_codebooks, n))
    _assert_grow_rule(lambda: HC.DACCodec.load(ctx, cfg, w), lambda h, n: h.decode_from_codes(codes(n)), (4, 12, 4))


def test_grow_rule_dac_encode(ctx):
    from mlx_swift_audio_amd import codec as HC
    cfg, w = _dac_weights(True)
    audio = lambda n: np.random.default_rng(n).standard_normal(n).astype(np.float32) * 0.3
    _assert_grow_rule(lambda: HC.DACCodec.load(ctx, cfg, w), lambda h, n: h.encode(audio(n)), (64, 403, 64))


def test_grow_rule_s3_encode(ctx):
    from mlx_swift_audio_amd import s3tok as HS
    cfg = S.S3_CONFIGS["s3_micro"]
    w = S.s3_weights(cfg, 2)
    _assert_grow_rule(lambda: HS.S3Tokenizer.load(ctx, cfg, w), lambda h, T: _flat(h.quantize(_s3_mel(cfg, T), [T])), (19, 61, 19))


def test_grow_rule_hift_vocode(ctx):
    from mlx_swift_audio_amd import hift as HH
    cfg = S.HIFT_CONFIGS["hift_micro"]
    w = S.hift_weights(cfg)

    def run(h, T):
        mel, noise = _hift_inputs(cfg, T)
        return np.concatenate(h(mel, noise=noise))

    _assert_grow_rule(lambda: HH.HiFTGenerator.load(ctx, cfg, w), run, (2, 7, 2))
