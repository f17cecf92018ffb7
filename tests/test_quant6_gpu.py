"""Packed 6-bit weights on the GPU below Marvis: the load-time de-quantiser (mia_dequant_affine, bits 6) against the numpy restatement
of the storage rule (tests/_quant6.py), and the LM step on 6-bit codes (mia_lm_attach_quantized, bits 6) -- the 4- / 8-bit tests of
tests/test_lm_gpu.py at the new width, with the project's own bounds (they bound the 16-bit rounding, not the code width)."""
import numpy as np
import pytest

import _quant6 as Q6
import _skinny_ref as ref
from mlx_swift_audio_amd import synthetic as S
from oracle import lm as OL

pytestmark = pytest.mark.gpu


def _dt(name):
    import mlx_swift_audio_amd as m
    return m.BF16 if name == "bf16" else m.F16


# ---- de-quantiser ----------------------------------------------------------------------------------------------------------------------
def _scales(rng, shape, sdt):
    from mlx_swift_audio_amd import audio
    s, b = rng.uniform(0.01, 0.1, shape).astype(np.float32), rng.uniform(-2, 2, shape).astype(np.float32)
    if sdt == "f16":
        s, b = s.astype(np.float16), b.astype(np.float16)
        return s, b, s.astype(np.float32), b.astype(np.float32)
    if sdt == "bf16":
        s, b = audio.f32_to_bf16(s), audio.f32_to_bf16(b)
        return s, b, audio.bf16_to_f32(s), audio.bf16_to_f32(b)
    return s, b, s, b


@pytest.mark.parametrize("cols", [64, 192])
@pytest.mark.parametrize("sdt", ["f32", "f16", "bf16"])
def test_dequant6_matches_numpy(ctx, cols, sdt):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import checkpoint as CK
    rng = np.random.default_rng(cols)
    rows = 3
    q = rng.integers(0, 64, (rows, cols))
    q[0, :64] = np.arange(64)                                      # every code value, every position of a 16-code triple
    wq = Q6.pack6(q)
    s, b, s32, b32 = _scales(rng, (rows, cols // 64), sdt)
    want = Q6.dequant6(wq, s32, b32)
    got = CK.dequantize_affine(ctx, wq, s, b, 64, 6)
    assert got.shape == (rows, cols) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6)       # one fma vs mul + add (the 4- / 8-bit test's comparison)
    # the 16-bit outputs: that fp32 value rounded once more -- half an ulp of the type at it
    tag = {"f32": m._lib.F32, "f16": m._lib.F16, "bf16": m._lib.BF16}
    for odt in ("f16", "bf16"):
        out = np.full((rows + 1, cols), 0x7777, np.uint16)
        ctx.check(ctx.lib.mia_dequant_affine(ctx.h, wq.ctypes.data, s.ctypes.data, b.ctypes.data, rows, cols, 64, 6, tag[sdt], out.ctypes.data, tag[odt], m._lib.MEM_HOST))
        assert (out[rows] == 0x7777).all()
        val = ref.load16(out[:rows].view(np.float16) if odt == "f16" else out[:rows], tag[odt])
        tol = 1e-6 + 1e-6 * np.abs(want)
        assert (np.abs(val - want) <= tol + ref.half_ulp16(np.abs(want) + tol, tag[odt])).all(), odt
    # expand_checkpoint infers the width from the packed shape
    dense = CK.expand_checkpoint(ctx, {"x.weight": wq, "x.scales": s, "x.biases": b, "y.weight": np.ones((2, 2), np.float32)})
    assert set(dense) == {"x.weight", "y.weight"}
    np.testing.assert_array_equal(dense["x.weight"], got)


def test_dequant_refuses_odd_widths_and_ragged_6_bit_rows(ctx):
    import mlx_swift_audio_amd as m
    wq, s, out = np.zeros((2, 12), np.uint32), np.ones((2, 1), np.float32), np.zeros((2, 64), np.float32)
    call = lambda cols, group, bits: ctx.lib.mia_dequant_affine(ctx.h, wq.ctypes.data, s.ctypes.data, s.ctypes.data, 2, cols, group, bits, m._lib.F32,
                                                               out.ctypes.data, m._lib.F32, m._lib.MEM_HOST)
    for bits in (3, 5, 7):
        assert call(64, 64, bits) == m._lib.ERR_INVALID_ARGUMENT
    assert call(32, 32, 6) == m._lib.ERR_INVALID_ARGUMENT          # 6-bit rows are whole groups of 64
    assert call(64, 64, 6) == 0


def test_whisper_still_refuses_6_bits(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import checkpoint as CK, whisper as HW
    dims = S.DIMS["micro.en"]
    w = S.synthetic_weights(dims, seed=5)
    model = HW.WhisperModel.load(ctx, dims, w, m.F16)
    packed = {}
    for k, v in w.items():
        if k.startswith("decoder.") and k.endswith(".weight") and v.ndim == 2 and v.shape[1] % 64 == 0:
            packed[k], packed[k[:-7] + ".scales"], packed[k[:-7] + ".biases"] = CK.quantize_affine(v, 64, 6, np.float16)
    assert packed
    with pytest.raises(m.MiaError) as e:
        model.attach_quantized(packed, bits=6)
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
    with pytest.raises(m.MiaError):
        model.use_packed(True)
    model.close()


# ---- the LM step -------------------------------------------------------------------------------------------------------------------------
def _quantized_checkpoint6(cfg, seed, scale_dtype=np.float16):
    """tests/test_lm_gpu.py's _quantized_checkpoint at 6 bits: every step Linear (and the tied embedding) quantised, the packing and the
    de-quantisation by tests/_quant6.py"""
    from mlx_swift_audio_amd import checkpoint as CK
    w = S.lm_weights(cfg, seed=seed)
    packed, dense = {}, dict(w)
    names = ["model.embed_tokens"] if cfg.tie_embeddings else ["lm_head"]
    for l in range(cfg.n_layers):
        p = f"model.layers.{l}"
        names += [p + ".self_attn." + n + "_proj" for n in "qkvo"] + [p + ".mlp." + n + "_proj" for n in ("gate", "up", "down")]
    for n in names:
        pk, sc, bi = CK.quantize_affine(w[n + ".weight"], 64, 6, scale_dtype)
        np.testing.assert_array_equal(pk, Q6.pack6(Q6.unpack6(pk)))
        packed[n + ".weight"], packed[n + ".scales"], packed[n + ".biases"] = pk, sc, bi
        dense[n + ".weight"] = Q6.dequant6(pk, sc.astype(np.float32), bi.astype(np.float32)).astype(np.float32)
    return packed, dense


@pytest.mark.parametrize("cfg_name,dtype_name", [("llama-micro128", "bf16"), ("qwen-micro", "f16")])
def test_packed6_step_matches_oracle_and_expanded_checkpoint(ctx, cfg_name, dtype_name):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = S.LM_CONFIGS[cfg_name]
    packed, dense = _quantized_checkpoint6(cfg, seed=11)
    model = HL.CausalLM.load(ctx, cfg, dense, _dt(dtype_name))
    ids = np.random.default_rng(2).integers(0, cfg.vocab, 9).tolist()
    model.attach_q4(packed, bits=6)
    with pytest.raises(m.MiaError):
        model.attach_q4(packed, bits=6)             # one attach per handle
    model.use_q4(False)                             # the 16-bit weights of the same handle (same cross-workgroup splits)
    ref_steps = [model.forward([t]).copy() for t in ids]
    model.use_q4(True)
    model.reset()
    q_steps = [model.forward([t]).copy() for t in ids]
    ora = OL.LMOracle(cfg, dense)                   # fp32 de-quantised weights, NOT rounded to 16 bit
    want = ora.forward(ids).numpy()
    for i, (got, w16) in enumerate(zip(q_steps, ref_steps)):
        sd = want[i].std()
        assert np.isfinite(got).all()
        print(f"step {i}: packed vs 16-bit {np.abs(got - w16).max() / sd:.4f}, packed vs oracle {np.abs(got - want[i]).max() / sd:.4f} of the logit std")
        assert np.abs(got - w16).max() <= (0.06 if dtype_name == "bf16" else 0.01) * sd, (i, np.abs(got - w16).max(), sd)
        assert np.abs(got - want[i]).max() <= (0.08 if dtype_name == "bf16" else 0.02) * sd, (i, np.abs(got - want[i]).max(), sd)
    # batched: sequence b of a batch equals its own single-sequence run; prompts token by token through the packed step
    model.set_debug(2)
    model.set_batch(4)
    prompts = [ids, ids[:3], ids[2:], ids[::-1]]
    ub = np.random.default_rng(5).random((4, 12)).astype(np.float32)
    kw = dict(temperature=0.7, top_p=0.9, rep_penalty=1.2, rep_window=16, max_new_tokens=12, stop_ids=(cfg.vocab - 1,))
    qa = model.generate_batch(prompts, ub, **kw)
    model.set_batch(1)
    for b, pr in enumerate(prompts):
        assert model.generate(pr, ub[b], **kw) == qa[b], b
    model.close()
    # an incomplete tensor set is rejected and leaves the handle on its 16-bit weights
    fresh = HL.CausalLM.load(ctx, cfg, dense, _dt(dtype_name))
    before = fresh.forward(ids[:1]).copy()
    fresh.reset()
    with pytest.raises(m.MiaError):
        fresh.attach_q4({k: v for k, v in packed.items() if "q_proj" not in k}, bits=6)
    with pytest.raises(m.MiaError):
        fresh.use_q4(True)
    assert np.array_equal(fresh.forward(ids[:1]), before)
    for bits in (3, 5, 7):
        with pytest.raises(m.MiaError):
            fresh.attach_q4(packed, bits=bits)
    fresh.close()


def test_packed6_step_mid_size_batch_32(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import lm as HL
    cfg = S.LM_CONFIGS["llama-q4mid"]
    packed, dense = _quantized_checkpoint6(cfg, seed=21)
    model = HL.CausalLM.load(ctx, cfg, dense, m.BF16)
    model.attach_q4(packed, bits=6)
    rng = np.random.default_rng(6)
    ids = rng.integers(0, cfg.vocab, 12).tolist()
    model.use_q4(False)
    want = [model.forward([t]).copy() for t in ids]
    model.use_q4(True)
    model.reset()
    oracle = OL.LMOracle(cfg, dense).forward(ids).numpy()
    for i, (t, w_) in enumerate(zip(ids, want)):
        got = model.forward([t])
        sd = oracle[i].std()
        assert np.isfinite(got).all() and np.abs(got - w_).max() <= 0.06 * sd, (i, np.abs(got - w_).max(), sd)
        assert np.abs(got - oracle[i]).max() <= 0.08 * sd, (i, np.abs(got - oracle[i]).max(), sd)
    model.set_debug(2)              # prompts token by token through the packed step
    model.set_batch(32)
    prompts = [rng.integers(0, cfg.vocab, int(n)).tolist() for n in rng.integers(1, 20, 32)]
    ub = rng.random((32, 16)).astype(np.float32)
    kw = dict(temperature=0.8, top_p=0.9, rep_penalty=1.1, rep_window=8, max_new_tokens=16, stop_ids=(cfg.vocab - 1,))
    q = model.generate_batch(prompts, ub, **kw)
    assert all(0 <= t < cfg.vocab for seq in q for t in seq)
    for b in (0, 7, 31):            # rows of a 32-row batch (both MFMA halves) equal the single-sequence (M16) kernel's ids on the same capacity
        assert model.generate(prompts[b], ub[b], **kw) == q[b], b
    model.close()
