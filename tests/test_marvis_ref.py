"""Marvis on the CPU (no GPU needed): what the GPU implementation relies on is proven on the float64 oracle of tests/_marvis_ref.py --
(a) the interleaved-RoPE stacks equal the row-permuted split-half stacks; (b) the two-row first decoder pass equals two single-row steps;
(c) the Swift-order frequency table agrees with the LM loader's Llama-3 table to a few fp32 ulps, and all three of its bands occur at
head dim 64 and 128; (d) the sampler rule on constructed rows; (e) the row builders against hand-written frames; (f) sanitize_marvis on
the raw key forms; and the derived logit bound of tests/_marvis_cases.py is what the oracle gives."""
import math

import numpy as np
import pytest

import _marvis_cases as MC
import _marvis_ref as R


@pytest.mark.parametrize("name", ["marvis-micro", "marvis-micro128"])
def test_permuted_split_half_and_single_rows_equal_the_literal_model(name):
    cfg, w = MC.config(name), MC.weights(name, "f16")
    lit = MC.forced_run(name, "f16", MC.N_CODEBOOKS)
    for kw in (dict(split_half=True), dict(single_rows=True), dict(split_half=True, single_rows=True)):
        ref = R.MarvisRef(cfg, w, **kw)
        tk, mk = MC.prompt()
        worst = 0.0
        for f in range(3):
            _, lg = ref.generate_frame(MC.N_CODEBOOKS, tk, mk, lambda x, i: 0, MC.FORCED[f])
            worst = max(worst, float(np.abs(lg - lit[f]).max()))
            tk, mk = MC.feedback(MC.FORCED[f])                   # full-width row with mask 0: the same sum as the narrower row
        print(name, kw, "max |delta logit| =", worst)
        assert worst <= 1e-12


def test_permute_rows_is_the_stated_permutation():
    w = np.arange(2 * 8 * 3).reshape(16, 3)
    p = R.permute_rows(w, 2, 8)
    for h in range(2):
        for i in range(4):
            assert (p[h * 8 + i] == w[h * 8 + 2 * i]).all() and (p[h * 8 + i + 4] == w[h * 8 + 2 * i + 1]).all()


def _lm_loader_inv_freq(dh, theta, factor=32.0, low=1.0, high=4.0, old=8192):
    """lm_load.hip's table (Llama3RoPE.swift:41-65 order), float32 operation by operation."""
    f = np.float32
    out = []
    for i in range(dh // 2):
        freq = f(math.pow(theta, 2 * i / dh))
        low_wl, high_wl = f(old) / f(low), f(old) / f(high)
        wl = f(2.0) * f(math.pi) * freq
        v = freq * f(factor) if wl > low_wl else freq
        if high_wl < wl < low_wl:
            smooth = (f(old) / wl - f(low)) / (f(high) - f(low))
            v = v / ((f(1.0) - smooth) / f(factor) + smooth)
        out.append(f(1.0) / v)
    return np.array(out, np.float32)


@pytest.mark.parametrize("dh", [64, 128])
def test_swift_order_frequencies(dh):
    th = R.swift_inv_freq(dh, 500000.0)
    ours = _lm_loader_inv_freq(dh, 500000.0)
    gap = np.abs(th.astype(np.float64) - ours) / np.spacing(np.abs(ours)).astype(np.float64)
    print(f"head dim {dh}: largest gap between the Swift-order and the loader's table = {gap.max():.1f} fp32 ulps")
    assert gap.max() <= 8
    bands = R.rope_bands(dh, 500000.0)
    assert min(bands) >= 1 and sum(bands) == dh // 2, bands        # unscaled, blended and divided frequencies all occur
    assert not np.allclose(th, R.swift_inv_freq(dh, 500000.0, None))


def test_micro_configs_use_the_real_scaling_constants():
    from mlx_swift_audio_amd import marvis
    for name in ("marvis-micro", "marvis-micro128"):
        cfg = MC.config(name)
        assert cfg.rope_scaling == R.ROPE == marvis._ROPE_LLAMA3
        assert (cfg.audio_vocab, cfg.n_codebooks, cfg.text_vocab, cfg.max_ctx) == (67, 5, 300, 96)
    assert MC.config("marvis-micro").decoder.head_dim == 64 and MC.config("marvis-micro128").decoder.head_dim == 128
    w = MC.weights("marvis-micro", "f16")
    assert np.abs(w["audio_embeddings.weight"][0]).max() > 0 and np.abs(w["text_embeddings.weight"][0]).max() > 0
    assert MC.forced_run("marvis-micro", "f16", 5).std(-1).min() > 1.0          # heads with a usable spread


EXPECT = {"ties, half kept": (2, [2, 3]), "ties, half kept, other pick": (3, [2, 3]), "cumulative exactly at 1 - top_p": (1, [1, 2, 3]),
          "top_p = 1": (8, [0, 2, 3, 5, 8, 9, 10, 11]), "top_p = 1 keeps no zero": (0, [0, 2, 3, 5, 8, 9, 10, 11]),
          "tiny top_p keeps the largest": (3, [3]), "NaN ranks lowest": (0, [0, 2, 3, 4]), "NaN, half kept": (4, [3, 4]),
          "u just below 1": (11, [8, 9, 10, 11]), "u = 0": (8, [8, 9, 10, 11]), "V 2051": (2050, [900, 2050]),
          "V 8192": (8186, list(range(8184, 8192)))}


def test_sampler_rule_on_constructed_rows():
    rows = MC.sampler_rows()
    assert {r[0] for r in rows} == set(EXPECT)
    for label, x, t, p, u in rows:
        got, kept, _ = R.sample_top_p_ascending(x, t, p, u)
        assert (got, list(kept)) == EXPECT[label], (label, got, list(kept))


def test_row_builders_against_hand_written_frames():
    from mlx_swift_audio_amd import marvis
    rows, mask = marvis.tokenize_text_rows([9, 4], 3)
    assert rows.tolist() == [[0, 0, 0, 9], [0, 0, 0, 4]] and mask.tolist() == [[0, 0, 0, 1], [0, 0, 0, 1]]
    codes = [[1, 2], [3, 4], [5, 6]]
    rows, mask = marvis.tokenize_audio_rows(codes, add_eos=True)
    assert rows.tolist() == [[1, 3, 5, 0], [2, 4, 6, 0], [0, 0, 0, 0]] and mask.tolist() == [[1, 1, 1, 0]] * 3
    rows, mask = marvis.tokenize_audio_rows(codes, add_eos=False)
    assert rows.tolist() == [[1, 3, 5, 0], [2, 4, 6, 0]]
    rows, mask = marvis.tokenize_start([9, 4], codes)
    assert rows.tolist() == [[0, 0, 0, 9], [0, 0, 0, 4], [1, 3, 5, 0], [2, 4, 6, 0]]
    assert mask.tolist() == [[0, 0, 0, 1], [0, 0, 0, 1], [1, 1, 1, 0], [1, 1, 1, 0]]
    assert rows.dtype == np.int32 and mask.dtype == np.int32
    assert marvis.QUALITY_CODEBOOKS == {"low": 8, "medium": 16, "high": 24, "maximum": 32} and marvis.MAX_AUDIO_FRAMES == 750


def test_sanitize_marvis_on_the_raw_key_forms():
    from mlx_swift_audio_amd.checkpoint import sanitize_marvis
    raw = ["model.backbone.layers.0.attn.q_proj.weight", "model.backbone.layers.0.attn.output_proj.weight", "model.decoder.layers.3.mlp.w1.weight",
           "model.decoder.layers.3.mlp.w2.weight", "model.decoder.layers.3.mlp.w3.weight", "model.backbone.layers.1.sa_norm.scale",
           "model.backbone.layers.1.mlp_norm.scale", "model.backbone.norm.scale", "model.decoder.norm.scale", "model.text_embeddings.weight",
           "model.audio_head", "backbone.layers.0.self_attn.k_proj.weight", "model.codebook0_head.weight", "model.projection.weight"]
    want = ["backbone.layers.0.self_attn.q_proj.weight", "backbone.layers.0.self_attn.o_proj.weight", "decoder.layers.3.mlp.gate_proj.weight",
            "decoder.layers.3.mlp.down_proj.weight", "decoder.layers.3.mlp.up_proj.weight", "backbone.layers.1.input_layernorm.weight",
            "backbone.layers.1.post_attention_layernorm.weight", "backbone.norm.weight", "decoder.norm.weight", "text_embeddings.weight",
            "audio_head", "backbone.layers.0.self_attn.k_proj.weight", "codebook0_head.weight", "projection.weight"]
    assert sanitize_marvis(raw) == want
    a = np.ones(3, np.float32)
    assert list(sanitize_marvis({"model.backbone.norm.scale": a})) == ["backbone.norm.weight"]
    cfg = MC.config("marvis-micro")
    assert sorted(sanitize_marvis(list(MC.weights("marvis-micro", "f16")))) == sorted(MC.weights("marvis-micro", "f16"))      # sanitised keys are fixed points
    assert len(MC.weights("marvis-micro", "f16")) == 2 * (9 * cfg.backbone.layers + 1) + 5


def test_config_forms():
    from mlx_swift_audio_amd import marvis
    c = marvis.MarvisConfig.from_flavors()
    assert (c.backbone.hidden, c.backbone.layers, c.backbone.heads, c.backbone.kv_heads, c.backbone.head_dim) == (2048, 16, 32, 8, 64)
    assert (c.decoder.hidden, c.decoder.layers, c.decoder.heads, c.decoder.kv_heads, c.decoder.head_dim) == (1024, 4, 8, 2, 128)
    stack = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64)
    j = dict(stack, text_vocab_size=300, audio_vocab_size=67, audio_num_codebooks=5, max_position_embeddings=96,
             rope_scaling={"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192, "rope_type": "llama3"},
             depth_decoder_config=dict(stack, hidden_size=128, intermediate_size=384, num_attention_heads=2, num_key_value_heads=1))
    assert marvis.MarvisConfig.from_json(j) == MC.config("marvis-micro")
    assert marvis.MarvisConfig.from_json(dict(text_vocab_size=128256, audio_vocab_size=2051, audio_num_codebooks=32, backbone_flavor="llama-1B",
                                              decoder_flavor="llama-100M")) == c


@pytest.mark.parametrize("name,dtype", sorted(MC.DERIVED))
def test_derived_logit_bound_is_what_the_oracle_gives(name, dtype):
    got = MC.derived_bound(name, dtype)
    print(f"{name} {dtype}: 4 x (float64 run - rounded-activation run) / std = {got:.4f}; table {MC.DERIVED[(name, dtype)]}; chain bound {MC.TOL[dtype]}")
    assert abs(got - MC.DERIVED[(name, dtype)]) <= 2e-4
