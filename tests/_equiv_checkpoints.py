"""Function-preserving checkpoint transforms (test infrastructure for tests/test_norm_carry_gpu.py).

Three hot paths hand a not-yet-normalised 16-bit operand x * gamma from one GEMM to the next and finish the norm in the consumer's
epilogue (LM step: SK_RESID; Whisper decode step: fused_ln; Whisper encoder: the ln_out epilogue).  The synthetic checkpoints keep
that operand O(1) with a zero row mean.  The transforms here rewrite a checkpoint into one that computes the SAME function in exact
arithmetic while moving the operand's magnitude or mean:

  residual scale s = 2^k   every tensor that writes the residual stream x s (norms are scale-invariant up to eps; the Whisper tied
                           head is compensated through decoder.ln / s, the LM uses an untied head)
  gain scale G = 2^g       gamma (and beta) of a carried norm x G, the consuming Linear's weight / G
  row shift c              c added to every channel of decoder.positional_embedding: each LayerNorm removes it, the residual keeps it
The Whisper encoder has no exact residual scale (the conv stem's GELU is not homogeneous): there the residual writers of the blocks
are scaled and only the oracle of the transformed checkpoint is the reference.

Everything is derived from oracle measurements (taps in oracle/lm.py and oracle/whisper.py); nothing here touches the GPU."""
import dataclasses
import math

import numpy as np

from mlx_swift_audio_amd import synthetic as S

F16_MAX = 65504.0
G_MAX = 32.0            # larger gain scales push the divided consumer weights into f16 subnormals in bulk


def pow2_floor(x):
    return 2.0 ** math.floor(math.log2(x))


def pow2_ceil(x):
    return 2.0 ** math.ceil(math.log2(x))


def round_weights(w, kind):
    return {k: S.round_array(v, kind) for k, v in w.items()}


def all_finite_in(w, kind):
    """Every tensor finite after rounding to the storage type `kind`."""
    return all(np.isfinite(S.round_array(v, kind)).all() for v in w.values())


def operand_rows(taps, weights):
    """taps: [(norm name, residual [..., D])] from an oracle run -> {norm name: per-row largest |x * gamma|} (rows concatenated)."""
    out = {}
    for name, x in taps:
        g = np.asarray(weights[name + ".weight"], np.float32)
        v = np.abs(x.numpy().reshape(-1, x.shape[-1]) * g).max(axis=1)
        out[name] = np.concatenate([out[name], v]) if name in out else v
    return out


def split_scale(f, scaled_tensors):
    """A wanted operand factor f = 2^n -> (s, G): as much as the residual writers can take while staying finite in f16, the rest as gain."""
    s_cap = pow2_floor(F16_MAX / max(float(np.abs(t).max()) for t in scaled_tensors))
    s = min(f, s_cap)
    return s, f / s


# ---- causal LM ------------------------------------------------------------------------------------------------------------------------
def lm_untied(cfg):
    return dataclasses.replace(cfg, tie_embeddings=False)


def lm_residual_writers(cfg):
    names = ["model.embed_tokens.weight"]
    for l in range(cfg.n_layers):
        names += [f"model.layers.{l}.self_attn.o_proj.weight", f"model.layers.{l}.mlp.down_proj.weight"]
    return names


def lm_carried_norms(cfg):
    """(norm, consuming Linear weights) of every hand-over of the fused step: o-proj -> post_attention_layernorm -> gate | up,
    down-proj -> the next input_layernorm -> q | k | v (or model.norm -> the head)."""
    out = []
    for l in range(cfg.n_layers):
        p = f"model.layers.{l}"
        out.append((p + ".post_attention_layernorm", [p + ".mlp.gate_proj.weight", p + ".mlp.up_proj.weight"]))
        if l + 1 < cfg.n_layers:
            q = f"model.layers.{l + 1}"
            out.append((q + ".input_layernorm", [q + ".self_attn." + n + "_proj.weight" for n in "qkv"]))
    out.append(("model.norm", ["lm_head.weight"]))
    return out


def lm_transform(cfg, w, s=1.0, G=1.0):
    assert not cfg.tie_embeddings
    out = {k: np.array(v, np.float32) for k, v in w.items()}
    for n in lm_residual_writers(cfg):
        out[n] = out[n] * np.float32(s)
    for norm, consumers in lm_carried_norms(cfg):
        out[norm + ".weight"] = out[norm + ".weight"] * np.float32(G)
        for n in consumers:
            out[n] = out[n] / np.float32(G)
    return out


def lm_run(ora_cls, cfg, w, id_lists):
    """Oracle logits of the calls in id_lists (one cache) and the hand-over residuals."""
    ora = ora_cls(cfg, w)
    ora.taps = []
    logits = np.concatenate([ora.forward(ids).numpy() for ids in id_lists])
    return logits, ora.taps


def layer_of(norm_name, n_layers):
    """The decoder / LM layer whose residual-writing projection stores this norm's operand."""
    if norm_name in ("model.norm",):
        return n_layers - 1
    l = int(norm_name.split(".")[2])
    return l - 1 if norm_name.endswith("input_layernorm") else l


def check_variant_position(variant, rows, n_layers):
    """The variant table of the issue, on oracle measurements: rows = {norm: per-row largest |x gamma|}."""
    top = max(float(v.max()) for v in rows.values())
    if variant == "near":
        assert 0.25 * F16_MAX <= top <= 0.5 * F16_MAX, top
    elif variant == "over":
        per_layer = {}
        for name, v in rows.items():
            l = layer_of(name, n_layers)
            per_layer[l] = max(per_layer.get(l, 0.0), float(v.min()))
        assert sorted(per_layer) == list(range(n_layers)) and min(per_layer.values()) >= 2 * F16_MAX, per_layer
    return top


def lm_variant(ora_cls, cfg, base, variant, id_lists):
    """base: untied checkpoint already rounded to the storage type.  Returns (transformed fp32 tensors -- NOT yet rounded --, info)."""
    base_logits, taps = lm_run(ora_cls, cfg, base, id_lists)
    rows = operand_rows(taps, base)
    writers = [base[n] for n in lm_residual_writers(cfg)]
    if variant == "near":
        f = pow2_floor(0.5 * F16_MAX / max(float(v.max()) for v in rows.values()))
        s, G = split_scale(f, writers)
    elif variant == "over":
        # per layer the better of its two hand-overs must clear 2 x 65504 in its weakest row
        need = {}
        for name, v in rows.items():
            l = layer_of(name, cfg.n_layers)
            need[l] = max(need.get(l, 0.0), float(v.min()))
        f = pow2_ceil(2 * F16_MAX / min(need.values()))
        s, G = split_scale(f, writers)
    elif variant == "down":
        G, s = 1.0, None
        for k in range(1, 40):
            lg, _ = lm_run(ora_cls, cfg, lm_transform(cfg, base, 2.0 ** -k), id_lists)
            if lg.std() < 0.5 * base_logits.std():
                break
            s = 2.0 ** -k
        assert s is not None
    else:
        raise ValueError(variant)
    assert G <= G_MAX, (s, G)
    return lm_transform(cfg, base, s, G), {"s": s, "G": G, "base_logits": base_logits}


# ---- Whisper --------------------------------------------------------------------------------------------------------------------------
def whisper_decoder_transform(dims, w, s=1.0, G=1.0, c=0.0):
    out = {k: np.array(v, np.float32) for k, v in w.items()}
    s32, G32 = np.float32(s), np.float32(G)
    out["decoder.token_embedding.weight"] *= s32
    out["decoder.positional_embedding"] = out["decoder.positional_embedding"] * s32 + np.float32(c)
    out["decoder.ln.weight"] /= s32
    out["decoder.ln.bias"] /= s32
    for l in range(dims.n_text_layer):
        p = f"decoder.blocks.{l}"
        for n in ("attn.out", "cross_attn.out", "mlp2"):
            out[f"{p}.{n}.weight"] *= s32
            out[f"{p}.{n}.bias"] *= s32
        for ln, lin in (("cross_attn_ln", "cross_attn.query"), ("mlp_ln", "mlp1")):
            out[f"{p}.{ln}.weight"] *= G32
            out[f"{p}.{ln}.bias"] *= G32
            out[f"{p}.{lin}.weight"] /= G32
    return out


def whisper_decoder_writers(dims, w):
    t = [w["decoder.token_embedding.weight"], w["decoder.positional_embedding"]]
    for l in range(dims.n_text_layer):
        for n in ("attn.out", "cross_attn.out", "mlp2"):
            t += [w[f"decoder.blocks.{l}.{n}.weight"], w[f"decoder.blocks.{l}.{n}.bias"]]
    return t


def whisper_encoder_transform(dims, w, s=1.0, G=1.0):
    """NOT function-preserving in s (see the module docstring): conv2 and the blocks' residual writers x s, mlp_ln gain x G with
    mlp1 / G.  conv2 goes along so that the stem's (mel-dependent) share of the residual keeps its proportion: scaling the blocks alone
    drowns it and two mels' features then differ by a third of what they differ on the base checkpoint (0.32 measured, 1.02 with conv2)."""
    out = {k: np.array(v, np.float32) for k, v in w.items()}
    s32, G32 = np.float32(s), np.float32(G)
    out["encoder.conv2.weight"] *= s32
    out["encoder.conv2.bias"] *= s32
    for l in range(dims.n_audio_layer):
        p = f"encoder.blocks.{l}"
        for n in ("attn.out", "mlp2"):
            out[f"{p}.{n}.weight"] *= s32
            out[f"{p}.{n}.bias"] *= s32
        out[f"{p}.mlp_ln.weight"] *= G32
        out[f"{p}.mlp_ln.bias"] *= G32
        out[f"{p}.mlp1.weight"] /= G32
    return out


def whisper_taps(ora, fn, prefix):
    """Run fn() with the oracle's taps on; returns (fn's result, the taps whose name starts with prefix)."""
    ora.taps = []
    try:
        r = fn()
        return r, [(n, x) for n, x in ora.taps if n.startswith(prefix)]
    finally:
        ora.taps = None


def whisper_decoder_run(ora_cls, dims, w, xa, token_lists):
    """Teacher-forced oracle logits [sum of rows, V] of the clips' token sequences and the decoder hand-over residuals."""
    ora = ora_cls(dims, w)
    def go():
        return np.concatenate([ora.decode(list(t), xa[b:b + 1])[0][0].numpy() for b, t in enumerate(token_lists)])
    return whisper_taps(ora, go, "decoder.")


def whisper_decoder_variant(ora_cls, dims, base, variant, xa, token_lists):
    """base: checkpoint already rounded to the storage type; xa: the oracle's audio features (the decoder transforms leave the encoder
    alone).  Returns (transformed fp32 tensors -- NOT yet rounded --, info)."""
    base_logits, taps = whisper_decoder_run(ora_cls, dims, base, xa, token_lists)
    rows = operand_rows(taps, base)
    writers = whisper_decoder_writers(dims, base)
    s, G, c = 1.0, 1.0, 0.0
    if variant == "near":
        s, G = split_scale(pow2_floor(0.5 * F16_MAX / max(float(v.max()) for v in rows.values())), writers)
    elif variant == "over":
        need = {}
        for name, v in rows.items():
            l = layer_of(name, dims.n_text_layer)
            need[l] = max(need.get(l, 0.0), float(v.min()))
        s, G = split_scale(pow2_ceil(2 * F16_MAX / min(need.values())), writers)
    elif variant == "down":
        s = None
        for k in range(1, 40):
            lg, _ = whisper_decoder_run(ora_cls, dims, whisper_decoder_transform(dims, base, 2.0 ** -k), xa, token_lists)
            if lg.std() < 0.5 * base_logits.std():
                break
            s = 2.0 ** -k
        assert s is not None
    elif variant == "shift":
        c = pow2_ceil(max(float((x - x.mean(dim=-1, keepdim=True)).abs().max()) for _, x in taps))
    else:
        raise ValueError(variant)
    assert G <= G_MAX, (s, G)
    return whisper_decoder_transform(dims, base, s, G, c), {"s": s, "G": G, "c": c, "base_logits": base_logits, "base_rows": rows}


def whisper_encoder_variant(ora_cls, dims, base, variant, mel):
    """Gain scale on mlp_ln first (up to G_MAX), the rest through the blocks' residual writers.  The factor is found by search in the
    oracle: scaling the writers is not a similarity of the encoder."""
    def rows_of(w):
        ora = ora_cls(dims, w)
        _, taps = whisper_taps(ora, lambda: ora.encode(mel), "encoder.")
        return operand_rows(taps, w)

    def reached(rows):
        if variant == "near":
            return max(float(v.max()) for v in rows.values()) > 0.5 * F16_MAX      # first factor PAST the window; the one before is taken
        return min(float(v.min()) for v in rows.values()) >= 2 * F16_MAX           # one hand-over per layer: every layer, every row

    prev = None
    for n in range(0, 40):
        f = 2.0 ** n
        G = min(f, G_MAX)
        cand = (f / G, G)
        hit = reached(rows_of(whisper_encoder_transform(dims, base, *cand)))
        if variant == "near" and hit:
            assert prev is not None
            return whisper_encoder_transform(dims, base, *prev), {"s": prev[0], "G": prev[1]}
        if variant == "over" and hit:
            return whisper_encoder_transform(dims, base, *cand), {"s": cand[0], "G": cand[1]}
        prev = cand
    raise AssertionError("no factor reaches the variant")
