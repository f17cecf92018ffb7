"""On-disk formats of the reference's checkpoints: a safetensors reader, `config.json` -> ModelDimensions,
and the expansion of MLX affine-quantised layers (`<path>.weight` uint32 + `.scales` + `.biases`, group 64, 4 / 8 bit -- the
reference's DEFAULT checkpoints, STT/Whisper/WhisperModel.swift:144-206) into the dense tensors the loaders of this package take.
De-quantisation runs on the GPU (mia_dequant_affine); nothing here falls back to the CPU."""
from __future__ import annotations

import json
import mmap
import struct

import numpy as np

from . import _abi, _lib

_DT = {"F32": (np.float32, 4), "F16": (np.float16, 2), "BF16": (np.uint16, 2), "I32": (np.int32, 4), "U32": (np.uint32, 4), "I64": (np.int64, 8),
       "U8": (np.uint8, 1), "I8": (np.int8, 1), "U16": (np.uint16, 2), "I16": (np.int16, 2), "F64": (np.float64, 8), "BOOL": (np.bool_, 1)}


class Tensor(np.ndarray):
    """ndarray view into the mapped file; `.st_dtype` keeps the safetensors dtype tag (bf16 payloads are exposed as uint16)."""
    st_dtype = "F32"


def read_safetensors(path: str) -> dict[str, np.ndarray]:
    """Zero-copy reader of the safetensors container: u64 header length, JSON header {name: {dtype, shape, data_offsets}}, raw little-endian
    tensors.  (What MLX.loadArrays(url:) does at WhisperModel.swift:184.)"""
    f = open(path, "rb")
    mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    (n,) = struct.unpack("<Q", mm[:8])
    header = json.loads(mm[8:8 + n].decode("utf-8"))
    base = 8 + n
    out: dict[str, np.ndarray] = {}
    for name, meta in header.items():
        if name == "__metadata__":
            continue
        if meta["dtype"] not in _DT:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"safetensors: unsupported dtype {meta['dtype']} for '{name}'")
        dt, sz = _DT[meta["dtype"]]
        b0, b1 = meta["data_offsets"]
        count = int(np.prod(meta["shape"], dtype=np.int64)) if meta["shape"] else 1
        if b1 - b0 != count * sz:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"safetensors: '{name}' has {b1 - b0} bytes for shape {meta['shape']}")
        a = np.frombuffer(mm, dtype=dt, count=count, offset=base + b0).reshape(meta["shape"]).view(Tensor)
        a.st_dtype = meta["dtype"]
        out[name] = a
    return out


def bf16_bits_to_f32(a: np.ndarray) -> np.ndarray:
    return (np.asarray(a, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_float32(a: np.ndarray) -> np.ndarray:
    if getattr(a, "st_dtype", None) == "BF16":
        return bf16_bits_to_f32(a)
    return np.asarray(a, np.float32)


def load_model_dimensions(config_path: str):
    """ModelDimensions.load(from:) (STT/Whisper/Config/WhisperConfig.swift:78-86): the ten n_* keys of config.json."""
    from .synthetic import ModelDimensions
    cfg = json.load(open(config_path))
    keys = ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer", "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")
    missing = [k for k in keys if k not in cfg]
    if missing:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"config.json lacks {missing}")
    return ModelDimensions(*[int(cfg[k]) for k in keys])


def _mia_dtype(a: np.ndarray) -> int:
    tag = _abi.dtype_tag(a)
    if tag in (_lib.F32, _lib.F16, _lib.BF16):
        return tag
    raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"scales / biases must be f32, f16 or bf16 (got {a.dtype})")


def dequantize_affine(ctx: _lib.Context, wq: np.ndarray, scales: np.ndarray, biases: np.ndarray, group_size: int = 64, bits: int = 4) -> np.ndarray:
    """GPU expansion of one quantised tensor to float32 [rows, cols]."""
    lib = ctx.lib
    w = np.ascontiguousarray(wq).view(np.uint32) if wq.dtype != np.uint32 else np.ascontiguousarray(wq)
    rows = int(np.prod(w.shape[:-1]))
    cols = w.shape[-1] * 32 // bits
    sdt = _mia_dtype(scales)
    s, b = np.ascontiguousarray(scales), np.ascontiguousarray(biases)
    if s.size != rows * (cols // group_size) or b.size != s.size or _mia_dtype(biases) != sdt:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "dequantize_affine: scales / biases do not match the packed weight")
    out = np.empty(tuple(w.shape[:-1]) + (cols,), np.float32)
    ctx.check(lib.mia_dequant_affine(ctx.h, w.ctypes.data, s.ctypes.data, b.ctypes.data, rows, cols, group_size, bits, sdt, out.ctypes.data, _lib.F32, _lib.MEM_HOST))
    return out


def expand_checkpoint(ctx: _lib.Context, tensors: dict[str, np.ndarray], bits: int | None = None, group_size: int = 64) -> dict[str, np.ndarray]:
    """Dense float32 tensors under the Module key schema: every `<p>.weight` that comes with `<p>.scales` is de-quantised (bits inferred
    from the packed width when not given), `.scales` / `.biases` are dropped, bf16 payloads become float32."""
    out: dict[str, np.ndarray] = {}
    for name, a in tensors.items():
        if name.endswith(".scales") or (name.endswith(".biases") and name[:-7] + ".scales" in tensors):
            continue
        if name.endswith(".weight") and name[:-7] + ".scales" in tensors:
            sc, bi = tensors[name[:-7] + ".scales"], tensors[name[:-7] + ".biases"]
            b = bits or (32 * a.shape[-1]) // (sc.shape[-1] * group_size)
            out[name] = dequantize_affine(ctx, a, sc, bi, group_size, b)
        else:
            out[name] = to_float32(a) if a.dtype.kind in "fu" and getattr(a, "st_dtype", "F32") in ("F32", "F16", "BF16") else np.asarray(a)
    return out


def packed_tensors(tensors: dict[str, np.ndarray]) -> dict[str, np.ndarray]:
    """The raw `<p>.weight` / `<p>.scales` / `<p>.biases` triples of a checkpoint's quantised modules (what expand_checkpoint de-quantises)."""
    return {n: a for n, a in tensors.items()
            if n.endswith((".weight", ".scales", ".biases")) and n.rsplit(".", 1)[0] + ".scales" in tensors}


def load_whisper_checkpoint(ctx: _lib.Context, model_dir: str, keep_packed: bool = False):
    """WhisperModel.load's file half (WhisperModel.swift:175-206): config.json + model.safetensors -> (ModelDimensions, dense tensors).
    keep_packed: a third value, the raw packed tensors of the quantised modules (empty for a dense checkpoint), for
    WhisperModel.attach_quantized -- the reference keeps them packed (WhisperModel.swift:189-196)."""
    import os
    dims = load_model_dimensions(os.path.join(model_dir, "config.json"))
    raw = read_safetensors(os.path.join(model_dir, "model.safetensors"))
    if keep_packed:
        return dims, expand_checkpoint(ctx, raw), packed_tensors(raw)
    return dims, expand_checkpoint(ctx, raw)


def quantize_affine(w: np.ndarray, group_size: int = 64, bits: int = 4, scale_dtype=np.float16):
    """A SIMPLIFIED min / max affine quantiser in MLX's storage layout -- the direction the reference's loaders take for checkpoints
    that are not already quantised (`quantize(model:) { (64, bits, .affine) }`, STT/Whisper/WhisperModel.swift:189-196): per group of
    `group_size` consecutive inputs, scale = (max - min) / (2^bits - 1), bias = min, code = round((w - bias) / scale); codes packed
    little end first into uint32 words (bits 4, 6 or 8: pack_codes).  mx.quantize additionally nudges scale / bias (edge and sign handling), which this does not
    reproduce: parity of the CODES with mx.quantize is unpinned; the contract of the hot path is de-quantisation (scale * code + bias),
    which is layout-exact.  Returns (codes uint32 [N, K*bits/32], scales, biases [N, K/group_size] in `scale_dtype`) -- the three
    tensors a quantised checkpoint stores for the layer (feed them to CausalLM.attach_q4 / expand them with dequantize_affine)."""
    w = np.asarray(w, np.float32)
    n, k = w.shape
    g = w.reshape(n, k // group_size, group_size)
    lo, hi = g.min(-1), g.max(-1)
    top = float((1 << bits) - 1)
    scale = np.where(hi > lo, (hi - lo) / top, 1.0).astype(scale_dtype)
    bias = lo.astype(scale_dtype)
    s32 = scale.astype(np.float32)[..., None]
    q = np.clip(np.rint((g - bias.astype(np.float32)[..., None]) / s32), 0, top).astype(np.uint32)
    return pack_codes(q.reshape(n, k), bits), scale, bias


def pack_codes(q: np.ndarray, bits: int) -> np.ndarray:
    """Codes [N, K] -> uint32 [N, K*bits/32] in MLX's storage: a row is one little-endian bit stream, code k in bits [k*bits, (k+1)*bits)
    (4 and 8 bit: whole codes per word; 6 bit: 4 codes in 3 bytes, codes straddle words)."""
    q = np.asarray(q, np.uint32)
    n, k = q.shape
    if bits not in (4, 6, 8) or (k * bits) % 32:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"pack_codes: {bits}-bit rows of {k} codes do not fill whole words")
    if bits == 6:
        q4 = q.reshape(n, k // 4, 4)
        v = q4[:, :, 0] | (q4[:, :, 1] << np.uint32(6)) | (q4[:, :, 2] << np.uint32(12)) | (q4[:, :, 3] << np.uint32(18))
        b = np.stack([v & 255, (v >> np.uint32(8)) & 255, v >> np.uint32(16)], -1).astype(np.uint8)
        return np.ascontiguousarray(b.reshape(n, -1)).view("<u4")
    per = 32 // bits
    q = q.reshape(n, k // per, per)
    packed = np.zeros(q.shape[:2], np.uint32)
    for j in range(per):
        packed |= q[:, :, j] << np.uint32(j * bits)
    return packed


def sanitize_mimi_name(raw: str) -> str:
    """Mimi.sanitize's renaming of one checkpoint key (TTS/Marvis/Mimi/Mimi.swift:308-354), replacement for replacement."""
    k = ".".join(seg[1:] if seg.startswith("_") else seg for seg in raw.split("."))
    if k.startswith("encoder.model."):
        k = k.replace("encoder.model.", "encoder.")
    if k.startswith("decoder.model."):
        k = k.replace("decoder.model.", "decoder.")
    if k.endswith(".in_proj_weight"):
        k = k.replace(".in_proj_weight", ".in_proj.weight")
    if k.endswith(".linear1.weight"):
        k = k.replace(".linear1.weight", ".gating.linear1.weight")
    if k.endswith(".linear2.weight"):
        k = k.replace(".linear2.weight", ".gating.linear2.weight")
    for layer, idx in enumerate((2, 5, 8, 11)):
        k = k.replace(f"decoder.{idx}.", f"decoder.layers.{layer}.upsample.")
        k = k.replace(f"decoder.{idx + 1}.", f"decoder.layers.{layer}.residuals.0.")
    for layer, idx in enumerate((1, 4, 7, 10)):
        k = k.replace(f"encoder.{idx}.", f"encoder.layers.{layer}.residuals.0.")
        k = k.replace(f"encoder.{idx + 2}.", f"encoder.layers.{layer}.downsample.")
    k = k.replace("decoder.0.", "decoder.init_conv1d.")
    k = k.replace("decoder.14.", "decoder.final_conv1d.")
    k = k.replace("encoder.0.", "encoder.init_conv1d.")
    k = k.replace("encoder.14.", "encoder.final_conv1d.")
    k = k.replace(".block.1.", ".block.0.")
    k = k.replace(".block.3.", ".block.1.")
    return k


def sanitize_mimi(tensors):
    """Mimi.sanitize (Mimi.swift:305-377): the checkpoint's own names -> the module key schema, and the axis swaps that take the
    PyTorch layouts to the reference's ([out, in, k] -> [out, k, in] for `.conv.weight` / `.output_proj.weight` / `.input_proj.weight`,
    [in, out, k] -> [out, k, in] for `.convtr.weight`).  A name -> array dict (the raw safetensors contents) gives the dict
    MimiCodec.load takes; a list of names gives the list of renamed keys."""
    if not isinstance(tensors, dict):
        return [sanitize_mimi_name(n) for n in tensors]
    out = {}
    for raw, v in tensors.items():
        k = sanitize_mimi_name(raw)
        v = np.asarray(v)
        if k.endswith((".conv.weight", ".output_proj.weight", ".input_proj.weight")) and v.ndim >= 2:
            v = np.swapaxes(v, -1, -2)
        if k.endswith(".convtr.weight") and v.ndim == 3:
            v = np.transpose(v, (1, 2, 0))
        out[k] = v
    return out


def sanitize_marvis_name(raw: str) -> str:
    """stripModelPrefix + sanitize of one Marvis checkpoint key (TTS/Marvis/MarvisTTS.swift:237-282), replacement for replacement."""
    k = raw[6:] if raw.startswith("model.") else raw
    if "attn" in k and "self_attn" not in k:
        k = k.replace("attn", "self_attn")
        k = k.replace("output_proj", "o_proj")
    if "mlp" in k:
        k = k.replace("w1", "gate_proj")
        k = k.replace("w2", "down_proj")
        k = k.replace("w3", "up_proj")
    if "sa_norm" in k or "mlp_norm" in k:
        k = k.replace("sa_norm", "input_layernorm")
        k = k.replace("scale", "weight")
        k = k.replace("mlp_norm", "post_attention_layernorm")
        k = k.replace("scale", "weight")
    if "decoder.norm" in k or "backbone.norm" in k:
        k = k.replace("scale", "weight")
    return k


def sanitize_marvis(tensors):
    """A name -> array dict (the raw safetensors contents) gives the dict MarvisModel.load takes; a list of names gives the renamed keys.
    No tensor changes its layout."""
    if not isinstance(tensors, dict):
        return [sanitize_marvis_name(n) for n in tensors]
    return {sanitize_marvis_name(n): v for n, v in tensors.items()}


_KOKORO_SCOPE = ("decoder.", "predictor.F0.", "predictor.N.", "predictor.F0_proj.", "predictor.N_proj.")


def sanitize_kokoro(tensors):
    """The decoder / F0 / N branch of KokoroWeightLoader.sanitizeWeights (TTSEngine/KokoroWeightLoader.swift:43-66,85-111) as a rule on
    shapes: noise_convs / F0_proj / N_proj `.weight` and every three-axis weight_v swap their last two axes ([Cout][Cin][K] of the
    checkpoint -> [Cout][K][Cin]; `ups`, stored [Cin][Cout][K], becomes [Cin][K][Cout] and `pool` [C][1][3] becomes [C][3][1]);
    everything else passes.  Keys outside the decoder and the F0 / N predictor blocks are dropped (they belong to the text half)."""
    out = {}
    for key, v in tensors.items():
        if not key.startswith(_KOKORO_SCOPE):
            continue
        a = np.asarray(v)
        swap = a.ndim == 3 and ("weight_v" in key or (key.endswith(".weight") and any(s in key for s in ("noise_convs", "F0_proj", "N_proj"))))
        out[key] = np.ascontiguousarray(a.transpose(0, 2, 1)) if swap else a
    return out
