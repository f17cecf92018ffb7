"""Shared set-up of the packed-weight Whisper tests (test infrastructure): a synthetic 'peaky' checkpoint quantised the way the
reference's loader does (`quantize(model:) { (64, bits, .affine) }`, STT/Whisper/WhisperModel.swift:189-196) and its fp32
de-quantisation s * code + b, which is what the oracle is built on and what the HIP handle is loaded from before the packed tensors are
attached."""
import numpy as np

from oracle import whisper as OW


def is_quantised(name, a):
    """Every 2-D `.weight` whose input width is a multiple of the group, outside the convolutions and the LayerNorms."""
    is_ln = "_ln." in name or ".ln." in name or "ln_post" in name
    return name.endswith(".weight") and a.ndim == 2 and a.shape[1] % 64 == 0 and not is_ln and "conv" not in name


def dequantize_numpy(codes, scales, biases, bits, group_size=64):
    per = 32 // bits
    q = (codes[:, :, None] >> (np.arange(per, dtype=np.uint32) * np.uint32(bits))) & np.uint32((1 << bits) - 1)
    n = codes.shape[0]
    q = q.reshape(n, -1, group_size).astype(np.float32)
    w = scales.astype(np.float32)[..., None] * q + biases.astype(np.float32)[..., None]
    return np.ascontiguousarray(w.reshape(n, -1), np.float32)


def quantised_checkpoint(dims, seed, bits, round_to, scale_dtype=np.float16, style="peaky"):
    """(dense fp32 weights with every quantised matrix replaced by its de-quantisation, packed tensors under the reference's key names)."""
    from mlx_swift_audio_amd.checkpoint import quantize_affine
    dense = OW.synthetic_weights(dims, seed=seed, style=style, round_to=round_to)
    packed = {}
    for name, a in list(dense.items()):
        if not is_quantised(name, a):
            continue
        codes, s, b = quantize_affine(a, 64, bits, scale_dtype)
        base = name[:-7]
        packed[base + ".weight"], packed[base + ".scales"], packed[base + ".biases"] = codes, s, b
        dense[name] = dequantize_numpy(codes, s, b, bits)
    return dense, packed
