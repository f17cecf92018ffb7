"""TEST INFRASTRUCTURE ONLY -- the quantised KV cache's rule in numpy (QuantizedKVCache(groupSize: 64, bits:), TransformerBlock.swift:182-201;
MLX's affine rule restated from its public documentation like oracle/quant.py, PARITY UNPINNED against MLX), and an LM oracle that
attends over cache rows handed to it.

Per group of 64 consecutive elements of a row that is already rounded to the 16-bit type `kind`:
  lo, hi = min, max;  n = 2^bits - 1;  scale = (hi - lo) / n in fp32, 1 when hi == lo;  bias = lo;  both rounded to `kind` (RNE);
  code = clamp(rint((x - bias) / scale), 0, n) with the rounded pair in fp32 (a NaN quotient -- 0 / 0 under a scale that rounded to
  zero -- counts as code 0);  value read back = scale * code + bias in fp32, a multiply then an add.
MLX's nudge that makes zero exactly representable is not reproduced."""
from __future__ import annotations

import math

import numpy as np
import torch

from mlx_swift_audio_amd.synthetic import round_array
from oracle import lm as OL

GROUP = 64


def quantise(x: np.ndarray, bits: int, kind: str):
    """x float32 [..., dh] (values of the 16-bit type `kind`) -> (codes uint32 [..., dh], scale, bias float32 [..., dh / 64], the pair
    already rounded to `kind`)."""
    x = np.ascontiguousarray(x, np.float32)
    *lead, dh = x.shape
    g = x.reshape(*lead, dh // GROUP, GROUP)
    lo, hi = g.min(-1), g.max(-1)
    n = np.float32((1 << bits) - 1)
    with np.errstate(all="ignore"):
        scale = np.where(hi == lo, np.float32(1.0), (hi - lo) / n).astype(np.float32)
        s, b = round_array(scale, kind), round_array(lo, kind)
        t = np.rint((g - b[..., None]) / s[..., None])
    t = np.where(np.isnan(t), np.float32(0.0), t)
    codes = np.clip(t, np.float32(0.0), n).astype(np.uint32)
    return codes.reshape(*lead, dh), s, b


def dequantise(codes: np.ndarray, scale: np.ndarray, bias: np.ndarray) -> np.ndarray:
    *lead, dh = codes.shape
    q = codes.reshape(*lead, dh // GROUP, GROUP).astype(np.float32)
    sq = (scale[..., None].astype(np.float32) * q).astype(np.float32)          # a multiply ...
    return (sq + bias[..., None].astype(np.float32)).astype(np.float32).reshape(*lead, dh)      # ... then an add


def pack(codes: np.ndarray, bits: int) -> np.ndarray:
    """codes [..., dh] -> uint32 [..., dh * bits / 32], little end first (the packing of oracle/quant.py)."""
    per = 32 // bits
    *lead, dh = codes.shape
    q = codes.reshape(*lead, dh // per, per).astype(np.uint32)
    out = np.zeros(q.shape[:-1], np.uint32)
    for j in range(per):
        out |= q[..., j] << np.uint32(j * bits)
    return out


def dq_rows(x: np.ndarray, bits: int, kind: str) -> np.ndarray:
    """What the quantised cache returns for rows x (fp32, any values): round to `kind`, quantise, read back."""
    codes, s, b = quantise(round_array(x, kind), bits, kind)
    return dequantise(codes, s, b)


class ForcedCacheOracle(OL.LMOracle):
    """LMOracle whose attention uses cache rows handed to it: hidden(h, forced_cache) with forced_cache[l] = (k, v), each
    [Hkv, T, dh] holding ALL T rows the L new positions attend over (their own rows included, as last ones).  Returns the final-norm
    hidden states and, per layer, the oracle's OWN (un-quantised) new k / v rows [Hkv, L, dh].  Set .offset to the first new position."""

    def hidden(self, h: torch.Tensor, forced_cache=None):
        if forced_cache is None:
            return super().hidden(h)
        c, W = self.cfg, self.w
        L = h.shape[0]
        own = []
        for l in range(c.n_layers):
            p = f"model.layers.{l}"
            xn = OL._rms(h, W[p + ".input_layernorm.weight"], c.rms_eps)
            q = xn @ W[p + ".self_attn.q_proj.weight"].t()
            k = xn @ W[p + ".self_attn.k_proj.weight"].t()
            v = xn @ W[p + ".self_attn.v_proj.weight"].t()
            if c.qkv_bias:
                q = q + W[p + ".self_attn.q_proj.bias"]
                k = k + W[p + ".self_attn.k_proj.bias"]
                v = v + W[p + ".self_attn.v_proj.bias"]
            q = q.reshape(L, c.n_heads, c.head_dim).transpose(0, 1)
            k = k.reshape(L, c.n_kv_heads, c.head_dim).transpose(0, 1)
            v = v.reshape(L, c.n_kv_heads, c.head_dim).transpose(0, 1)
            q, k = self._rope(q, self.offset), self._rope(k, self.offset)
            own.append((k.numpy().copy(), v.numpy().copy()))
            fk = torch.from_numpy(np.ascontiguousarray(forced_cache[l][0], np.float32))
            fv = torch.from_numpy(np.ascontiguousarray(forced_cache[l][1], np.float32))
            rep = c.n_heads // c.n_kv_heads
            kk, vv = fk.repeat_interleave(rep, dim=0), fv.repeat_interleave(rep, dim=0)
            s = (q @ kk.transpose(1, 2)) * (1.0 / math.sqrt(c.head_dim))
            if L > 1:
                T = kk.shape[1]
                mask = torch.ones(L, T, dtype=torch.bool).tril(T - L)
                s = s.masked_fill(~mask, -float("inf"))
            o = (torch.softmax(s, dim=-1) @ vv).transpose(0, 1).reshape(L, -1)
            h = h + o @ W[p + ".self_attn.o_proj.weight"].t()
            xn = OL._rms(h, W[p + ".post_attention_layernorm.weight"], c.rms_eps)
            g = xn @ W[p + ".mlp.gate_proj.weight"].t()
            u = xn @ W[p + ".mlp.up_proj.weight"].t()
            h = h + (torch.nn.functional.silu(g) * u) @ W[p + ".mlp.down_proj.weight"].t()
        self.offset += L
        return OL._rms(h, W["model.norm.weight"], c.rms_eps), own

    def step_logits(self, token: int, pos: int, forced_cache):
        """Logits [vocab] of `token` at position `pos` over forced_cache (rows [0, pos]), and the oracle's own new rows per layer."""
        self.offset = pos
        emb = self.w["model.embed_tokens.weight"]
        y, own = self.hidden(emb[torch.as_tensor([int(token)])], forced_cache)
        head = emb if self.cfg.tie_embeddings else self.w["lm_head.weight"]
        return (y @ head.t())[-1].numpy(), own
