"""CPU reference for the Qwen3 decoder of Fun-ASR (test helper, fp32 torch): LMOracle with the per-head q / k RMSNorm, the greedy
loop and the prompt merge.  Restated from STT/FunASR/Layers/Qwen3Model.swift:72-109 (attention: projections, head reshape, q_norm /
k_norm, RoPE, cache), STT/FunASR/FunASRSTT.swift:118-156 (the loop) and STT/FunASR/FunASRModel.swift:71-141 (mergeEmbeddings);
tests/test_qwen3_ref.py pins the block against transformers' Qwen3ForCausalLM."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import lm as OL


class Qwen3Oracle(OL.LMOracle):
    def hidden(self, h: torch.Tensor) -> torch.Tensor:
        """LMOracle.hidden with q_norm / k_norm (weight [head_dim], eps rms_eps) after the head reshape and before _rope."""
        c, W = self.cfg, self.w
        L = h.shape[0]
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
            q = OL._rms(q, W[p + ".self_attn.q_norm.weight"], c.rms_eps)
            k = OL._rms(k, W[p + ".self_attn.k_norm.weight"], c.rms_eps)
            q, k = self._rope(q, self.offset), self._rope(k, self.offset)
            if self.cache[l] is not None:
                k = torch.cat([self.cache[l][0], k], dim=1)
                v = torch.cat([self.cache[l][1], v], dim=1)
            self.cache[l] = (k, v)
            rep = c.n_heads // c.n_kv_heads
            kk, vv = k.repeat_interleave(rep, dim=0), v.repeat_interleave(rep, dim=0)
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
        return OL._rms(h, W["model.norm.weight"], c.rms_eps)

    def logits_of_rows(self, rows) -> np.ndarray:
        """Embedding rows [L, hidden] appended to the cache -> fp32 logits after the last one."""
        head = self.w["model.embed_tokens.weight"] if self.cfg.tie_embeddings else self.w["lm_head.weight"]
        y = self.hidden(torch.from_numpy(np.array(rows, np.float32)))
        return (y[-1] @ head.t()).numpy()


def argmax_lowest(logits: np.ndarray) -> int:
    """MLX.argMax: the first index of the maximum."""
    return int(np.argmax(np.asarray(logits)))


def greedy(model: Qwen3Oracle, prompt_embeds: np.ndarray, stop_ids, max_new_tokens: int, margins: list | None = None) -> list[int]:
    """FunASRSTT.swift:118-156 at temperature 0: one pass over the prompt rows, then one step per id; a stop id ends the loop and is not
    emitted.  `margins` (oracle-only) receives every step's top-1 minus top-2 logit over the logits' standard deviation."""
    model.reset()
    emb = model.w["model.embed_tokens.weight"].numpy()
    logits = model.logits_of_rows(prompt_embeds)
    out: list[int] = []
    for _ in range(max_new_tokens):
        tok = argmax_lowest(logits)
        if margins is not None:
            top2 = np.partition(logits, -2)[-2:]
            margins.append(float((top2[1] - top2[0]) / logits.std()))
        if tok in stop_ids:
            break
        out.append(tok)
        if len(out) < max_new_tokens:
            logits = model.logits_of_rows(emb[tok][None])
    return out


def merge_embeddings(embed: np.ndarray, input_ids, audio_embeddings: np.ndarray, sos_id: int, eos_id: int) -> np.ndarray:
    """mergeEmbeddings for one utterance: text rows 0 ... first sos, the audio rows, text rows first eos ...; text rows alone when
    either marker is absent."""
    ids = np.asarray(list(input_ids), np.int64)
    text = np.asarray(embed, np.float32)[ids]
    sos, eos = np.flatnonzero(ids == sos_id), np.flatnonzero(ids == eos_id)
    if sos.size == 0 or eos.size == 0:
        return text
    return np.concatenate([text[:sos[0] + 1], np.asarray(audio_embeddings, np.float32), text[eos[0]:]], axis=0)
