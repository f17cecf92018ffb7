"""NumPy restatement of Kokoro's ALBERT and bert_encoder (reference: TTS/Kokoro/Albert of mlx-swift-audio, KokoroTTS.swift:262-287),
callable in float64 and in float32.  B = 1; activations are time-major [N, C].  Every function cites the Swift it restates."""
import numpy as np
import torch

GROUP = "bert.encoder.albert_layer_groups.0.albert_layers.0."


def gelu(x):
    """MLXNN.gelu: 0.5 x (1 + erf(x / sqrt 2)), in the dtype of x."""
    return x.dtype.type(0.5) * x * (1 + torch.erf(torch.from_numpy(x / np.sqrt(x.dtype.type(2)))).numpy())


def mask_term(N, dtype=np.float64):
    """KokoroTTS.swift:266-282 with AlbertModel's (1 - mask) * -10000: the mask of the one padded sequence is all ones."""
    return (1 - np.ones((1, 1, N), dtype)) * dtype(-10000.0)


class KokoroBertRef:
    def __init__(self, cfg, weights, dtype=np.float64):
        self.cfg, self.dt, self.w = cfg, dtype, {k: np.asarray(v, dtype) for k, v in weights.items() if k.startswith("bert")}

    def linear(self, p, x):
        return x @ self.w[p + ".weight"].T + self.w[p + ".bias"]

    def norm(self, p, x):
        """MLXNN.LayerNorm with eps 1e-12: biased variance over the last axis."""
        mean = x.mean(axis=-1, keepdims=True)
        var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
        return (x - mean) / np.sqrt(var + self.dt(1e-12)) * self.w[p + ".weight"] + self.w[p + ".bias"]

    def embeddings(self, ids):
        """AlbertEmbeddings.swift:58-62: word + position + token type 0, in that order, then LayerNorm."""
        t = {k: self.w[f"bert.embeddings.{k}_embeddings.weight"] for k in ("word", "position", "token_type")}
        return self.norm("bert.embeddings.LayerNorm", t["word"][np.asarray(ids)] + t["position"][:len(ids)] + t["token_type"][0])

    def layer(self, x):
        """AlbertSelfAttention.swift:55-88 and AlbertLayer.swift:27-41 on x [N, hidden]."""
        N, H = x.shape[0], self.cfg.bert_heads
        q, k, v = (self.linear(GROUP + "attention." + n, x).reshape(N, H, -1).transpose(1, 0, 2) for n in ("query", "key", "value"))
        s = q @ k.transpose(0, 2, 1) / self.dt(np.sqrt(q.shape[-1])) + mask_term(N, self.dt)
        s = np.exp(s - s.max(axis=-1, keepdims=True))
        ctx = ((s / s.sum(axis=-1, keepdims=True)) @ v).transpose(1, 0, 2).reshape(N, -1)
        a = self.norm(GROUP + "attention.LayerNorm", self.linear(GROUP + "attention.dense", ctx) + x)
        f = self.linear(GROUP + "ffn_output", gelu(self.linear(GROUP + "ffn", a)))
        return self.norm(GROUP + "full_layer_layer_norm", f + a)

    def encode(self, ids, n_layers=None):
        """AlbertEncoder.swift:30-36, then bert_encoder: -> (ALBERT's sequence output [N, hidden], d_en [N, d_model])."""
        x = self.linear("bert.encoder.embedding_hidden_mapping_in", self.embeddings(ids))
        for _ in range(n_layers or self.cfg.bert_layers):
            x = self.layer(x)
        return x, self.linear("bert_encoder", x)
