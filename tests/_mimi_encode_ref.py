"""NumPy restatement of the reference's Mimi encoder (package/TTS/Marvis/Mimi/*.swift), module for module: the oracle of the Mimi
encode tests.  Mimi.encode (Mimi.swift:174-182) = SeanetEncoder -> encoder transformer (fresh cache, mask nil: full bidirectional
attention at RoPE offset 0) -> ConvDownsample1d (.edge padding) -> SplitResidualVectorQuantizer.encode.

Arrays are [T, C].  dtype = float64 (the oracle) or float32 (every operation in float32: the reference's own arithmetic noise, from
which the GPU tolerances are set).  Weights: the names Mimi.sanitize produces.
"""
import math

import numpy as np

from _mimi_ref import conv1d, elu, gelu_approx


def extra_padding(length, ksize, stride, padding_total):
    """getExtraPaddingForConv1d (Conv.swift:157-164), literally."""
    nframes = max(length + padding_total - ksize, 0)
    nf = float(nframes) / float(stride) + 1.0
    ideal = (int(math.ceil(nf)) - 1) * stride + ksize - padding_total
    return max(0, ideal - length)


def streamable_conv1d(x, w, b, stride=1, mode="constant"):
    """StreamableConv1d.callAsFunction (Conv.swift:212-230) with causal = true, dilation 1: k - stride rows in front, the extra ones behind."""
    k = w.shape[1]
    total = k - stride
    extra = extra_padding(x.shape[0], k, stride, total)
    return conv1d(np.pad(x, ((total, extra), (0, 0)), mode=mode), w, b, stride)


def chain_lengths(cfg, n_samples):
    """(positions P, frames T): every strided stage maps L to ceil(L / r)."""
    L = n_samples
    for r in reversed(cfg.seanet.ratios):
        L = -(-L // r)
    return L, -(-L // cfg.upsample_stride)


class MimiEncodeRef:
    def __init__(self, cfg, weights, dtype=np.float64):
        self.cfg, self.dt = cfg, np.dtype(dtype)
        self.W = {k: np.asarray(v).astype(dtype) for k, v in weights.items()}
        self.hd = cfg.transformer.d_model // cfg.transformer.num_heads
        W = self.W
        # EuclideanCodebook (Quantization.swift:38-56): e = embedding_sum / max(cluster_usage, 1e-5), c2 = ||e||^2 / 2
        self.books, self.c2 = [], []
        for i in range(cfg.quantizer_nq):
            p = "quantizer.rvq_first.vq.layers.0.codebook." if i == 0 else f"quantizer.rvq_rest.vq.layers.{i - 1}.codebook."
            e = W[p + "embedding_sum"] / np.maximum(W[p + "cluster_usage"], self.dt.type(1e-5))[:, None]
            self.books.append(e)
            self.c2.append((e * e).sum(-1) / self.dt.type(2))

    def _conv(self, p, x, stride=1, mode="constant"):
        return streamable_conv1d(x, self.W[p + ".weight"], self.W.get(p + ".bias"), stride, mode)

    # ---- SEANet encoder (Seanet.swift:167-276)
    def seanet(self, pcm):
        s = self.cfg.seanet
        x = self._conv("encoder.init_conv1d.conv.conv", np.asarray(pcm).astype(self.dt).reshape(-1, 1))
        for i, r in enumerate(reversed(s.ratios)):
            p = f"encoder.layers.{i}."
            h = self._conv(p + "residuals.0.block.0.conv.conv", elu(x))
            x = x + self._conv(p + "residuals.0.block.1.conv.conv", elu(h))
            x = self._conv(p + "downsample.conv.conv", elu(x), stride=r)
        return self._conv("encoder.final_conv1d.conv.conv", elu(x))

    # ---- encoder transformer (Transformer.swift), mask nil over all positions
    def _rope(self, x):
        hd = self.hd
        pos = np.arange(x.shape[1]).astype(self.dt)
        inv = np.exp(-np.arange(hd // 2).astype(self.dt) * self.dt.type(np.log(self.cfg.transformer.max_period) / (hd // 2)))
        ang = pos[:, None] * inv[None, :]
        c, s = np.cos(ang), np.sin(ang)
        out = np.empty_like(x)
        out[..., 0::2] = x[..., 0::2] * c - x[..., 1::2] * s
        out[..., 1::2] = x[..., 0::2] * s + x[..., 1::2] * c
        return out

    def _layer_norm(self, x, p):
        mu = x.mean(-1, keepdims=True)
        var = ((x - mu) ** 2).mean(-1, keepdims=True)
        return (x - mu) / np.sqrt(var + self.dt.type(1e-5)) * self.W[p + ".weight"] + self.W[p + ".bias"]

    def transformer(self, x):
        t = self.cfg.transformer
        H, hd, n = t.num_heads, self.hd, x.shape[0]
        for l in range(t.num_layers):
            p = f"encoder_transformer.transformer.layers.{l}."
            qkv = (self._layer_norm(x, p + "norm1") @ self.W[p + "self_attn.in_proj.weight"].T).reshape(n, 3, H, hd)
            q, k, v = (np.swapaxes(qkv[:, i], 0, 1) for i in range(3))
            if t.positional_embedding == "rope":
                q, k = self._rope(q), self._rope(k)
            sc = np.einsum("hqd,hkd->hqk", q, k) * self.dt.type(1.0 / np.sqrt(hd))
            sc = np.exp(sc - sc.max(-1, keepdims=True))
            a = np.einsum("hqk,hkd->hqd", (sc / sc.sum(-1, keepdims=True)).astype(self.dt), v)
            a = np.swapaxes(a, 0, 1).reshape(n, H * hd) @ self.W[p + "self_attn.out_proj.weight"].T
            x = x + a * self.W[p + "layer_scale_1.scale"]
            h = gelu_approx(self._layer_norm(x, p + "norm2") @ self.W[p + "gating.linear1.weight"].T) @ self.W[p + "gating.linear2.weight"].T
            x = x + h * self.W[p + "layer_scale_2.scale"]
        return x

    # ---- ConvDownsample1d (Conv.swift:341-355): padMode .edge
    def downsample(self, x):
        return streamable_conv1d(x, self.W["downsample.conv.conv.weight"], None, self.cfg.upsample_stride, mode="edge")

    def encode_latent(self, pcm):
        return self.downsample(self.transformer(self.seanet(pcm)))

    # ---- SplitResidualVectorQuantizer.encode (Quantization.swift:50-56, 84-88, 110-120, 164-168, 203-210)
    def quantize(self, latent, n_q=None, forced=None):
        """-> (codes [n_q, T] int32, gap [n_q, T]: second-best minus best distance, dist: per stage the [T, bins] distances).
        forced: codes that replace the argmin when the residual is updated (teacher forcing for the noise measurement)."""
        n_q = self.cfg.quantizer_nq if n_q is None else n_q
        z = np.asarray(latent).astype(self.dt)
        first = z @ self.W["quantizer.rvq_first.input_proj.weight"][:, 0, :].T
        rest = z @ self.W["quantizer.rvq_rest.input_proj.weight"][:, 0, :].T if n_q > 1 else None
        codes, gaps, dist = [], [], []
        for i in range(n_q):
            r = first if i == 0 else rest
            d = self.c2[i][None, :] - r @ self.books[i].T
            idx = np.argmin(d, axis=-1)                                  # the lowest index on equal distances
            two = np.partition(d, 1, axis=-1)[:, :2] if d.shape[1] > 1 else np.concatenate([d, d + np.inf], -1)
            codes.append(idx.astype(np.int32))
            gaps.append(two[:, 1] - two[:, 0])
            dist.append(d)
            if i >= 1:
                rest = rest - self.books[i][idx if forced is None else forced[i]]
        return np.stack(codes), np.stack(gaps), dist

    def encode(self, pcm, n_q=None):
        return self.quantize(self.encode_latent(pcm), n_q)[0]
