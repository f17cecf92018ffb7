"""NumPy restatement of the reference's Mimi decoder (package/TTS/Marvis/Mimi/*.swift), module for module: the oracle of the Mimi tests.

Two entry points, as in the reference, and they are different functions of the same codes:
  * MimiRef.decode(codes)         Mimi.decode (Mimi.swift:184-192): whole-clip convolutions, a fresh KV cache and mask nil, i.e. full
                                  bidirectional attention over all 2 T positions at RoPE offset 0.
  * MimiRef.decode_frames(codes)  MimiStreamingDecoder.decodeFrames (Mimi.swift:227-238): the LITERAL step loop -- one decodeStep per
                                  frame, prevXs / prevYs in every convolution (Conv.swift:233-268, 313-336), a growing key / value
                                  list per layer and the kTargetLen trim (Transformer.swift:162-170).  No mask is derived here.
decode_frames_onepass is the derived form the kernels implement (one pass, whole-clip convolutions, explicit key range
[max(0, 2 f - context), 2 f + 2) per frame f); tests/test_mimi_ref.py proves it equal to the literal loop.

Arrays are [T, C] (the reference's NCL <-> NLC hops are layout only).  dtype = float64 (the oracle) or float32 (every operation in
float32: the reference's own arithmetic noise, from which the GPU tolerance is set).  Weights: the names Mimi.sanitize produces.
"""
import numpy as np


def elu(x):
    return np.where(x > 0, x, np.expm1(np.minimum(x, 0))).astype(x.dtype)


def gelu_approx(x):
    # Transformer.swift:91-97
    dt = x.dtype.type
    return dt(0.5) * x * (dt(1) + np.tanh(dt(0.7978845608028654) * (x + dt(0.044715) * (x * x * x))))


def conv1d(x, w, b, stride=1, dilation=1):
    """MLX conv1d without padding: x [T, Cin], w [Cout, K, Cin] -> [T_out, Cout]."""
    K = w.shape[1]
    T_out = (x.shape[0] - (K - 1) * dilation - 1) // stride + 1
    y = np.zeros((max(T_out, 0), w.shape[0]), x.dtype)
    for k in range(K):
        y += x[k * dilation:k * dilation + (T_out - 1) * stride + 1:stride] @ w[:, k, :].T
    return y if b is None else y + b


def conv_transpose1d(x, w, b, stride, depthwise=False):
    """MLX convTransposed1d without padding: y[t * stride + j] += x[t] . w[:, j, :]; w [Cout, K, Cin] ([1, K, C] when depthwise)."""
    K = w.shape[1]
    T = x.shape[0]
    Cout = x.shape[1] if depthwise else w.shape[0]
    y = np.zeros(((T - 1) * stride + K, Cout), x.dtype)
    for j in range(K):
        y[j:j + (T - 1) * stride + 1:stride] += x * w[0, j] if depthwise else x @ w[:, j, :].T
    return y if b is None else y + b


class StreamableConv1d:
    """Conv.swift:176-269 with causal = true, padMode = .constant, stride 1."""

    def __init__(self, w, b, dilation=1):
        self.w, self.b, self.dil = w, b, dilation
        self.reset()

    def reset(self):
        self.prev, self.left_pad_applied = None, False

    def __call__(self, x):
        k_eff = (self.w.shape[1] - 1) * self.dil + 1
        pad = k_eff - 1
        return conv1d(np.concatenate([np.zeros((pad, x.shape[1]), x.dtype), x]), self.w, self.b, 1, self.dil)

    def step(self, x):
        if x.shape[0] == 0:
            return np.zeros((0, self.w.shape[0]), x.dtype)
        stride = 1
        k_eff = (self.w.shape[1] - 1) * self.dil + 1
        if not self.left_pad_applied:
            self.left_pad_applied = True
            x = np.concatenate([np.zeros((k_eff - stride, x.shape[1]), x.dtype), x])
        if self.prev is not None:
            x = np.concatenate([self.prev, x])
        L = x.shape[0]
        nframes = max(L + stride - k_eff, 0) // stride
        if nframes > 0:
            offset = nframes * stride
            self.prev = x[offset:]
            in_len = (nframes - 1) * stride + k_eff
            return conv1d(x[:in_len], self.w, self.b, 1, self.dil)
        self.prev = x
        return np.zeros((0, self.w.shape[0]), x.dtype)


class StreamableConvTranspose1d:
    """Conv.swift:273-337 with causal = true."""

    def __init__(self, w, b, stride, depthwise=False):
        self.w, self.b, self.stride, self.depthwise = w, b, stride, depthwise
        self.ksize = w.shape[1]
        self.reset()

    def reset(self):
        self.prev = None

    def __call__(self, x):
        y = conv_transpose1d(x, self.w, self.b, self.stride, self.depthwise)
        return y[:y.shape[0] - max(self.ksize - self.stride, 0)]

    def step(self, x):
        if x.shape[0] == 0:
            return np.zeros((0, x.shape[1] if self.depthwise else self.w.shape[0]), x.dtype)
        y = conv_transpose1d(x, self.w, self.b, self.stride, self.depthwise)
        ot = y.shape[0]
        if self.prev is not None:
            prev = self.prev
            pt = prev.shape[0]
            if self.b is not None:
                prev = prev - self.b
            y = np.concatenate([y[:pt] + prev, y[pt:]])
        invalid = self.ksize - self.stride
        cut = max(ot - invalid, 0)
        self.prev = y[cut:] if cut < ot else None
        return y[:cut]


class ResnetBlock:
    """Seanet.swift:100-163, trueSkip: x + conv_k1(elu(conv_k3(elu(x)))); the streaming add holds nothing when both sides are as long."""

    def __init__(self, c3, c1):
        self.block = [c3, c1]

    def reset(self):
        for b in self.block:
            b.reset()

    def __call__(self, xs):
        x = xs
        for b in self.block:
            x = b(elu(x))
        return x + xs

    def step(self, xs):
        x = xs
        for b in self.block:
            x = b.step(elu(x))
        assert x.shape == xs.shape          # StreamingAdd with equal lengths: l + r
        return x + xs


class MimiRef:
    def __init__(self, cfg, weights, dtype=np.float64):
        self.cfg, self.dt = cfg, np.dtype(dtype)
        W = {k: np.asarray(v).astype(dtype) for k, v in weights.items()}
        self.W = W
        s, t = cfg.seanet, cfg.transformer
        # EuclideanCodebook.updateInPlace (Quantization.swift:38-42)
        self.books = []
        for i in range(cfg.quantizer_nq):
            p = "quantizer.rvq_first.vq.layers.0.codebook." if i == 0 else f"quantizer.rvq_rest.vq.layers.{i - 1}.codebook."
            usage = np.maximum(W[p + "cluster_usage"], self.dt.type(1e-5))
            self.books.append(W[p + "embedding_sum"] / usage[:, None])
        self.upsample = StreamableConvTranspose1d(W["upsample.convtr.convtr.weight"], None, cfg.upsample_stride, depthwise=True)
        self.init_conv = StreamableConv1d(W["decoder.init_conv1d.conv.conv.weight"], W["decoder.init_conv1d.conv.conv.bias"])
        self.layers = []
        for i, r in enumerate(s.ratios):
            p = f"decoder.layers.{i}."
            up = StreamableConvTranspose1d(W[p + "upsample.convtr.convtr.weight"], W[p + "upsample.convtr.convtr.bias"], r)
            res = ResnetBlock(StreamableConv1d(W[p + "residuals.0.block.0.conv.conv.weight"], W[p + "residuals.0.block.0.conv.conv.bias"]),
                              StreamableConv1d(W[p + "residuals.0.block.1.conv.conv.weight"], W[p + "residuals.0.block.1.conv.conv.bias"]))
            self.layers.append((up, res))
        self.final_conv = StreamableConv1d(W["decoder.final_conv1d.conv.conv.weight"], W["decoder.final_conv1d.conv.conv.bias"])
        self.hd = t.d_model // t.num_heads
        self.reset()

    # ---- state (Mimi.resetState / MimiStreamingDecoder.reset)
    def reset(self):
        self.upsample.reset()
        self.init_conv.reset()
        self.final_conv.reset()
        for up, res in self.layers:
            up.reset()
            res.reset()
        self.cache = [{"k": None, "v": None, "offset": 0} for _ in range(self.cfg.transformer.num_layers)]

    # ---- quantizer (Quantization.swift:212-219, 170-175, 122-129)
    def quantizer_decode(self, codes):
        codes = np.asarray(codes)
        first = self.books[0][codes[0]] @ self.W["quantizer.rvq_first.output_proj.weight"][:, 0, :].T
        if codes.shape[0] > 1:
            q = self.books[1][codes[1]]
            for i in range(2, codes.shape[0]):
                q = q + self.books[i][codes[i]]
            first = first + q @ self.W["quantizer.rvq_rest.output_proj.weight"][:, 0, :].T
        return first

    # ---- transformer (Transformer.swift)
    def rope(self, x, offset):
        # MLXNN.RoPE(dimensions: headDim, traditional: true, base: maxPeriod): pairs (2 i, 2 i + 1), frequency base^(-2 i / dims); x [H, T, hd]
        hd = self.hd
        pos = (offset + np.arange(x.shape[1])).astype(self.dt)
        inv = np.exp(-np.arange(hd // 2).astype(self.dt) * self.dt.type(np.log(self.cfg.transformer.max_period) / (hd // 2)))
        ang = pos[:, None] * inv[None, :]
        c, s = np.cos(ang), np.sin(ang)
        x0, x1 = x[..., 0::2], x[..., 1::2]
        out = np.empty_like(x)
        out[..., 0::2] = x0 * c - x1 * s
        out[..., 1::2] = x0 * s + x1 * c
        return out

    def layer_norm(self, x, p):
        mu = x.mean(-1, keepdims=True)
        var = ((x - mu) ** 2).mean(-1, keepdims=True)
        return (x - mu) / np.sqrt(var + self.dt.type(1e-5)) * self.W[p + ".weight"] + self.W[p + ".bias"]

    def attention(self, xs, l, cache, ranges=None):
        t_cfg = self.cfg.transformer
        p = f"decoder_transformer.transformer.layers.{l}.self_attn."
        t, H, hd = xs.shape[0], t_cfg.num_heads, self.hd
        qkv = (xs @ self.W[p + "in_proj.weight"].T).reshape(t, 3, H, hd)
        q, k, v = (np.swapaxes(qkv[:, i], 0, 1) for i in range(3))          # [H, t, hd]
        if t_cfg.positional_embedding == "rope":
            q, k = self.rope(q, cache["offset"]), self.rope(k, cache["offset"])
        # KVCacheSimple.update: append, return everything
        k = k if cache["k"] is None else np.concatenate([cache["k"], k], 1)
        v = v if cache["v"] is None else np.concatenate([cache["v"], v], 1)
        cache["k"], cache["v"], cache["offset"] = k, v, cache["offset"] + t
        k_len = k.shape[1]
        k_target = t + min(t_cfg.context, k_len - t)
        if k_target < k_len:
            k, v = k[:, k_len - k_target:], v[:, k_len - k_target:]
        sc = np.einsum("hqd,hkd->hqk", q, k) * self.dt.type(1.0 / np.sqrt(hd))
        if ranges is not None:                                               # (only the derived one-pass form passes a mask)
            kk = np.arange(k.shape[1])
            sc = np.where((kk[None, :] >= ranges[0][:, None]) & (kk[None, :] < ranges[1][:, None]), sc, -np.inf)
        sc = np.exp(sc - sc.max(-1, keepdims=True))
        out = np.einsum("hqk,hkd->hqd", (sc / sc.sum(-1, keepdims=True)).astype(self.dt), v)
        return np.swapaxes(out, 0, 1).reshape(t, H * hd) @ self.W[p + "out_proj.weight"].T

    def transformer(self, x, ranges=None):
        for l, cache in enumerate(self.cache):
            p = f"decoder_transformer.transformer.layers.{l}."
            n1 = self.attention(self.layer_norm(x, p + "norm1"), l, cache, ranges)
            x = x + n1 * self.W[p + "layer_scale_1.scale"]
            h = gelu_approx(self.layer_norm(x, p + "norm2") @ self.W[p + "gating.linear1.weight"].T) @ self.W[p + "gating.linear2.weight"].T
            x = x + h * self.W[p + "layer_scale_2.scale"]
        return x

    # ---- SEANet decoder (Seanet.swift:334-387)
    def seanet(self, x):
        x = self.init_conv(x)
        for up, res in self.layers:
            x = res(up(elu(x)))
        return self.final_conv(elu(x))

    def seanet_step(self, x):
        x = self.init_conv.step(x)
        for up, res in self.layers:
            x = res.step(up.step(elu(x)))
        return self.final_conv.step(elu(x))

    # ---- the two entry points
    def decode(self, codes):
        codes = np.asarray(codes)
        self.reset()
        if codes.shape[1] == 0:
            return np.zeros(0, self.dt)
        z = self.upsample(self.quantizer_decode(codes))
        return self.seanet(self.transformer(z))[:, 0]

    def decode_step(self, codes):
        z = self.upsample.step(self.quantizer_decode(codes))
        return self.seanet_step(self.transformer(z))[:, 0]

    def decode_frames(self, codes):
        """The streaming decoder on a stream that has NOT been reset here (call reset() for a new one): one decodeStep per frame."""
        codes = np.asarray(codes)
        return np.concatenate([np.zeros(0, self.dt)] + [self.decode_step(codes[:, t:t + 1]) for t in range(codes.shape[1])])

    def decode_frames_onepass(self, codes):
        """The derived form: whole-clip convolutions and ONE attention pass in which the rows of frame f see keys [max(0, 2 f - context), 2 f + 2)."""
        codes = np.asarray(codes)
        self.reset()
        us, ctx = self.cfg.upsample_stride, self.cfg.transformer.context
        f = np.arange(codes.shape[1] * us) // us
        ranges = (np.maximum(0, us * f - ctx), us * f + us)
        z = self.upsample(self.quantizer_decode(codes))
        return self.seanet(self.transformer(z, ranges))[:, 0]
