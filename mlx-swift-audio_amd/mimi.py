"""Host-side mirror of the reference's Mimi interface (TTS/Marvis/Mimi/Mimi.swift), backed by the gfx950 HIP layer:
Mimi.decode (:184-192) and MimiStreamingDecoder (:213-239), the two calls of MarvisTTS.swift:534-536, and Mimi.encode (:174-182), the
codec call of tokenizeAudio (MarvisTTS.swift:323).  No arithmetic happens in Python.  Whole-clip and streamed decodes are different
functions of the same codes, as in the reference ("Mimi").  The encode side is there when the weights carry it."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._abi import MimiConfig as _CConfig, tensor_views


@dataclass(frozen=True)
class SeanetConfig:
    dimension: int = 512
    channels: int = 1
    causal: bool = True
    nfilters: int = 64
    nresidual_layers: int = 1
    ratios: tuple = (8, 6, 5, 4)
    ksize: int = 7
    residual_ksize: int = 3
    last_ksize: int = 3
    dilation_base: int = 2
    pad_mode: str = "constant"
    true_skip: bool = True
    compress: int = 2


@dataclass(frozen=True)
class MimiTransformerConfig:
    d_model: int = 512
    num_heads: int = 8
    num_layers: int = 8
    layer_scale: float | None = 0.01
    positional_embedding: str = "rope"
    gating: bool = False
    norm: str = "layer_norm"
    context: int = 250
    max_period: int = 10000
    kv_repeat: int = 1
    dim_feedforward: int = 2048


@dataclass(frozen=True)
class MimiConfig:
    """MimiConfig (Mimi.swift:17-49), the fields the decoder uses."""
    sample_rate: float = 24000.0
    frame_rate: float = 12.5
    seanet: SeanetConfig = field(default_factory=SeanetConfig)
    transformer: MimiTransformerConfig = field(default_factory=MimiTransformerConfig)
    quantizer_nq: int = 32
    quantizer_bins: int = 2048
    quantizer_dim: int = 256

    @property
    def upsample_stride(self) -> int:
        return int(self.sample_rate / int(np.prod(self.seanet.ratios)) / self.frame_rate)          # Mimi.swift:128-129

    @property
    def samples_per_frame(self) -> int:
        return self.upsample_stride * int(np.prod(self.seanet.ratios))

    @staticmethod
    def mimi_202407(num_codebooks: int = 32) -> "MimiConfig":
        return MimiConfig(quantizer_nq=num_codebooks)


def mimi_202407(num_codebooks: int = 32) -> MimiConfig:
    """mimi_202407(numCodebooks:) (Mimi.swift:53-103)."""
    return MimiConfig.mimi_202407(num_codebooks)


def _c_config(cfg: MimiConfig) -> _CConfig:
    s, t = cfg.seanet, cfg.transformer
    return _CConfig(int(cfg.sample_rate), cfg.upsample_stride, cfg.quantizer_nq, cfg.quantizer_bins, cfg.quantizer_dim,
                    s.dimension, s.nfilters, len(s.ratios), (C.c_int32 * 8)(*s.ratios),
                    s.ksize, s.residual_ksize, s.last_ksize, s.nresidual_layers, s.dilation_base, s.compress,
                    int(s.causal), int(s.true_skip), int(s.pad_mode == "constant"),
                    t.d_model, t.num_heads, t.num_layers, t.dim_feedforward, t.context, t.kv_repeat,
                    int(t.gating), int(t.norm == "layer_norm"), int(t.layer_scale is not None), int(t.positional_embedding == "rope"),
                    int(t.max_period))


def _codes(codes) -> np.ndarray:
    """[n_q, T] int32; a leading batch axis of 1 is accepted, as in decodeFrames (Mimi.swift:228)."""
    c = np.asarray(codes)
    if c.ndim == 3 and c.shape[0] == 1:
        c = c[0]
    if c.ndim != 2:
        raise ValueError("codes must be [n_q, T] (or [1, n_q, T])")
    return np.ascontiguousarray(c, np.int32)


class MimiCodec:
    def __init__(self, ctx, h, cfg):
        self.ctx, self.h, self.cfg = ctx, h, cfg
        self._streams = []
        ctx.adopt(self)

    @staticmethod
    def load(ctx: _lib.Context, cfg: MimiConfig, weights: dict[str, np.ndarray]) -> "MimiCodec":
        """weights: float32 under the names Mimi.sanitize produces (checkpoint.sanitize_mimi maps a raw checkpoint)."""
        c = _c_config(cfg)
        views, n, keep = tensor_views(weights)
        h = ctx.lib.mia_mimi_load(ctx.h, C.byref(c), views, n)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return MimiCodec(ctx, h, cfg)

    def output_len(self, n_frames: int) -> int:
        return int(self.ctx.lib.mia_mimi_output_len(self.h, n_frames))

    # ---- encode side (present when the weights carried the encoder tensors)
    @property
    def has_encoder(self) -> bool:
        return self.encode_frames(1) > 0

    def encode_frames(self, n_samples: int) -> int:
        """Code frames of n_samples samples: every strided stage rounds up (0 without an encoder or for n_samples < 1)."""
        return int(self.ctx.lib.mia_mimi_encode_frames(self.h, int(n_samples)))

    def _n_q(self, n_q) -> int:
        return self.cfg.quantizer_nq if n_q is None else int(n_q)

    def encode(self, pcm, n_q: int | None = None) -> np.ndarray:
        """Mimi.encode: float32 [n_samples] at the codec's rate -> int32 [n_q, T], the first n_q stages of the split quantiser."""
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        k = self._n_q(n_q)
        T = self.encode_frames(x.size)
        codes = np.zeros((max(k, 1), max(T, 1)), np.int32)
        nf = C.c_int64(0)
        self.ctx.check(self.ctx.lib.mia_mimi_encode(self.h, x.ctypes.data if x.size else None, x.size, k, codes.ctypes.data, max(T, 1), C.byref(nf), _lib.MEM_HOST))
        return np.ascontiguousarray(codes.reshape(-1)[:k * nf.value].reshape(k, nf.value))

    def encode_latent(self, pcm) -> np.ndarray:
        """The rows the quantiser sees: float32 [T, d_model] (SEANet encoder, encoder transformer, edge-padded downsample)."""
        x = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        T = max(self.encode_frames(x.size), 1)
        lat = np.empty((T, self.cfg.transformer.d_model), np.float32)
        nf = C.c_int64(0)
        self.ctx.check(self.ctx.lib.mia_mimi_encode_latent(self.h, x.ctypes.data if x.size else None, x.size, lat.ctypes.data, T, C.byref(nf), _lib.MEM_HOST))
        return lat[:nf.value]

    def quantize(self, latent, n_q: int | None = None) -> np.ndarray:
        """SplitResidualVectorQuantizer.encode alone: float32 [T, d_model] -> int32 [n_q, T]."""
        z = np.ascontiguousarray(latent, np.float32)
        if z.ndim != 2 or z.shape[1] != self.cfg.transformer.d_model:
            raise ValueError(f"latent must be [T, {self.cfg.transformer.d_model}]")
        k = self._n_q(n_q)
        codes = np.zeros((max(k, 1), max(z.shape[0], 1)), np.int32)
        self.ctx.check(self.ctx.lib.mia_mimi_quantize(self.h, z.ctypes.data if z.size else None, z.shape[0], k, codes.ctypes.data, _lib.MEM_HOST))
        return codes[:k, :z.shape[0]]

    def decode(self, codes) -> np.ndarray:
        """Mimi.decode: codes int [n_q, T] -> float32 [T * samples_per_frame] (full bidirectional attention over the clip)."""
        c = _codes(codes)
        n_q, T = c.shape
        pcm = np.empty(max(T * self.cfg.samples_per_frame, 1), np.float32)
        ns = C.c_int64(0)
        self.ctx.check(self.ctx.lib.mia_mimi_decode(self.h, c.ctypes.data, n_q, T, pcm.ctypes.data, pcm.size, C.byref(ns), _lib.MEM_HOST))
        return pcm[:ns.value]

    def new_stream(self) -> "MimiStream":
        h = self.ctx.lib.mia_mimi_stream_create(self.h)
        if not h:
            raise _lib.MiaError(_lib.ERR_OUT_OF_MEMORY, self.ctx.lib.mia_last_error(self.ctx.h).decode())
        s = MimiStream(self, h)
        import weakref
        self._streams.append(weakref.ref(s))
        return s

    def close(self):
        if self.h and getattr(self.ctx, "h", None):
            for ref in self._streams:               # a stream points into its codec: release it first
                s = ref()
                if s is not None:
                    s.close()
            self._streams = []
            self.ctx.lib.mia_mimi_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MimiStream:
    """MimiStreamingDecoder: device-resident state carried from call to call."""

    def __init__(self, codec: MimiCodec, h):
        self.codec, self.h = codec, h

    def decode_frames(self, codes) -> np.ndarray:
        """decodeFrames: codes int [n_q, n] -> float32 [n * samples_per_frame], one pass over the n frames."""
        c = _codes(codes)
        n_q, n = c.shape
        ctx = self.codec.ctx
        ns = C.c_int64(0)
        pcm = np.empty(max(n * self.codec.cfg.samples_per_frame, 1), np.float32)
        ctx.check(ctx.lib.mia_mimi_stream_decode(self.h, c.ctypes.data, n_q, n, pcm.ctypes.data, pcm.size, C.byref(ns), _lib.MEM_HOST))
        return pcm[:ns.value]

    def reset(self) -> None:
        self.codec.ctx.check(self.codec.ctx.lib.mia_mimi_stream_reset(self.h))

    def close(self) -> None:
        if self.h and self.codec.h and getattr(self.codec.ctx, "h", None):
            self.codec.ctx.lib.mia_mimi_stream_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
