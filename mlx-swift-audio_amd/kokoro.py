"""Host-side mirror of Kokoro's waveform half (TTS/Kokoro), backed by the gfx950 HIP layer: KokoroDecoder.callAsFunction
(Decoder/KokoroDecoder.swift:83-112) with its Generator (Decoder/Generator.swift:133-192), and the F0 / N blocks of
Predictor.F0NTrain behind `shared` (TTSEngine/KokoroModel.swift:66-89).  No arithmetic happens in Python.  Text to phoneme ids, ALBERT,
the text encoder, the BiLSTMs and the alignment stay with the caller ("Kokoro")."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._abi import KokoroConfig as _CConfig, tensor_views


@dataclass(frozen=True)
class KokoroConfig:
    """The constructor arguments of KokoroDecoder and Predictor (KokoroModel.swift:26-64,116-129)."""
    dim_in: int = 512
    style_dim: int = 128
    hidden: int = 1024                 # width of the encode / decode blocks
    asr_res_dim: int = 64
    pred_dim: int = 512                # Predictor's dModel; 0 = no F0 / N blocks
    up_initial: int = 512
    up_rates: tuple = (10, 6)
    up_kernels: tuple = (20, 12)
    res_kernels: tuple = (3, 7, 11)
    dilations: tuple = (1, 3, 5)
    n_fft: int = 20
    hop: int = 5
    n_harmonics: int = 8
    voiced_threshold: int = 10
    sample_rate: int = 24000

    @property
    def upsample_scale(self) -> int:
        """Source samples per generator row (300)."""
        return int(np.prod(self.up_rates)) * self.hop


KOKORO_CONFIGS = {"kokoro_82m": KokoroConfig(),
                  "kokoro_micro": KokoroConfig(dim_in=64, style_dim=32, hidden=96, asr_res_dim=32, pred_dim=64, up_initial=64)}


def _pad4(v):
    return (C.c_int32 * 4)(*(list(v) + [0] * (4 - len(v))))


def _c_config(cfg: KokoroConfig) -> _CConfig:
    return _CConfig(cfg.dim_in, cfg.style_dim, cfg.hidden, cfg.asr_res_dim, cfg.pred_dim, cfg.up_initial, len(cfg.up_rates),
                    _pad4(cfg.up_rates), _pad4(cfg.up_kernels), len(cfg.res_kernels), _pad4(cfg.res_kernels), len(cfg.dilations),
                    _pad4(cfg.dilations), cfg.n_fft, cfg.hop, cfg.n_harmonics, cfg.voiced_threshold, cfg.sample_rate)


def _f32(a, shape, what):
    x = np.ascontiguousarray(a, np.float32)
    if x.shape != tuple(shape):
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: {what} must be {list(shape)} (got {list(x.shape)})")
    return x


class KokoroDecoder:
    def __init__(self, ctx, h, cfg):
        self.ctx, self.h, self.cfg = ctx, h, cfg
        ctx.adopt(self)

    @staticmethod
    def load(ctx: _lib.Context, cfg: KokoroConfig, weights: dict[str, np.ndarray]) -> "KokoroDecoder":
        """weights: float32 under the reference's keys as sanitizeWeights leaves them (checkpoint.sanitize_kokoro maps a raw
        checkpoint).  The predictor.F0 / predictor.N tensors are optional: without them f0n raises."""
        c = _c_config(cfg)
        views, n, keep = tensor_views(weights)
        h = ctx.lib.mia_kokoro_load(ctx.h, C.byref(c), views, n)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return KokoroDecoder(ctx, h, cfg)

    def close(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.mia_kokoro_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def output_len(self, T: int) -> int:
        return int(self.ctx.lib.mia_kokoro_output_len(self.h, int(T)))

    def _noise(self, noise, L):
        if noise is None:
            return None
        return _f32(noise, (L * self.cfg.upsample_scale, self.cfg.n_harmonics + 1), "noise")

    def f0n(self, x, s_pred):
        """x [pred_dim, T] (the output of Predictor.shared, channel-major), s_pred [style_dim] -> (F0 [2 T], N [2 T])."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[0] != self.cfg.pred_dim:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: x must be [{self.cfg.pred_dim}, T]")
        T = x.shape[1]
        s = _f32(s_pred, (self.cfg.style_dim,), "s_pred")
        f0 = np.empty(2 * T, np.float32)
        n = np.empty(2 * T, np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_f0n(self.h, x.ctypes.data, T, s.ctypes.data, f0.ctypes.data, n.ctypes.data, _lib.MEM_HOST))
        return f0, n

    def source(self, f0, noise=None):
        """f0 [L] -> (source [300 L], har [60 L + 1, 22]: magnitudes, then phases)."""
        f = np.ascontiguousarray(f0, np.float32).reshape(-1)
        L = f.shape[0]
        nz = self._noise(noise, L)
        n = L * self.cfg.upsample_scale
        src = np.empty(max(n, 1), np.float32)
        har = np.empty((n // self.cfg.hop + 1, self.cfg.n_fft + 2), np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_source(self.h, f.ctypes.data if L else None, L, nz.ctypes.data if nz is not None else None,
                                                      src.ctypes.data, har.ctypes.data, _lib.MEM_HOST))
        return src[:n], har

    def generate(self, x, s, har):
        """Generator.callAsFunction from a given har: x [up_initial, L], s [style_dim], har [60 L + 1, 22] -> waveform [300 L]."""
        x = np.ascontiguousarray(x, np.float32)
        if x.ndim != 2 or x.shape[0] != self.cfg.up_initial:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: x must be [{self.cfg.up_initial}, L]")
        L = x.shape[1]
        n = L * self.cfg.upsample_scale
        sv = _f32(s, (self.cfg.style_dim,), "s")
        hr = _f32(har, (n // self.cfg.hop + 1, self.cfg.n_fft + 2), "har")
        pcm = np.empty(max(n, 1), np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_generate(self.h, x.ctypes.data, L, sv.ctypes.data, hr.ctypes.data, pcm.ctypes.data, _lib.MEM_HOST))
        return pcm[:n]

    def decode(self, asr, f0, n, s, noise=None):
        """KokoroDecoder.callAsFunction: asr [dim_in, T], F0 [2 T], N [2 T], s [style_dim] -> waveform [600 T]."""
        a = np.ascontiguousarray(asr, np.float32)
        if a.ndim != 2 or a.shape[0] != self.cfg.dim_in:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: asr must be [{self.cfg.dim_in}, T]")
        T = a.shape[1]
        f = _f32(f0, (2 * T,), "F0")
        nn = _f32(n, (2 * T,), "N")
        sv = _f32(s, (self.cfg.style_dim,), "s")
        nz = self._noise(noise, 2 * T)
        ns = 2 * T * self.cfg.upsample_scale
        pcm = np.empty(max(ns, 1), np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_decode(self.h, a.ctypes.data, T, f.ctypes.data, nn.ctypes.data, sv.ctypes.data,
                                                      nz.ctypes.data if nz is not None else None, pcm.ctypes.data, _lib.MEM_HOST))
        return pcm[:ns]

    __call__ = decode


def instance_norm(ctx: _lib.Context, x: np.ndarray, ld: int | None = None):
    """mia_op_instance_norm on a host array x [T, C] (staged through device memory, row stride ld >= C): (mean [C], rstd [C])."""
    import torch
    x = np.ascontiguousarray(x, np.float32)
    T, Cn = x.shape
    ld = Cn if ld is None else int(ld)
    buf = np.zeros((T, ld), np.float32)
    buf[:, :Cn] = x
    dev = torch.device("cuda", ctx.device)
    d = torch.from_numpy(buf).to(dev)
    mean = torch.empty(Cn, dtype=torch.float32, device=dev)
    rstd = torch.empty(Cn, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.mia_op_instance_norm(ctx.h, d.data_ptr(), ld, T, Cn, mean.data_ptr(), rstd.data_ptr()))
    ctx.synchronize()
    return mean.cpu().numpy(), rstd.cpu().numpy()
