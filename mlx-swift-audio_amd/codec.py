"""Host-side mirror of the reference's codec-decoder interface, backed by the gfx950 HIP layer (include/mia.h):
SNACDecoder.decode(codes:) (TTS/Orpheus/SNAC/SNACDecoder.swift:281-289) and DACCodec.decodeFromCodes
(Codec/DAC/DACModel.swift:303-306).  No arithmetic happens in Python."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import DacConfig, DacEncoderConfig, SnacConfig, tensor_views


MAX_BATCH = 64          # utterances per mia_*_decode_batch call


class _Codec:
    def __init__(self, ctx, h, cfg):
        self.ctx, self.h, self.cfg = ctx, h, cfg
        ctx.adopt(self)

    def output_len(self, latent_len: int) -> int:
        return int(self.ctx.lib.mia_codec_output_len(self.h, latent_len))

    def noise_len(self, latent_len: int) -> int:
        return int(self.ctx.lib.mia_codec_noise_len(self.h, latent_len))

    def set_stack_budget(self, n_bytes: int) -> None:
        """mia_codec_set_stack_budget: up to which activation size a stage of decode_batch runs stacked (negative = default)."""
        self.ctx.check(self.ctx.lib.mia_codec_set_stack_budget(self.h, n_bytes))

    def close(self):
        if self.h and getattr(self.ctx, 'h', None):
            self.ctx.lib.mia_codec_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SNACDecoder(_Codec):
    @staticmethod
    def load(ctx: _lib.Context, cfg, weights: dict[str, np.ndarray]) -> "SNACDecoder":
        c = SnacConfig(cfg.latent_dim, cfg.decoder_dim, len(cfg.decoder_rates), (C.c_int32 * 8)(*cfg.decoder_rates), len(cfg.vq_strides),
                       (C.c_int32 * 4)(*cfg.vq_strides), cfg.codebook_size, cfg.codebook_dim, 1 if cfg.noise else 0, 1 if cfg.depthwise else 0)
        views, n, keep = tensor_views(weights)
        h = ctx.lib.mia_snac_load(ctx.h, C.byref(c), views, n)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return SNACDecoder(ctx, h, cfg)

    def decode(self, codes: list[list[int]], noise: np.ndarray | None = None) -> np.ndarray:
        """decode(codes:) -> float32 [samples]; `noise` = explicit N(0,1) draws for the NoiseBlocks (None = none)."""
        arrs = [np.ascontiguousarray(c, np.int32) for c in codes]
        n = np.asarray([a.size for a in arrs], np.int32)
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        T0 = max(int(a.size) * s for a, s in zip(arrs, self.cfg.vq_strides))
        pcm = np.empty(self.output_len(T0), np.float32)
        ns = C.c_int64(0)
        nz = None if noise is None else np.ascontiguousarray(noise, np.float32)
        self.ctx.check(self.ctx.lib.mia_snac_decode(self.h, ptrs, n.ctypes.data, len(arrs), None if nz is None else nz.ctypes.data,
                                                    0 if nz is None else nz.size, pcm.ctypes.data, pcm.size, C.byref(ns), _lib.MEM_HOST))
        return pcm[:ns.value]

    def decode_batch(self, codes_list: list[list[list[int]]], noises: list | None = None) -> list[np.ndarray]:
        """mia_snac_decode_batch: several utterances in one pass (at most MAX_BATCH); codes_list[u] is what decode() takes, noises a
        matching list of arrays or None.  Every waveform equals its own decode(...) bit for bit."""
        U, nl = len(codes_list), max(len(c) for c in codes_list)
        n = np.zeros((U, nl), np.int32)
        flat, T0 = [], []
        for u, codes in enumerate(codes_list):
            arrs = [np.ascontiguousarray(c, np.int32).reshape(-1) for c in codes]
            n[u, :len(arrs)] = [a.size for a in arrs]
            flat += arrs
            T0.append(max([int(a.size) * s for a, s in zip(arrs, self.cfg.vq_strides)], default=0))
        codes = np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros(0, np.int32))
        nz = None if noises is None else np.ascontiguousarray(np.concatenate([np.asarray(z, np.float32).reshape(-1) for z in noises]))
        off = np.zeros(U + 1, np.int64)
        off[1:] = np.cumsum([self.output_len(t) for t in T0])
        pcm = np.empty(max(int(off[-1]), 1), np.float32)
        ns = np.zeros(U, np.int64)
        self.ctx.check(self.ctx.lib.mia_snac_decode_batch(self.h, U, codes.ctypes.data, n.ctypes.data, nl, None if nz is None else nz.ctypes.data,
                                                          0 if nz is None else nz.size, pcm.ctypes.data, off.ctypes.data, ns.ctypes.data, _lib.MEM_HOST))
        return [pcm[off[u]:off[u] + ns[u]].copy() for u in range(U)]


class DACCodec(_Codec):
    @staticmethod
    def load(ctx: _lib.Context, cfg, weights: dict[str, np.ndarray]) -> "DACCodec":
        c = DacConfig(cfg.latent_dim, cfg.decoder_dim, len(cfg.decoder_rates), (C.c_int32 * 8)(*cfg.decoder_rates), cfg.n_codebooks,
                      cfg.codebook_size, cfg.codebook_dim)
        views, n, keep = tensor_views(weights)
        h = ctx.lib.mia_dac_load(ctx.h, C.byref(c), views, n)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        codec = DACCodec(ctx, h, cfg)
        if "encoder.block.layers.0.weight_v" in weights:            # checkpoints carry the encoder; decode-only callers may drop it
            e = DacEncoderConfig(cfg.encoder_dim, len(cfg.encoder_rates), (C.c_int32 * 8)(*cfg.encoder_rates))
            ctx.check(ctx.lib.mia_dac_load_encoder(h, C.byref(e), views, n))
        return codec

    def encode(self, audio: np.ndarray, n_quantizers: int | None = None) -> np.ndarray:
        """DACCodec.encode(_:nQuantizers:) for one mono sequence (DACModel.swift:284-296): float32 [samples] -> codes int32 [n_q, T]."""
        if hasattr(audio, "device_ptr"):
            return self._encode_resident(audio, n_quantizers)
        a = np.ascontiguousarray(audio, np.float32).reshape(-1)
        T = int(self.ctx.lib.mia_dac_code_len(self.h, a.size))
        nq = self.cfg.n_codebooks if not n_quantizers else min(n_quantizers, self.cfg.n_codebooks)
        codes = np.zeros((nq, max(T, 1)), np.int32)
        ns = C.c_int64(0)
        self.ctx.check(self.ctx.lib.mia_dac_encode(self.h, a.ctypes.data, a.size, nq, codes.ctypes.data, codes.shape[1], C.byref(ns), _lib.MEM_HOST))
        return codes[:, :ns.value]

    def _encode_resident(self, audio, n_quantizers: int | None = None) -> np.ndarray:
        """encode of an outetts.SpeakerAudio: the clip is read where it lies (device mode, no upload); the codes land in a torch
        buffer on the same device and come back once."""
        import torch
        n = len(audio)
        T = int(self.ctx.lib.mia_dac_code_len(self.h, n))
        nq = self.cfg.n_codebooks if not n_quantizers else min(n_quantizers, self.cfg.n_codebooks)
        codes = torch.zeros((nq, max(T, 1)), dtype=torch.int32, device=f"cuda:{self.ctx.device}")
        torch.cuda.synchronize(self.ctx.device)               # the buffer's zero fill runs on torch's stream, the encode on the context's
        ns = C.c_int64(0)
        self.ctx.check(self.ctx.lib.mia_dac_encode(self.h, audio.device_ptr, n, nq, codes.data_ptr(), codes.shape[1], C.byref(ns), _lib.MEM_DEVICE))
        self.ctx.synchronize()
        return codes[:, :ns.value].cpu().numpy()

    def decode_from_codes(self, codes: np.ndarray) -> np.ndarray:
        """decodeFromCodes: codes int [B, n_codebooks, T] (or [n_codebooks, T]) -> float32 [B, samples] (or [samples]).  B > 1 goes
        through mia_dac_decode_batch, MAX_BATCH sequences per call."""
        codes = np.ascontiguousarray(codes, np.int32)
        single = codes.ndim == 2
        if single:
            codes = codes[None]
        B, ncb, T = codes.shape
        out = np.empty((B, self.output_len(T)), np.float32)
        if B == 1:
            ns = C.c_int64(0)
            self.ctx.check(self.ctx.lib.mia_dac_decode(self.h, codes[0].ctypes.data, ncb, T, out[0].ctypes.data, out.shape[1], C.byref(ns), _lib.MEM_HOST))
        for b in range(0, B if B > 1 else 0, MAX_BATCH):
            n = min(MAX_BATCH, B - b)
            Ts = np.full(n, T, np.int64)
            off = np.arange(n + 1, dtype=np.int64) * out.shape[1]
            ns = np.zeros(n, np.int64)
            self.ctx.check(self.ctx.lib.mia_dac_decode_batch(self.h, n, codes[b].ctypes.data, ncb, Ts.ctypes.data, out[b].ctypes.data, off.ctypes.data,
                                                             ns.ctypes.data, _lib.MEM_HOST))
        return out[0] if single else out

    def decode_batch(self, codes_list: list[np.ndarray]) -> list[np.ndarray]:
        """mia_dac_decode_batch on ragged input: codes_list[u] int [n_codebooks, T_u] (at most MAX_BATCH) -> one float32 [samples_u] each,
        bit-identical to decode_from_codes of each alone."""
        arrs = [np.ascontiguousarray(c, np.int32) for c in codes_list]
        U, ncb = len(arrs), arrs[0].shape[0]
        if any(a.ndim != 2 or a.shape[0] != ncb for a in arrs):
            raise ValueError("decode_batch: every utterance must be [n_codebooks, T]")
        Ts = np.asarray([a.shape[1] for a in arrs], np.int64)
        codes = np.ascontiguousarray(np.concatenate([a.reshape(-1) for a in arrs]))
        off = np.zeros(U + 1, np.int64)
        off[1:] = np.cumsum([self.output_len(int(t)) for t in Ts])
        pcm = np.empty(max(int(off[-1]), 1), np.float32)
        ns = np.zeros(U, np.int64)
        self.ctx.check(self.ctx.lib.mia_dac_decode_batch(self.h, U, codes.ctypes.data, ncb, Ts.ctypes.data, pcm.ctypes.data, off.ctypes.data,
                                                         ns.ctypes.data, _lib.MEM_HOST))
        return [pcm[off[u]:off[u] + ns[u]].copy() for u in range(U)]
