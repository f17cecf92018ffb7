"""Host-side mirror of Fun-ASR's audio half (STT/FunASR/FunASRModel.swift:41-58): the fbank + LFR + CMVN front end, the SenseVoice SANM
encoder and the audio adaptor on the gfx950 HIP layer, and FunASRModel = that encoder + the Qwen3 decoder of lm.FunASRDecoder: waveform ->
token ids.  The tokenizer and the prompt builder stay with the caller (text code)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, fields, replace

import numpy as np

from . import _abi, _lib
from .lm import FunASRDecoder


@dataclass
class SenseVoiceConfig:
    """SenseVoiceEncoderConfig + AudioAdaptorConfig (STT/FunASR/Config/FunASRConfig.swift:79-214), in mia_sensevoice_config's order."""
    input_dim: int = 560
    encoder_dim: int = 512
    n_heads: int = 4
    ffn_dim: int = 2048
    kernel_size: int = 11
    sanm_shift: int = 0
    n_encoders0: int = 1
    n_encoders: int = 49
    n_tp_encoders: int = 20
    adaptor_k: int = 2
    llm_dim: int = 1024
    adaptor_ffn_dim: int = 2048
    adaptor_layers: int = 2
    adaptor_heads: int = 8


_MICRO = SenseVoiceConfig(560, 256, 2, 512, 11, 0, 1, 2, 2, 2, 256, 512, 1, 2)
SENSEVOICE_CONFIGS = {
    "sensevoice": SenseVoiceConfig(),
    # head dim stays 128 in both stacks: 256 / 2 heads
    "sensevoice-micro": _MICRO,
    "sensevoice-micro-shift2": replace(_MICRO, sanm_shift=2),
}


def _stack_clips(clips):
    clips = [np.ascontiguousarray(c, np.float32).reshape(-1) for c in clips]
    offs = np.zeros(len(clips) + 1, np.int64)
    np.cumsum([c.size for c in clips], out=offs[1:])
    return np.ascontiguousarray(np.concatenate(clips)), offs


def _split(rows: np.ndarray, counts) -> list[np.ndarray]:
    edges = np.cumsum([0] + [int(n) for n in counts])
    return [rows[edges[i]:edges[i + 1]] for i in range(len(counts))]


def features(ctx: _lib.Context, clips) -> list[np.ndarray]:
    """preprocessAudio (STT/FunASR/FunASRAudio.swift:197-216) per clip of 16 kHz audio: fp32 [ceil((1 + L // 160) / 6), 560] each."""
    pcm, offs = _stack_clips(clips)
    rows = int(ctx.lib.mia_sensevoice_feature_rows(offs.ctypes.data, len(clips)))
    if rows < 0:
        raise _lib.MiaError(_lib.ERR_INVALID_AUDIO, "sensevoice_features: empty clip")
    out = np.zeros((rows, 560), np.float32)
    t = np.zeros(len(clips), np.int32)
    ctx.check(ctx.lib.mia_sensevoice_features(ctx.h, pcm.ctypes.data, offs.ctypes.data, len(clips), out.ctypes.data, t.ctypes.data, 560, _lib.MEM_HOST))
    return _split(out, t)


def log_mel(ctx: _lib.Context, clips) -> list[np.ndarray]:
    """funASRLogMelSpectrogram per clip (mia_op_funasr_logmel, the front end's test tap): fp32 [1 + L // 160, 80], natural log."""
    pcm, offs = _stack_clips(clips)
    frames = [1 + int(offs[i + 1] - offs[i]) // 160 for i in range(len(clips))]
    out = np.zeros((sum(frames), 80), np.float32)
    ctx.check(ctx.lib.mia_op_funasr_logmel(ctx.h, pcm.ctypes.data, offs.ctypes.data, len(clips), out.ctypes.data, _lib.MEM_HOST))
    return _split(out, frames)


class SenseVoiceEncoder:
    def __init__(self, ctx, h, cfg, dtype):
        self.ctx, self.h, self.cfg, self.dtype = ctx, h, cfg, dtype
        ctx.adopt(self)

    @staticmethod
    def load(ctx: _lib.Context, cfg: SenseVoiceConfig, weights: dict[str, np.ndarray], dtype: int = _lib.BF16) -> "SenseVoiceEncoder":
        """weights: float32 arrays under the reference's Module keys (audio_encoder.*, audio_adaptor.*); a quantised checkpoint goes through
        checkpoint.expand_checkpoint first."""
        c = _abi.SensevoiceConfig(*[getattr(cfg, f.name) for f in fields(SenseVoiceConfig)])
        views, n, keep = _abi.tensor_views(weights)
        h = ctx.lib.mia_sensevoice_load(ctx.h, C.byref(c), views, n, dtype)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return SenseVoiceEncoder(ctx, h, cfg, dtype)

    def close(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.mia_sensevoice_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def features(self, clips) -> list[np.ndarray]:
        return features(self.ctx, clips)

    def encode(self, feats, want_encoder_out: bool = False):
        """SenseVoiceEncoder + AudioAdaptor on a list of feature arrays [T_b, input_dim], stacked in one pass: the audio embeddings
        [(T_b - 1) // k + 1, llm_dim] per utterance (and the encoder outputs [T_b, encoder_dim] when asked for)."""
        c = self.cfg
        feats = [np.ascontiguousarray(f, np.float32).reshape(-1, c.input_dim) for f in feats]
        t = np.ascontiguousarray([f.shape[0] for f in feats], np.int32)
        flat = np.ascontiguousarray(np.concatenate(feats, axis=0))
        n = np.zeros(len(feats), np.int32)
        enc = np.zeros((int(t.sum()), c.encoder_dim), np.float32) if want_encoder_out else None
        emb = np.zeros((int(((t - 1) // c.adaptor_k + 1).sum()), c.llm_dim), np.float32)
        self.ctx.check(self.ctx.lib.mia_sensevoice_encode(self.h, flat.ctypes.data, t.ctypes.data, len(feats), None if enc is None else enc.ctypes.data,
                                                          emb.ctypes.data, n.ctypes.data, _lib.MEM_HOST))
        embs = _split(emb, n)
        return (_split(enc, t), embs) if want_encoder_out else embs

    def encode_audio(self, clips) -> list[np.ndarray]:
        """features -> encode with nothing leaving the device in between: the audio embeddings per clip."""
        pcm, offs = _stack_clips(clips)
        rows = int(self.ctx.lib.mia_sensevoice_feature_rows(offs.ctypes.data, len(clips)))
        if rows < 0:
            raise _lib.MiaError(_lib.ERR_INVALID_AUDIO, "sensevoice_encode_audio: empty clip")
        emb = np.zeros((rows, self.cfg.llm_dim), np.float32)
        n = np.zeros(len(clips), np.int32)
        self.ctx.check(self.ctx.lib.mia_sensevoice_encode_audio(self.h, pcm.ctypes.data, offs.ctypes.data, len(clips), emb.ctypes.data, n.ctypes.data, _lib.MEM_HOST))
        return _split(emb, n)


class FunASRModel:
    """FunASRModel (STT/FunASR/FunASRModel.swift) from the waveform to token ids: encodeAudio on the SenseVoice handle, mergeEmbeddings and
    the greedy loop on the decoder (FunASRSTT.transcribe, STT/FunASR/FunASRSTT.swift:111-156)."""

    def __init__(self, encoder: SenseVoiceEncoder, decoder: FunASRDecoder):
        if encoder.cfg.llm_dim != decoder.lm.cfg.hidden:
            raise ValueError(f"adaptor llm_dim {encoder.cfg.llm_dim} != decoder hidden {decoder.lm.cfg.hidden}")
        self.encoder, self.decoder = encoder, decoder

    def encode_audio(self, pcm):
        """One clip -> its audio embeddings [n, llm_dim]; a list of clips -> a list of them (one stacked pass)."""
        if isinstance(pcm, (list, tuple)):
            return self.encoder.encode_audio(pcm)
        return self.encoder.encode_audio([pcm])[0]

    def transcribe_tokens(self, pcm, input_ids, sos_id: int, eos_id: int, stop_ids, max_tokens: int = 512,
                          temperature: float = 0.0, top_p: float = 0.95, top_k: int = 0, uniforms=None):
        """One clip + its prompt ids -> token ids (FunASRDecoder.transcribe_tokens on the clip's audio rows).  A list of clips, with one
        prompt per clip, is encoded in one stacked pass and decoded side by side (generate_greedy_batch; lm.set_batch(n) first).
        temperature > 0 samples (top-k, then top-p, FunASRModel.swift:165-198) with the caller's uniforms: [max_tokens] for one clip,
        [n, max_tokens] for a list."""
        if temperature != 0 and uniforms is None:
            raise ValueError("temperature > 0 needs `uniforms`: the draw takes explicit uniforms")
        if not isinstance(pcm, (list, tuple)):
            return self.decoder.transcribe_tokens(input_ids, self.encode_audio(pcm), sos_id, eos_id, stop_ids, max_tokens, temperature, top_p, top_k, uniforms)
        embs = self.encode_audio(list(pcm))
        prompts = [self.decoder.merge_embeddings(ids, e, sos_id, eos_id) for ids, e in zip(input_ids, embs)]
        if temperature == 0:
            return self.decoder.lm.generate_greedy_batch(prompts, stop_ids, max_tokens)
        return self.decoder.lm.generate_topk_batch(prompts, uniforms, stop_ids, max_tokens, temperature, top_p, top_k)
