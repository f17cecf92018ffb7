"""CPU reference for Fun-ASR's audio half (test helper): the fbank + LFR + CMVN front end in fp64 numpy, the SenseVoice SANM encoder
and the audio adaptor in fp32 torch.  Restated from the reference's Swift, cited per function:

  STT/FunASR/FunASRAudio.swift                          front end (window :35-45, log-mel :57-94, LFR :108-154, CMVN :165-180,
                                                        STFT :240-277, reflect pad :280-310, filterbank :322-396)
  STT/FunASR/Layers/MultiHeadAttentionSANM.swift        SANM attention :124-175, FSMN :90-116, plain MHA :221-260
  STT/FunASR/Layers/EncoderLayerSANM.swift              SANM layer :75-94, adaptor block :144-158
  STT/FunASR/Layers/SenseVoiceEncoder.swift             stack order :98-135
  STT/FunASR/Layers/AudioAdaptor.swift                  :67-118
  Codec/S3Gen/Transformer/PositionwiseFeedForward.swift w_2(relu(w_1 x))
  STT/FunASR/FunASRModel.swift:41-58                    encodeAudio

tests/test_sensevoice_ref.py pins these against torch's own attention, conv1d and LayerNorm.  `round_kind` ("bf16" | "f16" | None) rounds
every GEMM operand (activation and weight) the way the device's 16-bit GEMMs see them; nothing else of the arithmetic changes.  The three
`mutate` switches exist for the discriminating checks only."""
from __future__ import annotations

import math

import numpy as np
import torch

SAMPLE_RATE, N_FFT, HOP, N_MELS, LFR_M, LFR_N = 16000, 400, 160, 80, 7, 6      # FunASRAudio.swift:13-20

# max / mean |device - reference| of a LayerNorm-ed output: the Whisper encoder's bounds (tests/test_whisper_gpu.py); the adaptor's output
# is held to the same two numbers times the reference output's standard deviation
BOUNDS = {"bf16": (0.06, 0.008), "f16": (0.01, 0.0015)}


# ---- front end (fp64) ---------------------------------------------------------------------------------------------------------------
def hamming_window(n: int = N_FFT) -> np.ndarray:
    """hammingWindow (:35-45): symmetric, 0.54 - 0.46 cos(2 pi i / (n - 1))."""
    if n == 1:
        return np.ones(1)
    return 0.54 - 0.46 * np.cos(np.arange(n, dtype=np.float64) * (2.0 * math.pi / (n - 1)))


def reflect_pad(x: np.ndarray, pad: int) -> np.ndarray:
    """reflectPad1D (:280-310) for a clip longer than the padding (the short-clip loops of :299-307 are not restated: the device
    refuses clips of <= 200 samples)."""
    n = len(x)
    assert n > pad
    return np.concatenate([x[1:pad + 1][::-1], x, x[n - pad - 1:n - 1][::-1]])


def mel_filters(n_mels: int = N_MELS, n_fft: int = N_FFT, sr: int = SAMPLE_RATE) -> np.ndarray:
    """funASRMelFilters (:322-396), HTK scale, Slaney normalisation -> [n_mels, n_fft / 2].  The bin frequencies are
    linspace(0, sr / 2, n_fft / 2) (:363-364), i.e. 8000 / 199 Hz apart and not the DFT's 40 Hz: the reference's own grid, kept."""
    n_freqs = n_fft // 2
    all_freqs = np.linspace(0.0, sr / 2.0, n_freqs)
    m_max = 2595.0 * math.log10(1.0 + (sr / 2.0) / 700.0)
    m_pts = np.linspace(0.0, m_max, n_mels + 2)
    f_pts = 700.0 * (np.power(10.0, m_pts / 2595.0) - 1.0)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = np.maximum(0.0, np.minimum(down, up))
    fb = fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels]))[None, :]
    return fb.T


def mel_power(pcm: np.ndarray) -> np.ndarray:
    """The mel energies before the clamp and the log (:64-88) -> [1 + L / 160, 80]."""
    x = reflect_pad(np.asarray(pcm, np.float64), N_FFT // 2)
    n_frames = 1 + (len(x) - N_FFT) // HOP                      # :262 -- the last frame is kept
    idx = np.arange(n_frames)[:, None] * HOP + np.arange(N_FFT)[None, :]
    spec = np.fft.rfft(x[idx] * hamming_window()[None, :], axis=1)[:, :N_FFT // 2]      # bins 0 .. 199 (:76)
    return (np.abs(spec) ** 2) @ mel_filters().T


def log_mel(pcm: np.ndarray) -> np.ndarray:
    """funASRLogMelSpectrogram (:57-94): ln(max(mel, 1e-10))."""
    return np.log(np.maximum(mel_power(pcm), 1e-10))


def n_frames_of(n_samples: int) -> int:
    return 1 + n_samples // HOP


def t_lfr_of(n_samples: int) -> int:
    return -(-n_frames_of(n_samples) // LFR_N)                  # ceil(T / 6) (:117)


def apply_lfr(feats: np.ndarray, m: int = LFR_M, n: int = LFR_N) -> np.ndarray:
    """applyLFR (:108-154), written as the reference writes it: pad, then gather."""
    T = feats.shape[0]
    t_lfr = -(-T // n)
    left = (m - 1) // 2
    padded = np.concatenate([np.repeat(feats[:1], left, axis=0), feats], axis=0)
    need = (t_lfr - 1) * n + m
    if need > padded.shape[0]:
        padded = np.concatenate([padded, np.repeat(padded[-1:], need - padded.shape[0], axis=0)], axis=0)
    idx = np.arange(t_lfr)[:, None] * n + np.arange(m)[None, :]
    return padded[idx].reshape(t_lfr, m * feats.shape[1])


def apply_cmvn(feats: np.ndarray) -> np.ndarray:
    """applyCMVN without precomputed statistics (:176-179): population variance, eps added to the standard deviation."""
    mean = feats.mean(axis=0, keepdims=True)
    std = np.sqrt(feats.var(axis=0, keepdims=True)) + 1e-6
    return (feats - mean) / std


def features(pcm: np.ndarray) -> np.ndarray:
    """preprocessAudio (:197-216)."""
    return apply_cmvn(apply_lfr(log_mel(pcm)))


# ---- model (fp32 torch) -------------------------------------------------------------------------------------------------------------
def _round(t: torch.Tensor, kind) -> torch.Tensor:
    if kind is None:
        return t
    return t.to(torch.bfloat16 if kind == "bf16" else torch.float16).to(torch.float32)


def fsmn_taps(w: np.ndarray, D: int) -> np.ndarray:
    """fsmn_block.weight as the checkpoint ([D][1][K], torch Conv1d) or as MLX holds it ([D][K][1], FunASRModel.sanitize) -> [K][D]."""
    w = np.asarray(w, np.float32)
    assert w.ndim == 3 and w.shape[0] == D and 1 in w.shape[1:], w.shape
    return np.ascontiguousarray(w.reshape(D, -1).T)


def fsmn_pads(kernel_size: int, sanm_shift: int) -> tuple[int, int]:
    """MultiHeadAttentionSANM.init (:73-79)."""
    left = (kernel_size - 1) // 2 + (sanm_shift if sanm_shift > 0 else 0)
    return left, kernel_size - 1 - left


def fsmn_memory(v: torch.Tensor, taps: torch.Tensor, left: int) -> torch.Tensor:
    """forwardFSMN without a mask (:90-116): v [T, D], taps [K, D] -> conv(pad(v)) + v."""
    T, D = v.shape
    K = taps.shape[0]
    padded = torch.cat([v.new_zeros(left, D), v, v.new_zeros(K - 1 - left, D)], dim=0)
    out = v.clone()
    for k in range(K):
        out = out + taps[k][None, :] * padded[k:k + T]
    return out


def mha(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, n_heads: int) -> torch.Tensor:
    """scaledDotProductAttention with scale d_k^-0.5 (:155-162, :245-251): [T, D] each -> [T, D]."""
    T, D = q.shape
    dk = D // n_heads
    qh, kh, vh = (t.reshape(T, n_heads, dk).transpose(0, 1) for t in (q, k, v))
    s = (qh @ kh.transpose(1, 2)) * (dk ** -0.5)
    return (torch.softmax(s, dim=-1) @ vh).transpose(0, 1).reshape(T, D)


def layer_norm(x: torch.Tensor, g: torch.Tensor, b: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


class SenseVoiceRef:
    def __init__(self, cfg, weights: dict, round_kind=None, mutate: str | None = None):
        assert mutate in (None, "zero_fsmn", "layer0_residual", "no_input_scale")
        self.cfg, self.kind, self.mutate = cfg, round_kind, mutate
        self.w = {k: torch.from_numpy(np.asarray(v, np.float32)) for k, v in weights.items()}

    def _lin(self, x, name, relu=False):
        y = _round(x, self.kind) @ _round(self.w[name + ".weight"], self.kind).t() + self.w[name + ".bias"]
        return torch.relu(y) if relu else y

    def _ln(self, x, name):
        return layer_norm(x, self.w[name + ".weight"], self.w[name + ".bias"])

    def _ffn(self, x, p):
        return self._lin(self._lin(x, p + ".w_1", relu=True), p + ".w_2")

    def sanm_attention(self, x, p):
        """MultiHeadAttentionSANM.callAsFunction (:124-175).  The device keeps q | k | v in the 16-bit type: so does the rounded run."""
        c = self.cfg
        D = c.encoder_dim
        q, k, v = _round(self._lin(x, p + ".linear_q_k_v"), self.kind).split(D, dim=-1)
        taps = torch.from_numpy(fsmn_taps(self.w[p + ".fsmn_block.weight"].numpy(), D))
        if self.mutate == "zero_fsmn":
            taps = torch.zeros_like(taps)
        left, right = fsmn_pads(c.kernel_size, c.sanm_shift)
        assert right >= 0
        ctx = _round(mha(q, k, v, c.n_heads), self.kind)
        return self._lin(ctx, p + ".linear_out") + fsmn_memory(v, taps, left)

    def sanm_layer(self, x, p, in_size):
        """EncoderLayerSANM.callAsFunction (:75-94)."""
        out = self.sanm_attention(self._ln(x, p + ".norm1"), p + ".self_attn")
        if in_size == self.cfg.encoder_dim:
            out = out + x
        elif self.mutate == "layer0_residual":
            out = out + x[:, :self.cfg.encoder_dim]
        return out + self._ffn(self._ln(out, p + ".norm2"), p + ".feed_forward")

    def encode(self, feats: np.ndarray) -> torch.Tensor:
        """SenseVoiceEncoder.callAsFunction (:98-135) on one utterance: [T, input_dim] -> [T, encoder_dim]."""
        c = self.cfg
        x = torch.from_numpy(np.asarray(feats, np.float32))
        if self.mutate != "no_input_scale":
            x = x * float(math.sqrt(c.encoder_dim))
        for i in range(c.n_encoders0):
            x = self.sanm_layer(x, f"audio_encoder.encoders0.{i}", c.input_dim if i == 0 else c.encoder_dim)
        for i in range(c.n_encoders):
            x = self.sanm_layer(x, f"audio_encoder.encoders.{i}", c.encoder_dim)
        x = self._ln(x, "audio_encoder.after_norm")
        for i in range(c.n_tp_encoders):
            x = self.sanm_layer(x, f"audio_encoder.tp_encoders.{i}", c.encoder_dim)
        return self._ln(x, "audio_encoder.tp_norm")

    def adapt(self, enc: torch.Tensor) -> torch.Tensor:
        """AudioAdaptor.callAsFunction (:67-118) on one utterance: [T, encoder_dim] -> [(T - 1) / k + 1, llm_dim]."""
        c = self.cfg
        T, D = enc.shape
        n = (T - 1) // c.adaptor_k + 1
        x = torch.cat([enc, enc.new_zeros(n * c.adaptor_k - T, D)], dim=0).reshape(n, D * c.adaptor_k)
        x = self._lin(self._lin(x, "audio_adaptor.linear1", relu=True), "audio_adaptor.linear2")
        for i in range(c.adaptor_layers):
            p = f"audio_adaptor.blocks.{i}"
            h = self._ln(x, p + ".norm1")                                       # FunASREncoderLayer (:144-158)
            q, k, v = (_round(self._lin(h, f"{p}.self_attn.linear_{n_}"), self.kind) for n_ in "qkv")
            x = x + self._lin(_round(mha(q, k, v, c.adaptor_heads), self.kind), p + ".self_attn.linear_out")
            x = x + self._ffn(self._ln(x, p + ".norm2"), p + ".feed_forward")
        return x

    def encode_audio(self, feats: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
        """FunASRModel.encodeAudio (:41-58) from the features on: (encoder output, audio embeddings)."""
        with torch.no_grad():
            enc = self.encode(feats)
            return enc.numpy(), self.adapt(enc).numpy()
