"""Host-side mirror of Kokoro (TTS/Kokoro), backed by the gfx950 HIP layer.  Waveform half (KokoroDecoder): KokoroDecoder.callAsFunction
(Decoder/KokoroDecoder.swift:83-112) with its Generator (Decoder/Generator.swift:133-192), and the F0 / N blocks of
Predictor.F0NTrain behind `shared` (TTSEngine/KokoroModel.swift:66-89).  Text half (KokoroText): DurationEncoder, predictor.lstm and the
duration head, TextEncoder, the alignment and predictor.shared (KokoroTTS.swift:303-407).  KokoroBert: ALBERT and bert_encoder
(TTS/Kokoro/Albert, KokoroTTS.swift:262-287).  KokoroPipeline chains them from padded phoneme ids (or from a d_en the caller brings) to
PCM.  No arithmetic happens in Python.  Text to phoneme ids and reading voice-pack files stay with the caller ("Kokoro")."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._abi import KokoroBertConfig as _CBertConfig, KokoroConfig as _CConfig, KokoroTextConfig as _CTextConfig, tensor_views


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
    d_model: int = 512                 # text half: Predictor's dModel = TextEncoder's channels (= dim_in = pred_dim)
    n_symbols: int = 178
    text_kernel: int = 5
    text_depth: int = 3
    bert_embed: int = 128              # ALBERT (AlbertConfig.swift); its vocabulary is n_symbols, bert_encoder's output width d_model
    bert_hidden: int = 768
    bert_heads: int = 12
    bert_intermediate: int = 2048
    bert_layers: int = 12
    bert_positions: int = 512
    bert_types: int = 2

    @property
    def upsample_scale(self) -> int:
        """Source samples per generator row (300)."""
        return int(np.prod(self.up_rates)) * self.hop


KOKORO_CONFIGS = {"kokoro_82m": KokoroConfig(),
                  "kokoro_micro": KokoroConfig(dim_in=64, style_dim=32, hidden=96, asr_res_dim=32, pred_dim=64, up_initial=64,
                                               d_model=64, n_symbols=24, bert_embed=32, bert_hidden=128, bert_heads=2,
                                               bert_intermediate=192, bert_layers=3, bert_positions=160)}


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

    def use_w16(self, on: bool = True) -> None:
        """Run the tap-GEMM convolutions of f0n / generate / decode on bf16 copies of the folded weights (formed by the first on=True;
        the activations stay fp32 and are not rounded).  on=False returns to the fp32 weights.  Off by default."""
        self.ctx.check(self.ctx.lib.mia_kokoro_use_w16(self.h, 1 if on else 0))

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


LSTM_KEYS = tuple(f"{t}_l0{d}" for d in ("", "_reverse") for t in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def bilstm(ctx: _lib.Context, x: np.ndarray, weights: dict[str, np.ndarray]):
    """mia_op_bilstm on a host array x [T, In] (staged through device memory) with the eight tensors of one BiLSTM under LSTM_KEYS:
    -> [T, 2 H], forward | reverse."""
    import torch
    x = np.ascontiguousarray(x, np.float32)
    T, In = x.shape
    H = int(np.asarray(weights["weight_hh_l0"]).shape[-1])
    dev = torch.device("cuda", ctx.device)
    w = [torch.from_numpy(np.ascontiguousarray(weights[k], np.float32)).to(dev) for k in LSTM_KEYS]
    d = torch.from_numpy(x).to(dev)
    out = torch.empty((T, 2 * H), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.check(ctx.lib.mia_op_bilstm(ctx.h, d.data_ptr(), In, T, In, H, *[t.data_ptr() for t in w], out.data_ptr(), 2 * H))
    ctx.synchronize()
    return out.cpu().numpy()


class KokoroText:
    """The text half behind ALBERT.  Token-side arrays are time-major [N, C]; `asr` and the output of `shared` are channel-major, as
    KokoroDecoder takes them."""

    def __init__(self, ctx, h, cfg):
        self.ctx, self.h, self.cfg = ctx, h, cfg
        ctx.adopt(self)

    @staticmethod
    def load(ctx: _lib.Context, cfg: KokoroConfig, weights: dict[str, np.ndarray]) -> "KokoroText":
        """weights: float32 under the reference's sanitised keys (checkpoint.sanitize_kokoro(raw, text=True))."""
        c = _CTextConfig(cfg.d_model, cfg.style_dim, cfg.n_symbols, cfg.text_kernel, cfg.text_depth)
        views, n, keep = tensor_views(weights)
        h = ctx.lib.mia_kokoro_text_load(ctx.h, C.byref(c), views, n)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return KokoroText(ctx, h, cfg)

    def close(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.mia_kokoro_text_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def width(self) -> int:
        return self.cfg.d_model + self.cfg.style_dim

    def durations(self, d_en, s_pred, speed: float = 1.0):
        """d_en [N, d_model], s_pred [style_dim] -> (d [N, d_model + style_dim], durations int32 [N], their value before rounding [N])."""
        x = np.ascontiguousarray(d_en, np.float32)
        if x.ndim != 2 or x.shape[1] != self.cfg.d_model:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: d_en must be [N, {self.cfg.d_model}]")
        N = x.shape[0]
        s = _f32(s_pred, (self.cfg.style_dim,), "s_pred")
        d = np.empty((N, self.width), np.float32)
        dur = np.empty(max(N, 1), np.int32)
        raw = np.empty(max(N, 1), np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_text_durations(self.h, x.ctypes.data, N, s.ctypes.data, float(speed), d.ctypes.data,
                                                              dur.ctypes.data, raw.ctypes.data, _lib.MEM_HOST))
        return d, dur[:N], raw[:N]

    def encode(self, ids):
        """ids [N] (padded as the reference pads them) -> t_en [N, d_model]."""
        i = np.ascontiguousarray(ids, np.int32).reshape(-1)
        out = np.empty((i.shape[0], self.cfg.d_model), np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_text_encode(self.h, i.ctypes.data, i.shape[0], out.ctypes.data, _lib.MEM_HOST))
        return out

    def align(self, d, t_en, dur):
        """d [N, d_model + style_dim], t_en [N, d_model], durations [N] -> (en [T, d_model + style_dim], asr [d_model, T]), T = sum."""
        dur = np.ascontiguousarray(dur, np.int32).reshape(-1)
        N = dur.shape[0]
        d = _f32(d, (N, self.width), "d")
        t = _f32(t_en, (N, self.cfg.d_model), "t_en")
        cap = int(min(max(int(dur.astype(np.int64).sum()), 1), 10001))
        en = np.empty((cap, self.width), np.float32)
        asr = np.empty(cap * self.cfg.d_model, np.float32)
        T = C.c_int(cap)
        self.ctx.check(self.ctx.lib.mia_kokoro_text_align(self.h, d.ctypes.data, t.ctypes.data, dur.ctypes.data, N, en.ctypes.data,
                                                          asr.ctypes.data, C.byref(T), _lib.MEM_HOST))
        return en[:T.value], asr[:T.value * self.cfg.d_model].reshape(self.cfg.d_model, T.value)

    def shared(self, en):
        """en [T, d_model + style_dim] -> predictor.shared's output [d_model, T], what KokoroDecoder.f0n takes."""
        e = np.ascontiguousarray(en, np.float32)
        if e.ndim != 2 or e.shape[1] != self.width:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: en must be [T, {self.width}]")
        T = e.shape[0]
        x = np.empty((self.cfg.d_model, max(T, 1)), np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_text_shared(self.h, e.ctypes.data, T, x.ctypes.data, _lib.MEM_HOST))
        return x


class KokoroBert:
    """ALBERT and bert_encoder (TTS/Kokoro/Albert, KokoroTTS.swift:262-287): padded phoneme ids -> d_en, what KokoroText.durations
    takes.  One shared layer applied cfg.bert_layers times; B = 1, so the all-ones attention mask adds zero and is not implemented."""

    def __init__(self, ctx, h, cfg):
        self.ctx, self.h, self.cfg = ctx, h, cfg
        ctx.adopt(self)

    @staticmethod
    def load(ctx: _lib.Context, cfg: KokoroConfig, weights: dict[str, np.ndarray]) -> "KokoroBert":
        """weights: float32 under the checkpoint's own names (checkpoint.sanitize_kokoro(raw, bert=True)); bert.pooler.* is ignored."""
        c = _CBertConfig(cfg.n_symbols, cfg.bert_embed, cfg.bert_hidden, cfg.bert_heads, cfg.bert_intermediate, cfg.bert_layers,
                         cfg.bert_positions, cfg.bert_types, cfg.d_model)
        views, n, keep = tensor_views(weights)
        h = ctx.lib.mia_kokoro_bert_load(ctx.h, C.byref(c), views, n)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return KokoroBert(ctx, h, cfg)

    def close(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.mia_kokoro_bert_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode(self, ids, n_layers=None, return_hidden: bool = False):
        """ids [N] (padded with 0 at both ends, as the reference pads them) -> d_en [N, d_model], or (ALBERT's sequence output
        [N, bert_hidden], d_en) with `return_hidden`.  n_layers: stop after that many applications of the layer (default: all)."""
        i = np.ascontiguousarray(ids, np.int32).reshape(-1)
        N = i.shape[0]
        hidden = np.empty((N, self.cfg.bert_hidden), np.float32) if return_hidden else None
        d_en = np.empty((N, self.cfg.d_model), np.float32)
        self.ctx.check(self.ctx.lib.mia_kokoro_bert_encode(self.h, i.ctypes.data if N else None, N, int(n_layers or 0),
                                                           hidden.ctypes.data if return_hidden else None, d_en.ctypes.data, _lib.MEM_HOST))
        return (hidden, d_en) if return_hidden else d_en


def voice_row(pack, n: int):
    """The voice-pack row of an utterance of n >= 1 phoneme ids (KokoroTTS.swift:294-300): pack [P, 1, 2 style] or [P, 2 style] ->
    row min(n - 1, P - 1), [2 style]."""
    p = np.asarray(pack)
    if p.ndim == 3 and p.shape[1] == 1:
        p = p[:, 0]
    if p.ndim != 2 or p.shape[0] < 1 or n < 1:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "Kokoro: the voice pack must be [P, 1, 2 style_dim] or [P, 2 style_dim] and n >= 1")
    return p[min(n - 1, p.shape[0] - 1)]


class KokoroPipeline:
    """generateAudioForTokens (KokoroTTS.swift:262-415).  synthesize_ids: phoneme ids and a voice pack to PCM; synthesize: from line 303
    on, d_en, the padded ids and a voice-pack row to PCM.  Activations stay on the device between the stages; only the durations (and
    their sum) come back to the host.  The device buffers are torch tensors, so `torch` must be imported before the context is created
    (as for every hook here that takes device tensors)."""

    def __init__(self, text: KokoroText, decoder: KokoroDecoder, bert: KokoroBert | None = None):
        cfg = text.cfg
        if text.ctx is not decoder.ctx or (cfg.d_model, cfg.d_model, cfg.style_dim) != (decoder.cfg.dim_in, decoder.cfg.pred_dim, decoder.cfg.style_dim):
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "Kokoro: the two halves must share a context, d_model = dim_in = pred_dim and style_dim")
        if bert is not None and (bert.ctx is not text.ctx or (bert.cfg.d_model, bert.cfg.n_symbols) != (cfg.d_model, cfg.n_symbols)):
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "Kokoro: bert must share the context, d_model and n_symbols of the text half")
        self.text, self.decoder, self.bert, self.ctx, self.cfg = text, decoder, bert, text.ctx, cfg
        self.last_durations = None

    def synthesize_ids(self, phoneme_ids, voice_pack, speed: float = 1.0, noise=None, durations=None):
        """phoneme ids [n] (unpadded, n + 2 <= 512) and a voice pack -> waveform [600 T]: pads [0] + ids + [0], takes
        voice_row(voice_pack, n) and runs bert -> durations -> encode -> align -> shared -> f0n -> decode on the device."""
        if self.bert is None:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "Kokoro: synthesize_ids needs a pipeline built with bert")
        i = np.ascontiguousarray(phoneme_ids, np.int32).reshape(-1)
        return self.synthesize(None, np.concatenate([[0], i, [0]]).astype(np.int32), voice_row(voice_pack, i.shape[0]), speed, noise, durations)

    def synthesize(self, d_en, ids, voice_row, speed: float = 1.0, noise=None, durations=None):
        """d_en [N, d_model], ids [N], voice_row [2 style_dim] (decoder style | predictor style) -> waveform [600 T].  `durations`
        [N] forces the alignment; `noise` [600 T, n_harmonics + 1] stands in for the source's random draw.  d_en = None (a pipeline
        with bert): it is computed from the ids on the device."""
        import torch
        cfg, ctx, lib, DEV = self.cfg, self.ctx, self.ctx.lib, _lib.MEM_DEVICE
        D, S = cfg.d_model, cfg.style_dim
        i = np.ascontiguousarray(ids, np.int32).reshape(-1)
        N = i.shape[0]
        if d_en is None and self.bert is None:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "Kokoro: synthesize needs d_en, or a pipeline built with bert")
        x = None if d_en is None else np.ascontiguousarray(d_en, np.float32)
        if (x is not None and x.shape != (N, D)) or i.min(initial=0) < 0 or i.max(initial=0) >= cfg.n_symbols:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: d_en must be [N, {D}] and ids [N] inside the symbol table")
        v = _f32(voice_row, (2 * S,), "voice_row")
        dev = torch.device("cuda", ctx.device)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

        def new(*shape, dtype=torch.float32):
            return torch.empty(shape, dtype=dtype, device=dev)

        dx, di, s_dec, s_pred = new(N, D) if x is None else up(x), up(i), up(v[:S]), up(v[S:])
        d, predicted, raw, t_en = new(N, D + S), new(N, dtype=torch.int32), new(N), new(N, D)
        dur = predicted if durations is None else up(np.ascontiguousarray(durations, np.int32).reshape(N))     # forced: d is still needed
        torch.cuda.synchronize(dev)
        if x is None:
            ctx.check(lib.mia_kokoro_bert_encode(self.bert.h, i.ctypes.data if N else None, N, 0, None, dx.data_ptr(), DEV))
        ctx.check(lib.mia_kokoro_text_durations(self.text.h, dx.data_ptr(), N, s_pred.data_ptr(), float(speed), d.data_ptr(),
                                                predicted.data_ptr(), raw.data_ptr(), DEV))
        ctx.check(lib.mia_kokoro_text_encode(self.text.h, di.data_ptr(), N, t_en.data_ptr(), DEV))
        ctx.synchronize()
        self.last_durations = dur.cpu().numpy()
        T = int(self.last_durations.astype(np.int64).sum())
        if T < 1 or T > 10000:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"Kokoro: the durations sum to {T} rows, outside [1, 10000]")
        nz = up(self.decoder._noise(noise, 2 * T)) if noise is not None else None
        en, asr, xs, f0, n = new(T, D + S), new(D, T), new(D, T), new(2 * T), new(2 * T)
        pcm = new(self.decoder.output_len(T))
        torch.cuda.synchronize(dev)
        Tc = C.c_int(T)
        ctx.check(lib.mia_kokoro_text_align(self.text.h, d.data_ptr(), t_en.data_ptr(), dur.data_ptr(), N, en.data_ptr(), asr.data_ptr(),
                                            C.byref(Tc), DEV))
        ctx.check(lib.mia_kokoro_text_shared(self.text.h, en.data_ptr(), T, xs.data_ptr(), DEV))
        ctx.check(lib.mia_kokoro_f0n(self.decoder.h, xs.data_ptr(), T, s_pred.data_ptr(), f0.data_ptr(), n.data_ptr(), DEV))
        ctx.check(lib.mia_kokoro_decode(self.decoder.h, asr.data_ptr(), T, f0.data_ptr(), n.data_ptr(), s_dec.data_ptr(),
                                        nz.data_ptr() if nz is not None else None, pcm.data_ptr(), DEV))
        ctx.synchronize()
        return pcm.cpu().numpy()
