"""Host-side mirror of the reference's Marvis TTS interface (TTS/Marvis/Models/MarvisModel.swift, TTS/Marvis/MarvisTTS.swift), backed by
the gfx950 HIP layer: MarvisModel.generateFrame and the decodePrompt loop run on the device (csrc/marvis.hip); the codes go to the Mimi
decoder of mimi.py, and a voice prompt's codes come from its encoder (tokenize_audio, MarvisTTS.reference_prompt).  Python builds rows
and calls; no arithmetic of the model happens here.

Out of scope: the text tokenizer and the sentence splitter."""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from ._abi import BF16, F16, F32, U32, MarvisConfig as _CConfig, tensor_views

QUALITY_CODEBOOKS = {"low": 8, "medium": 16, "high": 24, "maximum": 32}      # MarvisEngine.QualityLevel.codebookCount (MarvisEngine.swift:55-68)
MAX_AUDIO_FRAMES = int(60000 / 80.0)                                         # decodePrompt (MarvisTTS.swift:471)


@dataclass(frozen=True)
class MarvisStackConfig:
    """MarvisBackboneConfig (MarvisModel.swift:305-361), the fields the Llama stack uses."""
    hidden: int
    inter: int
    layers: int
    heads: int
    kv_heads: int
    head_dim: int
    rms_eps: float = 1e-5
    rope_theta: float = 500000.0


_ROPE_LLAMA3 = {"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192.0}
FLAVORS = {
    "llama-1B": MarvisStackConfig(2048, 8192, 16, 32, 8, 64),
    "llama-100M": MarvisStackConfig(1024, 8192, 4, 8, 2, 128),
}


@dataclass(frozen=True)
class MarvisConfig:
    backbone: MarvisStackConfig
    decoder: MarvisStackConfig
    text_vocab: int = 128256
    audio_vocab: int = 2051
    n_codebooks: int = 32
    max_ctx: int = 2048
    rope_scaling: dict | None = field(default_factory=lambda: dict(_ROPE_LLAMA3))
    attention_bias: bool = False
    mlp_bias: bool = False

    @staticmethod
    def from_flavors(backbone: str = "llama-1B", decoder: str = "llama-100M", **kw) -> "MarvisConfig":
        """The two Swift flavours (createMarvisBackboneConfig, MarvisModel.swift:305-361)."""
        return MarvisConfig(FLAVORS[backbone], FLAVORS[decoder], **kw)

    @staticmethod
    def from_json(cfg) -> "MarvisConfig":
        """A checkpoint's config.json (a path or the parsed dict): the `depth_decoder_config` form (createMarvisBackboneConfigForBackbone /
        ...ForDecoder, MarvisModel.swift:265-303) or the flavour form."""
        if not isinstance(cfg, dict):
            with open(cfg) as f:
                cfg = json.load(f)
        common = dict(text_vocab=int(cfg["text_vocab_size"]), audio_vocab=int(cfg["audio_vocab_size"]),
                      n_codebooks=int(cfg.get("audio_num_codebooks", cfg.get("num_codebooks", 32))))
        d = cfg.get("depth_decoder_config")
        if d is None:
            return MarvisConfig.from_flavors(cfg["backbone_flavor"], cfg["decoder_flavor"], **common)

        def stack(c):
            return MarvisStackConfig(int(c["hidden_size"]), int(c["intermediate_size"]), int(c["num_hidden_layers"]), int(c["num_attention_heads"]),
                                     int(c["num_key_value_heads"]), int(c["head_dim"]), float(c.get("rms_norm_eps", 1e-5)), float(c.get("rope_theta", 500000)))
        rs = cfg.get("rope_scaling")
        return MarvisConfig(stack(cfg), stack(d), max_ctx=int(cfg.get("max_position_embeddings", 2048)),
                            rope_scaling=None if rs is None else {k: float(v) for k, v in rs.items() if k in _ROPE_LLAMA3},
                            attention_bias=bool(cfg.get("attention_bias", False)), mlp_bias=bool(cfg.get("mlp_bias", False)), **common)


def _c_config(cfg: MarvisConfig) -> _CConfig:
    b, d = cfg.backbone, cfg.decoder
    rs = dict(_ROPE_LLAMA3, **(cfg.rope_scaling or {}))
    return _CConfig(cfg.text_vocab, cfg.audio_vocab, cfg.n_codebooks, cfg.max_ctx,
                    b.hidden, b.inter, b.layers, b.heads, b.kv_heads, b.head_dim,
                    d.hidden, d.inter, d.layers, d.heads, d.kv_heads, d.head_dim,
                    b.rms_eps, d.rms_eps, b.rope_theta, d.rope_theta,
                    int(cfg.rope_scaling is not None), rs["factor"], rs["low_freq_factor"], rs["high_freq_factor"], rs["original_max_position_embeddings"],
                    int(cfg.attention_bias), int(cfg.mlp_bias))


# ---- rows (MarvisTTS.swift:286-365) ----------------------------------------------------------------------------------------------

def tokenize_text_rows(ids, n_codebooks: int):
    """tokenizeTextSegment: ids = the caller's tokenizer output for "[speaker]" + text -> (rows, mask) int32 [T][K+1], the id in the
    last column."""
    ids = np.asarray(ids, np.int32).reshape(-1)
    rows = np.zeros((ids.size, n_codebooks + 1), np.int32)
    mask = np.zeros_like(rows)
    rows[:, -1] = ids
    mask[:, -1] = 1
    return rows, mask


def tokenize_audio_rows(codes, add_eos: bool = True):
    """tokenizeAudio behind the codec: codes int [K][T] -> (rows, mask) int32 [T (+1)][K+1], an all-zero EOS frame appended when asked."""
    codes = np.asarray(codes, np.int32)
    if codes.ndim != 2:
        raise ValueError("codes must be [K, T]")
    K = codes.shape[0]
    if add_eos:
        codes = np.concatenate([codes, np.zeros((K, 1), np.int32)], axis=1)
    T = codes.shape[1]
    rows = np.zeros((T, K + 1), np.int32)
    mask = np.zeros_like(rows)
    rows[:, :K] = codes.T
    mask[:, :K] = 1
    return rows, mask


def tokenize_audio(codec, pcm, n_codebooks: int, add_eos: bool = True):
    """tokenizeAudio (MarvisTTS.swift:318-348) including the codec call: pcm float32 at the codec's rate -> (rows, mask) of the first
    n_codebooks rows of MimiCodec.encode (they do not depend on the later stages, so only they are computed)."""
    return tokenize_audio_rows(codec.encode(pcm, n_q=n_codebooks), add_eos=add_eos)


def tokenize_segment(text_ids, codec, pcm, n_codebooks: int, add_eos: bool = True):
    """tokenizeSegment (MarvisTTS.swift:350-354): the text rows, then the audio rows of the clip."""
    tr, tm = tokenize_text_rows(text_ids, n_codebooks)
    ar, am = tokenize_audio(codec, pcm, n_codebooks, add_eos=add_eos)
    return np.concatenate([tr, ar], 0), np.concatenate([tm, am], 0)


def tokenize_start(text_ids, codes, pcm=None, n_codebooks: int | None = None):
    """tokenizeStart: the text rows, then the voice prompt's audio rows without EOS.  The prompt is either its codes [K, T], or a
    MimiCodec with an encoder and the clip: tokenize_start(text_ids, codec, pcm, n_codebooks)."""
    if pcm is not None:
        codec = codes
        return tokenize_segment(text_ids, codec, pcm, codec.cfg.quantizer_nq if n_codebooks is None else n_codebooks, add_eos=False)
    codes = np.asarray(codes, np.int32)
    tr, tm = tokenize_text_rows(text_ids, codes.shape[0])
    ar, am = tokenize_audio_rows(codes, add_eos=False)
    return np.concatenate([tr, ar], 0), np.concatenate([tm, am], 0)


def _rows(rows, mask, width):
    r = np.ascontiguousarray(rows, np.int32)
    m = np.ascontiguousarray(mask, np.int32)
    if r.ndim != 2 or r.shape[1] != width or m.shape != r.shape:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"rows and mask must both be [T, {width}]")
    return r, m


class MarvisModel:
    def __init__(self, ctx, h, cfg, dtype):
        self.ctx, self.h, self.cfg, self.dtype = ctx, h, cfg, dtype
        ctx.adopt(self)

    @staticmethod
    def load(ctx: _lib.Context, cfg: MarvisConfig, weights: dict, dtype: int = BF16) -> "MarvisModel":
        """weights: the Module key schema (checkpoint.sanitize_marvis maps a raw checkpoint), dense float32 / float16 / bfloat16."""
        c = _c_config(cfg)
        views, n, keep = tensor_views(weights, kinds=(F32, F16, BF16))
        status = C.c_int32(0)
        h = ctx.lib.mia_marvis_load(ctx.h, C.byref(c), views, n, dtype, C.byref(status))
        if not h:
            raise _lib.MiaError(status.value or _lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return MarvisModel(ctx, h, cfg, dtype)

    @staticmethod
    def load_quantized(ctx: _lib.Context, cfg: MarvisConfig, raw_tensors: dict, dtype: int = BF16) -> "MarvisModel":
        """The whole path for a published (MLX-affine quantised) checkpoint, as MarvisTTS.installWeights takes it (MarvisTTS.swift:220-226):
        raw_tensors = the safetensors contents under the file's own keys.  sanitize_marvis, expand_checkpoint for the dense 16-bit copy
        (embedding tables included), load, then attach the packed Linears; the frame runs on the packed weights."""
        from . import checkpoint
        tensors = checkpoint.sanitize_marvis(raw_tensors)
        model = MarvisModel.load(ctx, cfg, checkpoint.expand_checkpoint(ctx, tensors), dtype)
        model.attach_quantized(tensors)
        return model

    def attach_quantized(self, tensors: dict, bits: int | None = None, group_size: int = 64) -> None:
        """mia_marvis_attach_quantized: `tensors` holds the Linears of both stacks, `projection` and (when stored quantised)
        `codebook0_head` as the checkpoint stores them, under the keys of checkpoint.sanitize_marvis -- `<p>.weight` uint32 codes,
        `<p>.scales` / `<p>.biases` float16 or bf16 (uint16 arrays tagged .st_dtype == "BF16"); anything without a `.scales` is left out,
        and quantised embedding tables are ignored (they stay 16-bit tables).  bits (4 | 6 | 8): inferred from the packed width when not
        given, as checkpoint.expand_checkpoint does.  The handle must have been loaded from the de-quantised tensors of the same
        checkpoint.  One attach per handle; the frame then runs on the packed weights (use_packed(False) switches back)."""
        packed = {}
        for name, arr in tensors.items():
            base = name.rsplit(".", 1)[0]
            if name.endswith((".weight", ".scales", ".biases")) and base + ".scales" in tensors and not base.endswith("_embeddings"):
                packed[name] = arr
        if bits is None:
            for name, arr in packed.items():
                if name.endswith(".weight"):
                    bits = (32 * arr.shape[-1]) // (packed[name[:-7] + ".scales"].shape[-1] * group_size)
                    break
        views, n, keep = tensor_views(packed, (U32, F16, BF16), "attach_quantized: '{name}' must be uint32 codes or 16-bit scales / biases (got {dtype})")
        self.ctx.check(self.ctx.lib.mia_marvis_attach_quantized(self.h, views, n, int(group_size), int(bits or 0)))

    def use_packed(self, on: bool) -> None:
        """mia_marvis_use_packed: the frame reads the attached packed weights (True) or the 16-bit copy (False)."""
        self.ctx.check(self.ctx.lib.mia_marvis_use_packed(self.h, 1 if on else 0))

    def use_packed_prompt(self, on: bool) -> None:
        """mia_marvis_use_packed_prompt: the backbone's prompt pass on the attached packed weights (True) or the 16-bit copy (False)."""
        self.ctx.check(self.ctx.lib.mia_marvis_use_packed_prompt(self.h, 1 if on else 0))

    def release_dense(self) -> None:
        """mia_marvis_release_dense: frame and prompt pass on the packed weights, then free both stacks' 16-bit layer Linears.  Not
        reversible: use_packed(False) and use_packed_prompt(False) raise ERR_UNSUPPORTED afterwards."""
        self.ctx.check(self.ctx.lib.mia_marvis_release_dense(self.h))

    def codebooks(self, max_codebooks: int) -> int:
        return min(self.cfg.n_codebooks, max_codebooks)

    def reset(self) -> None:
        """resetCaches."""
        self.ctx.check(self.ctx.lib.mia_marvis_reset(self.h))

    def set_debug(self, flags: int) -> None:
        self.ctx.check(self.ctx.lib.mia_marvis_set_debug(self.h, flags))

    def frame(self, rows, mask, max_codebooks: int, uniforms, temperature: float = 0.9, top_p: float = 0.8, forced=None, return_logits: bool = False):
        """generateFrame: append the rows, draw one frame -> ids int32 [codebooks] (and the fp32 logits [codebooks][audio_vocab])."""
        r, m = _rows(rows, mask, self.cfg.n_codebooks + 1)
        cb = self.codebooks(max(max_codebooks, 1))
        u = np.ascontiguousarray(uniforms, np.float32).reshape(-1)
        if u.size < cb:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"frame needs {cb} uniforms")
        f = None if forced is None else np.ascontiguousarray(forced, np.int32).reshape(-1)
        if f is not None and f.size < cb:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"forced needs {cb} ids")
        ids = np.zeros(cb, np.int32)
        logits = np.zeros((cb, self.cfg.audio_vocab), np.float32) if return_logits else None
        self.ctx.check(self.ctx.lib.mia_marvis_frame(self.h, r.ctypes.data, m.ctypes.data, r.shape[0], max_codebooks, temperature, top_p, u.ctypes.data,
                                                     None if f is None else f.ctypes.data, ids.ctypes.data, None if logits is None else logits.ctypes.data))
        return (ids, logits) if return_logits else ids

    def generate(self, rows, mask, max_codebooks: int, uniforms, max_frames: int | None = None, temperature: float = 0.9, top_p: float = 0.8) -> np.ndarray:
        """decodePrompt's loop: frames int32 [n][codebooks].  rows = None (or zero rows) continues the sentence of the previous call."""
        W = self.cfg.n_codebooks + 1
        if rows is None:
            r, m = np.zeros((0, W), np.int32), np.zeros((0, W), np.int32)
        else:
            r, m = _rows(rows, mask, W)
        cb = self.codebooks(max(max_codebooks, 1))
        u = np.ascontiguousarray(uniforms, np.float32).reshape(-1, cb)
        n_max = u.shape[0] if max_frames is None else max_frames
        if u.shape[0] < n_max:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"generate needs uniforms [{n_max}][{cb}]")
        out = np.zeros((max(n_max, 1), cb), np.int32)
        n = C.c_int32(0)
        T = r.shape[0]
        self.ctx.check(self.ctx.lib.mia_marvis_generate(self.h, r.ctypes.data if T else None, m.ctypes.data if T else None, T, max_codebooks, temperature, top_p,
                                                        n_max, u.ctypes.data, out.ctypes.data, C.byref(n)))
        return out[:n.value].copy()

    def set_batch(self, max_batch: int) -> None:
        """Capacity for max_batch sentences side by side (re-allocates the per-sequence state and resets the handle)."""
        self.ctx.check(self.ctx.lib.mia_marvis_set_batch(self.h, max_batch))

    def generate_batch(self, prompts, max_codebooks: int, uniforms, temperature: float = 0.9, top_p: float = 0.8) -> list:
        """decodePrompt's loop for several sentences side by side: prompts = [(rows, mask), ...], uniforms [n_seq][max_frames][codebooks]
        -> one frames array [n_b][codebooks] per sentence, each equal to its own generate() on the same capacity."""
        W = self.cfg.n_codebooks + 1
        pairs = [_rows(r, m, W) for r, m in prompts]
        cb = self.codebooks(max(max_codebooks, 1))
        u = np.ascontiguousarray(uniforms, np.float32)
        if u.ndim != 3 or u.shape[0] != len(pairs) or u.shape[2] != cb:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, f"generate_batch needs uniforms [{len(pairs)}][max_frames][{cb}]")
        rows = np.ascontiguousarray(np.concatenate([r for r, _ in pairs], 0)) if pairs else np.zeros((0, W), np.int32)
        mask = np.ascontiguousarray(np.concatenate([m for _, m in pairs], 0)) if pairs else np.zeros((0, W), np.int32)
        off = np.concatenate([[0], np.cumsum([r.shape[0] for r, _ in pairs])]).astype(np.int32)
        out = np.zeros((max(len(pairs), 1), max(u.shape[1], 1), cb), np.int32)
        n = np.zeros(max(len(pairs), 1), np.int32)
        self.ctx.check(self.ctx.lib.mia_marvis_generate_batch(self.h, rows.ctypes.data, mask.ctypes.data, off.ctypes.data, len(pairs), max_codebooks, temperature,
                                                              top_p, u.shape[1], u.ctypes.data, out.ctypes.data, n.ctypes.data))
        return [out[b, :n[b]].copy() for b in range(len(pairs))]

    def close(self) -> None:
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.mia_marvis_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_top_p_ascending(ctx: _lib.Context, logits, temperature: float, top_p: float, uniform: float):
    """One draw of the frame sampler on caller logits -> (id, kept ids in ascending order of p)."""
    x = np.ascontiguousarray(logits, np.float32).reshape(-1)
    out, nk = C.c_int32(0), C.c_int32(0)
    kept = np.zeros(x.size, np.int32)
    ctx.check(ctx.lib.mia_sample_top_p_ascending(ctx.h, x.ctypes.data, x.size, temperature, top_p, uniform, C.byref(out), kept.ctypes.data, C.byref(nk)))
    return out.value, kept[:nk.value].copy()


class MarvisTTS:
    """generateCore for one sentence (MarvisTTS.swift:402-547): frames from MarvisModel, PCM from the Mimi decoder."""

    def __init__(self, model: MarvisModel, mimi):
        self.model, self.mimi = model, mimi
        self._stream = None

    def _uniforms(self, uniforms, cb):
        return np.ascontiguousarray(uniforms, np.float32).reshape(-1, cb)

    def reference_prompt(self, text_ids, samples, rate: int):
        """makeContext + tokenizeStart (MarvisTTS.swift:356-398) for a caller's reference clip: resample to the codec's rate
        (AudioResampler, on the device), encode, and build the prompt -> (rows, mask) for generate / generate_streaming.
        text_ids = the caller's tokenizer output for "[0]" + the clip's transcript."""
        from . import audio_io
        wav = audio_io.resample(self.model.ctx, np.ascontiguousarray(samples, np.float32).reshape(-1), int(rate), int(self.mimi.cfg.sample_rate))
        return tokenize_start(text_ids, self.mimi, wav, self.model.cfg.n_codebooks)

    def generate(self, prompt_rows, mask, quality: str, uniforms, temperature: float = 0.9, top_p: float = 0.8) -> np.ndarray:
        """Whole sentence -> float32 PCM through MimiCodec.decode ([codebooks][n] codes)."""
        cb = self.model.codebooks(QUALITY_CODEBOOKS[quality])
        self.model.reset()
        frames = self.model.generate(prompt_rows, mask, QUALITY_CODEBOOKS[quality], self._uniforms(uniforms, cb), temperature=temperature, top_p=top_p)
        if frames.shape[0] == 0:
            return np.zeros(0, np.float32)
        return self.mimi.decode(np.ascontiguousarray(frames.T))

    def generate_streaming(self, prompt_rows, mask, quality: str, uniforms, interval: float = 0.5, temperature: float = 0.9, top_p: float = 0.8):
        """Yields float32 PCM every int(interval * 12.5) frames through one MimiStream (reset per sentence, as generateCore does); each
        chunk after the first continues the sentence with the T = 0 form of the loop."""
        cb = self.model.codebooks(QUALITY_CODEBOOKS[quality])
        step = max(int(interval * 12.5), 1)
        u = self._uniforms(uniforms, cb)
        self.model.reset()
        if self._stream is None:
            self._stream = self.mimi.new_stream()
        self._stream.reset()
        rows, done = prompt_rows, 0
        while done < u.shape[0]:
            n = min(step, u.shape[0] - done)
            frames = self.model.generate(rows, mask if rows is not None else None, QUALITY_CODEBOOKS[quality], u[done:done + n], temperature=temperature, top_p=top_p)
            rows = None
            done += n
            if frames.shape[0]:
                yield self._stream.decode_frames(np.ascontiguousarray(frames.T))
            if frames.shape[0] < n:
                break


__all__ = ["MarvisConfig", "MarvisStackConfig", "MarvisModel", "MarvisTTS", "FLAVORS", "QUALITY_CODEBOOKS", "tokenize_text_rows", "tokenize_audio_rows",
           "tokenize_audio", "tokenize_segment", "tokenize_start", "sample_top_p_ascending"]
