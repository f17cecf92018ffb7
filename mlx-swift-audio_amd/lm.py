"""Host-side mirror of the reference's causal-LM interface (OrpheusLMHeadModel / Qwen2 blocks + sampleNextToken + parseOutput),
backed by the gfx950 HIP layer (include/mia.h).  parse_output is integer bookkeeping and stays on the host, as in the Swift."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._abi import LmConfig, LmSampler, RasParams, tensor_views

END_TOKEN = 128258                    # OrpheusTTS.swift:75-85
CODE_OFFSET = 128266
AUDIO_CODE_DATA_START_MARKER = 128257
MAX_TOKEN_COUNT = 1200
REPETITION_CONTEXT_SIZE = 20


class CausalLM:
    def __init__(self, ctx, h, cfg):
        self.ctx, self.h, self.cfg = ctx, h, cfg
        ctx.adopt(self)

    @staticmethod
    def load(ctx: _lib.Context, cfg, weights: dict[str, np.ndarray], dtype: int = _lib.BF16) -> "CausalLM":
        c = LmConfig(cfg.vocab, cfg.hidden, cfg.inter, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.max_ctx, cfg.rms_eps,
                     cfg.rope_theta, 1 if cfg.rope_llama3 else 0, cfg.rope_factor, cfg.rope_low, cfg.rope_high, cfg.rope_old_ctx,
                     1 if cfg.qkv_bias else 0, 1 if cfg.tie_embeddings else 0)
        views, n, keep = tensor_views(weights, (_lib.F32, _lib.F16, _lib.BF16))
        h = ctx.lib.mia_lm_load(ctx.h, C.byref(c), views, n, dtype)
        if not h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        return CausalLM(ctx, h, cfg)

    def attach_q4(self, packed: dict[str, np.ndarray], group_size: int = 64, bits: int = 4) -> None:
        """mia_lm_attach_quantized (bits 4 | 6 | 8): `packed` holds every step Linear as the checkpoint stores it -- `<name>.weight` uint32 codes,
        `<name>.scales` / `<name>.biases` float16 (or uint16 arrays tagged .st_dtype == "BF16", as checkpoint.read_safetensors returns
        bf16 payloads).  The handle must have been loaded from the de-quantised tensors of the same checkpoint."""
        lib = self.ctx.lib
        views, n, keep = tensor_views(packed, (_lib.U32, _lib.F16, _lib.BF16), "attach_q4: '{name}' must be uint32 codes or 16-bit scales / biases (got {dtype})")
        self.ctx.check(lib.mia_lm_attach_quantized(self.h, views, n, group_size, bits))

    def set_debug(self, flags: int) -> None:
        """Test hook (mia_lm_set_debug): bit 0 = no hipGraph, bit 1 = prompts token by token (no batched prompt pass)."""
        lib = self.ctx.lib
        self.ctx.check(lib.mia_lm_set_debug(self.h, int(flags)))

    def set_prompt_attention(self, mode: int) -> None:
        """mia_lm_set_prompt_attention: 0 = the prompt pass's row kernel (default), 1 = the tiled matrix-core kernel on the 16-bit cache."""
        lib = self.ctx.lib
        self.ctx.check(lib.mia_lm_set_prompt_attention(self.h, int(mode)))

    def use_q4(self, on: bool) -> None:
        lib = self.ctx.lib
        self.ctx.check(lib.mia_lm_use_q4(self.h, 1 if on else 0))

    def set_prompt_weights(self, packed: bool) -> None:
        """mia_lm_set_prompt_weights: the batched prompt pass on the attached packed weights (True) or on the 16-bit copy (False, the
        default).  True needs attach_q4 first."""
        self.ctx.check(self.ctx.lib.mia_lm_set_prompt_weights(self.h, 1 if packed else 0))

    def release_dense(self) -> None:
        """mia_lm_release_dense: step and prompt pass on the packed weights, then free the layers' 16-bit Linears.  Not reversible:
        use_q4(False) and set_prompt_weights(False) raise ERR_UNSUPPORTED afterwards."""
        self.ctx.check(self.ctx.lib.mia_lm_release_dense(self.h))

    def weight_bytes(self) -> tuple[int, int]:
        """mia_lm_weight_bytes: (dense, packed) device bytes of weight matrices the handle holds now."""
        d, q = C.c_int64(0), C.c_int64(0)
        self.ctx.check(self.ctx.lib.mia_lm_weight_bytes(self.h, C.byref(d), C.byref(q)))
        return int(d.value), int(q.value)

    def close(self):
        if self.h and getattr(self.ctx, 'h', None):
            self.ctx.lib.mia_lm_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.ctx.check(self.ctx.lib.mia_lm_reset(self.h))

    def forward(self, ids) -> np.ndarray:
        """model(ids, cache)[0, -1]: fp32 logits after the last of `ids` (appended to the KV cache)."""
        a = np.ascontiguousarray(ids, np.int32)
        out = np.empty(self.cfg.vocab, np.float32)
        self.ctx.check(self.ctx.lib.mia_lm_forward(self.h, a.ctypes.data, a.size, out.ctypes.data))
        return out

    def generate(self, prompt, uniforms, temperature=0.6, top_p=0.8, rep_penalty=1.3, rep_window=REPETITION_CONTEXT_SIZE,
                 max_new_tokens=MAX_TOKEN_COUNT, stop_ids=(END_TOKEN,)) -> list[int]:
        a = np.ascontiguousarray(prompt, np.int32)
        u = np.ascontiguousarray(uniforms, np.float32)
        if u.size < max_new_tokens:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "need one uniform per possible draw")
        sp = LmSampler(temperature, top_p, rep_penalty, rep_window, max_new_tokens, len(stop_ids), (C.c_int32 * 4)(*(list(stop_ids) + [0] * (4 - len(stop_ids)))), 0)
        out = np.zeros(max_new_tokens, np.int32)
        n = C.c_int32(0)
        self.ctx.check(self.ctx.lib.mia_lm_generate(self.h, a.ctypes.data, a.size, C.byref(sp), u.ctypes.data, out.ctypes.data, C.byref(n)))
        return out[:n.value].tolist()


def _set_batch(self, max_batch: int) -> None:
    """Size the per-sequence state for up to `max_batch` (<= 32) sequences decoded side by side."""
    self.ctx.check(self.ctx.lib.mia_lm_set_batch(self.h, int(max_batch)))


def _generate_batch(self, prompts, uniforms, temperature=0.6, top_p=0.8, rep_penalty=1.3, rep_window=REPETITION_CONTEXT_SIZE,
                    max_new_tokens=MAX_TOKEN_COUNT, stop_ids=(END_TOKEN,)) -> list[list[int]]:
    """generate() for several prompts at once (sentence-level batching): uniforms [n_seq, max_new_tokens]; sequence b's ids equal
    generate(prompts[b], uniforms[b]).  Call set_batch(n) first."""
    u = np.ascontiguousarray(uniforms, np.float32)
    n_seq = len(prompts)
    if u.ndim != 2 or u.shape[0] != n_seq or u.shape[1] < max_new_tokens:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "uniforms must be [n_seq, >= max_new_tokens]")
    u = np.ascontiguousarray(u[:, :max_new_tokens])
    offs = np.zeros(n_seq + 1, np.int32)
    np.cumsum([len(p) for p in prompts], out=offs[1:])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32) for p in prompts]))
    sp = LmSampler(temperature, top_p, rep_penalty, rep_window, max_new_tokens, len(stop_ids), (C.c_int32 * 4)(*(list(stop_ids) + [0] * (4 - len(stop_ids)))), 0)
    out = np.zeros((n_seq, max_new_tokens), np.int32)
    n = np.zeros(n_seq, np.int32)
    self.ctx.check(self.ctx.lib.mia_lm_generate_batch(self.h, flat.ctypes.data, offs.ctypes.data, n_seq, C.byref(sp), u.ctypes.data, out.ctypes.data, n.ctypes.data))
    return [out[b, :n[b]].tolist() for b in range(n_seq)]


CausalLM.set_batch = _set_batch
CausalLM.generate_batch = _generate_batch


def _new_cache(self, quantized: bool = False, group_size: int = 64, bits: int = 4) -> None:
    """OrpheusModel.newCache(quantized:groupSize:bits:) (TransformerBlock.swift:182-201): quantized=True keeps K/V as 4- / 8-bit codes plus
    a (scale, bias) pair per 64 values (mia_lm_set_kv_quant), False restores the 16-bit caches.  Every sequence is reset either way."""
    lib = self.ctx.lib
    self.ctx.check(lib.mia_lm_set_kv_quant(self.h, int(bits) if quantized else 0, int(group_size)))


def _read_kv(self, layer: int, seq: int, pos0: int, n: int) -> tuple[np.ndarray, np.ndarray]:
    """Test hook (mia_lm_read_kv): cache rows [pos0, pos0 + n) of (layer, seq) as fp32 (k, v), each [n_kv_heads, n, head_dim]."""
    lib = self.ctx.lib
    k = np.empty((self.cfg.n_kv_heads, max(int(n), 0), self.cfg.head_dim), np.float32)
    v = np.empty_like(k)
    self.ctx.check(lib.mia_lm_read_kv(self.h, int(layer), int(seq), int(pos0), int(n), k.ctypes.data, v.ctypes.data))
    return k, v


CausalLM.new_cache = _new_cache
CausalLM.read_kv = _read_kv


def _generate_ras(self, prompt_embeds, uniforms, min_len, max_len, eos, top_p=0.8, top_k=25, win=10, tau=0.1) -> list[int]:
    """mia_lm_generate_ras: embedding-row prompt -> RAS-sampled ids (stops at `eos` once min_len ids are out, or at max_len)."""
    lib = self.ctx.lib
    x = np.ascontiguousarray(prompt_embeds, np.float32)
    rp = RasParams(top_p, top_k, win, tau, eos, min_len, max_len)
    u = np.ascontiguousarray(uniforms, np.float32)
    out = np.zeros(max_len + 1, np.int32)
    n = C.c_int32(0)
    self.ctx.check(lib.mia_lm_generate_ras(self.h, x.ctypes.data, x.shape[0], C.byref(rp), u.ctypes.data, u.size, out.ctypes.data, C.byref(n)))
    return out[:n.value].tolist()


CausalLM.generate_ras = _generate_ras


def _generate_ras_batch(self, prompt_embeds, uniforms, min_lens, max_lens, eos, top_p=0.8, top_k=25, win=10, tau=0.1) -> list[list[int]]:
    """mia_lm_generate_ras_batch: one embedding-row prompt, (min_len, max_len) pair and uniform row per utterance; set_batch(n) first."""
    lib = self.ctx.lib
    n_seq = len(prompt_embeds)
    xs = [np.ascontiguousarray(x, np.float32) for x in prompt_embeds]
    offs = np.zeros(n_seq + 1, np.int32)
    np.cumsum([x.shape[0] for x in xs], out=offs[1:])
    flat = np.ascontiguousarray(np.concatenate(xs, axis=0))
    rps = (RasParams * n_seq)(*[RasParams(top_p, top_k, win, tau, eos, int(min_lens[b]), int(max_lens[b])) for b in range(n_seq)])
    u = np.ascontiguousarray(uniforms, np.float32)
    if u.ndim != 2 or u.shape[0] != n_seq:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "uniforms must be [n_seq, n_uniforms]")
    stride = int(max(max_lens)) + 1
    out = np.zeros((n_seq, stride), np.int32)
    n = np.zeros(n_seq, np.int32)
    self.ctx.check(lib.mia_lm_generate_ras_batch(self.h, flat.ctypes.data, offs.ctypes.data, n_seq, rps, u.ctypes.data, u.shape[1], out.ctypes.data, stride, n.ctypes.data))
    return [out[b, :n[b]].tolist() for b in range(n_seq)]


CausalLM.generate_ras_batch = _generate_ras_batch


def _stop_array(stop_ids) -> np.ndarray:
    return np.ascontiguousarray(list(stop_ids), np.int32)


def _generate_greedy(self, prompt_embeds, stop_ids, max_new_tokens: int) -> list[int]:
    """mia_lm_generate_greedy: embedding-row prompt [n, hidden] -> argmax ids (lowest index on ties) until one of `stop_ids` (1..4 of them;
    the stop id is not returned) or `max_new_tokens` ids."""
    lib = self.ctx.lib
    x = np.ascontiguousarray(prompt_embeds, np.float32).reshape(-1, self.cfg.hidden)
    stop = _stop_array(stop_ids)
    out = np.zeros(max(int(max_new_tokens), 1), np.int32)
    n = C.c_int32(0)
    self.ctx.check(lib.mia_lm_generate_greedy(self.h, x.ctypes.data, x.shape[0], stop.ctypes.data, stop.size, int(max_new_tokens), out.ctypes.data, C.byref(n)))
    return out[:n.value].tolist()


def _generate_greedy_batch(self, prompt_embeds, stop_ids, max_new_tokens: int) -> list[list[int]]:
    """mia_lm_generate_greedy_batch: one embedding-row prompt per utterance, decoded side by side (set_batch(n) first); utterance b's ids
    equal generate_greedy(prompt_embeds[b], ...) on the same handle capacity."""
    lib = self.ctx.lib
    n_seq = len(prompt_embeds)
    xs = [np.ascontiguousarray(x, np.float32).reshape(-1, self.cfg.hidden) for x in prompt_embeds]
    offs = np.zeros(n_seq + 1, np.int32)
    np.cumsum([x.shape[0] for x in xs], out=offs[1:])
    flat = np.ascontiguousarray(np.concatenate(xs, axis=0))
    stop = _stop_array(stop_ids)
    stride = max(int(max_new_tokens), 1)
    out = np.zeros((n_seq, stride), np.int32)
    n = np.zeros(n_seq, np.int32)
    self.ctx.check(lib.mia_lm_generate_greedy_batch(self.h, flat.ctypes.data, offs.ctypes.data, n_seq, stop.ctypes.data, stop.size, int(max_new_tokens),
                                                    out.ctypes.data, stride, n.ctypes.data))
    return [out[b, :n[b]].tolist() for b in range(n_seq)]


CausalLM.generate_greedy = _generate_greedy
CausalLM.generate_greedy_batch = _generate_greedy_batch


def _generate_topk(self, prompt_embeds, uniforms, stop_ids, max_new_tokens: int, temperature: float, top_p: float = 0.95, top_k: int = 0) -> list[int]:
    """mia_lm_generate_topk: generate_greedy's loop with sampleNextToken's temperature > 0 branch (top-k, 50 when top_k == 0, then top-p inside
    the top-k set, then an inverse-CDF draw).  uniforms: at least max_new_tokens values in [0, 1), one per drawn id."""
    lib = self.ctx.lib
    x = np.ascontiguousarray(prompt_embeds, np.float32).reshape(-1, self.cfg.hidden)
    stop = _stop_array(stop_ids)
    u = np.ascontiguousarray(uniforms, np.float32).reshape(-1)
    if u.size < max_new_tokens:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "uniforms must hold max_new_tokens values")
    out = np.zeros(max(int(max_new_tokens), 1), np.int32)
    n = C.c_int32(0)
    self.ctx.check(lib.mia_lm_generate_topk(self.h, x.ctypes.data, x.shape[0], float(temperature), int(top_k), float(top_p), stop.ctypes.data, stop.size,
                                            int(max_new_tokens), u.ctypes.data, out.ctypes.data, C.byref(n)))
    return out[:n.value].tolist()


def _generate_topk_batch(self, prompt_embeds, uniforms, stop_ids, max_new_tokens: int, temperature: float, top_p: float = 0.95,
                         top_k: int = 0) -> list[list[int]]:
    """mia_lm_generate_topk_batch: one embedding-row prompt and one uniform row [max_new_tokens] per utterance, decoded side by side
    (set_batch(n) first); utterance b's ids equal generate_topk(prompt_embeds[b], uniforms[b], ...) on the same handle capacity."""
    lib = self.ctx.lib
    n_seq = len(prompt_embeds)
    xs = [np.ascontiguousarray(x, np.float32).reshape(-1, self.cfg.hidden) for x in prompt_embeds]
    offs = np.zeros(n_seq + 1, np.int32)
    np.cumsum([x.shape[0] for x in xs], out=offs[1:])
    flat = np.ascontiguousarray(np.concatenate(xs, axis=0))
    stop = _stop_array(stop_ids)
    u = np.ascontiguousarray(uniforms, np.float32)
    if u.ndim != 2 or u.shape[0] != n_seq or u.shape[1] < max_new_tokens:
        raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, "uniforms must be [n_seq, >= max_new_tokens]")
    u = np.ascontiguousarray(u[:, :max(int(max_new_tokens), 0)])
    stride = max(int(max_new_tokens), 1)
    out = np.zeros((n_seq, stride), np.int32)
    n = np.zeros(n_seq, np.int32)
    self.ctx.check(lib.mia_lm_generate_topk_batch(self.h, flat.ctypes.data, offs.ctypes.data, n_seq, float(temperature), int(top_k), float(top_p),
                                                  stop.ctypes.data, stop.size, int(max_new_tokens), u.ctypes.data, out.ctypes.data, stride, n.ctypes.data))
    return [out[b, :n[b]].tolist() for b in range(n_seq)]


CausalLM.generate_topk = _generate_topk
CausalLM.generate_topk_batch = _generate_topk_batch


def sample_top_k_top_p(ctx: _lib.Context, logits: np.ndarray, uniform: float, temperature: float, top_p: float = 0.95, top_k: int = 0, want_kept: bool = False):
    """FunASRModel.sampleNextToken with temperature > 0 (mia_sample_top_k_top_p) on one row of logits, with an explicit uniform for the draw:
    the picked id, or (id, kept ids in kept order) with want_kept."""
    lg = np.ascontiguousarray(logits, np.float32).reshape(-1)
    out, nk = C.c_int32(0), C.c_int32(0)
    kept = np.zeros(1024, np.int32)
    ctx.check(ctx.lib.mia_sample_top_k_top_p(ctx.h, lg.ctypes.data, lg.size, float(temperature), int(top_k), float(top_p), float(uniform), C.byref(out),
                                             kept.ctypes.data if want_kept else None, C.byref(nk)))
    return (out.value, kept[:nk.value].tolist()) if want_kept else out.value


def sample_next_token(ctx: _lib.Context, logits: np.ndarray, history, uniform: float, temperature=0.6, top_p=0.8, rep_penalty=1.3) -> int:
    """sampleNextToken(logits:history:temperature:topP:repetitionPenalty:) with an explicit uniform for the categorical draw."""
    lg = np.ascontiguousarray(logits, np.float32)
    h = np.ascontiguousarray(history, np.int32)
    out = C.c_int32(0)
    ctx.check(ctx.lib.mia_sample_top_p(ctx.h, lg.ctypes.data, lg.size, h.ctypes.data if h.size else None, h.size, rep_penalty, temperature, top_p,
                                       uniform, C.byref(out)))
    return out.value


def parse_output(tokens: list[int]) -> list[list[int]]:
    """parseOutput (OrpheusTTS.swift:472-508): generated ids -> SNAC code lists [N, 2N, 4N] (host integer logic, as in the Swift)."""
    last = max((i for i, t in enumerate(tokens) if t == AUDIO_CODE_DATA_START_MARKER), default=-1)
    rel = tokens[last + 1:] if last >= 0 else tokens
    f = [t for t in rel if t != END_TOKEN and t >= CODE_OFFSET]
    f = [t - CODE_OFFSET for t in f[:(len(f) // 7) * 7]]
    l1, l2, l3 = [], [], []
    for i in range(len(f) // 7):
        b = 7 * i
        l1.append(f[b]); l2.append(f[b + 1] - 4096); l3.append(f[b + 2] - 2 * 4096); l3.append(f[b + 3] - 3 * 4096)
        l2.append(f[b + 4] - 4 * 4096); l3.append(f[b + 5] - 5 * 4096); l3.append(f[b + 6] - 6 * 4096)
    return [l1, l2, l3]


class Qwen2LM:
    """Qwen2LM.inference (TTS/CosyVoice2/LLM/Qwen2LM.swift:335-376): the prompt is assembled from three embedding tables on the
    host (row gathers, no arithmetic) and handed to the device loop as embedding rows."""

    SOS_EOS, TASK_ID = 0, 1

    def __init__(self, lm: CausalLM, weights: dict[str, np.ndarray], speech_token_size: int = 6561):
        self.lm, self.speech_token_size = lm, speech_token_size
        self.text_emb = weights["model.embed_tokens.weight"]
        self.llm_emb = weights["llm_embedding.weight"]
        self.speech_emb = weights["speech_embedding.weight"]

    def lm_input(self, text, prompt_text, prompt_speech_tokens) -> np.ndarray:
        from .synthetic import round_array
        rows = [self.llm_emb[self.SOS_EOS][None], self.text_emb[np.asarray(list(prompt_text) + list(text), np.int64)],
                self.llm_emb[self.TASK_ID][None]]
        if len(prompt_speech_tokens):
            rows.append(self.speech_emb[np.asarray(prompt_speech_tokens, np.int64)])
        return np.ascontiguousarray(np.concatenate(rows, axis=0), np.float32)

    def inference(self, text, prompt_text, prompt_speech_tokens, uniforms, max_token_text_ratio=20.0, min_token_text_ratio=2.0,
                  top_p=0.8, top_k=25, win=10, tau=0.1) -> list[int]:
        x = self.lm_input(text, prompt_text, prompt_speech_tokens)
        min_len, max_len = int(len(text) * min_token_text_ratio), int(len(text) * max_token_text_ratio)
        return self.lm.generate_ras(x, uniforms, min_len, max_len, self.speech_token_size, top_p, top_k, win, tau)


def merge_embeddings(text_embeddings: np.ndarray, input_ids, audio_embeddings: np.ndarray, sos_id: int, eos_id: int) -> np.ndarray:
    """FunASRModel.mergeEmbeddings (STT/FunASR/FunASRModel.swift:71-141) for one utterance, on rows already looked up:
    [text up to and including the first sos | audio rows | text from the first eos on]; the text rows alone when a marker is missing."""
    ids = [int(t) for t in input_ids]
    text = np.asarray(text_embeddings, np.float32)
    if sos_id not in ids or eos_id not in ids:
        return np.ascontiguousarray(text)
    sos, eos = ids.index(sos_id), ids.index(eos_id)
    return np.ascontiguousarray(np.concatenate([text[:sos + 1], np.asarray(audio_embeddings, np.float32), text[eos:]], axis=0))


class FunASRDecoder:
    """The decoder half of Fun-ASR (STT/FunASR/FunASRSTT.swift:111-156): prompt ids + audio embeddings -> greedy token ids on a Qwen3
    CausalLM.  The audio rows (SenseVoice encoder + adaptor output, [n, hidden]) are an input; embed_weight is the checkpoint's
    model.embed_tokens.weight (the host gathers the prompt's text rows from it, no arithmetic)."""

    def __init__(self, lm: CausalLM, embed_weight: np.ndarray):
        self.lm, self.embed = lm, embed_weight

    def merge_embeddings(self, input_ids, audio_embeddings, sos_id: int, eos_id: int) -> np.ndarray:
        text = np.asarray(self.embed[np.asarray(list(input_ids), np.int64)], np.float32)
        return merge_embeddings(text, input_ids, audio_embeddings, sos_id, eos_id)

    def transcribe_tokens(self, input_ids, audio_embeddings, sos_id: int, eos_id: int, stop_ids, max_tokens: int = 512,
                          temperature: float = 0.0, top_p: float = 0.95, top_k: int = 0, uniforms=None) -> list[int]:
        """temperature == 0: the greedy loop (the reference's `if temperature == 0`).  temperature > 0: sampleNextToken's top-k / top-p
        branch; the RNG stays with the caller, who passes max_tokens uniforms."""
        x = self.merge_embeddings(input_ids, audio_embeddings, sos_id, eos_id)
        if temperature == 0:
            return self.lm.generate_greedy(x, stop_ids, max_tokens)
        if uniforms is None:
            raise ValueError("temperature > 0 needs `uniforms` (max_tokens values in [0, 1)): the draw takes explicit uniforms")
        return self.lm.generate_topk(x, uniforms, stop_ids, max_tokens, temperature, top_p, top_k)


class OrpheusTTS:
    """generateChunk (TTS/Orpheus/TTSEngine/OrpheusTTS.swift:224-373) from token ids onward: LM sampling loop ->
    parseOutput -> SNAC decode.  Text tokenisation / voice prefix / sentence splitting stay with the caller (CPU text code)."""

    def __init__(self, lm: CausalLM, snac, kv_bits: int | None = None, packed_prompt: bool | None = None):
        self.lm, self.snac = lm, snac
        if packed_prompt is not None:                # the prompt pass on the attached packed weights (CausalLM.set_prompt_weights); None leaves the handle's mode alone
            lm.set_prompt_weights(packed_prompt)
        if kv_bits is not None:                      # newCache(quantized: kv_bits != 0, bits: kv_bits); None leaves the handle's mode alone
            lm.new_cache(quantized=kv_bits != 0, bits=kv_bits or 4)

    def generate_chunk(self, input_ids, uniforms, noise=None, temperature=0.6, top_p=0.8, max_new_tokens=MAX_TOKEN_COUNT):
        gen = self.lm.generate(input_ids, uniforms, temperature=temperature, top_p=top_p, rep_penalty=1.3,
                               rep_window=REPETITION_CONTEXT_SIZE, max_new_tokens=max_new_tokens, stop_ids=(END_TOKEN,))
        codes = parse_output(list(input_ids) + gen)
        if not codes[0]:
            return gen, np.zeros(0, np.float32)
        n = len(codes[0])
        lim = self.snac.cfg.codebook_size
        codes = [[min(max(c, 0), lim - 1) for c in lv] for lv in codes]     # random-init LMs emit out-of-layer ids; real ones do not
        nz = noise
        if noise is not None:
            nz = np.ascontiguousarray(noise[:self.snac.noise_len(4 * n)], np.float32)
        return gen, self.snac.decode(codes, nz)

    def generate_chunks(self, input_ids_list, uniforms, noises=None, temperature=0.6, top_p=0.8, max_new_tokens=MAX_TOKEN_COUNT):
        """The sentence loop of OrpheusTTS.generate (OrpheusTTS.swift:179-191) with the sentences' LM loops side by side
        (CausalLM.generate_batch; call lm.set_batch(n) first): one (ids, pcm) pair per sentence, identical to generate_chunk per
        sentence with the same uniforms / noise.  uniforms [n, max_new_tokens]; noises: one array per sentence or None."""
        gens = self.lm.generate_batch(input_ids_list, uniforms, temperature=temperature, top_p=top_p, rep_penalty=1.3,
                                      rep_window=REPETITION_CONTEXT_SIZE, max_new_tokens=max_new_tokens, stop_ids=(END_TOKEN,))
        out = [(gen, np.zeros(0, np.float32)) for gen in gens]
        lim = self.snac.cfg.codebook_size
        todo = []                                    # (sentence, codes, noise) of every sentence that has codes
        for b, gen in enumerate(gens):
            codes = parse_output(list(input_ids_list[b]) + gen)
            if not codes[0]:
                continue
            n = len(codes[0])
            codes = [[min(max(c, 0), lim - 1) for c in lv] for lv in codes]
            nz = None if noises is None or noises[b] is None else np.ascontiguousarray(noises[b][:self.snac.noise_len(4 * n)], np.float32)
            todo.append((b, codes, nz))
        # one stacked SNAC pass per group (SNACDecoder.decode_batch, at most 64 utterances); noise is all-or-none inside a call
        for with_noise in (False, True):
            grp = [t for t in todo if (t[2] is not None) == with_noise]
            for i in range(0, len(grp), 64):
                part = grp[i:i + 64]
                pcms = self.snac.decode_batch([c for _, c, _ in part], [z for _, _, z in part] if with_noise else None)
                for (b, _, _), pcm in zip(part, pcms):
                    out[b] = (gens[b], pcm)
        return out
