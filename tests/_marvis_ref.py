"""Float64 restatement of the reference's Marvis model, written literally (tests only): Llama3ScaledRoPE with its interleaved pairs and its
applyScaling formula (TTS/Marvis/Models/MarvisLlamaBackbone.swift:18-165), the Llama blocks (:169-292), MarvisModel._embedTokens with
its mask, generateFrame with the two-row first decoder pass and the per-frame decoder cache (MarvisModel.swift:466-586), the sampler rule
of mia.h ("Marvis TTS") and decodePrompt's loop with the all-zero stop (MarvisTTS.swift:452-523).

Switches used by the tests: `split_half` runs the stack on row-permuted q / k weights with split-half RoPE (what the GPU does),
`single_rows` runs the first decoder pass as two single-row steps, `rnd` rounds the activations to a 16-bit storage type at the places
the GPU rounds them (the bound of the logits test is derived from the difference)."""
import numpy as np

ROPE = {"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192.0}


def round_to(a, kind):
    """fp32 values rounded to f16 / bf16 storage (round to nearest even), as float64."""
    a = np.asarray(a, np.float32)
    if kind == "f16":
        return a.astype(np.float16).astype(np.float64)
    if kind == "bf16":
        u = a.view(np.uint32).astype(np.uint64)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        return u.astype(np.uint32).view(np.float32).astype(np.float64)
    return a.astype(np.float64)


def swift_inv_freq(dims, base, scaling=ROPE):
    """ropeInit + applyScaling (:75-127) operation by operation in float32; scaling None = plain RoPE."""
    f = np.float32
    idx = np.arange(0, dims, 2).astype(np.float32)
    freqs = np.power(f(base), -(idx / f(dims))).astype(np.float32)
    if scaling is None:
        return freqs
    sf, lo, hi, old = (f(scaling[k]) for k in ("factor", "low_freq_factor", "high_freq_factor", "original_max_position_embeddings"))
    wavelens = (f(2.0) * f(np.pi)) / freqs
    hi_thr, lo_thr = old / hi, old / lo
    freq_div = freqs / sf
    smooth = np.clip((old / wavelens - lo) / (hi - lo), f(0.0), f(1.0)).astype(np.float32)
    blend = (f(1.0) - smooth) * freq_div + smooth * freqs
    mid = np.where(wavelens > lo_thr, freq_div, blend)
    return np.where(wavelens < hi_thr, freqs, mid).astype(np.float32)


def rope_bands(dims, base, scaling=ROPE):
    """How many frequencies fall in each of applyScaling's three bands: (unscaled, blended, divided)."""
    freqs = np.power(np.float32(base), -(np.arange(0, dims, 2).astype(np.float32) / np.float32(dims)))
    wl = 2.0 * np.pi / freqs.astype(np.float64)
    old, lo, hi = scaling["original_max_position_embeddings"], scaling["low_freq_factor"], scaling["high_freq_factor"]
    return int((wl < old / hi).sum()), int(((wl >= old / hi) & (wl <= old / lo)).sum()), int((wl > old / lo).sum())


def permute_rows(w, heads, dh):
    """q_proj / k_proj rows for split-half RoPE: new[i] = old[2i], new[i + dh/2] = old[2i + 1] inside every head."""
    w = np.asarray(w).reshape(heads, dh // 2, 2, -1)
    return np.concatenate([w[:, :, 0], w[:, :, 1]], axis=1).reshape(heads * dh, -1)


def rope(x, pos, theta, split_half):
    """x [T][H][dh], pos [T]: interleaved pairs (x[2i], x[2i+1]) (:129-164), or the split-half pairs (x[i], x[i + dh/2])."""
    ang = (np.asarray(pos, np.float32)[:, None] * theta[None, :]).astype(np.float32).astype(np.float64)     # idxTheta is fp32
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    if split_half:
        h = x.shape[-1] // 2
        x0, x1 = x[..., :h], x[..., h:]
        return np.concatenate([x0 * c - x1 * s, x1 * c + x0 * s], -1)
    x0, x1 = x[..., 0::2], x[..., 1::2]
    y = np.empty_like(x)
    y[..., 0::2] = x0 * c - x1 * s
    y[..., 1::2] = x1 * c + x0 * s
    return y


def rms_norm(x, w, eps):
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * w


class Stack:
    """MarvisBackbone: blocks with a growing KV cache, final norm."""

    def __init__(self, sc, weights, prefix, scaling, split_half=False, rnd=None):
        self.sc, self.split_half, self.rnd = sc, split_half, (lambda a: round_to(a, rnd)) if rnd else (lambda a: a)
        self.theta = swift_inv_freq(sc.head_dim, sc.rope_theta, scaling)
        g = lambda n: np.asarray(weights[f"{prefix}.{n}"], np.float64)
        self.layers = []
        for l in range(sc.layers):
            p = f"layers.{l}."
            q, k = g(p + "self_attn.q_proj.weight"), g(p + "self_attn.k_proj.weight")
            if split_half:
                q, k = permute_rows(q, sc.heads, sc.head_dim), permute_rows(k, sc.kv_heads, sc.head_dim)
            self.layers.append(dict(q=q, k=k, v=g(p + "self_attn.v_proj.weight"), o=g(p + "self_attn.o_proj.weight"),
                                    gate=g(p + "mlp.gate_proj.weight"), up=g(p + "mlp.up_proj.weight"), down=g(p + "mlp.down_proj.weight"),
                                    n1=g(p + "input_layernorm.weight"), n2=g(p + "post_attention_layernorm.weight")))
        self.norm = g("norm.weight")
        self.reset()

    def reset(self):
        self.cache = [[np.zeros((0, self.sc.kv_heads, self.sc.head_dim)), np.zeros((0, self.sc.kv_heads, self.sc.head_dim))] for _ in self.layers]

    def __call__(self, h):
        sc, r = self.sc, self.rnd
        T = h.shape[0]
        for L, kv in zip(self.layers, self.cache):
            off = kv[0].shape[0]
            pos = np.arange(off, off + T)
            x = r(rms_norm(h, L["n1"], sc.rms_eps))
            q = r(rope((x @ L["q"].T).reshape(T, sc.heads, sc.head_dim), pos, self.theta, self.split_half))
            k = r(rope((x @ L["k"].T).reshape(T, sc.kv_heads, sc.head_dim), pos, self.theta, self.split_half))
            v = r((x @ L["v"].T).reshape(T, sc.kv_heads, sc.head_dim))
            kv[0], kv[1] = np.concatenate([kv[0], k], 0), np.concatenate([kv[1], v], 0)
            rep = sc.heads // sc.kv_heads
            out = np.empty((T, sc.heads, sc.head_dim))
            for hd in range(sc.heads):
                s = q[:, hd] @ kv[0][:, hd // rep].T * sc.head_dim ** -0.5            # [T][off + T]
                s = np.where(np.arange(off + T)[None, :] <= pos[:, None], s, -np.inf)      # causal
                p = np.exp(s - s.max(-1, keepdims=True))
                out[:, hd] = (p / p.sum(-1, keepdims=True)) @ kv[1][:, hd // rep]
            h = h + r(out.reshape(T, -1)) @ L["o"].T
            x = r(rms_norm(h, L["n2"], sc.rms_eps))
            gt = x @ L["gate"].T
            h = h + r(gt / (1.0 + np.exp(-gt)) * (x @ L["up"].T)) @ L["down"].T
        return r(rms_norm(h, self.norm, sc.rms_eps))


def sample_top_p_ascending(x, temperature, top_p, u):
    """The sampler rule of mia.h in float64 (the threshold 1 - top_p in float32) -> (id, kept ids ascending, margins).  margins: the
    distances the fp32 implementation must not cross -- `keep`: of the cumulative sums next to the threshold from it; `order`: the smallest
    relative gap between neighbours from the last dropped entry up; `pick`: of u from the pick's two CDF edges (as fractions of the sum)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    V = x.size
    z = x / np.float64(np.float32(temperature))
    nan = np.isnan(z)
    if nan.all() or not np.isfinite(np.nanmax(z)):
        return 0, np.zeros(0, np.int64), dict(keep=np.inf, order=np.inf, pick=np.inf)
    e = np.where(nan, 0.0, np.exp(np.where(nan, -np.inf, z) - np.nanmax(z)))
    p = e / e.sum()
    order = np.lexsort((np.arange(V), p, ~nan))          # NaN first, then ascending p, the lower index first on equal p
    ps = p[order]
    c = np.cumsum(ps)
    thr = np.float64(np.float32(1.0) - np.float32(top_p))
    above = np.nonzero(c > thr)[0]
    j0 = int(above[0]) if above.size else V - 1
    kept = order[j0:]
    cum = np.cumsum(ps[j0:])
    total = cum[-1]
    hit = np.nonzero(cum > np.float64(np.float32(u)) * total)[0]
    k = int(hit[0]) if hit.size else kept.size - 1
    gaps = [(ps[j + 1] - ps[j]) / ps[j + 1] for j in range(max(j0 - 1, 0), V - 1) if ps[j + 1] > 0]
    lo_edge = cum[k - 1] / total if k > 0 else -np.inf
    margins = dict(keep=min(c[j0] - thr, thr - c[j0 - 1] if j0 > 0 else np.inf) if above.size else thr - c[-1],
                   order=min(gaps) if gaps else np.inf,
                   pick=min(np.float64(np.float32(u)) - lo_edge, cum[k] / total - np.float64(np.float32(u)) if k < kept.size - 1 else np.inf))
    return int(kept[k]), kept, margins


class MarvisRef:
    def __init__(self, cfg, weights, split_half=False, single_rows=False, rnd=None):
        self.cfg, self.single_rows = cfg, single_rows
        self.rnd = (lambda a: round_to(a, rnd)) if rnd else (lambda a: a)
        self.backbone = Stack(cfg.backbone, weights, "backbone", cfg.rope_scaling, split_half, rnd)
        self.decoder = Stack(cfg.decoder, weights, "decoder", cfg.rope_scaling, split_half, rnd)
        g = lambda n: np.asarray(weights[n], np.float64)
        self.text_emb, self.audio_emb, self.proj, self.c0_head, self.audio_head = (g(n) for n in (
            "text_embeddings.weight", "audio_embeddings.weight", "projection.weight", "codebook0_head.weight", "audio_head"))

    def reset(self):
        self.backbone.reset()
        self.decoder.reset()

    def embed_tokens(self, tokens, mask):
        """_embedTokens * mask, summed over the row (MarvisModel.swift:474-476,553-577); rows of any width Cb + 1."""
        tokens, mask = np.asarray(tokens), np.asarray(mask)
        Cb = tokens.shape[1] - 1
        audio = self.audio_emb[tokens[:, :Cb] + np.arange(Cb)[None, :] * self.cfg.audio_vocab]      # [T][Cb][D]
        text = self.text_emb[tokens[:, Cb]][:, None, :]
        return (np.concatenate([audio, text], 1) * mask[:, :, None]).sum(1)

    def embed_audio(self, codebook, ids):
        return self.audio_emb[np.asarray(ids) + codebook * self.cfg.audio_vocab]

    def generate_frame(self, max_codebooks, tokens, mask, sampler, forced=None):
        """generateFrame -> (ids [codebooks], logits [codebooks][V]); sampler(logits, i) -> id; forced[i] replaces id i after its draw."""
        h = self.backbone(self.embed_tokens(tokens, mask))
        last_h = h[-1]
        logits = [self.c0_head @ last_h]
        take = lambda i, d: int(d if forced is None else forced[i])
        ids = [take(0, sampler(logits[0], 0))]
        self.decoder.reset()                                                     # a fresh decoder cache for every frame
        curr = np.stack([last_h, self.embed_audio(0, ids[0])])
        codebooks = min(self.cfg.n_codebooks, max_codebooks)
        for i in range(1, codebooks):
            x = curr @ self.proj.T                                               # (fp32 on the GPU: no rounding here)
            if self.single_rows and x.shape[0] == 2:
                self.decoder(x[:1])
                dec_h = self.decoder(x[1:])
            else:
                dec_h = self.decoder(x)
            logits.append(dec_h[-1] @ self.audio_head[i - 1])                    # matmul(lastDec, Wi)
            ids.append(take(i, sampler(logits[i], i)))
            curr = self.embed_audio(i, ids[i])[None, :]
        return np.array(ids, np.int64), np.stack(logits)

    def decode_prompt(self, tokens, mask, max_codebooks, sampler, max_frames=750):
        """decodePrompt: frames [n][codebooks] (the all-zero frame ends the sentence and is not emitted)."""
        frames = []
        for f in range(max_frames):
            ids, _ = self.generate_frame(max_codebooks, tokens, mask, lambda lg, i: sampler(lg, f, i))
            if ids.sum() == 0:
                break
            frames.append(ids)
            tokens = np.concatenate([ids, [0]])[None, :]
            mask = np.concatenate([np.ones(ids.size, np.int64), [0]])[None, :]
        return np.array(frames, np.int64).reshape(len(frames), -1)
