"""Test-side helpers for the OuteTTS engine (mlx_swift_audio_amd/outetts.py): a toy tokenizer over the engine's special tokens, and a
restatement of the reference's sampling loop (OuteTTS.swift:421-482) on the fp32 oracle.

The toy vocabulary (3 000 ids, the micro LMs' size) is laid out so that most of it is audio-code tokens, which makes a random-init model
emit codes: [0, 96) newline + printable ASCII, one id per character (any other character maps to '?'); then the nine markers and
<|im_end|>; <|t_0.00|> .. <|t_2.00|>; the energy / spectral-centroid / pitch tokens 0 .. 100; <|c1_0|> .. <|c1_1023|> at C1_BASE and
<|c2_0|> .. <|c2_1023|> at C2_BASE.  (<|c1_1024|> / <|c2_1024|> and the times above 2 s are not in it: the processor must cope.)"""
import re

import numpy as np

from mlx_swift_audio_amd import outetts as OT

CHARS = "\n" + "".join(chr(c) for c in range(32, 127))
SPECIALS: dict[str, int] = {}
for _c in (*OT.MARKERS, OT.EOS):
    SPECIALS[_c] = len(CHARS) + len(SPECIALS)
for _i in range(201):
    SPECIALS[OT.format_time(_i / 100.0)] = len(CHARS) + len(SPECIALS)
for _i in range(101):
    for _n in ("energy", "spectral_centroid", "pitch"):
        SPECIALS["<|%s_%d|>" % (_n, _i)] = len(CHARS) + len(SPECIALS)
C1_BASE = len(CHARS) + len(SPECIALS)
for _i in range(1024):
    SPECIALS[OT.format_c1(_i)] = C1_BASE + _i
C2_BASE = C1_BASE + 1024
for _i in range(1024):
    SPECIALS[OT.format_c2(_i)] = C2_BASE + _i
VOCAB = C2_BASE + 1024
EOS_ID = SPECIALS[OT.EOS]
_SPLIT = re.compile(r"(<\|[^|]*\|>)")


def convert_token_to_id(tok: str):
    return SPECIALS.get(tok)


def encode(text: str) -> list[int]:
    """<|...|> specials in the table -> their id; everything else one id per character."""
    out = []
    for part in _SPLIT.split(text):
        if part in SPECIALS:
            out.append(SPECIALS[part])
        else:
            out += [CHARS.index(ch) if ch in CHARS else CHARS.index("?") for ch in part]
    return out


def processor(drop=()):
    p = OT.OuteTTSPromptProcessor()
    p.build_token_maps(lambda t: None if t in drop else convert_token_to_id(t), encode)
    return p


def seeded_speaker(seed: int, n_words: int, n_pairs: int, code_max: int = 1024) -> OT.SpeakerProfile:
    """A profile with n_words lower-case words and n_pairs code pairs spread over them (every word gets at least one)."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, n_pairs), n_words - 1, replace=False)) if n_words > 1 else np.zeros(0, int)
    counts = np.diff(np.concatenate([[0], cuts, [n_pairs]])).astype(int)
    words = []
    for n in counts:
        w = "".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 8))))
        words.append(OT.WordData(w, round(float(n) / 75.0, 2), rng.integers(0, code_max, n).tolist(), rng.integers(0, code_max, n).tolist(),
                                 OT.AudioFeatures(int(rng.integers(0, 101)), int(rng.integers(0, 101)), int(rng.integers(0, 101)))))
    return OT.SpeakerProfile(" ".join(w.word for w in words), words, OT.AudioFeatures(10, 20, 30), 3)


# ---- the reference's loop on the oracle ----
def _scaled(logits, hist, temperature, rep_penalty):
    """OuteTTS's order (OuteTTS.swift:428-444): divide by the temperature FIRST, then the penalty on the scaled logits (fp32)."""
    lg = (np.asarray(logits, np.float32) / np.float32(max(temperature, 1e-6))).astype(np.float32)
    if rep_penalty != 1.0 and len(hist):
        idx = np.asarray(hist, np.int64)
        g = lg[idx]
        lg[idx] = np.where(g < 0, g * np.float32(rep_penalty), g / np.float32(rep_penalty))
    return lg


def generate(ora, prompt, temperature, top_p, max_tokens, eos_id, uniforms, trace=None, rep_penalty=1.1, rep_window=64):
    """generateChunk's loop: returns the generated ids WITHOUT the EOS (the reference breaks before appending it).  trace receives one
    oracle.lm.sample_boundary_distance pair per draw, taken on the scaled and penalised logits."""
    from oracle import lm as OL
    ora.reset()
    logits = ora.forward(prompt)[-1].numpy()
    out = []
    for i in range(max_tokens):
        lg = _scaled(logits, out[-rep_window:], temperature, rep_penalty)
        f = OL.top_p_filter(lg, [], 1.0, 1.0, top_p)
        nxt = OL.sample_with_uniform(f, float(uniforms[i]))
        if trace is not None:
            trace.append(OL.sample_boundary_distance(lg, [], 1.0, 1.0, top_p, float(uniforms[i])))
        if nxt == eos_id:
            break
        out.append(nxt)
        if i + 1 < max_tokens:
            logits = ora.forward([nxt])[-1].numpy()
    return out
