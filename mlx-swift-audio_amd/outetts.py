"""Host-side mirror of the reference's OuteTTS engine (TTS/OuteTTS): speaker profile (OuteTTSTokens.swift:88-165), prompt processor
(OuteTTSPromptProcessor.swift) and generateChunk (OuteTTS.swift:380-511), backed by the gfx950 HIP layer -- a Llama CausalLM (lm.py) for
the token loop and the DAC codec (codec.py) for the waveform.  The tokenizer and the sentence splitter stay with the caller, as
everywhere in this package; speaker profiles arrive as JSON (createSpeakerFromTranscription, OuteTTSAudioProcessor.swift:15-278, is CPU
feature extraction that is not built here)."""
from __future__ import annotations

import json
import re
from dataclasses import dataclass, field

import numpy as np

# ---- OuteTTSSpecialTokens (OuteTTSTokens.swift:9-85) ----
BOS, EOS = "<|im_start|>", "<|im_end|>"
TEXT_START, TEXT_END = "<|text_start|>", "<|text_end|>"
AUDIO_START, AUDIO_END = "<|audio_start|>", "<|audio_end|>"
WORD_START, WORD_END = "<|word_start|>", "<|word_end|>"
FEATURES, CODE = "<|features|>", "<|code|>"
GLOBAL_FEATURES_START, GLOBAL_FEATURES_END = "<|global_features_start|>", "<|global_features_end|>"
MARKERS = (BOS, TEXT_START, TEXT_END, AUDIO_START, AUDIO_END, WORD_START, WORD_END, FEATURES, CODE)      # the nine cached at :71-81

REPETITION_PENALTY, REPETITION_CONTEXT_SIZE = 1.1, 64       # OuteTTSConfig; topK and minP sit there too and are never read


def format_c1(v: int) -> str:
    return "<|c1_%d|>" % v


def format_c2(v: int) -> str:
    return "<|c2_%d|>" % v


def format_time(d: float) -> str:
    return "<|t_%.2f|>" % d


def _feature_tokens(f: "AudioFeatures") -> list[str]:
    return ["<|energy_%d|>" % f.energy, "<|spectral_centroid_%d|>" % f.spectral_centroid, "<|pitch_%d|>" % f.pitch]


@dataclass
class AudioFeatures:
    energy: int = 0
    spectral_centroid: int = 0
    pitch: int = 0


@dataclass
class WordData:
    word: str
    duration: float
    c1: list[int]
    c2: list[int]
    features: AudioFeatures = field(default_factory=AudioFeatures)


@dataclass
class SpeakerProfile:
    """OuteTTSSpeakerProfile: the reference's JSON (text, words[{word, duration, c1, c2, features}], global_features, interface_version)."""
    text: str
    words: list[WordData]
    global_features: AudioFeatures = field(default_factory=AudioFeatures)
    interface_version: int | None = None

    @staticmethod
    def from_dict(d: dict) -> "SpeakerProfile":
        feat = lambda f: AudioFeatures(int(f["energy"]), int(f["spectral_centroid"]), int(f["pitch"]))
        words = [WordData(w["word"], float(w["duration"]), [int(c) for c in w["c1"]], [int(c) for c in w["c2"]], feat(w["features"])) for w in d["words"]]
        return SpeakerProfile(d["text"], words, feat(d["global_features"]), d.get("interface_version"))

    @staticmethod
    def load(path: str) -> "SpeakerProfile":
        with open(path, encoding="utf-8") as f:
            return SpeakerProfile.from_dict(json.load(f))


# CharacterSet.whitespaces: general category Zs and the tab; ICU's \\s: [\\t\\n\\f\\r\\p{Z}] (Zs, U+2028, U+2029)
_ZS = "\u0020\u00a0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u202f\u205f\u3000"
_TRIM = _ZS + "\t"
_SPACE_RUN = re.compile("[\t\n\f\r\u2028\u2029" + _ZS + "]+")


def normalize_text(text: str) -> str:
    """normalizeText (OuteTTSPromptProcessor.swift:208-224), statement for statement."""
    r = _SPACE_RUN.sub(" ", text)
    r = r.replace("\u2026", "...")
    r = r.strip(_TRIM)
    for a, b in (("\u201c", '"'), ("\u201d", '"'), ("\u2018", "'"), ("\u2019", "'"), ("\u2013", "-"), ("\u2014", "-")):
        r = r.replace(a, b)
    return "".join(ch for ch in r if not (ord(ch) <= 0x1F or 0x7F <= ord(ch) <= 0x9F))


def _separator(text: str) -> str:
    """getSeparator (:168-181): kana or Han -> the ideographic full stop; everything else (Hangul included) ". "."""
    if any(0x3040 <= ord(c) <= 0x309F or 0x30A0 <= ord(c) <= 0x30FF or 0x4E00 <= ord(c) <= 0x9FFF for c in text):
        return "\u3002"
    return ". "


def merge_speaker_text(input_text: str, speaker_text: str) -> tuple[str, str]:
    """mergeSpeakerText (:184-205) -> (merged text, the separator to append to the last speaker word, trimmed)."""
    spk = speaker_text.strip(_TRIM)
    sep = _separator(spk)
    allowed = ("\u3002", "\uff1f", "\uff01", "?", "!") if sep == "\u3002" else (".", "?", "!")
    rs = ""
    if spk:
        if spk[-1] not in allowed:
            rs = sep
        elif sep != "\u3002":
            rs = " "
    return spk + rs + input_text.strip(_TRIM), rs.strip(_TRIM)


class OuteTTSPromptProcessor:
    def __init__(self):
        self.c1_map: dict[int, int] = {}          # token id -> code value
        self.c2_map: dict[int, int] = {}
        self.c1_base = 0
        self.c2_base = 0
        self.cached: dict[str, int] = {}
        self.newline_id = 198
        self.encode = None

    def build_token_maps(self, convert_token_to_id, encode) -> None:
        """buildTokenMaps (:44-112): convert_token_to_id(str) -> id or None, encode(str) -> ids."""
        self.encode = encode
        for base, fmt in (("c1_base", format_c1), ("c2_base", format_c2)):
            i = convert_token_to_id(fmt(0))
            if i is not None:
                setattr(self, base, i)
        for v in range(1025):
            for m, fmt in ((self.c1_map, format_c1), (self.c2_map, format_c2)):
                i = convert_token_to_id(fmt(v))
                if i is not None:
                    m[i] = v
        names = list(MARKERS) + [format_time(i / 100.0) for i in range(3001)]
        for i in range(101):
            names += ["<|energy_%d|>" % i, "<|spectral_centroid_%d|>" % i, "<|pitch_%d|>" % i]
        for tok in names:
            i = convert_token_to_id(tok)
            if i is not None:
                self.cached[tok] = i
        nl = encode("\n")
        if len(nl):
            self.newline_id = int(nl[0])

    def create_codes(self, words: list[WordData]) -> str:
        """createCodes (:133-155)."""
        out = []
        for w in words:
            pairs = "".join(format_c1(a) + format_c2(b) for a, b in zip(w.c1, w.c2))
            out.append(WORD_START + w.word + FEATURES + format_time(w.duration) + "".join(_feature_tokens(w.features)) + CODE + pairs + WORD_END)
        return "\n".join(out)

    @staticmethod
    def _init_prompt(text: str) -> str:
        return BOS + "\n" + TEXT_START + text + TEXT_END + "\n" + AUDIO_START + "\n"

    @staticmethod
    def _speaker_words(text: str, speaker: SpeakerProfile) -> tuple[str, list[WordData]]:
        merged, sep = merge_speaker_text(text, speaker.text)
        words = list(speaker.words)
        if words:
            last = words[-1]
            words[-1] = WordData(last.word + sep, last.duration, last.c1, last.c2, last.features)
        return merged, words

    def get_completion_prompt(self, text: str, speaker: SpeakerProfile | None) -> str:
        """getCompletionPrompt (:228-252), the string form."""
        text = normalize_text(text)
        if speaker is None:
            return self._init_prompt(text)
        merged, words = self._speaker_words(text, speaker)
        return self._init_prompt(merged) + self.create_codes(words) + "\n" + WORD_START

    def get_completion_prompt_tokens(self, text: str, speaker: SpeakerProfile | None) -> list[int]:
        """getCompletionPromptTokens (:264-345), the id form; a special token missing from the map is skipped, as there."""
        if self.encode is None:
            return []
        text = normalize_text(text)
        toks: list[int] = []

        def add(tok: str) -> None:
            i = self.cached.get(tok)
            if i is not None:
                toks.append(i)

        add(BOS); toks.append(self.newline_id); add(TEXT_START)
        words: list[WordData] = []
        if speaker is not None:
            text, words = self._speaker_words(text, speaker)
        toks.extend(int(t) for t in self.encode(text))
        add(TEXT_END); toks.append(self.newline_id); add(AUDIO_START); toks.append(self.newline_id)
        for w in words:
            add(WORD_START)
            toks.extend(int(t) for t in self.encode(w.word))
            add(FEATURES)
            add(format_time(w.duration))
            for f in _feature_tokens(w.features):
                add(f)
            add(CODE)
            for a, b in zip(w.c1, w.c2):
                toks.append(self.c1_base + a)
                toks.append(self.c2_base + b)
            add(WORD_END)
            toks.append(self.newline_id)
        add(WORD_START)
        return toks

    def extract_audio_from_tokens(self, tokens) -> list[list[int]]:
        """extractAudioFromTokens (:362-380): both maps, truncated to the shorter codebook."""
        cb1 = [self.c1_map[t] for t in tokens if t in self.c1_map]
        cb2 = [self.c2_map[t] for t in tokens if t in self.c2_map]
        n = min(len(cb1), len(cb2))
        return [cb1[:n], cb2[:n]]


class OuteTTS:
    """generateChunk (OuteTTS.swift:380-511): prompt ids -> sampled ids -> (c1, c2) codes -> DAC waveform.  The sampler is the top-p kernel
    of lm_sample.hip with OuteTTS's parameters (penalty 1.1 over the last 64 generated ids, top-p keeping the first token that crosses p).
    The reference divides by the temperature before the penalty, the kernel after: the same function in real arithmetic, one fp32 rounding
    apart.  The prompt repeats the whole speaker profile for every sentence (:327-340, about 1 900 ids for the bundled profile), so the
    constructor puts the handle's prompt pass on the tiled attention kernel; prompt_attention=None leaves the handle's mode alone."""

    def __init__(self, lm, dac, processor: OuteTTSPromptProcessor, eos_id: int, default_speaker: SpeakerProfile | None = None,
                 prompt_attention: int | None = 1):
        self.lm, self.dac, self.processor, self.eos_id, self.default_speaker = lm, dac, processor, int(eos_id), default_speaker
        if prompt_attention is not None:
            lm.set_prompt_attention(prompt_attention)

    def _kw(self, temperature, top_p, max_tokens):
        return dict(temperature=temperature, top_p=top_p, rep_penalty=REPETITION_PENALTY, rep_window=REPETITION_CONTEXT_SIZE,
                    max_new_tokens=max_tokens, stop_ids=(self.eos_id,))

    def _strip(self, gen: list[int]) -> list[int]:
        return gen[:-1] if gen and gen[-1] == self.eos_id else gen      # the reference breaks before appending the EOS

    def _codes(self, gen: list[int]) -> np.ndarray:
        c = self.processor.extract_audio_from_tokens(gen)
        if not c[0] or not c[1]:
            raise ValueError("No audio codes found in generated tokens")
        return np.asarray(c, np.int32)

    def generate_chunk(self, text: str, uniforms, speaker: SpeakerProfile | None = None, temperature: float = 0.4, top_p: float = 0.9,
                       max_tokens: int = 4096) -> tuple[list[int], np.ndarray]:
        """One sentence -> (generated ids without the EOS, float32 waveform).  uniforms: one per possible draw (>= max_tokens)."""
        prompt = self.processor.get_completion_prompt_tokens(text, speaker or self.default_speaker)
        gen = self._strip(self.lm.generate(prompt, uniforms, **self._kw(temperature, top_p, max_tokens)))
        codes = self._codes(gen)
        return gen, np.asarray(self.dac.decode_from_codes(codes[None]), np.float32).reshape(-1)

    def generate_chunks(self, texts: list[str], uniforms, speaker: SpeakerProfile | None = None, temperature: float = 0.4, top_p: float = 0.9,
                        max_tokens: int = 4096) -> list[tuple[list[int], np.ndarray]]:
        """The sentence loop of OuteTTS.generate (:327-340) with the sentences side by side (CausalLM.generate_batch, call lm.set_batch(n)
        first; DACCodec.decode_batch): one (ids, waveform) pair per sentence, identical to generate_chunk per sentence with uniforms[b]."""
        spk = speaker or self.default_speaker
        prompts = [self.processor.get_completion_prompt_tokens(t, spk) for t in texts]
        gens = [self._strip(g) for g in self.lm.generate_batch(prompts, uniforms, **self._kw(temperature, top_p, max_tokens))]
        codes = [self._codes(g) for g in gens]
        pcms: list[np.ndarray] = []
        from .codec import MAX_BATCH
        for i in range(0, len(codes), MAX_BATCH):
            pcms += self.dac.decode_batch(codes[i:i + MAX_BATCH])
        return list(zip(gens, pcms))
