"""Host-side mirror of the reference's OuteTTS engine (TTS/OuteTTS): speaker profile (OuteTTSTokens.swift:88-165), prompt processor
(OuteTTSPromptProcessor.swift), generateChunk (OuteTTS.swift:380-511) and speaker-profile creation (OuteTTSAudioProcessor.swift:363-453,
OuteTTSEngine.swift:233-327), backed by the gfx950 HIP layer -- a Llama CausalLM (lm.py) for the token loop, the DAC codec (codec.py)
for the waveform and for the reference clip's codes, and speaker_features.hip for the loudness preprocessing and the three audio
features (energy, spectral centroid, pitch) of the clip and of every word.  The tokenizer, the sentence splitter and the silence
trimmer (AudioTrimmer.findSpeechBounds) stay with the caller, as everywhere in this package.  A profile is created from audio here
(create_speaker_profile) or loaded from the reference's JSON (SpeakerProfile.load); SpeakerProfile.save writes that JSON.

Rounding: the Swift's Int(x) truncates and its round() rounds half away from zero; Python's round() is half-to-even and is not used."""
from __future__ import annotations

import ctypes as C
import json
import math
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

    def to_dict(self) -> dict:
        """The inverse of from_dict: the reference's JSON keys (OuteTTSTokens.swift:104-165); interface_version only when set."""
        feat = lambda f: {"energy": int(f.energy), "spectral_centroid": int(f.spectral_centroid), "pitch": int(f.pitch)}
        d = {"text": self.text,
             "words": [{"word": w.word, "duration": float(w.duration), "c1": [int(c) for c in w.c1], "c2": [int(c) for c in w.c2],
                        "features": feat(w.features)} for w in self.words],
             "global_features": feat(self.global_features)}
        if self.interface_version is not None:
            d["interface_version"] = self.interface_version
        return d

    def save(self, path: str) -> None:
        with open(path, "w", encoding="utf-8") as f:
            json.dump(self.to_dict(), f, ensure_ascii=False)


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
    of lm_sample_top_p.hip with OuteTTS's parameters (penalty 1.1 over the last 64 generated ids, top-p keeping the first token that crosses p).
    The reference divides by the temperature before the penalty, the kernel after: the same function in real arithmetic, one fp32 rounding
    apart.  The prompt repeats the whole speaker profile for every sentence (:327-340, about 1 900 ids for the bundled profile), so the
    constructor puts the handle's prompt pass on the tiled attention kernel; prompt_attention=None leaves the handle's mode alone.
    packed_prompt (True / False) forwards to CausalLM.set_prompt_weights -- the prompt pass on the attached packed weights -- and None,
    the default, leaves the handle's mode alone."""

    def __init__(self, lm, dac, processor: OuteTTSPromptProcessor, eos_id: int, default_speaker: SpeakerProfile | None = None,
                 prompt_attention: int | None = 1, packed_prompt: bool | None = None):
        self.lm, self.dac, self.processor, self.eos_id, self.default_speaker = lm, dac, processor, int(eos_id), default_speaker
        if prompt_attention is not None:
            lm.set_prompt_attention(prompt_attention)
        if packed_prompt is not None:
            lm.set_prompt_weights(packed_prompt)

    def get_speaker(self, reference_audio, reference_text: str, reference_words, processor: "OuteTTSAudioProcessor | None" = None) -> SpeakerProfile:
        """getSpeaker (OuteTTS.swift): a profile from a 24 kHz clip, its text and its [(word, start, end)] list."""
        p = processor or OuteTTSAudioProcessor(self.dac.ctx, self.dac)
        return p.create_speaker_from_transcription(reference_audio, reference_text, reference_words)

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


# ---- speaker-profile creation (OuteTTSAudioProcessor.swift, OuteTTSEngine.swift:233-327) ----
TOKENS_PER_SECOND, MAX_EXTENSION = 75.0, 20          # createSpeakerFromTranscription :395-396


def _round_half_away(x: float) -> float:
    """Swift's round(): half away from zero."""
    return math.floor(x + 0.5) if x >= 0 else -math.floor(-x + 0.5)


@dataclass
class WordSlice:
    """One word of slice_words: codes [c_start, c_end) and samples [a_start, a_end) (a_end == a_start: default features)."""
    c_start: int
    c_end: int
    a_start: int
    a_end: int
    duration: float


def slice_words(words, n_codes: int, n_samples: int, sample_rate: int) -> list[WordSlice]:
    """The slicing rule of createSpeakerFromTranscription (:398-446) as integer arithmetic: words = [(word, start s, end s)].
    Code bounds chain (each word starts where the previous one ended; the first start backs off MAX_EXTENSION codes and clamps to 0, the
    last end extends by MAX_EXTENSION and clamps to n_codes; end < start gives an empty slice).  Audio bounds are Int(t * sr), used only
    if start < end <= n_samples."""
    out: list[WordSlice] = []
    start = None
    for i, (_, t0, t1) in enumerate(words):
        if start is None:
            start = max(0, int(t0 * TOKENS_PER_SECOND) - MAX_EXTENSION)
        raw_end = min(n_codes, int(t1 * TOKENS_PER_SECOND) + MAX_EXTENSION) if i == len(words) - 1 else int(t1 * TOKENS_PER_SECOND)
        end = max(start, raw_end)
        c0, c1 = min(start, n_codes), max(min(start, n_codes), min(end, n_codes))     # c1[start ..< min(end, count)]; start > count traps there
        a0, a1 = int(t0 * float(sample_rate)), int(t1 * float(sample_rate))
        if not (a0 < a1 and a1 <= n_samples):
            a0 = a1 = 0
        out.append(WordSlice(c0, c1, a0, a1, _round_half_away((c1 - c0) / TOKENS_PER_SECOND * 100) / 100))
        start = end
    return out


def adjust_words_after_trim(words, leading_trim_seconds: float, trimmed_duration: float):
    """OuteTTSEngine.swift:282-297: shift by the leading trim, drop words that end before the trimmed audio starts or start after it
    ends, clip the rest to [0, trimmed_duration]."""
    out = []
    for w, t0, t1 in words:
        s, e = t0 - float(leading_trim_seconds), t1 - float(leading_trim_seconds)
        if not e > 0 or not s < float(trimmed_duration):
            continue
        out.append((w, max(0.0, s), min(float(trimmed_duration), e)))
    return out


class SpeakerAudio:
    """mia_speaker_audio: preprocessAudioForSpeaker (:289-336) of a clip, resident on the device.  features(segments) is
    extractAudioFeatures (:191-216) of every (start, length) segment in one call."""

    def __init__(self, ctx, pcm, sample_rate: int = 24000, target_loudness: float = -18.0, peak_limit: float = -1.0):
        from . import _lib
        a = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        self.ctx, self.sample_rate = ctx, int(sample_rate)
        self.h = ctx.lib.mia_speaker_audio_create(ctx.h, a.ctypes.data, a.size, int(sample_rate), float(target_loudness), float(peak_limit))
        if not self.h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        ctx.adopt(self)

    def __len__(self) -> int:
        return int(self.ctx.lib.mia_speaker_audio_len(self.h))

    @property
    def device_ptr(self) -> int:
        return int(self.ctx.lib.mia_speaker_audio_data(self.h) or 0)

    @property
    def launches(self) -> int:
        """Kernels launched by the last features call: it depends on the set of FFT sizes among the segments, not on their number."""
        return int(self.ctx.lib.mia_speaker_audio_launches(self.h))

    def read(self, first: int = 0, n: int | None = None) -> np.ndarray:
        n = len(self) - first if n is None else n
        out = np.empty(max(n, 0), np.float32)
        self.ctx.check(self.ctx.lib.mia_speaker_audio_read(self.h, int(first), int(n), out.ctypes.data))
        return out

    def _features(self, segments, want_raw: bool):
        seg = np.ascontiguousarray(segments, np.int64).reshape(-1, 2)
        start, length = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
        feat = np.zeros((seg.shape[0], 3), np.int32)
        raw = np.zeros((seg.shape[0], 3), np.float32) if want_raw else None
        self.ctx.check(self.ctx.lib.mia_speaker_audio_features(self.h, start.ctypes.data, length.ctypes.data, seg.shape[0], feat.ctypes.data,
                                                               None if raw is None else raw.ctypes.data))
        return feat, raw

    def features(self, segments) -> list[AudioFeatures]:
        """segments: [(start sample, length)]; length 0 gives the default features."""
        return [AudioFeatures(int(e), int(c), int(p)) for e, c, p in self._features(segments, False)[0]]

    def raw_features(self, segments) -> np.ndarray:
        """float32 [S][3] = RMS, centroid in Hz, normalised pitch: the values before min(., 1) and the x100 rounding."""
        return self._features(segments, True)[1]

    def close(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.mia_speaker_audio_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OuteTTSAudioProcessor:
    """OuteTTSAudioProcessor (:341-453) over a DACCodec with its encoder loaded."""

    def __init__(self, ctx, dac, sample_rate: int = 24000):
        self.ctx, self.dac, self.sample_rate = ctx, dac, int(sample_rate)

    def extract_audio_features(self, audio) -> AudioFeatures:
        """extractAudioFeatures (:191-216) of samples taken as they are (target_loudness NaN: no gain); an empty array gives the defaults."""
        a = np.ascontiguousarray(audio, np.float32).reshape(-1)
        if a.size == 0:
            return AudioFeatures()
        sa = SpeakerAudio(self.ctx, a, self.sample_rate, target_loudness=float("nan"))
        try:
            return sa.features([(0, a.size)])[0]
        finally:
            sa.close()

    def create_speaker_from_transcription(self, audio, text: str, words) -> SpeakerProfile:
        """createSpeakerFromTranscription: one SpeakerAudio, one encode, ONE features call for the clip and all words."""
        sa = SpeakerAudio(self.ctx, audio, self.sample_rate)
        try:
            codes = self.dac.encode(sa)
            c1 = [int(v) for v in codes[0]] if codes.shape[0] > 0 else []
            c2 = [int(v) for v in codes[1]] if codes.shape[0] > 1 else []
            n = len(sa)
            sl = slice_words(words, len(c1), n, self.sample_rate)
            feats = sa.features([(0, n)] + [(w.a_start, w.a_end - w.a_start) for w in sl])
        finally:
            sa.close()
        out = [WordData(w[0].strip(_TRIM), s.duration, c1[s.c_start:s.c_end], c2[s.c_start:min(s.c_end, len(c2))], f)
               for w, s, f in zip(words, sl, feats[1:])]
        return SpeakerProfile(normalize_text(text), out, feats[0])


def create_speaker_profile(samples, sample_rate: int, stt, *, leading_trim_seconds: float = 0.0, transcribe_samples=None, processor=None,
                           ctx=None, dac=None, target_rate: int = 24000, transcribe_sample_rate: int = 16000, trim=None,
                           **transcribe_kw) -> SpeakerProfile:
    """createSpeakerProfile(from:) (OuteTTSEngine.swift:233-327) behind the file reader.  With `trim` (a trim.AudioTrimConfig; the engine
    uses trim.DEFAULT) `samples` is the raw clip at `sample_rate`: its speech bounds are found on the device at the clip's own rate
    (:250-266), the clip is sliced to them, the leading trim is Float(start) / Float(sampleRate), the untrimmed clip is transcribed, and
    no bounds found means the whole clip with a trim of 0.  Without it `samples` is the already trimmed clip, `leading_trim_seconds`
    what was cut from the front and `transcribe_samples` the untrimmed clip the reference transcribes (default: `samples`), at the same
    rate; giving either of the two together with `trim` is a ValueError.  stt: a WhisperSTT (transcribe(clips at
    transcribe_sample_rate, word_timestamps=True)).  processor: an OuteTTSAudioProcessor, or ctx and dac to make one.  Rate conversions
    run on the device (mia_resample_sinc) and only when the rates differ."""
    from . import audio_io
    if trim is not None and (leading_trim_seconds != 0.0 or transcribe_samples is not None):
        raise ValueError("trim computes leading_trim_seconds and transcribe_samples itself: pass it alone")
    if processor is None:
        processor = OuteTTSAudioProcessor(ctx, dac, target_rate)
    ctx = processor.ctx
    samples = np.ascontiguousarray(samples, np.float32).reshape(-1)
    if trim is not None:
        from . import trim as T
        transcribe_samples = samples
        bounds = T.find_speech_bounds(ctx, samples, sample_rate, trim)
        if bounds is not None:
            samples = samples[bounds[0]:bounds[1]]
            leading_trim_seconds = float(np.float32(bounds[0]) / np.float32(sample_rate))
    full = samples if transcribe_samples is None else np.ascontiguousarray(transcribe_samples, np.float32).reshape(-1)
    resample = lambda a, to: a if to == sample_rate else audio_io.resample(ctx, a, sample_rate, to)
    result = stt.transcribe([resample(full, transcribe_sample_rate)], word_timestamps=True, **transcribe_kw)[0]
    words = []
    for seg in result.segments:                                   # transcribeAudio (:394-426): strip, drop empty words
        for w in seg.words or []:
            t = w.word.strip(_TRIM)
            if t:
                words.append((t, float(w.start), float(w.end)))
    if not words:
        raise ValueError("Could not transcribe audio - no words detected")
    trimmed_duration = float(np.float32(samples.size) / np.float32(sample_rate))
    words = adjust_words_after_trim(words, leading_trim_seconds, trimmed_duration)
    if not words:
        raise ValueError("No words remain after silence trimming")
    audio = resample(samples, processor.sample_rate)
    text = " ".join(w for w, _, _ in words).strip()
    return processor.create_speaker_from_transcription(audio, text, words)
