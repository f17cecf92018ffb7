"""Host-side mirror of Utils/AudioTrimmer.swift: silence trimming of a reference clip and clipping at a word boundary.

The sample arithmetic -- the frame energies and the two threshold scans of findSpeechBounds (:218-274) / trimSilence (:142-207) -- runs
on the device (csrc/audio_trim.hip behind `Clip`); there is no CPU version of it.  The word logic (:285-390) and the two combined entry
points (:404-567) are host integer and float code, as outetts.slice_words is.  Words are timing.Word (word, start, end, probability):
start / end are doubles and probability a float32 in the reference, and every fp32 step below is the Swift's."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _lib

_f32 = np.float32


@dataclass
class AudioTrimConfig:
    """AudioTrimConfig (:15-79).  Lengths in seconds, top_db in dB below the loudest frame."""
    top_db: float = 60.0
    frame_length: float = 0.025
    hop_length: float = 0.0125
    trailing_words_to_drop: int = 1
    min_word_probability: float = 0.3
    max_word_duration: float = 2.0

    def frame_samples(self, sample_rate: int) -> int:
        """Int(frameLength * Float(sampleRate)): the fp32 product, truncated."""
        return int(_f32(self.frame_length) * _f32(sample_rate))

    def hop_samples(self, sample_rate: int) -> int:
        return int(_f32(self.hop_length) * _f32(sample_rate))


COSYVOICE2 = AudioTrimConfig(top_db=60.0)
CHATTERBOX = AudioTrimConfig(top_db=20.0)         # more aggressive trimming
DEFAULT = AudioTrimConfig()


def num_frames(n: int, frame: int, hop: int) -> int:
    """max(1, (n - frame) / hop + 1) with Swift's division, which truncates toward zero (Python's // floors)."""
    d = n - frame
    q = d // hop if d >= 0 else -((-d) // hop)
    return max(1, q + 1)


class Clip:
    """mia_clip: a clip uploaded once and kept on the device as given."""

    def __init__(self, ctx, pcm, sample_rate: int):
        a = np.ascontiguousarray(pcm, np.float32).reshape(-1)
        self.ctx, self.sample_rate = ctx, int(sample_rate)
        self.h = ctx.lib.mia_clip_create(ctx.h, a.ctypes.data, a.size, int(sample_rate))
        if not self.h:
            raise _lib.MiaError(_lib.ERR_INVALID_ARGUMENT, ctx.lib.mia_last_error(ctx.h).decode())
        ctx.adopt(self)

    def __len__(self) -> int:
        return int(self.ctx.lib.mia_clip_len(self.h))

    @property
    def device_ptr(self) -> int:
        return int(self.ctx.lib.mia_clip_data(self.h) or 0)

    @property
    def launches(self) -> int:
        """Kernels launched by the last bounds call: the same for every clip length (0 after a refused call)."""
        return int(self.ctx.lib.mia_clip_launches(self.h))

    def read(self, first: int = 0, n: int | None = None) -> np.ndarray:
        n = len(self) - first if n is None else n
        out = np.empty(max(n, 0), np.float32)
        self.ctx.check(self.ctx.lib.mia_clip_read(self.h, int(first), int(n), out.ctypes.data))
        return out

    def bounds(self, frame: int, hop: int, top_db: float) -> tuple[int, int, bool]:
        """(start, end, found) of mia_clip_speech_bounds for frame / hop in samples."""
        import ctypes as C
        s, e, f = C.c_int64(0), C.c_int64(0), C.c_int(0)
        self.ctx.check(self.ctx.lib.mia_clip_speech_bounds(self.h, int(frame), int(hop), float(top_db), C.byref(s), C.byref(e), C.byref(f)))
        return s.value, e.value, bool(f.value)

    def speech_bounds(self, config: AudioTrimConfig = DEFAULT) -> tuple[int, int] | None:
        """findSpeechBounds of the clip at its own rate; None when the frame or hop is not positive or no speech is found."""
        frame, hop = config.frame_samples(self.sample_rate), config.hop_samples(self.sample_rate)
        if frame <= 0 or hop <= 0:
            return None
        s, e, found = self.bounds(frame, hop, config.top_db)
        return (s, e) if found else None

    def frame_energy(self, frame: int, hop: int, first_frame: int = 0, n_frames: int | None = None) -> np.ndarray:
        """Mean squares (float64) of frames [first_frame, first_frame + n_frames); default: up to the clip's last frame."""
        if n_frames is None:
            n_frames = num_frames(len(self), frame, hop) - first_frame
        out = np.empty(max(n_frames, 0), np.float64)
        self.ctx.check(self.ctx.lib.mia_clip_frame_energy(self.h, int(frame), int(hop), int(first_frame), int(n_frames), out.ctypes.data))
        return out

    def close(self):
        if self.h and getattr(self.ctx, "h", None):
            self.ctx.lib.mia_clip_free(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def find_speech_bounds(ctx, audio, sample_rate: int, config: AudioTrimConfig = DEFAULT) -> tuple[int, int] | None:
    """findSpeechBounds (:218-274): (start, end) in samples, or None (empty audio, a non-positive frame or hop, nothing found)."""
    a = np.ascontiguousarray(audio, np.float32).reshape(-1)
    if a.size == 0 or config.frame_samples(sample_rate) <= 0 or config.hop_samples(sample_rate) <= 0:
        return None
    clip = Clip(ctx, a, sample_rate)
    try:
        return clip.speech_bounds(config)
    finally:
        clip.close()


def trim_silence(ctx, audio, sample_rate: int, config: AudioTrimConfig = DEFAULT) -> np.ndarray:
    """trimSilence (:142-207): the same search with the reference's early returns -- empty audio and a non-positive frame or hop give
    the input back, no qualifying frame falls back to frames 0 .. numFrames - 1, and start >= end gives the input back."""
    a = np.ascontiguousarray(audio, np.float32).reshape(-1)
    frame, hop = config.frame_samples(sample_rate), config.hop_samples(sample_rate)
    if a.size == 0 or frame <= 0 or hop <= 0:
        return a
    clip = Clip(ctx, a, sample_rate)
    try:
        start, end, found = clip.bounds(frame, hop, config.top_db)
    finally:
        clip.close()
    if not found:                                         # startFrame = 0, endFrame = numFrames - 1
        start, end = 0, min(num_frames(a.size, frame, hop) * hop, a.size)
    return a[start:end] if start < end else a


# ---- word logic (:285-390) ------------------------------------------------------------------------------------------------------------
def word_anomaly_score(word) -> float:
    """AudioTrimmer.wordAnomalyScore (:285-306) -- not timing.word_anomaly_score: the duration is Float(end - start), subtracted in
    double and rounded once."""
    score = _f32(0)
    if _f32(word.probability) < _f32(0.15):
        score += _f32(1.0)
    d = _f32(float(word.end) - float(word.start))
    if d < _f32(0.133):
        score += (_f32(0.133) - d) * _f32(15)
    if d > _f32(2.0):
        score += d - _f32(2.0)
    return float(score)


def drop_unreliable_trailing_words(words, audio_duration: float, config: AudioTrimConfig = DEFAULT) -> list:
    """dropUnreliableTrailingWords (:318-355): drop trailing words that end after the audio (+ 0.05 s, in fp32), then trailing words
    with an anomaly above 0.5 or a probability below the minimum, then the safety-margin words while more than one word is left."""
    out = list(words)
    limit = _f32(audio_duration) + _f32(0.05)
    while out and _f32(out[-1].end) > limit:
        out.pop()
    while out and (_f32(word_anomaly_score(out[-1])) > _f32(0.5) or _f32(out[-1].probability) < _f32(config.min_word_probability)):
        out.pop()
    for _ in range(config.trailing_words_to_drop):
        if len(out) > 1:
            out.pop()
    return out


def find_word_boundary_clip_point(words, max_duration: float, sample_rate: int, safety_margin: float = 0.1):
    """findWordBoundaryClipPoint (:368-390): (clip sample, words kept) or None.  clipSample = Int(Float(end) * Float(sampleRate))."""
    target = _f32(max_duration) - _f32(safety_margin)
    valid = [w for w in words if _f32(w.end) <= target]
    if not valid:
        if words and _f32(words[0].end) <= _f32(max_duration):       # no word fits: try the first one alone
            return int(_f32(words[0].end) * _f32(sample_rate)), [words[0]]
        return None
    return int(_f32(valid[-1].end) * _f32(sample_rate)), valid


# ---- combined entry points (:404-567) ---------------------------------------------------------------------------------------------------
@dataclass
class AudioTrimResult:
    """AudioTrimResult (:84-123)."""
    audio: np.ndarray
    sample_rate: int
    transcription: str | None = None
    words: list | None = None
    original_duration: float = 0.0
    trimmed_duration: float = 0.0
    clipped_at_word_boundary: bool = False


def _seconds(n: int, sample_rate: int) -> float:
    return float(_f32(n) / _f32(sample_rate))


def trim(ctx, audio, sample_rate: int, max_duration: float | None = None, config: AudioTrimConfig = DEFAULT) -> AudioTrimResult:
    """AudioTrimmer.trim (:404-434): silence trimming, then a plain cut at max_duration."""
    a = np.ascontiguousarray(audio, np.float32).reshape(-1)
    trimmed = trim_silence(ctx, a, sample_rate, config)
    if max_duration is not None:
        trimmed = trimmed[:max(int(_f32(max_duration) * _f32(sample_rate)), 0)]
    return AudioTrimResult(trimmed, sample_rate, None, None, _seconds(a.size, sample_rate), _seconds(trimmed.size, sample_rate), False)


def transcribed_words(result) -> list:
    """result.segments.flatMap { $0.words ?? [] }."""
    return [w for seg in result.segments for w in (seg.words or [])]


def trim_at_word_boundary(ctx, audio, sample_rate: int, max_duration: float, stt, config: AudioTrimConfig = DEFAULT,
                          **transcribe_kw) -> AudioTrimResult:
    """trimAtWordBoundary (:453-567).  stt: a WhisperSTT (transcribe([clip at 16 kHz], word_timestamps=True)); the clip is resampled for
    it by audio_io.resample.  Both fall-backs to plain truncation report trimmed_duration = max_duration, as the reference does."""
    from . import audio_io
    a = np.ascontiguousarray(audio, np.float32).reshape(-1)
    original = _seconds(a.size, sample_rate)
    trimmed = trim_silence(ctx, a, sample_rate, config)
    trimmed_duration = _seconds(trimmed.size, sample_rate)
    if _f32(trimmed_duration) <= _f32(max_duration):
        return AudioTrimResult(trimmed, sample_rate, None, None, original, trimmed_duration, False)
    result = stt.transcribe([audio_io.resample(ctx, trimmed, sample_rate, 16000)], word_timestamps=True, **transcribe_kw)[0]
    words = transcribed_words(result)
    truncated = lambda kept: AudioTrimResult(trimmed[:max(int(_f32(max_duration) * _f32(sample_rate)), 0)], sample_rate, result.text, kept, original,
                                             float(_f32(max_duration)), False)
    if not words:
        return truncated(None)
    words = drop_unreliable_trailing_words(words, trimmed_duration, config)
    point = find_word_boundary_clip_point(words, max_duration, sample_rate)
    if point is None:
        return truncated(words)
    clip_sample, valid = point
    clipped = trimmed[:max(clip_sample, 0)]
    return AudioTrimResult(clipped, sample_rate, "".join(w.word for w in valid), valid, original, _seconds(clipped.size, sample_rate), True)
