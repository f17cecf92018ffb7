"""numpy restatement of the sample arithmetic of OuteTTS speaker-profile creation, written from the Swift
(TTS/OuteTTS/OuteTTSAudioProcessor.swift): preprocessAudioForSpeaker (:289-336), extractAudioFeatures (:191-216),
computeSpectralCentroid (:219-277), calculatePitch / extractSinglePitchValue (:15-161).  float64 arithmetic on the fp32 samples by
default; `dt=np.float32` evaluates the same formulas in fp32, which is what sets the scale of the GPU tolerances (tests only).

vDSP_fft_zrip is restated through numpy.fft with Apple's documented conventions: the forward real transform is 2 x the mathematical
DFT, packed as realp[k] = Re X[k], imagp[k] = Im X[k] for 0 < k < N/2, realp[0] = X[0], imagp[0] = X[N/2]; the inverse is unnormalised
(forward then inverse = 2N x the input); vDSP_HANN_NORM is 0.8165 (1 - cos(2 pi n / N)).  None of these numbers is in the
reference's tree."""
import numpy as np

SR = 24000
FRAME, HOP = 400, 160
MIN_F, MAX_F, VOICING = 75.0, 600.0, 0.3
FORWARD_SCALE, ROUND_TRIP, HANN_NORM = 2.0, 2.0 * 800.0, 0.8165


def test_signal(scale: float = 1.0) -> np.ndarray:
    """2.3 s at 24 kHz: a chirp 140 -> 278 Hz and a 1900 Hz tone under a 1.3 Hz envelope, plus noise (seed 3)."""
    rng = np.random.default_rng(3)
    n = int(2.3 * SR)
    t = np.arange(n) / SR
    env = 0.5 * (1 + np.sin(2 * np.pi * 1.3 * t))
    x = 0.3 * env * np.sin(2 * np.pi * (140 + 60 * t) * t) + 0.1 * env * np.sin(2 * np.pi * 1900 * t) + 0.02 * rng.standard_normal(n)
    return (x * scale).astype(np.float32)


def preprocess(a, sr: int = SR, target: float = -18.0, peak: float = -1.0, dt=np.float64) -> np.ndarray:
    """preprocessAudioForSpeaker, the reference's two multiplications; returns dt."""
    a = np.asarray(a, np.float32).astype(dt)
    n0, m = a.size, int(np.float32(0.4) * np.float32(sr))
    if n0 < m:
        a = np.concatenate([a, np.zeros(m - n0, dt)])
    rms_db = dt(20) * np.log10(np.sqrt(np.sum(a * a, dtype=dt) / dt(a.size)) + dt(1e-10))
    gain = np.power(dt(10), (dt(target) - rms_db) / dt(20))
    g = a * gain
    mx = np.abs(g).max()
    thr = np.power(dt(10), dt(peak) / dt(20))
    if mx > thr:
        g = g * (thr / mx)
    return g[:n0]


def hann_norm(n: int = FRAME) -> np.ndarray:
    return HANN_NORM * (1 - np.cos(2 * np.pi * np.arange(n) / n))


def zrip_forward(x):
    """real x [N] -> packed (realp, imagp) [N/2] of vDSP_fft_zrip forward."""
    N = len(x)
    X = np.fft.rfft(np.asarray(x, np.float64)) * FORWARD_SCALE
    re, im = X[:N // 2].real.copy(), X[:N // 2].imag.copy()
    im[0] = X[N // 2].real
    return re, im


def zrip_inverse(re, im, N):
    """packed spectrum -> (realp, imagp) = even and odd samples of the unnormalised inverse."""
    X = np.zeros(N // 2 + 1, complex)
    X[:N // 2] = re + 1j * im
    X[0], X[N // 2] = re[0], im[0]
    x = np.fft.irfft(X, N) * N
    return x[0::2].copy(), x[1::2].copy()


def autocorr_literal(windowed_frame) -> np.ndarray:
    """The reference's :61-95 for one windowed frame: pad to 800, forward, inverse (no conjugate product), realPart[0..<400]."""
    p = np.concatenate([np.asarray(windowed_frame, np.float64), np.zeros(FRAME)])
    re, im = zrip_forward(p)
    re2, _ = zrip_inverse(re, im, 2 * FRAME)
    return re2[:FRAME]


def autocorr_closed(windowed_frame, dt=np.float64) -> np.ndarray:
    ac = np.zeros(FRAME, dt)
    ac[:FRAME // 2] = dt(ROUND_TRIP) * np.asarray(windowed_frame, dt)[0::2]
    return ac


def n_frames(n: int) -> int:
    total = n + (FRAME - n % HOP) % HOP
    return 0 if total < FRAME else (total - FRAME) // HOP + 1           # n <= 80 traps in the Swift; 0 frames here


def pitch_frames(a, sr: int = SR, dt=np.float64, detail: list | None = None) -> np.ndarray:
    """calculatePitch with the closed-form autocorrelation; detail (optional) collects (peak, runner-up, parabola denominator) of
    every voiced frame."""
    a = np.asarray(a, np.float32).astype(dt)
    nf = n_frames(a.size)
    a = np.concatenate([a, np.zeros((FRAME - a.size % HOP) % HOP, dt)])
    w = hann_norm().astype(dt)
    lo, hi = max(1, int(np.float32(sr) / np.float32(MAX_F))), min(FRAME, int(np.float32(sr) / np.float32(MIN_F)))
    out = np.zeros(nf, dt)
    for i in range(nf):
        ac = autocorr_closed(a[i * HOP:i * HOP + FRAME] * w, dt)
        k = lo + int(np.argmax(ac[lo:hi]))                                # first index among equal maxima
        peak = ac[k]
        if peak / (ac[0] + dt(1e-8)) > dt(VOICING) and k > 0:
            delta = dt(0)
            den = ac[k - 1] - dt(2) * peak + ac[k + 1] + dt(1e-8)
            if k < FRAME - 1:
                delta = dt(0.5) * (ac[k - 1] - ac[k + 1]) / den
            period = (dt(k) + delta) / dt(sr)
            p = dt(1) / period if period > 0 else dt(0)
            out[i] = min(max(p, dt(MIN_F)), dt(MAX_F))
            if detail is not None:
                rest = np.delete(ac[lo:hi], k - lo)
                detail.append((float(peak), float(rest.max()), float(den)))
    return out


def single_pitch(a, sr: int = SR, dt=np.float64, detail=None) -> float:
    p = np.clip(pitch_frames(a, sr, dt, detail), dt(MIN_F), dt(MAX_F))
    avg = p.sum(dtype=dt) / dt(p.size) if p.size else dt(0)
    return float(min(max((avg - dt(MIN_F)) / dt(MAX_F - MIN_F), dt(0)), dt(1)))


def centroid(a, sr: int = SR, dt=np.float64) -> float:
    """computeSpectralCentroid: N = 2^ceil(log2 n), packed bins, Hz."""
    a = np.asarray(a, np.float32)
    n = a.size
    N = 1
    while N < n:
        N *= 2
    if N < 2:
        return 0.0
    x = np.zeros(N, dt)
    x[:n] = a
    if dt == np.float32:
        import torch
        X = (torch.fft.rfft(torch.from_numpy(x)) * 2).numpy()
    else:
        X = np.fft.rfft(x) * FORWARD_SCALE
    re, im = X[:N // 2].real.astype(dt), X[:N // 2].imag.astype(dt)
    im[0] = X[N // 2].real
    mag = np.sqrt(re * re + im * im)
    f = np.arange(N // 2).astype(dt) * (dt(sr) / dt(N))
    s = mag.sum(dtype=dt)
    return float((f * mag).sum(dtype=dt) / s) if s > 1e-10 else 0.0


def raw_features(a, sr: int = SR, dt=np.float64, detail=None) -> tuple:
    """(RMS, centroid in Hz, normalised pitch); an empty or non-finite segment gives zeros."""
    a = np.asarray(a, np.float32)
    if a.size == 0 or not np.isfinite(a).all():
        return (0.0, 0.0, 0.0)
    x = a.astype(dt)
    rms = float(np.sqrt(np.sum(x * x, dtype=dt) / dt(a.size)))
    return (rms, centroid(a, sr, dt), single_pitch(a, sr, dt, detail))


def scaled(raw, sr: int = SR) -> tuple:
    """The three v * 100 before rounding."""
    return (min(raw[0], 1.0) * 100, min(raw[1] / (sr // 2), 1.0) * 100, raw[2] * 100)


def features(raw, sr: int = SR) -> tuple:
    """Int(round(v * 100)), half away from zero (all v >= 0)."""
    return tuple(int(np.floor(v + 0.5)) for v in scaled(raw, sr))
