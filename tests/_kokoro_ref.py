"""NumPy restatement of Kokoro's waveform half (reference: TTS/Kokoro of mlx-swift-audio), callable in float64 and in float32: the F0 / N
blocks of Predictor.F0NTrain, KokoroDecoder, Generator, the harmonic source and the STFT pair.  Every function cites the Swift it
restates.  Activations are time-major [T, C] (the reference swaps axes around every convolution); the public entry points take the
reference's channel-major [C, T].  Sizes use the Swift's own float32 expressions.  B = 1 throughout, as the reference runs it.

Three readings that nothing here can pin against a run of the reference are written down in DESIGN.md ("Kokoro"): a negative gather
index counts from the end (interpolate1d), the imaginary part of STFT bins 0 and n_fft / 2 -- and of every bin of frame 0 -- is +0, and
the weight orientation rule."""
import math

import numpy as np

EPS = 1e-5          # InstanceNorm1d.swift (eps)


# ---- ConvWeighted.swift ---------------------------------------------------------------------------------------------------------------
def weight_norm(v, g):
    """weightNorm(dim: 0) (ConvWeighted.swift:36-63): g v / (||v|| + 1e-7), the norm over every axis but 0."""
    dt = v.dtype.type
    axes = tuple(range(1, v.ndim))
    norm = np.sqrt(np.sum(v * v, axis=axes, keepdims=True))
    return v / (norm + dt(1e-7)) * g


def oriented(w, x_channels, groups=1):
    """ConvWeighted.callAsFunction (:118-122): the weight as it is when its last axis is the input's channel count (or the convolution is
    grouped), transposed() -- every axis reversed -- otherwise."""
    return w if (w.shape[-1] == x_channels or groups > 1) else w.transpose()


def conv1d(x, w, b=None, stride=1, pad=0, dil=1):
    """MLX.conv1d on x [T, Cin] with w [Cout, K, Cin]."""
    T, K = x.shape[0], w.shape[1]
    xp = np.concatenate([np.zeros((pad, x.shape[1]), x.dtype), x, np.zeros((pad, x.shape[1]), x.dtype)], 0)
    To = (T + 2 * pad - dil * (K - 1) - 1) // stride + 1
    y = np.zeros((To, w.shape[0]), x.dtype)
    for k in range(K):
        y += xp[k * dil:k * dil + stride * (To - 1) + 1:stride] @ w[:, k, :].T
    return y if b is None else y + b


def conv_transpose1d(x, w, b, stride, pad):
    """MLX.convTransposed1d on x [T, Cin] with w [Cout, K, Cin]: y[t stride + k - pad] += x[t] w[:, k, :]."""
    T, K = x.shape[0], w.shape[1]
    full = np.zeros(((T - 1) * stride + K, w.shape[0]), x.dtype)
    for k in range(K):
        full[k:k + (T - 1) * stride + 1:stride] += x @ w[:, k, :].T
    y = full[pad:full.shape[0] - pad]
    return y if b is None else y + b


def conv_transpose1d_depthwise(x, w, b, stride, pad):
    """The same with groups = C: w [C, K, 1]."""
    T, K = x.shape[0], w.shape[1]
    full = np.zeros(((T - 1) * stride + K, x.shape[1]), x.dtype)
    for k in range(K):
        full[k:k + (T - 1) * stride + 1:stride] += x * w[:, k, 0]
    return full[pad:full.shape[0] - pad] + b


def leaky_relu(x, slope):
    return np.where(x > 0, x, x * x.dtype.type(slope))


# ---- InstanceNorm1d.swift:63-110, AdaIN1d.swift:20-29 ----------------------------------------------------------------------------------
def instance_norm_stats(x):
    """mean and 1 / sqrt(var + eps) per channel over the rows of x [T, C]; MLX.variance is the population variance."""
    dt = x.dtype.type
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    return mean, dt(1) / np.sqrt(var + dt(EPS))


def adain(x, fc_w, fc_b, s):
    h = fc_w @ s + fc_b
    C = x.shape[1]
    gamma, beta = h[:C], h[C:]
    mean, rstd = instance_norm_stats(x)
    return (1 + gamma) * ((x - mean) * rstd) + beta


def adain_affine(x, fc_w, fc_b, s):
    """The same as a x + b (what a fused prologue would apply)."""
    h = fc_w @ s + fc_b
    C = x.shape[1]
    mean, rstd = instance_norm_stats(x)
    a = (1 + h[:C]) * rstd
    return a * x + (h[C:] - a * mean)


# ---- Interpolate.swift ------------------------------------------------------------------------------------------------------------------
def interp_size(width, factor):
    """interpolate (:37-40): max(1, Int(ceil(Float(width) * factor))) in float32."""
    return max(1, int(math.ceil(np.float32(width) * np.float32(factor))))


def interpolate1d_linear(inp, size):
    """interpolate1d (:54-111), mode linear, alignCorners nil, on inp [C, W].  xLow = floor(x) is -1 where x < 0; the gather takes a
    negative index from the end, as NumPy does."""
    dt = inp.dtype.type
    W = inp.shape[1]
    if size == 1:
        x = np.zeros(1, inp.dtype)
    else:
        scale = dt(W) / dt(size)
        x = np.arange(size).astype(inp.dtype) * scale + dt(0.5) * scale - dt(0.5)
    if W == 1:
        return np.broadcast_to(inp, (inp.shape[0], size)).copy()
    lo = np.floor(x).astype(np.int64)
    hi = np.minimum(lo + 1, W - 1)
    frac = x - lo.astype(inp.dtype)
    return inp[:, lo] * (1 - frac) + inp[:, hi] * frac


# ---- MLXSTFT.swift ------------------------------------------------------------------------------------------------------------------------
def hanning(length, dt):
    """hanning (:12-20)."""
    if length == 1:
        return np.ones(1, dt)
    n = np.arange(1 - length, length, 2).astype(dt)
    return (dt(0.5) + dt(0.5) * np.cos(n * dt(math.pi / (length - 1)))).astype(dt)


def window(n_fft, dt):
    """getWindow (:48-67): hanning(winLen + 1)[0 ..< winLen]."""
    return hanning(n_fft + 1, dt)[:n_fft]


def unwrap(p):
    """unwrap (:23-46) along axis 1 of p [bins, frames]."""
    dt = p.dtype.type
    period = dt(2.0 * math.pi)
    d = p[:, 1:] - p[:, :-1]
    hi = period / 2
    lo = -hi
    dm = d - lo
    dm = (((dm % period) + period) % period) + lo
    sign = np.where(d > 0, hi, dm)
    dm = np.where(dm == lo, sign, dm)
    corr = dm - d
    corr = np.where(np.abs(d) < period / 2, dt(0), corr)
    return np.concatenate([p[:, :1], p[:, 1:] + np.cumsum(corr, axis=1)], axis=1)


def _dft(n_fft, dt):
    k = np.arange(n_fft // 2 + 1)[:, None] * np.arange(n_fft)[None, :]
    ang = 2.0 * np.pi * (k % n_fft) / n_fft
    return np.cos(ang).astype(dt), np.sin(ang).astype(dt)


def stft_complex(x, n_fft=20, hop=5):
    """mlxStft (:69-113), reflect padding, as (re, im) [frames, bins].  The imaginary part of bins 0 and n_fft / 2 is +0: a real
    transform has none there, and numpy.fft.rfft returns exactly that.  So is every imaginary part of frame 0: that frame is centred
    on sample 0 of the reflect-padded signal and the window is symmetric about the same point, so the windowed frame is even about its
    centre and its transform is real -- and since the window is 0 at the frame's first sample, the real parts sum to zero over the
    bins, so some bin of frame 0 ALWAYS has a negative real part, whose phase would be +pi or -pi by rounding alone."""
    dt = x.dtype.type
    p = n_fft // 2
    xp = np.concatenate([x[1:p + 1][::-1], x, x[-(p + 1):-1][::-1]])
    F = 1 + (xp.shape[0] - n_fft) // hop
    frames = np.stack([xp[i * hop:i * hop + n_fft] for i in range(F)]) * window(n_fft, dt)
    c, s = _dft(n_fft, dt)
    re, im = frames @ c.T, -(frames @ s.T)
    im[:, 0] = 0
    im[:, n_fft // 2] = 0
    im[0, :] = 0
    return re, im


def stft_transform(x, n_fft=20, hop=5):
    """MLXSTFT.transform (:181-209): (magnitude, phase) [frames, bins]."""
    re, im = stft_complex(x, n_fft, hop)
    return np.sqrt(re * re + im * im), np.arctan2(im, re)


def istft(mag, phase, n_fft=20, hop=5, use_unwrap=True):
    """MLXSTFT.inverse (:211-235) + mlxIstft (:115-163) on [frames, bins]: window-SUM normalisation where the sum is not zero, then the
    centre trim."""
    dt = mag.dtype.type
    ph = unwrap(phase.T).T if use_unwrap else phase
    re, im = mag * np.cos(ph), mag * np.sin(ph)
    F = mag.shape[0]
    c, s = _dft(n_fft, dt)
    wgt = np.full(n_fft // 2 + 1, 2, dt)
    wgt[0] = wgt[-1] = 1
    im = im.copy()
    im[:, 0] = 0
    im[:, -1] = 0                      # irfft ignores them
    frames = ((re * wgt) @ c - (im * wgt) @ s) / dt(n_fft)
    w = window(n_fft, dt)
    t = (F - 1) * hop + n_fft
    rec, ws = np.zeros(t, dt), np.zeros(t, dt)
    for f in range(F):
        rec[f * hop:f * hop + n_fft] += frames[f] * w
        ws[f * hop:f * hop + n_fft] += w
    nz = ws != 0
    rec[nz] = rec[nz] / ws[nz]
    return rec[n_fft // 2:t - n_fft // 2]


# ---- the model ------------------------------------------------------------------------------------------------------------------------
class KokoroRef:
    def __init__(self, cfg, weights, dtype=np.float64):
        self.cfg, self.dt = cfg, dtype
        self.w = {k: np.asarray(v, dtype) for k, v in weights.items()}
        self.up = int(np.prod(cfg.up_rates)) * cfg.hop

    # ConvWeighted on time-major x
    def cw(self, p, x, stride=1, pad=0, dil=1, bias=True):
        w = oriented(weight_norm(self.w[p + ".weight_v"], self.w[p + ".weight_g"]), x.shape[1])
        return conv1d(x, w, self.w[p + ".bias"] if bias else None, stride, pad, dil)

    def ada(self, p, x, s):
        return adain(x, self.w[p + ".fc.weight"], self.w[p + ".fc.bias"], s)

    def adain_resblk(self, p, x, s, up):
        """AdainResBlk1d (AdainResBlk1d.swift:78-125)."""
        dt = self.dt
        h = leaky_relu(self.ada(p + ".norm1", x, s), 0.2)
        if up:
            w = weight_norm(self.w[p + ".pool.weight_v"], self.w[p + ".pool.weight_g"])          # grouped: used as stored
            h = conv_transpose1d_depthwise(h, w, self.w[p + ".pool.bias"], 2, 1)
            h = np.concatenate([np.zeros((1, h.shape[1]), dt), h], 0)
        h = self.cw(p + ".conv1", h, pad=1)
        h = leaky_relu(self.ada(p + ".norm2", h, s), 0.2)
        h = self.cw(p + ".conv2", h, pad=1)
        sc = x
        if up:                                                                                 # UpSample1d: nearest x 2
            sc = np.repeat(sc, 2, axis=0)
        if (p + ".conv1x1.weight_v") in self.w:
            sc = self.cw(p + ".conv1x1", sc, bias=False)
        return (h + sc) / dt(np.sqrt(dt(2.0)))

    def ada_resblock1(self, p, x, s, k, dils):
        """AdaINResBlock1 (AdaINResBlock1.swift:77-105)."""
        for i, d in enumerate(dils):
            a1 = self.w[f"{p}.alpha1.{i}"].reshape(-1)
            a2 = self.w[f"{p}.alpha2.{i}"].reshape(-1)
            xt = self.ada(f"{p}.adain1.{i}", x, s)
            xt = xt + (1 / a1) * np.sin(a1 * xt) ** 2
            xt = self.cw(f"{p}.convs1.{i}", xt, pad=(k * d - d) // 2, dil=d)
            xt = self.ada(f"{p}.adain2.{i}", xt, s)
            xt = xt + (1 / a2) * np.sin(a2 * xt) ** 2
            xt = self.cw(f"{p}.convs2.{i}", xt, pad=(k - 1) // 2)
            x = xt + x
        return x

    def f0n(self, x, s):
        """Predictor.F0NTrain behind `shared` (KokoroModel.swift:70-88): x [pred_dim, T] -> (F0 [2 T], N [2 T])."""
        x = np.asarray(x, self.dt).T
        s = np.asarray(s, self.dt)
        out = []
        for name in ("F0", "N"):
            h = x
            for i in range(3):
                h = self.adain_resblk(f"predictor.{name}.{i}", h, s, i == 1)
            out.append(conv1d(h, self.w[f"predictor.{name}_proj.weight"], self.w[f"predictor.{name}_proj.bias"])[:, 0])
        return out[0], out[1]

    def sine_source(self, f0, noise=None, rand_ini=None):
        """f0Upsample + KokoroSourceModuleHnNSF / KokoroSineGen (Generator.swift:135-140, KokoroSineGen.swift:43-87,
        KokoroSourceModuleHnNSF.swift:47-55): f0 [L] -> source [up L]."""
        dt, c = self.dt, self.cfg
        f0 = np.asarray(f0, dt)
        L, H = f0.shape[0], c.n_harmonics + 1
        f0u = np.repeat(f0, self.up)                                                          # Upsample(scaleFactor: up), nearest
        fn = f0u[:, None] * np.arange(1, H + 1).astype(dt)
        rad = np.mod(fn / dt(c.sample_rate), dt(1))
        if rand_ini is not None:                                                               # randIni, its first column zeroed
            ri = np.asarray(rand_ini, dt).copy()
            ri[0] = 0
            rad[0, :] = rad[0, :] + ri
        rad = interpolate1d_linear(rad.T, interp_size(rad.shape[0], np.float32(1) / np.float32(self.up))).T
        phase = np.cumsum(rad, axis=0) * dt(2) * dt(np.float32(math.pi) if dt is np.float32 else math.pi)
        phase = interpolate1d_linear(phase.T * dt(self.up), interp_size(phase.shape[0], np.float32(self.up))).T
        sine = np.sin(phase) * dt(0.1)
        uv = (f0u > c.voiced_threshold).astype(dt)[:, None]
        amp = uv * dt(0.003) + (1 - uv) * dt(0.1) / 3
        res = sine * uv
        if noise is not None:
            res = res + amp * np.asarray(noise, dt)
        lw, lb = self.w["decoder.generator.m_source.l_linear.weight"], self.w["decoder.generator.m_source.l_linear.bias"]
        return np.tanh(res @ lw.T + lb)[:, 0]

    def phase_rows(self, f0):
        """The phase track the up-interpolation reads (for the test that pins the negative index)."""
        dt, c = self.dt, self.cfg
        f0 = np.asarray(f0, dt)
        rad = np.mod(f0[:, None] * np.arange(1, c.n_harmonics + 2).astype(dt) / dt(c.sample_rate), dt(1))
        return np.cumsum(rad, axis=0) * dt(2) * dt(math.pi) * dt(self.up)

    def har(self, src):
        """Generator.swift:141-143: [frames, 22] = magnitudes | phases."""
        mag, ph = stft_transform(np.asarray(src, self.dt), self.cfg.n_fft, self.cfg.hop)
        return np.concatenate([mag, ph], axis=1)

    def generate(self, x, s, har):
        """Generator.callAsFunction (Generator.swift:145-191) from har: x [up_initial, L] -> waveform [up L]."""
        dt, c = self.dt, self.cfg
        G = "decoder.generator."
        x = np.asarray(x, dt).T
        s = np.asarray(s, dt)
        har = np.asarray(har, dt)
        n_up, nk = len(c.up_rates), len(c.res_kernels)
        for i in range(n_up):
            x = leaky_relu(x, 0.1)
            if i + 1 < n_up:
                dr = int(np.prod(c.up_rates[i + 1:]))
                xs = conv1d(har, self.w[f"{G}noise_convs.{i}.weight"], self.w[f"{G}noise_convs.{i}.bias"], stride=dr, pad=(dr + 1) // 2)
                xs = self.ada_resblock1(f"{G}noise_res.{i}", xs, s, 7, (1, 3, 5))
            else:
                xs = conv1d(har, self.w[f"{G}noise_convs.{i}.weight"], self.w[f"{G}noise_convs.{i}.bias"])
                xs = self.ada_resblock1(f"{G}noise_res.{i}", xs, s, 11, (1, 3, 5))
            w = oriented(weight_norm(self.w[f"{G}ups.{i}.weight_v"], self.w[f"{G}ups.{i}.weight_g"]), x.shape[1])
            k, u = c.up_kernels[i], c.up_rates[i]
            x = conv_transpose1d(x, w, self.w[f"{G}ups.{i}.bias"], u, (k - u) // 2)
            if i == n_up - 1:
                x = np.concatenate([x[1:2], x], 0)                                             # ReflectionPad1d((1, 0))
            x = x + xs
            acc = None
            for j in range(nk):
                r = self.ada_resblock1(f"{G}resblocks.{i * nk + j}", x, s, c.res_kernels[j], c.dilations)
                acc = r if acc is None else acc + r
            x = acc / dt(nk)
        x = leaky_relu(x, 0.01)
        x = self.cw(G + "conv_post", x, pad=3)
        nb = c.n_fft // 2 + 1
        spec, phase = np.exp(x[:, :nb]), np.sin(x[:, nb:])
        return istft(spec, phase, c.n_fft, c.hop)

    def decoder_blocks(self, asr, f0, n, s):
        """KokoroDecoder.callAsFunction up to the generator (KokoroDecoder.swift:84-107): -> x [2 T, up_initial] time-major."""
        dt = self.dt
        D = "decoder."
        asr = np.asarray(asr, dt).T
        s = np.asarray(s, dt)
        F0 = self.cw(D + "F0_conv", np.asarray(f0, dt)[:, None], stride=2, pad=1)
        N = self.cw(D + "N_conv", np.asarray(n, dt)[:, None], stride=2, pad=1)
        x = np.concatenate([asr, F0, N], axis=1)
        x = self.adain_resblk(D + "encode", x, s, False)
        ar = self.cw(D + "asr_res.0", asr)
        for i in range(4):
            x = np.concatenate([x, ar, F0, N], axis=1)
            x = self.adain_resblk(f"{D}decode.{i}", x, s, i == 3)
            if i == 3:
                break
        return x

    def decode(self, asr, f0, n, s, noise=None):
        """KokoroDecoder.callAsFunction: -> (waveform [2 T up], source, (re, im) of the source STFT)."""
        x = self.decoder_blocks(asr, f0, n, s)
        src = self.sine_source(f0, noise)
        return self.generate(x.T, s, self.har(src)), src
