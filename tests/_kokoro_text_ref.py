"""NumPy restatement of Kokoro's text half (reference: TTS/Kokoro of mlx-swift-audio), callable in float64 and in float32: BiLSTM,
AdaLayerNorm, DurationEncoder, the duration head, the alignment and TextEncoder.  Every function cites the Swift it restates.  B = 1, as
the reference runs it, so every MLX.where(mask, ...) is a no-op.  Activations are time-major [N, C]; `asr` and the output of `shared`
are channel-major, as the reference holds them."""
import numpy as np

import _kokoro_ref as R

LSTM_KEYS = tuple(f"{t}_l0{d}" for d in ("", "_reverse") for t in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def bilstm(x, w, p=""):
    """BiLSTM.callAsFunction from zero state (LSTM.swift:56-185) on x [T, In] with the tensors w[p + key]: -> [T, 2 H]."""
    T, out = x.shape[0], []
    for sfx, order in (("", range(T)), ("_reverse", range(T - 1, -1, -1))):
        wih, whh = w[f"{p}weight_ih_l0{sfx}"], w[f"{p}weight_hh_l0{sfx}"]
        xp = (w[f"{p}bias_ih_l0{sfx}"] + w[f"{p}bias_hh_l0{sfx}"]) + x @ wih.T              # addMM(bias_ih + bias_hh, x, W_ih^T)
        H = whh.shape[1]
        h, c, hs = np.zeros(H, x.dtype), np.zeros(H, x.dtype), np.zeros((T, H), x.dtype)
        for t in order:
            g = xp[t] + h @ whh.T
            i, f, gg, o = sigmoid(g[:H]), sigmoid(g[H:2 * H]), np.tanh(g[2 * H:3 * H]), sigmoid(g[3 * H:])
            c = f * c + i * gg
            h = o * np.tanh(c)
            hs[t] = h
        out.append(hs)
    return np.concatenate(out, axis=1)


def _normalised(x):
    dt = x.dtype.type
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    return (x - mean) / np.sqrt(var + dt(R.EPS))


def ada_layer_norm(x, fc_w, fc_b, s):
    """AdaLayerNorm.swift:20-32 on x [N, D]."""
    h = fc_w @ s + fc_b
    D = x.shape[1]
    return (1 + h[:D]) * _normalised(x) + h[D:]


def layer_norm(x, gamma, beta):
    """LayerNormInference.swift:22-24."""
    return _normalised(x) * gamma + beta


def alignment_matrix(dur, dtype=np.float64):
    """pred_aln_trg (KokoroTTS.swift:318-386): [N, T], a single 1 per column."""
    idx = np.repeat(np.arange(len(dur)), dur)
    m = np.zeros((len(dur), len(idx)), dtype)
    m[idx, np.arange(len(idx))] = 1
    return m


def align(d, t_en, dur):
    """KokoroTTS.swift:397,407 as the row gathers they are: (en [T, D + S], asr [D, T])."""
    idx = np.repeat(np.arange(len(dur)), dur)
    return d[idx], t_en[idx].T


class KokoroTextRef:
    def __init__(self, cfg, weights, dtype=np.float64):
        self.cfg, self.dt, self.raw, self.w = cfg, dtype, weights, {}

    def __getitem__(self, k):
        if k not in self.w:
            self.w[k] = np.asarray(self.raw[k], self.dt)
        return self.w[k]

    def lstm(self, p, x):
        return bilstm(x, self, p + ".")

    def duration_encoder(self, d_en, s):
        """DurationEncoder.swift:46-73: d_en [N, D], s [S] -> [N, D + S]."""
        d_en, s = np.asarray(d_en, self.dt), np.asarray(s, self.dt)
        st = np.broadcast_to(s, (d_en.shape[0], s.shape[0]))
        x = np.concatenate([d_en, st], axis=1)
        for i in range(3):
            p = f"predictor.text_encoder.norm{i}.fc."
            h = ada_layer_norm(self.lstm(f"predictor.text_encoder.lstm{i}", x), self[p + "weight"], self[p + "bias"], s)
            x = np.concatenate([h, st], axis=1)
        return x

    def durations(self, d_en, s, speed=1.0):
        """KokoroTTS.swift:303-315: -> (d, durations int32 [N], their value before rounding)."""
        d = self.duration_encoder(d_en, s)
        z = self.lstm("predictor.lstm", d) @ self["predictor.duration_proj.weight"].T + self["predictor.duration_proj.bias"]
        raw = sigmoid(z).sum(axis=-1) / self.dt(np.float32(speed))
        return d, np.maximum(np.rint(raw), 1).astype(np.int32), raw

    def encode(self, ids):
        """TextEncoder.swift:68-92: ids [N] -> [N, D]."""
        x = self["text_encoder.embedding.weight"][np.asarray(ids)]
        for i in range(self.cfg.text_depth):
            p = f"text_encoder.cnn.{i}."
            w = R.oriented(R.weight_norm(self[p + "conv.weight_v"], self[p + "conv.weight_g"]), x.shape[1])
            x = R.conv1d(x, w, self[p + "conv.bias"], pad=(self.cfg.text_kernel - 1) // 2)
            x = R.leaky_relu(layer_norm(x, self[p + "norm.gamma"], self[p + "norm.beta"]), 0.2)
        return self.lstm("text_encoder.lstm", x)

    def shared(self, en):
        """Predictor.F0NTrain's first line (KokoroModel.swift:68): en [T, D + S] -> [D, T]."""
        return self.lstm("predictor.shared", np.asarray(en, self.dt)).T
