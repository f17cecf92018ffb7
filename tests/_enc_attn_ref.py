"""fp64 references for the Whisper encoder's attention (csrc/attention.hip) and for the two special GEMM store layouts that feed it
(csrc/gemm.hip: MIA_EPI_QKV_VT, MIA_EPI_HEADMAJOR), plus a plain restatement of the attention kernel's lazy-rescale rule.

The restatement (tile_rule) only CLASSIFIES inputs -- which queries move their reference point in which key tile, how large P gets before
its 16-bit rounding -- so that a test can assert that a spiked case reaches the path it was built for.  Expected values always come from
attention_ref / epilogue_ref.  The `wrong` arguments produce deliberately wrong references: tests/test_enc_attn_ref.py uses them to show
that every comparison the GPU tests make can fail."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 0.125                       # (64^-1/4)^2
KINDS = {"bf16": (2.0 ** -8, 7), "f16": (2.0 ** -11, 10)}          # half an ulp of a value in [1, 2) relative to it; mantissa bits


def kernel_constants():
    """(KV_TILE, LAZY_LOG2) as attention.hip states them."""
    text = open(os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "attention.hip")).read()
    tile = re.search(r"constexpr\s+int\s+KV_TILE\s*=\s*(\d+)\s*;", text)
    lazy = re.search(r"constexpr\s+float\s+LAZY_LOG2\s*=\s*([0-9.]+)f?\s*;", text)
    assert tile and lazy, "attention.hip no longer states KV_TILE / LAZY_LOG2 as constexpr"
    return int(tile.group(1)), float(lazy.group(1))


def round16(a, kind):
    from mlx_swift_audio_amd.synthetic import round_array
    return round_array(np.asarray(a, np.float32), kind).astype(np.float64)


def swap23(i):
    i = np.asarray(i)
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


def _heads(q, k, v, B, T, H):
    for b in range(B):
        for h in range(H):
            sl = (slice(b * T, (b + 1) * T), slice(h * 64, (h + 1) * 64))
            yield b, h, sl, q[sl], k[sl], v[sl]


def attention_ref(q, k, v, B, T, H, kind, wrong=None):
    """softmax(q k^T / 8) v per (b, h) in fp64 of the inputs rounded to `kind`; q / k / v [B*T, H*64].  Returns (out [B*T, H*64],
    vmax [B, H] = the largest |v| of each head).
    wrong: None | "drop_last_key" | "swap23_v" | "no_rescale" | "scale_twice" | "scale_none"."""
    q, k, v = (round16(a, kind) for a in (q, k, v))
    out = np.zeros((B * T, H * 64))
    vmax = np.zeros((B, H))
    scale = {"scale_twice": SCALE * SCALE, "scale_none": 1.0}.get(wrong, SCALE)
    for b, h, sl, qh, kh, vh in _heads(q, k, v, B, T, H):
        vmax[b, h] = np.abs(vh).max()
        if wrong == "no_rescale":
            out[sl] = _tiled(qh, kh, vh, rescale_o=False)
            continue
        if wrong == "swap23_v":
            vh = vh[np.minimum(swap23(np.arange(T)), T - 1)]
        n = T - 1 if wrong == "drop_last_key" and T > 1 else T
        s = qh @ kh[:n].T * scale
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[sl] = (p / p.sum(axis=1, keepdims=True)) @ vh[:n]
    return out, vmax


def tile_rule(qh, kh):
    """The kernel's reference-point rule for one head in fp64: qh, kh [T, 64] (already rounded).  Walks the keys in tiles of KV_TILE; a
    query's reference point m moves to the tile's maximum raw score when (tile max - m) * scale * log2(e) > LAZY_LOG2.  Returns a dict of
    [T, n_tiles] arrays: moved (bool), log2p (the largest log2 p of the tile against the reference point in force for it) and margin
    (|(tile max - m) * c - LAZY_LOG2| of the decision: how far the fp32 kernel is from deciding otherwise), and raw (the score matrix)."""
    tile, lazy = kernel_constants()
    c = SCALE * np.log2(np.e)
    T = qh.shape[0]
    s = qh @ kh.T
    nt = (T + tile - 1) // tile
    m = np.full(T, -np.inf)
    moved, log2p, margin = np.zeros((T, nt), bool), np.zeros((T, nt)), np.zeros((T, nt))
    for j in range(nt):
        smax = s[:, j * tile:(j + 1) * tile].max(axis=1)
        with np.errstate(invalid="ignore"):
            excess = (smax - m) * c
        grow = excess > lazy
        margin[:, j] = np.abs(excess - lazy)
        m = np.where(grow, smax, m)
        moved[:, j] = grow
        log2p[:, j] = (smax - m) * c
    return dict(moved=moved, log2p=log2p, margin=margin, raw=s)


def _tiled(qh, kh, vh, rescale_o=True):
    """The online softmax walked tile by tile under tile_rule's reference points; rescale_o=False is the wrong kernel that forgets to
    rescale O (but not l) when the reference point moves.  With rescale_o=True it equals the plain softmax (asserted by the CPU test)."""
    tile, lazy = kernel_constants()
    c = SCALE * np.log2(np.e)
    T = qh.shape[0]
    s = qh @ kh.T
    m, l, o = np.full(T, -np.inf), np.zeros(T), np.zeros((T, 64))
    for j in range((T + tile - 1) // tile):
        st = s[:, j * tile:(j + 1) * tile]
        smax = st.max(axis=1)
        with np.errstate(invalid="ignore"):
            grow = (smax - m) * c > lazy
        m_new = np.where(grow, smax, m)
        with np.errstate(invalid="ignore"):
            alpha = np.where(np.isinf(m), 0.0, np.exp2((m - m_new) * c))
        m = m_new
        l = l * alpha
        if rescale_o:
            o = o * alpha[:, None]
        p = np.exp2((st - m[:, None]) * c)
        l = l + p.sum(axis=1)
        o = o + p @ vh[j * tile:(j + 1) * tile]
    return o / l[:, None]


def ulp16(mag, kind):
    """The spacing of `kind` at magnitude mag (f16 subnormals share the ulp of 2^-14; bf16 has fp32's exponent range)."""
    floor = 2.0 ** -14 if kind == "f16" else 2.0 ** -126
    return 2.0 ** (np.floor(np.log2(np.maximum(mag, floor))) - KINDS[kind][1])


def attention_bound(ref, vmax, kind, B, T, H):
    """Per element: rel * vmax of the element's (b, h), rel = 2^-8 (bf16) | 2^-11 (f16): P is rounded to the 16-bit type before P V, and
    sum_j p_j (1 + d_j) v_j / sum_j p_j with |d_j| <= half an ulp is a convex combination of v moved by at most rel * max|v| (the lazy
    reference point does not matter: the rounding is relative) -- plus 1 ulp of the output type at the largest magnitude the unrounded
    result can then have, |ref| + rel * vmax.
    Not in the bound: the fp32 score sum.  A score is 64 products accumulated in fp32, off by at most 64 * 2^-23 * sum_d |q_d k_d|, which
    moves a normalised weight by about 2 * scale * that; at the spiked cases' largest scores (sum_d |q_d k_d| ~ 300) that is 0.05 (bf16) /
    0.4 (f16) of rel.  The spiked cases pass without it (worst error / bound 0.42), so the bound is not widened by it."""
    rel = KINDS[kind][0]
    term = rel * np.repeat(np.repeat(vmax, 64, axis=1), T, axis=0)         # [B*T, H*64]
    return term + ulp16(np.abs(ref) + term, kind)


# ---- the fused-QKV / head-major store layouts -----------------------------------------------------------------------------------------
def epilogue_ref(x, w, bias, kind, epi, B, T, H, Tpad=0, ldy=None, wrong=None):
    """fp64 x @ w.T + bias of the operands rounded to `kind`, scattered by the formulas in gemm.hip.  Returns (y, vt, y_mask, vt_mask): the
    expected values in the destinations' shapes and boolean masks of the elements the GEMM writes.
      "qkv_vt":    y [M, ldy], y[m][n] for n < 2D;  vt [B, H, 64, Tpad] flat index ((b*H + h)*64 + d)*Tpad + t
      "headmajor": y [B, H, T, 64] flat index ((b*H + h)*T + t)*64 + d; vt None
    wrong: None | "tpad_is_t" (vt rows packed with stride T) | "hd_swapped" (the column read as d*H + h instead of h*64 + d)."""
    full = round16(x, kind) @ round16(w, kind).T + (0.0 if bias is None else np.asarray(bias, np.float64))
    M = B * T
    assert full.shape[0] == M
    D = H * 64

    def heads(cols):                                                       # [M, H*64] -> [B, H, T, 64]
        if wrong == "hd_swapped":
            return cols.reshape(B, T, 64, H).transpose(0, 3, 1, 2)
        return cols.reshape(B, T, H, 64).transpose(0, 2, 1, 3)

    if epi == "headmajor":
        assert full.shape[1] == D
        y = np.ascontiguousarray(heads(full))
        return y, None, np.ones(y.shape, bool), None
    assert full.shape[1] == 3 * D
    ldy = 2 * D if ldy is None else ldy
    y, y_mask = np.zeros((M, ldy)), np.zeros((M, ldy), bool)
    y[:, :2 * D], y_mask[:, :2 * D] = full[:, :2 * D], True
    v = heads(full[:, 2 * D:]).transpose(0, 1, 3, 2)                       # [B, H, 64, T]
    vt, vt_mask = np.zeros(B * H * 64 * Tpad), np.zeros(B * H * 64 * Tpad, bool)
    stride = T if wrong == "tpad_is_t" else Tpad
    idx = (np.arange(B * H * 64)[:, None] * stride + np.arange(T)[None, :]).ravel()
    vt[idx], vt_mask[idx] = v.reshape(-1), True
    return y, vt.reshape(B, H, 64, Tpad), y_mask, vt_mask.reshape(B, H, 64, Tpad)


def epilogue_bound(ref, kind):
    """`got` is the 16-bit rounding of an fp32 value inside the band tests/test_ops_gpu.py holds this GEMM's fp32 output to,
    2e-4 + 1e-4 |ref| (accumulation order only): the band plus half an ulp of the type at the largest magnitude inside the band."""
    band = 2e-4 + 1e-4 * np.abs(ref)
    return band + 0.5 * ulp16(np.abs(ref) + band, kind)
