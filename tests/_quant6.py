"""MLX's affine packing at 6 bits, restated in numpy for the tests (oracle/quant.py restates the 4- and 8-bit rule, where a word holds whole
codes).  A row of K codes is one little-endian bit stream: code k occupies bits [6 k, 6 k + 6) of the row's bytes -- 4 codes in 3 bytes,
`weight` is uint32 [N][K * 6 / 32], codes straddle word boundaries, a group of 64 codes is 12 whole words.  Restated from MLX's kernels;
unpinned against MLX itself.  Written bit by bit, on purpose unlike checkpoint.pack_codes (which packs 4 codes into 24-bit integers)."""
import numpy as np


def pack6(q: np.ndarray) -> np.ndarray:
    """codes [N][K] (0..63, K % 16 == 0) -> uint32 [N][K * 6 / 32]"""
    q = np.asarray(q)
    assert q.ndim == 2 and q.shape[1] % 16 == 0 and q.min() >= 0 and q.max() < 64
    bits = ((q.astype(np.uint8)[:, :, None] >> np.arange(6, dtype=np.uint8)) & 1).reshape(q.shape[0], -1)      # the stream, bit by bit
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4")


def unpack6(w: np.ndarray) -> np.ndarray:
    """uint32 [N][W] -> codes uint8 [N][W * 32 / 6]"""
    w = np.ascontiguousarray(w, "<u4")
    bits = np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").reshape(w.shape[0], -1, 6)
    return (bits << np.arange(6, dtype=np.uint8)).sum(-1).astype(np.uint8)


def dequant6(w: np.ndarray, scales: np.ndarray, biases: np.ndarray, group: int = 64) -> np.ndarray:
    """float64 scale * code + bias per group of `group` inputs"""
    q = unpack6(w).astype(np.float64)
    n, k = q.shape
    s, b = np.asarray(scales, np.float64), np.asarray(biases, np.float64)
    return (q.reshape(n, k // group, group) * s[:, :, None] + b[:, :, None]).reshape(n, k)


def decode_wfrag6(wf: np.ndarray, N: int, K: int) -> np.ndarray:
    """mia_quant_repack(bits = 6)'s code array, by the layout documented at the top of csrc/skinny_quant.hip, back to codes [tiles * 16][K]
    (rows past N repeat the last one): per (tile, 128-input block) 384 words -- the low-nibble plane [lane = 16 c + r][4 words], word st =
    the nibbles of W[16 tile + r][128 blk + 32 st + 8 c .. + 7], K-value 2 i at bits [4 i, 4 i + 4) and 2 i + 1 at [16 + 4 i, ..); then the
    plane of 2-bit high parts [lane][2 words], word g = the lane's K-steps st = 2 g and 2 g + 1, pair slot j = 4 (st & 1) + i: K-value 2 i
    at bits [2 j, 2 j + 2), 2 i + 1 at [16 + 2 j, ..)."""
    tiles, nblk = (N + 15) // 16, K // 128
    wf = np.asarray(wf, np.uint32).reshape(tiles, nblk, 384)
    lo, hi = wf[:, :, :256].reshape(tiles, nblk, 64, 4), wf[:, :, 256:].reshape(tiles, nblk, 64, 2)
    out = np.zeros((tiles * 16, K), np.uint8)
    for c in range(4):
        for st in range(4):
            for i in range(4):
                for odd in (0, 1):
                    k = 32 * st + 8 * c + 2 * i + odd
                    nib = (lo[:, :, 16 * c:16 * c + 16, st] >> np.uint32(4 * i + 16 * odd)) & 15                       # [tiles][nblk][r]
                    top = (hi[:, :, 16 * c:16 * c + 16, st // 2] >> np.uint32(2 * (4 * (st & 1) + i) + 16 * odd)) & 3
                    v = (nib | (top << np.uint32(4))).astype(np.uint8)
                    out.reshape(tiles, 16, nblk, 128)[:, :, :, k] = v.transpose(0, 2, 1)
    return out
