"""Inputs for the encoder-attention tests, shared by tests/test_enc_attn_ref.py (which asserts, without a GPU, that every spiked case has
the structure it claims) and tests/test_enc_attn_gpu.py (which runs them through the kernel).

Spikes are keys k[j] = a * q[i]: their raw score against query i is a |q_i|^2, about 64 a, i.e. 11.5 a in the exponent's log2 units, while
a standard-normal background reaches about 4 units in a tile of 64 keys.  The value rows of spiked keys carry +-VSPIKE in column D0 of
their head, the largest |v| of the head, so that a result that weights them wrongly is wrong by the whole of max|v|.  The constants
below were chosen by running tests/_enc_attn_ref.tile_rule; the CPU test pins what they achieve."""
import functools

import numpy as np

D0 = 5             # the value column the spiked rows mark
VSPIKE = 6.0
HEAD = 1           # spiked cases have H = 2 and put their structure into head 1 (so a wrong head offset cannot hide)

EDGE_T = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 256, 257]
# (B, T, H): every edge length at H = 1 and H = 3, plus two stacks whose grid sizes (nqb * H * B = 18 and 5) are not multiples of 8
EDGES = [(1, T, H) for T in EDGE_T for H in (1, 3)] + [(3, 129, 3), (5, 65, 1)]
STRIDES = dict(B=2, T=100, H=2, ld_qk=2 * 128 + 8, ld_out=128 + 4, Tpad=192)


def random_qkv(B, T, H, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal((B * T, H * 64)).astype(np.float32) for _ in range(3))


def edge_inputs(B, T, H):
    return random_qkv(B, T, H, 100000 * B + 100 * T + H)


class Case:
    def __init__(self, name, T, seed, claim):
        self.name, self.B, self.T, self.H, self.claim = name, 1, T, 2, claim
        self.q, self.k, self.v = random_qkv(1, T, 2, seed)
        self.query = None          # the query the claim is about
        self.keys = []

    def cols(self):
        return slice(HEAD * 64, HEAD * 64 + 64)

    def spike(self, i, j, a, vval):
        """key j := a * query i (head HEAD); v[j][D0] := vval"""
        self.k[j, self.cols()] = a * self.q[i, self.cols()]
        self.v[j, HEAD * 64 + D0] = vval
        self.keys.append(j)

    def spike_to(self, i, j, log2_units, vval):
        """as spike, with a chosen so that the key's score against query i is `log2_units` in the exponent's units"""
        c = 0.125 * np.log2(np.e)
        qi = self.q[i, self.cols()].astype(np.float64)
        self.spike(i, j, log2_units / (c * float(qi @ qi)), vval)


@functools.lru_cache(maxsize=None)
def spiked_cases():
    """name -> Case.  Built once; the arrays are shared and must not be modified."""
    cases = {}

    # (a) query 5's reference point moves in the first tile and then in tiles 1, 2 and 3: each spike is 11.5 units above the one before.
    # The spiked value rows alternate in sign, so forgetting to rescale O when the point moves (which leaves the earlier tiles' P V at
    # full weight) changes column D0 by a multiple of VSPIKE.
    c = Case("three_moves", 321, 7, "reference point moves >= 3 times after the first tile")
    c.query = 5
    for tile, (units, vval) in enumerate([(15.5, VSPIKE), (27.0, VSPIKE), (38.5, -VSPIKE)], start=1):
        c.spike_to(5, 64 * tile + 9 + tile, units, vval)
    cases[c.name] = c

    # (b) query 140 (second query block) meets a key 7.5 units above its first-tile maximum in tile 2: P = 2^7.5 is rounded to 16 bits
    # without the point having moved.  The key index has bits 2 and 3 different, so a V tile fed in the wrong row order shows.
    c = Case("large_p", 257, 11, "log2 p >= 7 in some tile without a move")
    c.query = 140
    first_max = _first_tile_max(c, 140)
    c.spike_to(140, 128 + 4, first_max + 7.5, VSPIKE)
    cases[c.name] = c

    # (c) in the wave of queries 160 .. 191 (block 1, wave 1) only query 167 moves in tile 2; its 31 neighbours stay.
    c = Case("one_lane", 257, 13, "exactly one query of a wave moves in a tile after the first")
    c.query = 167
    c.spike_to(167, 128 + 33, 20.0, VSPIKE)
    cases[c.name] = c

    # (d) query 70's maximum lies in the first tile, 46 units up: every later p is below 2^-24 and an f16 P is zero from tile 1 on.
    c = Case("underflow", 129, 17, "maximum in the first tile, later scores > 24 log2 units below it")
    c.query = 70
    c.spike_to(70, 3, 46.0, VSPIKE)
    cases[c.name] = c

    # (e) query 100 moves in the tail tile (keys 192 .. 199), on the last key
    c = Case("tail_move", 200, 19, "a move in the tail tile")
    c.query = 100
    c.spike_to(100, 199, 20.0, VSPIKE)
    cases[c.name] = c

    # A plateau for the scale check: eight keys of tile 1 score 18 units against query 20 and carry VSPIKE, a ninth scores 4 raw units
    # (0.72 log2 units) more and carries 0.  At the right scale the ninth holds a fifth of the weight; with the scale left out it takes all.
    c = Case("plateau", 129, 23, "eight equal maxima and a ninth just above")
    c.query = 20
    for n in range(8):
        c.spike_to(20, 64 + 2 + 5 * n, 18.0, VSPIKE)
    c.spike_to(20, 64 + 60, 18.0 + 4.0 * 0.125 * np.log2(np.e), 0.0)
    cases[c.name] = c
    return cases


def _first_tile_max(case, i):
    from _enc_attn_ref import round16
    c = 0.125 * np.log2(np.e)
    qi = round16(case.q[i, case.cols()], "bf16")
    k0 = round16(case.k[:64, case.cols()], "bf16")
    return float((k0 @ qi).max() * c)


# ---- GEMM epilogues --------------------------------------------------------------------------------------------------------------------
# (B, T, H, K): the smallest legal shape; M = 300 with clips that straddle both tile heights; odd H, where a 256-wide tile straddles the
# k | V boundary (2D = 384); q | k | V of one head inside a single 256-wide tile column
QKV_SHAPES = [(1, 4, 1, 64), (3, 100, 2, 128), (2, 132, 3, 192), (1, 260, 1, 128)]
HEADMAJOR_SHAPES = [(2, 100, 2, 128), (1, 5, 1, 64)]
VARIANTS = [0, 1, 2, 4, 3]          # 3 = auto
SENTINEL = 0x7FC1                   # a NaN in both 16-bit types that no arithmetic produces (quiet NaNs come out as 0x7FC0 / 0x7E00)


@functools.lru_cache(maxsize=None)
def gemm_inputs(M, N, K):
    """x [M, K], w [N, K] / sqrt(K), bias [N] that varies along n (a ramp plus noise: a bias indexed along the wrong axis shows)."""
    rng = np.random.default_rng(1000 * M + N + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    bias = (np.linspace(-2.0, 2.0, N) + 0.1 * rng.standard_normal(N)).astype(np.float32)
    return x, w, bias
