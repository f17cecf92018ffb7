"""The cases of tests/test_f32_ops_gpu.py, shared with tests/test_f32_ops_ref.py, which proves on the CPU that every family's comparison
can fail (a deliberately wrong reference leaves the case's own tolerance by more than 100 x).

A tap-GEMM case is the keyword arguments of mia_conv_gemm_desc with numpy arrays for the pointers (two-dimensional X / Y / R / R2 carry
their row strides in their shapes); op = "conv1d" runs it through mia_op_conv1d_f32 instead of the hook."""
from __future__ import annotations

import functools
import os
import re
import zlib
from typing import NamedTuple

import numpy as np

import _f32_ops_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = np.float32(-7777.25)
BIG = np.float32(1e30)            # fills padding columns nothing may read
GARBAGE = 1e4                     # scale of the finite garbage in rows past a sequence's length


class Case(NamedTuple):
    id: str
    op: str                 # "conv1d" | "hook"
    d: dict
    phases: int = 1
    wrongs: tuple = ()      # mutations that must be visible in this case: "pad" | "tap" | "seq" | "phase" | "order"
    y_shift: int = 0        # the op gets Y + y_shift rows (HiFT's row_shift)
    singles: tuple = ()     # stacked cases: (u, single-call dict, phases, first row in the stacked Y, rows) per comparable sequence
    expect: str = ""        # tile instantiation the case must select


def rng_of(cid: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(cid.encode()))


def f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32)


def x_buf(rng, rows: int, Cin: int, ldx: int, scale: float = 1.0) -> np.ndarray:
    x = np.full((rows, ldx), BIG, np.float32)
    x[:, :Cin] = rng.standard_normal((rows, Cin)) * scale
    return x


def y_buf(rows: int, ldy: int) -> np.ndarray:
    return np.full((rows, ldy), SENTINEL, np.float32)


def weights(rng, N: int, K: int, scale: float = 1.0) -> np.ndarray:
    return f32(rng.standard_normal((N, K)) * (scale / np.sqrt(K)))


# ---- which kernel instantiation a launch selects: codec_conv_gemm_launch restated, its three constants read from the source -----------
@functools.lru_cache(None)
def launch_constants() -> tuple:
    src = open(os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "codec_kernels.hip")).read()
    body = src[src.index("int codec_conv_gemm_launch("):]
    body = body[:body.index("\n}\n")]
    big = re.search(r"if \(big_blocks < (\d+)\)", body)
    small = re.search(r"grid\.x \* grid\.y \* grid\.z <= (\d+) && g\.taps \* g\.Cin >= (\d+)\) hipLaunchKernelGGL\(\(conv_gemm_f32<1, 1, 4>\)", body)
    wide = re.search(r"else if \(g\.N > (\d+)\)", body)
    assert big and small and wide, "codec_conv_gemm_launch no longer reads as the tests restate it"
    for inst in ("<1, 1, 1>", "<2, 2, 1>", "<2, 1, 1>"):
        assert f"conv_gemm_f32{inst}" in body, inst
    return int(big.group(1)), int(small.group(1)), int(small.group(2)), int(wide.group(1))


def instantiation(M: int, N: int, K: int, phases: int = 1) -> str:
    big_min, wg_max, k_min, n_wide = launch_constants()
    cdiv = lambda a, b: (a + b - 1) // b
    if cdiv(M, 128) * cdiv(N, 128) * phases < big_min:
        return "<1,1,4>" if cdiv(M, 64) * cdiv(N, 64) * phases <= wg_max and K >= k_min else "<1,1,1>"
    return "<2,2,1>" if N > n_wide else "<2,1,1>"


# ---- plain op: every tile instantiation with M, N and K tails -------------------------------------------------------------------
def _plain(cid, M, N, Cin, taps, *, stride=1, dil=1, pad=None, T_in=None, act=0, bias=True, res=True, wscale=1.0, expect="", wrongs=("pad", "tap")):
    rng = rng_of(cid)
    pad = (taps // 2) * dil if pad is None else pad
    T_in = M * stride if T_in is None else T_in
    d = dict(X=x_buf(rng, T_in, Cin, Cin + 4), T_in=T_in, W=weights(rng, N, taps * Cin, wscale), Y=y_buf(M + 2, N + 3), T_out=M, M=M, N=N, Cin=Cin,
             taps=taps, dil=dil, pad=pad, x_row_mul=stride, act=act)
    if bias:
        d["bias"] = f32(rng.standard_normal(N))
    if res:
        d["R"] = f32(rng.standard_normal(d["Y"].shape))
    if taps == 1:
        wrongs = tuple(w for w in wrongs if w != "tap")
    return Case(cid, "conv1d", d, 1, wrongs, expect=expect)


def tile_cases():
    return [
        # <1,1,4>: 2 x 1 = 2 workgroups of 64 x 64 (1 big block < 384), K >= 256; stages are 128 wide
        _plain("tile-114-k288-c32", 65, 33, 32, 9, expect="<1,1,4>"),     # K = 288: two full stages, the third holds one chunk and three past K
        _plain("tile-114-k288-c96", 65, 33, 96, 3, expect="<1,1,4>"),     # the first stage ends 32 channels into tap 1, the second 64 into tap 2
        _plain("tile-114-k320-c160", 65, 33, 160, 2, expect="<1,1,4>"),   # K = 320: every stage crosses the tap boundary at 160 differently
        # <1,1,1> because K = 224 < 256 (2 workgroups)
        _plain("tile-111-k224", 65, 33, 32, 7, expect="<1,1,1>"),
        # <1,1,1> because 22 x 15 = 330 workgroups > 320 (11 x 8 = 88 big blocks < 384), K = 288; and its N = 1 mod 32 neighbour, 22 x 16 = 352
        _plain("tile-111-wg330", 1345, 960, 96, 3, expect="<1,1,1>"),
        _plain("tile-111-wg352", 1345, 961, 96, 3, expect="<1,1,1>"),
        # <2,2,1>: 192 x 2 = 384 big blocks, N = 129 > 64
        _plain("tile-221", 24449, 129, 32, 3, expect="<2,2,1>"),
        # <2,1,1>: 384 x 1 = 384 big blocks, N = 33 <= 64
        _plain("tile-211", 49025, 33, 32, 3, expect="<2,1,1>"),
        # the degenerate corner
        _plain("tile-1x1", 1, 1, 32, 1, expect="<1,1,1>"),
    ]


# ---- geometry: stride x dilation x where the window meets the ends of X ----------------------------------------------------------------
def geometry_cases():
    out = []
    M, N, taps = 70, 33, 3
    for stride in (1, 2, 3):
        for dil in (1, 3, 9):
            Cin = 32 if (stride + dil) % 2 == 0 else 64
            last = (M - 1) * stride + (taps - 1) * dil - dil          # row the last output's last tap reads with pad = dil
            for name, pad, T_in in (("last-in", dil, last + 1),       # ... is exactly T_in - 1 (the first rows read before row 0)
                                    ("last-at", dil, last),           # ... is T_in itself
                                    ("last-past", dil, last - 2),     # ... and its neighbours lie past T_in
                                    ("zero-row", taps * dil, M * stride)):   # pad >= taps * dil: output row 0 sees only zeros
                out.append(_plain(f"geom-s{stride}-d{dil}-{name}", M, N, Cin, taps, stride=stride, dil=dil, pad=pad, T_in=T_in))
    return out


# ---- activations -----------------------------------------------------------------------------------------------------------------
def activation_cases():
    # |pre-activation| reaches ~10 on both sides: unit inputs, weights of variance 3.5^2 / K
    return [_plain(f"act{act}-{'br' if br else 'plain'}", 70, 33, 32, 3, act=act, bias=br, res=br, wscale=3.5) for act in range(7) for br in (False, True)]


# ---- hook: transposed convolutions as output phases ------------------------------------------------------------------------------------
def snac_phase_weights(wm: np.ndarray, s: int) -> np.ndarray:
    """codec_load.hip convt_phases: kernel 2 s, MLX weight wm [Cout][K][Cin] -> [phase r][Cout][2][Cin], tap 0 (x[t-1]) = k r + s, tap 1 (x[t]) = k r."""
    Cout, K, Cin = wm.shape
    assert K == 2 * s
    ph = np.zeros((s, Cout, 2, Cin), np.float32)
    for r in range(s):
        ph[r, :, 0] = wm[:, r + s]
        ph[r, :, 1] = wm[:, r]
    return ph


def hift_phase_weights(wm: np.ndarray, s: int) -> np.ndarray:
    """hift.hip Loader::convt: nt = ceil(K / s) taps, tap q of phase r = kernel index r + (nt - 1 - q) s, zero beyond K."""
    Cout, K, Cin = wm.shape
    nt = (K + s - 1) // s
    ph = np.zeros((s, Cout, nt, Cin), np.float32)
    for r in range(s):
        for q in range(nt):
            k = r + (nt - 1 - q) * s
            if k < K:
                ph[r, :, q] = wm[:, k]
    return ph


def snac_convt_desc(x, wm, bias, s: int, T: int, T_rows_y=None) -> tuple[dict, int]:
    """codec.hip OP_CONVT: M = T + 1 two-row windows (pad 1), output row m s + r - p of phase r, p = ceil(s / 2)."""
    N, K, Cin = wm.shape
    p = (s + 1) // 2
    T_out = (T - 1) * s - 2 * p + 2 * s
    d = dict(X=x, T_in=T, W=snac_phase_weights(wm, s), w_phase_stride=N * 2 * Cin, bias=bias, M=T + 1, N=N, Cin=Cin, taps=2, dil=1, pad=1,
             Y=y_buf((T_out if T_rows_y is None else T_rows_y) + 2, N + 3), T_out=T_out, y_row_mul=s, y_row_off=-p, y_phase_step=1)
    return d, T_out


def hift_convt_desc(x, wm, bias, s: int, T: int, row_shift: int) -> tuple[dict, int]:
    """hift.hip run_convt: M = T + nt - 1 windows of nt rows (pad nt - 1), output row m s + r - p, p = (K - s) / 2; with row_shift the op
    writes T s - row_shift rows from row row_shift of the buffer on."""
    N, K, Cin = wm.shape
    nt = (K + s - 1) // s
    T_out = T * s - row_shift
    d = dict(X=x, T_in=T, W=hift_phase_weights(wm, s), w_phase_stride=N * nt * Cin, bias=bias, M=T + nt - 1, N=N, Cin=Cin, taps=nt, dil=1, pad=nt - 1,
             Y=y_buf(row_shift + T_out + 2, N + 3), T_out=T_out, y_row_mul=s, y_row_off=-(K - s) // 2, y_phase_step=1)
    return d, T_out


def rowmap_cases():
    out = []
    for s in (2, 4, 8):
        for T in (1, 2, 37):
            Cin, N = (64 if s == 4 else 32), (64 if T == 2 else 33)
            cid = f"convt-snac-s{s}-T{T}"
            rng = rng_of(cid)
            d, _ = snac_convt_desc(x_buf(rng, T, Cin, Cin + 4), f32(rng.standard_normal((N, 2 * s, Cin)) / np.sqrt(2 * Cin)), f32(rng.standard_normal(N)), s, T)
            out.append(Case(cid, "hook", d, s, ("phase", "tap", "pad")))
    for s, K in ((2, 6), (4, 10), (8, 16), (5, 11), (3, 7)):        # the last three are HiFT's own (kernel, stride) pairs
        for T in (1, 2, 37):
            Cin, N = (64 if s == 4 else 32), (64 if T == 2 else 33)
            shift = 1 if T == 37 else 0
            cid = f"convt-hift-s{s}-k{K}-T{T}"
            rng = rng_of(cid)
            d, _ = hift_convt_desc(x_buf(rng, T, Cin, Cin + 4), f32(rng.standard_normal((N, K, Cin)) / np.sqrt(K * Cin / s)), f32(rng.standard_normal(N)), s, T, shift)
            # (a single input row sits in the middle tap of its window: dropping the last tap cannot show at T = 1)
            out.append(Case(cid, "hook", d, s, ("phase", "pad") + (("tap",) if T > 1 else ()), y_shift=shift))
    return out


# ---- hook: prologues and epilogues ---------------------------------------------------------------------------------------------------
def epilogue_cases():
    M, N, Cin, taps = 70, 33, 64, 3

    def base(cid, xscale=1.0):
        rng = rng_of(cid)
        return rng, dict(X=x_buf(rng, M, Cin, Cin + 4, xscale), T_in=M, W=weights(rng, N, taps * Cin), Y=y_buf(M + 2, N + 3), T_out=M, M=M, N=N, Cin=Cin,
                         taps=taps, dil=1, pad=1, bias=f32(rng.standard_normal(N)))
    out = []
    alpha = f32(np.exp(np.linspace(np.log(0.05), np.log(20.0), Cin)))       # |alpha x| reaches a few hundred at |x| ~ 20
    rng, d = base("snake-default", 5.0)
    d["alpha"] = alpha
    out.append(Case("snake-default", "hook", d, 1, ("pad", "tap")))
    rng, d = base("snake-ralpha", 5.0)
    d["alpha"] = alpha
    d["ralpha"] = f32(rng.uniform(0.5, 2.0, Cin) / alpha)
    out.append(Case("snake-ralpha", "hook", d, 1, ("pad", "tap")))
    rng, d = base("lrelu")
    d["lrelu_slope"] = 0.1
    out.append(Case("lrelu", "hook", d, 1, ("pad", "tap")))
    rng, d = base("noise")
    d["R"] = f32(rng.standard_normal(d["Y"].shape))
    d["noise"] = f32(rng.standard_normal(M))
    out.append(Case("noise", "hook", d, 1, ("pad", "tap")))
    rng, d = base("scale-r-r2")
    d["R"] = f32(rng.standard_normal(d["Y"].shape))
    d["R2"] = f32(rng.standard_normal(d["Y"].shape))
    d["out_scale"] = 1.0 / 3.0
    out.append(Case("scale-r-r2", "hook", d, 1, ("pad", "tap", "order")))
    rng, d = base("tanh")
    d["tanh_out"] = 1
    out.append(Case("tanh", "hook", d, 1, ("pad", "tap")))
    rng, d = base("ldw")
    w = np.full((N, taps * Cin + 8), BIG, np.float32)
    w[:, :taps * Cin] = d["W"]
    d["W"], d["ldw"] = w, taps * Cin + 8
    out.append(Case("ldw", "hook", d, 1, ("pad", "tap")))
    rng, d = base("all-together", 5.0)
    d["alpha"] = alpha
    d["act"] = 2
    d["R"] = f32(rng.standard_normal(d["Y"].shape))
    d["R2"] = f32(rng.standard_normal(d["Y"].shape))
    d["out_scale"] = -0.5
    d["tanh_out"] = 1
    d["W"] = d["W"] * np.float32(0.25)            # keeps tanh away from saturation
    out.append(Case("all-together", "hook", d, 1, ("pad", "tap", "order")))
    return out


# ---- hook: stacked sequences -----------------------------------------------------------------------------------------------------------
def stacked_cases():
    T, N, Cin = 70, 33, 32
    lens = [T, 1, T - 5]
    out = []

    def stack_x(rng, xs):
        x = f32(rng.standard_normal((3 * xs, Cin + 4)) * GARBAGE)       # everything past a sequence's length is finite garbage
        x[:, Cin:] = BIG
        for u, L in enumerate(lens):
            x[u * xs:u * xs + L, :Cin] = rng.standard_normal((L, Cin))
        return x

    def one(d, u, xs, **kw):
        s = {k: v for k, v in d.items() if k not in ("n_seq", "x_seq_step", "y_seq_step", "seq_len", "noise_seq_off", "phase_len", "x_phase_step")}
        L = lens[u]
        s["X"] = np.ascontiguousarray(d["X"][u * xs:u * xs + L])
        s["T_in"] = L
        s.update(kw)
        s["Y"] = y_buf(s["T_out"] + 2, N + 3)
        return s

    # plain (taps 3, pad 1) and strided (stride 2) convolutions
    for name, stride in (("plain", 1), ("strided", 2)):
        cid = f"stack-{name}"
        rng = rng_of(cid)
        xs = T + 3
        rows = lambda L: (L + 2 - 3) // stride + 1
        ys = rows(T) + 2
        d = dict(X=stack_x(rng, xs), T_in=T, W=weights(rng, N, 3 * Cin), bias=f32(rng.standard_normal(N)), Y=y_buf(3 * ys, N + 3), T_out=rows(T), M=rows(T),
                 N=N, Cin=Cin, taps=3, dil=1, pad=1, x_row_mul=stride, n_seq=3, x_seq_step=xs, y_seq_step=ys, seq_len=np.asarray(lens, np.int32))
        singles = tuple((u, one(d, u, xs, T_out=rows(lens[u]), M=rows(lens[u])), 1, u * ys, rows(lens[u])) for u in range(3))
        out.append(Case(cid, "hook", d, 1, ("seq", "pad"), singles=singles))
    # transposed (SNAC form, stride 4)
    cid = "stack-convt"
    rng = rng_of(cid)
    s, xs = 4, T + 3
    wm, b = f32(rng.standard_normal((N, 2 * s, Cin)) / np.sqrt(2 * Cin)), f32(rng.standard_normal(N))
    d, T_out = snac_convt_desc(stack_x(rng, xs), wm, b, s, T)
    ys = T_out + 2
    d.update(Y=y_buf(3 * ys, N + 3), n_seq=3, x_seq_step=xs, y_seq_step=ys, seq_len=np.asarray(lens, np.int32))
    singles = []
    for u in range(3):
        du, Tu = snac_convt_desc(np.ascontiguousarray(d["X"][u * xs:u * xs + lens[u]]), wm, b, s, lens[u])
        singles.append((u, du, s, u * ys, Tu))
    out.append(Case(cid, "hook", d, s, ("seq", "phase"), singles=tuple(singles)))
    # noise form: Y = R + noise[noise_seq_off[u] + row] * (x W^T + bias), rows at or past seq_len[u] are not written
    cid = "stack-noise"
    rng = rng_of(cid)
    xs = ys = T + 2
    noise_off = np.asarray([5, 5 + T + 3, 5 + 2 * (T + 3)], np.int32)
    d = dict(X=stack_x(rng, xs), T_in=T, W=weights(rng, N, Cin), bias=f32(rng.standard_normal(N)), Y=y_buf(3 * ys, N + 3), T_out=T, M=T, N=N, Cin=Cin, taps=1,
             R=f32(rng.standard_normal((3 * ys, N + 3))), noise=f32(rng.standard_normal(5 + 3 * (T + 3))), n_seq=3, x_seq_step=xs, y_seq_step=ys,
             seq_len=np.asarray(lens, np.int32), noise_seq_off=noise_off)
    singles = tuple((u, one(d, u, xs, T_out=lens[u], M=lens[u], R=np.ascontiguousarray(d["R"][u * ys:u * ys + lens[u] + 2]),
                            noise=np.ascontiguousarray(d["noise"][noise_off[u]:noise_off[u] + lens[u]])), 1, u * ys, lens[u]) for u in range(3))
    out.append(Case(cid, "hook", d, 1, ("seq",), singles=singles))
    # the batched flow's form: grid phase = sequence (x_phase_step), phase_len under a window that looks one row ahead
    cid = "stack-phase-len"
    rng = rng_of(cid)
    x = stack_x(rng, T)
    d = dict(X=x, T_in=T, W=weights(rng, N, 3 * Cin), bias=f32(rng.standard_normal(N)), Y=y_buf(3 * T + 2, N + 3), T_out=3 * T, M=T, N=N, Cin=Cin, taps=3, pad=1,
             x_phase_step=T, y_phase_step=T, phase_len=np.asarray(lens, np.int32), act=4)
    singles = tuple((u, one(d, u, T, T_out=lens[u], M=lens[u], y_phase_step=0), 1, u * T, lens[u]) for u in range(3))
    out.append(Case(cid, "hook", d, 3, ("seq", "pad"), singles=singles))
    return out


FAMILIES = {"tiles": tile_cases, "geometry": geometry_cases, "activations": activation_cases, "rowmap": rowmap_cases, "epilogue": epilogue_cases,
            "stacked": stacked_cases}


@functools.lru_cache(None)
def family(name: str) -> tuple:
    return tuple(FAMILIES[name]())


def case_ids(name: str) -> list:
    return [c.id for c in family(name)]


@functools.lru_cache(None)
def case(name: str, cid: str) -> Case:
    return next(c for c in family(name) if c.id == cid)


def ref_args(c: Case, d=None) -> dict:
    """The reference's view of a case: Y (and R / R2) from the shifted row on, the prologue's allowance measured over the case's own X."""
    d = dict(c.d if d is None else d)
    if c.y_shift:
        d["Y"] = d["Y"][c.y_shift:]
    if d.get("alpha") is not None:
        d["allow_pre"] = ref.snake_allowance(d["X"][:, :d["Cin"]], d["alpha"], d.get("ralpha"))
    elif d.get("lrelu_slope", 0.0) > 0:
        d["allow_pre"] = ref.lrelu_allowance(d["X"][:, :d["Cin"]], d["lrelu_slope"])
    return d


def _embed(c: Case, r: ref.TapGemm) -> ref.TapGemm:
    if not c.y_shift:
        return r
    full = lambda a, fill, dt: np.concatenate([np.full((c.y_shift, a.shape[1]), fill, dt), a])
    return ref.TapGemm(full(r.Y, float(SENTINEL), np.float64), full(r.written, False, bool), full(r.tol, 0.0, np.float64), full(r.pre, 0.0, np.float64))


@functools.lru_cache(None)
def reference(name: str, cid: str) -> ref.TapGemm:
    """Computed once per case and shared (treat as read-only)."""
    c = case(name, cid)
    return _embed(c, ref.tap_gemm_ref(c.phases, **ref_args(c)))


def mutate(c: Case, wrong: str) -> ref.TapGemm:
    """The reference of a deliberately wrong kernel."""
    d = ref_args(c)
    kw = {}
    if wrong == "pad":
        d["pad"] = d.get("pad", 0) + 1
    elif wrong == "tap":
        K, Cin = d["taps"] * d["Cin"], d["Cin"]
        w = np.array(d["W"], np.float32).reshape(-1, d.get("ldw") or K)
        w[:, K - Cin:K] = 0
        d["W"] = w
    elif wrong == "seq":
        for k in ("seq_len", "phase_len"):
            if d.get(k) is not None:
                d[k] = np.full_like(d[k], d["T_in"])
    elif wrong == "phase":
        d["y_row_off"] = d.get("y_row_off", 0) + 1
    elif wrong == "order":
        kw["wrong"] = "order"
    else:
        raise ValueError(wrong)
    return _embed(c, ref.tap_gemm_ref(c.phases, **d, **kw))


# ---- attention ---------------------------------------------------------------------------------------------------------------------
class AttnCase(NamedTuple):
    id: str
    B: int
    T: int
    H: int
    qkv: np.ndarray         # fused [B*T][3*H*64]
    scale: float = 0.125
    p: np.ndarray | None = None
    bias_u: np.ndarray | None = None
    bias_v: np.ndarray | None = None
    seq_len: np.ndarray | None = None
    chunk: int = 0
    wrongs: tuple = ()
    one_hot: np.ndarray | None = None     # [B*T] winning key per query, where one key takes all the mass

    def parts(self):
        D = self.H * 64
        return self.qkv[:, :D], self.qkv[:, D:2 * D], self.qkv[:, 2 * D:]

    def valid_rows(self) -> np.ndarray:
        t = np.arange(self.B * self.T) % self.T
        return np.ones(self.B * self.T, bool) if self.seq_len is None else t < np.repeat(np.asarray(self.seq_len), self.T)


ATTN_T = (1, 31, 32, 33, 96, 97, 127, 128, 129, 300)


def _qkv(rng, B, T, H, seq_len=None):
    a = f32(rng.standard_normal((B * T, 3 * H * 64)))
    if seq_len is not None:
        for b, L in enumerate(seq_len):
            a[b * T + L:(b + 1) * T] = rng.standard_normal(((T - L), 3 * H * 64)) * GARBAGE
    return a


def attn_plain_cases():
    out = []
    for T in ATTN_T:
        for B, H in ((1, 1), (2, 3)):
            cid = f"attn-T{T}-B{B}H{H}"
            out.append(AttnCase(cid, B, T, H, _qkv(rng_of(cid), B, T, H), wrongs=("last_key",) if T > 1 else ()))
    # logits of +-200: query i is 25 x the key it is meant to find; every odd key is the negative of the even key before it, so the
    # winner's logit is 25 |k|^2 / 8 ~ +200, its partner's ~ -200 and all others within ~ +-90: one key takes all the mass
    cid, B, T, H = "attn-onehot", 2, 129, 3
    rng = rng_of(cid)
    a = _qkv(rng, B, T, H)
    D = H * 64
    k = a[:, D:2 * D]
    for b in range(B):
        k[b * T + 1:b * T + T:2] = -k[b * T:b * T + T - 1:2]
    win = np.array([(T - 1 - 7 * i) % T for i in range(T)] * B)
    for b in range(B):
        a[b * T:(b + 1) * T, :D] = 25.0 * k[b * T + win[b * T:(b + 1) * T]]
    out.append(AttnCase(cid, B, T, H, a, wrongs=("last_key",), one_hot=win))
    return out


def attn_ex_cases():
    out = []
    for T in (33, 129):
        cid, B, H = f"attn-pos-T{T}", 2, 3
        rng = rng_of(cid)
        out.append(AttnCase(cid, B, T, H, _qkv(rng, B, T, H), p=f32(rng.standard_normal((T, H * 64))), bias_u=f32(rng.standard_normal((H, 64)) * 0.5),
                            bias_v=f32(rng.standard_normal((H, 64)) * 0.5), wrongs=("bias", "last_key")))
    for chunk in (1, 7, 32, 50):
        cid = f"attn-chunk{chunk}"
        out.append(AttnCase(cid, 2, 129, 3, _qkv(rng_of(cid), 2, 129, 3), chunk=chunk, wrongs=("chunk",)))
    lens = np.asarray([129, 1, 40], np.int32)
    out.append(AttnCase("attn-seqlen", 3, 129, 2, _qkv(rng_of("attn-seqlen"), 3, 129, 2, lens), seq_len=lens, wrongs=("last_key",)))
    out.append(AttnCase("attn-seqlen-chunk32", 3, 129, 2, _qkv(rng_of("attn-seqlen-chunk32"), 3, 129, 2, lens), seq_len=lens, chunk=32, wrongs=("chunk", "last_key")))
    return out


ATTN_FAMILIES = {"attn-plain": attn_plain_cases, "attn-ex": attn_ex_cases}


@functools.lru_cache(None)
def attn_family(name: str) -> tuple:
    return tuple(ATTN_FAMILIES[name]())


def attn_ids(name: str) -> list:
    return [c.id for c in attn_family(name)]


def attn_case(name: str, cid: str) -> AttnCase:
    return next(c for c in attn_family(name) if c.id == cid)


def attn_eval(c: AttnCase, dtype=np.float64, wrong=None, b=None) -> np.ndarray:
    """The reference (float64), the naive float32 evaluation, or a wrong variant; b: that sequence alone, as its own B = 1, T = seq_len[b] call."""
    q, k, v = c.parts()
    if b is not None:
        L = int(c.seq_len[b])
        rows = slice(b * c.T, b * c.T + L)
        return ref.attention_ref(q[rows], k[rows], v[rows], c.scale, None if c.p is None else c.p[:L], c.bias_u, c.bias_v, None, c.chunk, B=1, T=L, H=c.H,
                                 dtype=dtype, wrong=wrong)
    return ref.attention_ref(q, k, v, c.scale, c.p, c.bias_u, c.bias_v, c.seq_len, c.chunk, B=c.B, T=c.T, H=c.H, dtype=dtype, wrong=wrong)


@functools.lru_cache(None)
def attn_reference(name: str, cid: str) -> tuple:
    """(float64 reference, tolerance): 8 x the naive float32 evaluation's largest error over the rows that mean something, plus the
    rounding of the output itself."""
    c = attn_case(name, cid)
    r64 = attn_eval(c)
    valid = c.valid_rows()
    return r64, ref.attention_tol(r64, attn_eval(c, np.float32), valid) + ref.EPS32 * float(np.abs(r64[valid]).max())
