"""Cases of the skinny-GEMM parity tests (tests/test_skinny_gpu.py), the plain-Python restatement of the two launchers' dispatch rules
(csrc/skinny_rowmajor.hip: skinny_flat_try / skinny_launch_t; csrc/skinny_quant.hip: skinny_qi_launch_m / _t -- change them together
with this file), and the operands of a case: random real values for the bounded comparison, small integers for the exact one."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field, replace

import numpy as np

import _skinny_ref as ref
from _skinny_ref import SK_OUTF32, SK_PARTIAL, SK_RESID, SK_SWIGLU
from mlx_swift_audio_amd import _lib
from mlx_swift_audio_amd import audio as _audio
from mlx_swift_audio_amd import checkpoint

ALL_M = (1, 4, 15, 16, 17, 31, 32, 33, 40)
FEW_M = (1, 17)
MODE_NAME = {SK_OUTF32: "outf32", SK_PARTIAL: "partial", SK_SWIGLU: "swiglu", SK_RESID: "resid"}


# ---- the dispatch rules, restated ----------------------------------------------------------------------------------------------------
def dispatch16(M: int, N: int, K: int, S: int, mode: int) -> dict:
    """skinny_gemm_launch: kernel, waves, whole register batches per wave (nb), how the leftover K-steps are taken, ring refills"""
    tiles, per = (N + 15) // 16, K // S
    few = tiles * S <= 1024 and K % (128 * S) == 0 and per >= 512          # per 32-row block: M does not enter
    if mode in (SK_PARTIAL, SK_SWIGLU) and few:
        for n in (10, 5, 8, 6, 4):
            if per == 128 * n:
                return dict(kernel=f"flat{n}", NW=4, nb=0, tail="none", wraps=0)
    if mode == SK_OUTF32:
        NT, KB, NW = 4, 2, 1
    elif mode == SK_RESID and K % 1024 == 0 and K >= 8192:
        NT, KB, NW = 1, 2, 16
    elif mode == SK_RESID and K % 256 == 0 and K >= 2048:
        NT, KB, NW = 1, 2, 8
    else:
        NT, KB, NW = (1, 2, 4) if few else (1, 4, 1)
    Kc = K // (S * NW)
    nb = Kc // (32 * KB)
    rem = (Kc - nb * 32 * KB) // 32
    return dict(kernel=f"ring<{NT},{KB},{NW}>", NW=NW, nb=nb, tail="none" if rem == 0 else ("early" if nb <= 3 else "loop"), wraps=max(0, (nb - 1) // 4))


def dispatch_q(M: int, N: int, K: int, S: int, mode: int, bits: int, M_cap: int = 0) -> dict:
    """skinny_gemm_q_launch: tiles per wave, waves, 128-input blocks per wave (bc), the 16-row variant, nibble planes"""
    tiles, per = (N + 15) // 16, K // 128 // S
    Mf = max(M, M_cap)
    zf = (Mf + 31) // 32
    nt4 = tiles * S * zf >= 16384 or (Mf > 16 and ((tiles + 3) // 4) * S * zf >= 192)
    nw = 1
    for cand in (4, 3, 2):
        if per % cand == 0 and (per // cand >= 2 or cand == 2):
            nw = cand
            break
    head41 = mode == SK_OUTF32 and tiles >= 4096 and Mf <= 16
    if mode == SK_RESID and not nt4 and per % 16 == 0 and per >= 64:
        NT, NW = 1, 16
    elif mode == SK_RESID and not nt4 and per % 8 == 0:
        NT, NW = 1, 8
    elif head41:
        NT, NW = 4, 1
    elif nt4:
        NT, NW = (4, 4) if per % 4 == 0 else (4, 1)
    else:
        NT, NW = 1, nw
    return dict(NT=NT, NW=NW, bc=per // NW, M16=M <= 16, NP=bits // 4, head41=head41, nt4=nt4 and not head41)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    fam: str                   # "h": 16-bit weights, "q": packed
    mode: int
    N: int
    K: int
    S: int = 1
    dtype: int = _lib.BF16
    bits: int = 0
    sdt: str = "f16"           # stored type of the packed scales / biases
    Ms: tuple = FEW_M
    bias: bool = True
    ldo_extra: int = 0         # out row stride = N (N / 2 for SK_SWIGLU) + this
    lda_extra: int = 0         # A row stride = K + this (A is then a view into a larger buffer, two rows and 8 columns in)
    carry: int = 0             # consumer side of the carried norm: ss_tiles (0 = none)
    rs_scale: float = 1.0
    note: str = ""

    def form(self, M: int, M_cap: int = 0) -> dict:
        return dispatch16(M, self.N, self.K, self.S, self.mode) if self.fam == "h" else dispatch_q(M, self.N, self.K, self.S, self.mode, self.bits, M_cap)

    def ksplit(self, M: int, M_cap: int = 0):
        f = self.form(M, M_cap)
        return (f["kernel"], f["NW"]) if self.fam == "h" else (f["NW"], f["bc"])

    @property
    def ncols(self) -> int:
        return self.N // 2 if self.mode == SK_SWIGLU else self.N


def _dt(dtype):
    return "f16" if dtype == _lib.F16 else "bf16"


def _h(mode, N, K, S=1, **kw):
    return [Case(id=f"h-{MODE_NAME[mode]}-N{N}-K{K}-S{S}-{_dt(dt)}" + (f"-{kw['note']}" if kw.get("note") else ""), fam="h", mode=mode, N=N, K=K, S=S, dtype=dt, **kw)
            for dt in (_lib.BF16, _lib.F16)]


def _q(mode, N, K, S=1, bits=(4, 8), dtypes=(_lib.BF16, _lib.F16), full=True, **kw):
    """full: every (bits, dtype) pair given; else, of the four, only (4 bit, bf16) and (8 bit, f16): both code widths, both types"""
    variants = [(b, dt) for b in bits for dt in dtypes]
    if not full and len(variants) == 4:
        variants = [(4, _lib.BF16), (8, _lib.F16)]
    return [Case(id=f"q{b}-{MODE_NAME[mode]}-N{N}-K{K}-S{S}-{_dt(dt)}-s{kw.get('sdt', 'f16')}" + (f"-{kw['note']}" if kw.get("note") else ""), fam="q", mode=mode, N=N, K=K,
                 S=S, dtype=dt, bits=b, **kw) for b, dt in variants]


def _build() -> list[Case]:
    c: list[Case] = []
    # -- 16-bit: SK_OUTF32, ring <4,2,1> (64 columns per wave): no whole batch / early tail after 1 and 3 batches / trailing loop / the ring
    #    wraps once and twice; N tails; odd ldo = scalar stores, even ldo = f32x2 stores
    for K, N, ext, Ms in ((32, 1, 0, FEW_M), (96, 63, 0, FEW_M), (224, 65, 1, ALL_M), (288, 130, 0, FEW_M), (320, 63, 3, FEW_M), (576, 130, 2, FEW_M)):
        c += _h(SK_OUTF32, N, K, ldo_extra=ext, Ms=Ms, lda_extra=8 if K == 224 else 0)
    # -- 16-bit: SK_PARTIAL / SK_SWIGLU: every flat form, the wide ring <1,2,4>, the narrow ring <1,4,1>
    for K, S, N, Ms in ((512, 1, 40, ALL_M), (640, 1, 36, FEW_M), (768, 1, 52, FEW_M), (1024, 1, 20, FEW_M), (1280, 1, 36, FEW_M), (1280, 2, 24, FEW_M),
                        (896, 1, 36, ALL_M), (1152, 1, 20, FEW_M), (1536, 1, 36, FEW_M),
                        (96, 1, 36, FEW_M), (224, 1, 52, ALL_M), (480, 1, 20, FEW_M), (544, 1, 36, FEW_M)):
        c += _h(SK_PARTIAL, N + 2, K, S, Ms=Ms, lda_extra=16 if K == 896 else 0)          # N % 4 != 0: scalar stores
        c += _h(SK_PARTIAL, N, K, S)                                                      # N % 16 != 0, N % 4 == 0: f32x4 stores
        if S == 1:
            c += _h(SK_SWIGLU, N, K, ldo_extra=1 if N % 16 == 4 else 0, Ms=Ms if K in (640, 1152, 480) else FEW_M)
    c += _h(SK_PARTIAL, 16416, 512, note="many-wgs")                                     # > 1024 workgroups: the narrow ring at a flat K
    c += _h(SK_PARTIAL, 9600, 512, Ms=(1, 33), note="rowblocks")                         # 600 tiles: two row blocks must not change the form
    # -- 16-bit: SK_RESID: 16 / 8 / 4 / 1 waves
    for K, N, bias, Ms in ((8192, 16, True, ALL_M), (2048, 48, False, ALL_M), (2304, 16, True, FEW_M), (1024, 48, True, ALL_M), (1152, 16, False, FEW_M),
                           (224, 48, True, ALL_M), (544, 16, False, FEW_M)):
        c += _h(SK_RESID, N, K, bias=bias, Ms=Ms, ldo_extra=4 if K == 2304 else 0)
    # -- packed: blocks per wave 1, 2, 3, 4, 5, 7 on one wave or several; nw = 1, 2, 3, 4 via K / S / 128 = 1, 2, 6, 8
    for K, S, N, Ms in ((128, 1, 40, ALL_M), (256, 1, 36, FEW_M), (384, 1, 52, FEW_M), (640, 1, 36, FEW_M), (896, 1, 40, ALL_M), (768, 1, 36, ALL_M),
                        (1024, 1, 20, ALL_M), (1536, 1, 36, FEW_M), (2048, 1, 20, FEW_M), (1536, 2, 24, FEW_M)):
        c += _q(SK_PARTIAL, N + 1, K, S, Ms=Ms, lda_extra=8 if K == 896 else 0)
        if S == 1:
            c += _q(SK_SWIGLU, N, K, Ms=FEW_M, ldo_extra=1 if N % 16 == 4 else 0, full=K in (128, 896))
            c += _q(SK_OUTF32, N + 1, K, Ms=FEW_M, ldo_extra=K // 128 % 2, full=K in (256, 768))
    c += (_q(SK_PARTIAL, 40, 896, sdt="bf16", full=False) + _q(SK_PARTIAL, 40, 768, sdt="f32", full=False) + _q(SK_OUTF32, 33, 256, sdt="bf16", full=False) +
          _q(SK_SWIGLU, 36, 640, sdt="f32", full=False))
    for K, N, bias, Ms in ((1024, 48, True, ALL_M), (8192, 16, False, ALL_M), (896, 16, True, FEW_M), (512, 48, False, FEW_M)):
        c += _q(SK_RESID, N, K, bias=bias, Ms=Ms)
    # -- packed: four tiles per wave: above 16 rows (one wave / four waves), by workgroup count at <= 16 rows, the one-wave vocabulary head
    c += _q(SK_PARTIAL, 3072, 512, 4, Ms=(1, 16, 17, 40), note="nt4") + _q(SK_PARTIAL, 3072, 2048, 4, Ms=(1, 16, 17, 40), note="nt4")
    c += _q(SK_PARTIAL, 65536, 512, 4, bits=(4,), dtypes=(_lib.BF16,), Ms=(1, 16), note="nt4-by-count")
    c += _q(SK_OUTF32, 65560, 128, Ms=(1, 16, 17), note="head41") + _q(SK_OUTF32, 65560, 512, bits=(4,), Ms=(1, 16, 17), note="head41")
    # Qwen2-0.5B's head K: 7 blocks in the one wave wrap the three-block ring with four tiles in flight (29 MB of codes, the largest case)
    c += _q(SK_OUTF32, 65560, 896, bits=(4,), dtypes=(_lib.BF16,), Ms=(1, 17), note="head41")
    # -- both families: the consumer side of the carried norm
    for t, rs in ((1, 0.125), (64, 0.125), (65, 3.0), (512, 0.125)):
        i = (1, 64, 65, 512).index(t) % 2         # the two 16-bit types alternate over the tile counts
        kw = dict(carry=t, rs_scale=rs, note=f"carry{t}")
        c += _h(SK_PARTIAL, 36, 896, **kw)[i:i + 1] + _h(SK_OUTF32, 65, 224, **kw)[1 - i:2 - i] + _h(SK_SWIGLU, 36, 512, **kw)[i:i + 1]
        c += _q(SK_PARTIAL, 37, 768, full=False, **kw)[i:i + 1] + _q(SK_SWIGLU, 36, 896, full=False, **kw)[1 - i:2 - i] + _q(SK_OUTF32, 33, 256, full=False, **kw)[i:i + 1]
    return c + _model_cases()


# The (N, K, S, mode) tuples of lm_enqueue_step for the four real models, fused-norm chain (capacity <= 4: q|k|v and gate|up and the head
# consume a carried norm, o and down are SK_RESID) and split chain (o and down are SK_PARTIAL).  S as lm_load.hip picks it: the largest
# s <= want with K % (32 s) == 0 (16 bit) or K % (128 s) == 0 (packed), want = 4 (q|k|v, o) or 8 (down).
MODELS = {   # hidden, Nq, Nkv, inter, vocab
    "qwen2-0.5b": (896, 896, 128, 4864, 151936),
    "qwen3-0.6b": (1024, 2048, 1024, 3072, 151936),
    "llama3.2-1b": (2048, 2048, 512, 8192, 128256),
    "orpheus-3b": (3072, 3072, 1024, 8192, 156940),
}
N_CUTS = (80, 1040, 3072, 4112, 12288)


def pick_split(K: int, want: int, unit: int) -> int:
    for s in range(want, 1, -1):
        if K % (unit * s) == 0:
            return s
    return 1


def model_tuples(name: str, fam: str):
    D, Nq, Nkv, inter, V = MODELS[name]
    unit = 32 if fam == "h" else 128
    Sq, So, Sd = pick_split(D, 4, unit), pick_split(Nq, 4, unit), pick_split(inter, 8, unit)
    t = D // 16
    return [("qkv", SK_PARTIAL, Nq + 2 * Nkv, D, Sq, 0), ("qkv-fused", SK_PARTIAL, Nq + 2 * Nkv, D, Sq, t), ("o-fused", SK_RESID, D, Nq, 1, 0), ("o", SK_PARTIAL, D, Nq, So, 0),
            ("gu", SK_SWIGLU, 2 * inter, D, 1, 0), ("gu-fused", SK_SWIGLU, 2 * inter, D, 1, t), ("down-fused", SK_RESID, D, inter, 1, 0), ("down", SK_PARTIAL, D, inter, Sd, 0),
            ("head", SK_OUTF32, V, D, 1, 0), ("head-fused", SK_OUTF32, V, D, 1, t)]


def cut_N(fam: str, mode: int, N: int, K: int, S: int, bits: int) -> int:
    """the smallest N at which both sides of the 16 / 17 row boundary get the kernel form of the full N (N enters the dispatch through
    the workgroup count only).  The packed vocabulary heads are the exception: their one-wave form needs N >= 65536, which at a real K
    is 30 to 100 MB of codes -- the form is covered by the three head41 cases (1, 4 and 7 blocks in the wave) and the head tuples run in the form of a narrow N."""
    full = Case("x", fam, mode, N, K, S, bits=bits)
    if fam == "q" and mode == SK_OUTF32:
        return N_CUTS[0]
    for n in N_CUTS:
        if n < N and all(replace(full, N=n).form(M) == full.form(M) for M in (1, 16, 17, 32)):
            return n
    return N


def _model_cases() -> list[Case]:
    out = []
    seen = set()
    for name in MODELS:
        for fam in ("h", "q"):
            for role, mode, N, K, S, carry in model_tuples(name, fam):
                n = cut_N(fam, mode, N, K, S, 4)
                if mode == SK_RESID:
                    n = min(N, 48)                   # N / 16 workgroups either way
                key = (fam, mode, n, K, S, carry)
                if key in seen:
                    continue
                seen.add(key)
                kw = dict(Ms=(1, 16, 17), carry=carry, rs_scale=0.125 if carry else 1.0, bias=role.startswith(("head", "o-fused")), note=f"{name}-{role}")
                i = len(out) % 2                 # the real tuples alternate between (bf16, 4 bit) and (f16, 8 bit); the largest stay at 4 bit
                if fam == "h":
                    out += _h(mode, n, K, S, **kw)[i:i + 1]
                else:
                    out += _q(mode, n, K, S, full=False, **kw)[0 if n * K > 8 << 20 else i:][:1]
    return out


def _all_rows_once_per_form(cases: list[Case]) -> list[Case]:
    """every row count of ALL_M on (at least) one small shape per kernel form and mode; {1, 17} elsewhere"""
    def key(c):
        f = c.form(1)
        return (c.fam, c.mode, f["kernel"], f["tail"], f["nb"]) if c.fam == "h" else (c.fam, c.mode, f["NT"], f["NW"], f["bc"], c.bits)
    have = {key(c) for c in cases if c.Ms == ALL_M}
    out = []
    for c in cases:
        if c.Ms == FEW_M and key(c) not in have and c.N * c.K <= 1 << 20 and not c.carry:
            have.add(key(c))
            c = replace(c, Ms=ALL_M)
        out.append(c)
    return out


CASES = _all_rows_once_per_form(_build())
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES), "duplicate case id"


def ids(fam: str | None = None, pred=None):
    return [c.id for c in CASES if (fam is None or c.fam == fam) and (pred is None or pred(c))]


# forms the table must reach (tests/test_skinny_ref.py: test_every_form_is_selected)
REQUIRED_16 = ([("flat%d" % n, "none", None) for n in (4, 5, 6, 8, 10)] +
               [("ring<4,2,1>", "early", 0), ("ring<4,2,1>", "early", 1), ("ring<4,2,1>", "early", 3), ("ring<4,2,1>", "loop", 4), ("ring<4,2,1>", "none", 5), ("ring<4,2,1>", "none", 9),
                ("ring<1,2,4>", "early", 3), ("ring<1,2,4>", "loop", 4), ("ring<1,2,4>", "none", 6),
                ("ring<1,4,1>", "early", 0), ("ring<1,4,1>", "early", 1), ("ring<1,4,1>", "early", 3), ("ring<1,4,1>", "loop", 4), ("ring<1,4,1>", "none", 4),
                ("ring<1,2,8>", "none", 4), ("ring<1,2,8>", "loop", 4), ("ring<1,2,16>", "none", 8)])
REQUIRED_Q = ([dict(NT=1, NW=1, bc=b) for b in (1, 3, 5, 7)] + [dict(NT=1, NW=2, bc=1), dict(NT=1, NW=3, bc=2), dict(NT=1, NW=4, bc=2), dict(NT=1, NW=4, bc=3),
              dict(NT=1, NW=4, bc=4), dict(NT=1, NW=8, bc=1), dict(NT=1, NW=16, bc=4), dict(NT=4, NW=1, bc=1, nt4=True), dict(NT=4, NW=4, bc=1, nt4=True),
              dict(NT=4, NW=1, nt4=True, M16=True), dict(NT=4, NW=1, bc=1, head41=True), dict(NT=4, NW=1, bc=4, head41=True), dict(NT=4, NW=1, bc=7, head41=True)])


# ---- operands ------------------------------------------------------------------------------------------------------------------------
M_MAX = max(ALL_M)
SDT = {"f16": _lib.F16, "bf16": _lib.BF16, "f32": _lib.F32}


def ref_tiles(c: Case) -> np.ndarray:
    """the 16-column tiles the float64 reference is evaluated on: every one (reference() walks wide matrices in column blocks)"""
    return np.arange((c.N + 15) // 16)


def tile_cols(c: Case, tiles: np.ndarray) -> np.ndarray:
    cols = (tiles[:, None] * 16 + np.arange(16)[None]).reshape(-1)
    return cols[cols < c.N]


@dataclass
class Data:
    rows: int
    A16: np.ndarray            # [rows][K] storage
    A: np.ndarray              # float64 values
    W16: np.ndarray = None     # [N][K] storage (16-bit family)
    W: np.ndarray = None
    codes: np.ndarray = None   # packed family: uint32 [N][K bits / 32], scales / biases storage and float64 values, unpacked codes
    scales: np.ndarray = None
    biases: np.ndarray = None
    s64: np.ndarray = None
    b64: np.ndarray = None
    q: np.ndarray = None
    bias: np.ndarray = None    # float32 [N]
    xres: np.ndarray = None    # float32 [rows][N]
    nw: np.ndarray = None      # float32 [N]
    ss_in: np.ndarray = None   # float32 [tiles][rows]
    ss_dim: int = 0
    eps: float = 1e-6
    extra: dict = field(default_factory=dict)


def _pack(q: np.ndarray, bits: int) -> np.ndarray:
    per = 32 // bits
    q3 = q.reshape(q.shape[0], -1, per).astype(np.uint32)
    out = np.zeros(q3.shape[:2], np.uint32)
    for j in range(per):
        out |= q3[:, :, j] << np.uint32(j * bits)
    return out


def _store_sdt(x: np.ndarray, sdt: str):
    if sdt == "f32":
        a = x.astype(np.float32)
        return a, a.astype(np.float64)
    if sdt == "f16":
        a = x.astype(np.float16)
        return a, a.astype(np.float64)
    a = _audio.f32_to_bf16(x.astype(np.float32))
    return a, _audio.bf16_to_f32(a).astype(np.float64)


def make_data(c: Case, kind: str, rows: int | None = None) -> Data:
    """kind "real": normal activations, weights scaled to unit-size outputs (packed: quantize_affine of such weights).
    kind "int": small integers for which every intermediate the kernel can form is an integer below 2^24 (skinny_ref reports the peak):
      16 bit: a in [-3, 3], w in [-8, 8] per (n, k); packed: a in {-1, 0, 1}, any code, scales 1 or 2, biases multiples of the scale."""
    rng = np.random.default_rng(zlib.crc32(f"{c.id}/{kind}".encode()))
    rows = rows or max(c.Ms)
    N, K = c.N, c.K
    real = kind == "real"
    if c.fam == "h":
        a = rng.standard_normal((rows, K)) if real else rng.integers(-3, 4, (rows, K))
        w = rng.standard_normal((N, K)) / np.sqrt(K) if real else rng.integers(-8, 9, (N, K))
        A16, W16 = ref.store16(a, c.dtype), ref.store16(w, c.dtype)
        d = Data(rows, A16, ref.load16(A16, c.dtype), W16=W16, W=ref.load16(W16, c.dtype))
    else:
        a = rng.standard_normal((rows, K)) if real else rng.integers(-1, 2, (rows, K))
        A16 = ref.store16(a, c.dtype)
        if real:
            codes, s, b = checkpoint.quantize_affine((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), 64, c.bits, np.float32)
            q = ref.unpack_codes(codes, c.bits)
        else:
            q = rng.integers(0, 1 << c.bits, (N, K))
            codes = _pack(q, c.bits)
            s = rng.integers(1, 3, (N, K // 64)).astype(np.float64)
            b = s * rng.integers(-8, 9, (N, K // 64))
        sc, s64 = _store_sdt(np.asarray(s, np.float64), c.sdt)
        bi, b64 = _store_sdt(np.asarray(b, np.float64), c.sdt)
        d = Data(rows, A16, ref.load16(A16, c.dtype), codes=codes, scales=sc, biases=bi, s64=s64, b64=b64, q=q)
    if c.bias and c.mode != SK_PARTIAL:
        d.bias = (rng.standard_normal(N) if real else rng.integers(-50, 51, N)).astype(np.float32)
    if c.mode == SK_RESID:
        d.nw = (1.0 + 0.1 * rng.standard_normal(N) if real else 2.0 ** rng.integers(-1, 2, N)).astype(np.float32)
        if real:
            d.xres = (3.0 * rng.standard_normal((rows, N))).astype(np.float32)
        else:
            # the updated residual is a small integer r (its squares stay exact): x0 = r - (acc + bias), itself an integer below 2^24
            y = (ref.acc16(d.A, d.W, 0, K)[0] if c.fam == "h" else ref.accq(d.A, d.q, d.s64, d.b64, c.bits, c.dtype, 0, K)[0])
            y = y + (0.0 if d.bias is None else d.bias.astype(np.float64)[None])
            x0 = rng.integers(-200, 201, (rows, N)) - y
            d.xres = x0.astype(np.float32)
            assert np.array_equal(d.xres.astype(np.float64), x0) and np.abs(x0).max() < ref.EXACT_LIMIT
    if c.carry and real:
        d.ss_in = rng.uniform(4.0, 40.0, (c.carry, rows)).astype(np.float32)
        d.ss_dim = 16 * c.carry
    return d


REF_BLOCK = 2048      # columns per block of the float64 reference (whole tiles and gate / up pairs)


def reference(c: Case, d: Data, cols: np.ndarray | None = None, silu_allow=0.0, rsqrt_allow=0.0, wrong=None, **over) -> dict:
    """skinny_ref of the case on all rows of d (cols: the columns to evaluate, whole tiles / gate-up pairs), in blocks of REF_BLOCK columns"""
    if cols is None:
        cols = np.arange(c.N)
    if len(cols) > REF_BLOCK and wrong is None:
        parts = [reference(c, d, cols[i:i + REF_BLOCK], silu_allow, rsqrt_allow, **over) for i in range(0, len(cols), REF_BLOCK)]
        out = {k: np.concatenate([p[k] for p in parts], axis=0 if k in ("ss_out", "ss_tol") else -1) for k in parts[0] if k != "peak"}
        out["peak"] = max(p["peak"] for p in parts)
        return out
    sel = cols
    kw = dict(mode=c.mode, dtype=c.dtype, A=d.A, S=c.S, bias=None if d.bias is None else d.bias.astype(np.float64)[sel], silu_allow=silu_allow, rsqrt_allow=rsqrt_allow,
              wrong=wrong)
    if c.fam == "h":
        kw.update(W=d.W[sel])
    else:
        kw.update(q=d.q[sel], scales=d.s64[sel], biases=d.b64[sel], bits=c.bits)
    if d.ss_in is not None:
        kw.update(ss_in=d.ss_in, ss_tiles=c.carry, ss_dim=d.ss_dim, eps=d.eps, rs_scale=c.rs_scale)
    if c.mode == SK_RESID:
        kw.update(xres=d.xres.astype(np.float64)[:, sel], nw=d.nw.astype(np.float64)[sel])
    kw.update(over)
    return ref.skinny_ref(**kw)
