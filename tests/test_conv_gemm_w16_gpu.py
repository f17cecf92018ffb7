"""conv_gemm_w16 (csrc/conv_gemm_w16.hip, through mia_op_conv_gemm_w16_tile) against tap_gemm_ref in float64 on the weights already rounded
to bf16 and widened.  Bound: 3.02 x tap_gemm_ref's per-element `tol`: the kernel adds 3 K exact products in fp32 where the formula
counts K, 3 (K + 2) >= 3 K + 2, and sum (|hi| + |mid| + |lo|) |w| <= (1 + 2^-8 + 2^-16) sum |x| |w|; nothing in it is measured (README.md,
"Kokoro", has an MI355X's worst err / tol).  Unwritten elements of Y are prefilled and must come back bit for bit.  The one-hot test
is the sharp one: a dropped or misplaced term, a wrong k-to-lane map or a swapped plane changes the bits."""
import numpy as np
import pytest
import torch

import _f32_ops_ref as ref
import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7777.25)
TILES = {1: (65, 32), 2: (129, 96), 3: (257, 160)}       # forced tile (64 x 64, 128 x 64, 128 x 128) -> ragged (M, N)


def _plain(M, N, Cin, taps, **kw):
    return dict(dict(M=M, N=N, Cin=Cin, taps=taps, pad=(taps - 1) // 2, T_in=M, T_out=M), **kw)


# id -> (descriptor fields, phases, forced tile)
CASES = {
    "rule-64x64": (_plain(*TILES[1], 64, 3), 1, 0),
    "tile-128x64": (_plain(*TILES[2], 64, 3), 1, 2),
    "tile-128x128": (_plain(*TILES[3], 64, 3), 1, 3),
    "cin32-two-taps-a-stage": (_plain(70, 40, 32, 3), 1, 0),
    "cin96-stage-ends-mid-tap": (_plain(70, 40, 96, 3), 1, 0),
    "dil3-pad9": (_plain(70, 40, 64, 7, dil=3, pad=9), 1, 0),
    "stride2": (_plain(70, 40, 64, 3, x_row_mul=2, pad=1, T_in=140), 1, 0),
    # ConvTransposed1d stride 3, kernel 6, padding 1 as run_convt launches it; T_out cuts the last rows
    "convt-s3-k6": (dict(M=41, N=40, Cin=64, taps=2, pad=1, T_in=40, T_out=118, y_row_mul=3, y_row_off=-1, y_phase_step=1,
                         w_phase_stride=40 * 2 * 64, lrelu_slope=0.1), 3, 0),
    "dup-two-phases": (dict(M=37, N=40, Cin=64, taps=1, pad=0, T_in=37, T_out=74, y_row_mul=2, y_phase_step=1), 2, 0),
    "epilogue": (_plain(70, 40, 64, 3, out_scale=0.70710678118654752, ldy=48, ldr=56, res=2), 1, 0),
}


def _build(cid):
    d, phases, tile = dict(CASES[cid][0]), *CASES[cid][1:]
    rng = np.random.default_rng(sorted(CASES).index(cid))
    N, K = d["N"], d["taps"] * d["Cin"]
    res = d.pop("res", 0)
    ldy, ldr = d.pop("ldy", N), d.pop("ldr", N)
    nw = phases if d.get("w_phase_stride") else 1
    w16 = torch.from_numpy((rng.standard_normal((nw, N, K)) / np.sqrt(K)).astype(np.float32)).to(torch.bfloat16)
    d["X"] = rng.standard_normal((d["T_in"], d["Cin"])).astype(np.float32)
    d["bias"] = rng.standard_normal(N).astype(np.float32)
    d["Y"] = np.full((d["T_out"] + 3, ldy), SENTINEL, np.float32)
    if res:
        d["R"], d["R2"] = (rng.standard_normal((d["T_out"], ldr)).astype(np.float32) for _ in range(2))
    return d, w16, phases, tile


@pytest.mark.parametrize("cid", sorted(CASES))
def test_against_float64(ctx, cid):
    d, w16, phases, tile = _build(cid)
    out = ops.conv_gemm_w16(ctx, w16.cuda(), phases, tile, **d)
    slope = d.get("lrelu_slope", 0.0)
    kw = dict(d, W=w16.float().numpy(), allow_pre=ref.lrelu_allowance(d["X"], slope) if slope else None)
    r = ref.tap_gemm_ref(phases, **kw)
    assert r.written.any() and not r.written.all()
    assert np.array_equal(out[~r.written], d["Y"][~r.written]), f"{cid}: an element the op must not write changed"
    err, tol = np.abs(out[r.written].astype(np.float64) - r.Y[r.written]), 3.02 * r.tol[r.written]
    worst = int(np.argmax(err / tol))
    print(f"{cid}: max err {err.max():.3e}, worst err / tol {err[worst] / tol[worst]:.3f} (tol {tol[worst]:.3e})")
    assert (err <= tol).all(), f"{cid}: err {err[worst]:.3e} > tol {tol[worst]:.3e}"
    if cid == "epilogue":      # the case can fail: out_scale applied after R2 is far outside the bound
        bad = ref.tap_gemm_ref(phases, wrong="order", **kw)
        assert (np.abs(out[r.written].astype(np.float64) - bad.Y[r.written]) > tol).any()


@pytest.mark.parametrize("Cin", [32, 96])
@pytest.mark.parametrize("tile", sorted(TILES))
def test_one_hot_weights_give_back_the_bits_of_x(ctx, tile, Cin):
    (M, N), taps = TILES[tile], 3
    rng = np.random.default_rng([tile, Cin])
    x = (rng.standard_normal((M, Cin)) * 2.0 ** rng.integers(-20, 21, (M, Cin))).astype(np.float32)      # 24-bit mantissas, mixed exponents
    tap, c, sign = rng.integers(0, taps, N), rng.integers(0, Cin, N), rng.choice([-1.0, 1.0], N)
    w = np.zeros((N, taps * Cin), np.float32)
    w[np.arange(N), tap * Cin + c] = sign
    out = ops.conv_gemm_w16(ctx, torch.from_numpy(w).to(torch.bfloat16).cuda(), 1, tile, X=x, Y=np.full((M, N), SENTINEL, np.float32),
                            M=M, N=N, Cin=Cin, taps=taps, pad=1, T_in=M, T_out=M)
    rows = np.arange(M)[:, None] + tap[None, :] - 1
    ok = (rows >= 0) & (rows < M)
    want = np.where(ok, sign[None, :].astype(np.float32) * x[np.clip(rows, 0, M - 1), c[None, :]], np.float32(0.0)).astype(np.float32)
    assert not ok.all() and np.array_equal(out.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("field,extra", [
    ("alpha", dict(alpha=np.ones(64, np.float32))), ("noise", dict(noise=np.zeros(8, np.float32), R=np.zeros((8, 32), np.float32))),
    ("tanh_out", dict(tanh_out=1)), ("act", dict(act=1)), ("n_seq", dict(n_seq=2, x_seq_step=8, y_seq_step=8)),
    ("W must be null", dict(W=np.zeros((32, 64), np.float32))), ("ldw", dict(ldw=68))])
def test_refuses_what_it_does_not_serve(ctx, field, extra):
    d = dict(dict(X=np.zeros((16, 64), np.float32), Y=np.zeros((16, 32), np.float32), M=8, N=32, Cin=64, T_in=8, T_out=8), **extra)
    with pytest.raises(m.MiaError, match=field) as e:
        ops.conv_gemm_w16(ctx, np.zeros((32, 72), np.uint16), 1, **d)
    assert e.value.code == (m._lib.ERR_INVALID_ARGUMENT if field == "ldw" else m._lib.ERR_UNSUPPORTED)
