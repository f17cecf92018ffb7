"""Operator-level parity of the two fp32 kernels that carry every codec, flow and vocoder stage: conv_gemm_f32 (codec_kernels.hip) through
mia_op_conv1d_f32 and the mia_op_conv_gemm_f32 hook, attn_f32_kernel (attn_f32.hip) through mia_op_attention_f32 and its _ex hook, each
against a float64 reference of the same operation (tests/_f32_ops_ref.py; pinned against torch and shown able to fail in
tests/test_f32_ops_ref.py; the cases are in tests/_f32_ops_cases.py).

Tolerances are derived per element, none is a chosen constant:
 * dot products: (K + 2) 2^-24 (sum |x w| + |bias|) for any summation order of exact fp32 products accumulated in fp32;
 * epilogue: that bound times the activation's Lipschitz constant (1; GELU 1.13; SiLU 1.1; |out_scale|; |noise[row]|), plus one
   rounding 2^-24 |result| per fp32 operation;
 * device intrinsics (__expf, the erf polynomial, tanhf, v_sin behind the Cody-Waite reduction): 4 x the error of the same function
   evaluated in float32 by torch against float64 over the case's own values.  Measured 2026-10-19 (LABNOTES), already times 4, at
   pre-activations up to |v| ~ 12: GELU 3.5e-6, SiLU 3.1e-6, ELU 1.2e-7, leaky-ReLU 2.3e-8, tanh 2.4e-7; the snake prologue per input
   channel 1.3e-6 ... 2.3e-5 (alpha 0.05 ... 20, |alpha x| up to ~400, where the rounding of alpha x alone is 2^-24 * 400 = 2.4e-5 rad),
   which includes ralpha * 2 * 2e-7 for the absolute error codec_kernels.hip documents for sin_cw; the leaky-ReLU prologue one rounding
   of slope * x, 2.5e-8.  All of them are small next to the dot product's own bound (1e-5 ... 7e-4 in these cases);
 * attention: 8 x the largest error of a naive float32 evaluation against float64 on the same inputs, plus one rounding of the output
   (the reference is float64, the kernel stores fp32): 1.5e-7 at T = 1, 1.9e-6 ... 1.1e-5 for the unit-scale cases, 2.6e-7 (the output
   rounding alone: the naive evaluation is exact there) where one key takes all the mass.
Observed on an MI355X the same day: worst error / bound 0.48 for the tap GEMM (stacked noise form; 0.06 over the tile cases), 0.33 for
attention (T = 31), 0 for the one-key case.  No bound was widened.

Every output buffer is filled with a sentinel first and sits between guard rows: elements the operation must not write (columns past N,
rows past T_out, rows the row mapping drops, rows past a stacked sequence's length under the noise form) must come back bit for bit."""
import numpy as np
import pytest
import torch

import _f32_ops_cases as cases
import mlx_swift_audio_amd as m
from mlx_swift_audio_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 16      # sentinel rows in front of and behind every Y


def _run_tap_gemm(ctx, c: cases.Case, d=None, phases=None):
    """The case on the GPU; returns Y's whole buffer with the guard rows checked."""
    shift = c.y_shift if d is None else 0
    d = dict(c.d if d is None else d)
    phases = c.phases if phases is None else phases
    y0 = d["Y"]
    big = torch.full((GUARD + y0.shape[0] + GUARD, y0.shape[1]), float(cases.SENTINEL), dtype=torch.float32, device="cuda")
    big[GUARD:GUARD + y0.shape[0]] = torch.from_numpy(y0).cuda()
    d["Y"] = big[GUARD + shift:GUARD + y0.shape[0]]
    if c.op == "conv1d":
        ops.conv1d_f32(ctx, d["X"], d["W"], d["Y"], Cin=d["Cin"], taps=d["taps"], stride=d["x_row_mul"], dil=d["dil"], pad=d["pad"], act=d["act"],
                       bias=d.get("bias"), r=d.get("R"), T_in=d["T_in"], T_out=d["T_out"], N=d["N"])
    else:
        ops.conv_gemm_f32(ctx, phases, **d)
    out = big.cpu().numpy()
    guard = np.full((GUARD, y0.shape[1]), cases.SENTINEL, np.float32)
    assert np.array_equal(out[:GUARD], guard) and np.array_equal(out[-GUARD:], guard), f"{c.id}: wrote outside Y"
    return out[GUARD:-GUARD]


def _check_tap_gemm(c: cases.Case, out: np.ndarray, r, prefill: np.ndarray):
    assert np.array_equal(out[~r.written], prefill[~r.written]), f"{c.id}: an element the op must not write changed"
    got = out[r.written].astype(np.float64)
    assert np.isfinite(got).all(), c.id
    err, tol = np.abs(got - r.Y[r.written]), r.tol[r.written]
    worst = int(np.argmax(err / np.maximum(tol, 1e-300)))
    print(f"{c.id}: max err {err.max():.3e}, worst err / tol {err[worst] / max(tol[worst], 1e-300):.3f} (tol {tol[worst]:.3e})")
    assert (err <= tol).all(), f"{c.id}: err {err[worst]:.3e} > tol {tol[worst]:.3e}"


def _tap_gemm_family(ctx, fam, cid):
    c = cases.case(fam, cid)
    out = _run_tap_gemm(ctx, c)
    _check_tap_gemm(c, out, cases.reference(fam, cid), c.d["Y"])
    return c, out


@pytest.mark.parametrize("cid", cases.case_ids("tiles"))
def test_conv1d_tile_instantiations(ctx, cid):
    c = cases.case("tiles", cid)
    assert cases.instantiation(c.d["M"], c.d["N"], c.d["taps"] * c.d["Cin"]) == c.expect
    _tap_gemm_family(ctx, "tiles", cid)


@pytest.mark.parametrize("cid", cases.case_ids("geometry"))
def test_conv1d_geometry(ctx, cid):
    c, out = _tap_gemm_family(ctx, "geometry", cid)
    if cid.endswith("zero-row"):      # a window of zeros only: exactly bias + r
        assert np.array_equal(out[0, :c.d["N"]], c.d["bias"] + c.d["R"][0, :c.d["N"]])


@pytest.mark.parametrize("cid", cases.case_ids("activations"))
def test_conv1d_activations(ctx, cid):
    _tap_gemm_family(ctx, "activations", cid)


@pytest.mark.parametrize("cid", cases.case_ids("rowmap"))
def test_hook_transposed_convolution_phases(ctx, cid):
    _tap_gemm_family(ctx, "rowmap", cid)


@pytest.mark.parametrize("cid", cases.case_ids("epilogue"))
def test_hook_prologues_and_epilogues(ctx, cid):
    _tap_gemm_family(ctx, "epilogue", cid)


@pytest.mark.parametrize("cid", cases.case_ids("stacked"))
def test_hook_stacked_sequences(ctx, cid):
    c, out = _tap_gemm_family(ctx, "stacked", cid)
    N = c.d["N"]
    for u, du, phases, row0, rows in c.singles:
        one = _run_tap_gemm(ctx, c, du, phases)
        assert rows > 0 and np.array_equal(out[row0:row0 + rows, :N], one[:rows, :N]), f"{cid}: sequence {u} differs from its own call"
        assert (one[:rows, :N] != cases.SENTINEL).all()


# ---- attention -----------------------------------------------------------------------------------------------------------------------
def _run_attention(ctx, c: cases.AttnCase, plain: bool, b=None):
    """b: sequence b alone as its own B = 1, T = seq_len[b] call.  q | k | v are three views of one fused device buffer."""
    D = c.H * 64
    B, T, rows = (c.B, c.T, slice(None)) if b is None else (1, int(c.seq_len[b]), slice(b * c.T, b * c.T + int(c.seq_len[b])))
    qkv = torch.from_numpy(np.ascontiguousarray(c.qkv[rows])).cuda()
    out0 = np.full((B * T + 2, D + 4), cases.SENTINEL, np.float32)
    kw = dict(ldq=3 * D, ldk=3 * D, ldv=3 * D)
    if plain:
        out = ops.attention_f32(ctx, qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out0, B, T, c.H, c.scale, **kw)
    else:
        out = ops.attention_f32_ex(ctx, qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], out0, B, T, c.H, c.scale, p=None if c.p is None else c.p[:T],
                                   bias_u=c.bias_u, bias_v=c.bias_v, seq_len=c.seq_len if b is None else None, chunk=c.chunk, **kw)
    assert np.array_equal(out[:, D:], out0[:, D:]) and np.array_equal(out[B * T:], out0[B * T:]), f"{c.id}: wrote outside out"
    return out[:B * T, :D]


def _check_attention(fam, c, out):
    r64, tol = cases.attn_reference(fam, c.id)
    valid = c.valid_rows()
    assert np.isfinite(out[valid]).all(), c.id
    err = np.abs(out.astype(np.float64) - r64)[valid].max()
    print(f"{c.id}: max err {err:.3e}, tol {tol:.3e}")
    assert err <= tol, f"{c.id}: err {err:.3e} > tol {tol:.3e}"


@pytest.mark.parametrize("cid", cases.attn_ids("attn-plain"))
def test_attention_f32(ctx, cid):
    c = cases.attn_case("attn-plain", cid)
    out = _run_attention(ctx, c, plain=True)
    _check_attention("attn-plain", c, out)
    if c.one_hot is not None:         # one key takes all the mass: the output is that key's V row (same bound)
        v = c.parts()[2]
        want = np.concatenate([v[b * c.T + c.one_hot[b * c.T:(b + 1) * c.T]] for b in range(c.B)])
        assert np.abs(out.astype(np.float64) - want).max() <= cases.attn_reference("attn-plain", cid)[1]


@pytest.mark.parametrize("cid", cases.attn_ids("attn-ex"))
def test_attention_f32_ex(ctx, cid):
    c = cases.attn_case("attn-ex", cid)
    out = _run_attention(ctx, c, plain=False)
    _check_attention("attn-ex", c, out)
    if c.seq_len is not None:
        for b, L in enumerate(c.seq_len):
            one = _run_attention(ctx, c, plain=False, b=b)
            assert np.array_equal(out[b * c.T:b * c.T + L], one), f"{cid}: sequence {b} differs from its own B = 1 call"


def test_attention_f32_ex_without_extras_is_the_plain_op(ctx):
    c = cases.attn_case("attn-plain", "attn-T129-B2H3")
    assert np.array_equal(_run_attention(ctx, c, plain=True), _run_attention(ctx, c, plain=False))


# ---- error paths ---------------------------------------------------------------------------------------------------------------------
def _good(ctx):
    _tap_gemm_family(ctx, "tiles", "tile-111-k224")


def _raises_invalid(ctx, fn):
    with pytest.raises(m.MiaError) as e:
        fn()
    assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, e.value
    _good(ctx)          # the context stays usable


def _small(**kw):
    rng = np.random.default_rng(5)
    d = dict(X=cases.f32(rng.standard_normal((8, 64))), T_in=8, W=cases.f32(rng.standard_normal((4, 64))), Y=cases.y_buf(8, 4), T_out=8, M=8, N=4, Cin=64)
    d.update(kw)
    return d


def test_conv_gemm_rejects_cin_48(ctx):
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(Cin=48)))
    _raises_invalid(ctx, lambda: ops.conv1d_f32(ctx, _small()["X"], _small()["W"], cases.y_buf(8, 4), Cin=48))


def test_conv_gemm_rejects_unaligned_rows(ctx):
    x = cases.f32(np.zeros((8, 66)))
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(X=x)))                       # ldx % 4 != 0
    _raises_invalid(ctx, lambda: ops.conv1d_f32(ctx, x, _small()["W"], cases.y_buf(8, 4), Cin=64))


def test_conv_gemm_rejects_a_pointer_off_by_four_bytes(ctx):
    flat = torch.zeros(8 * 64 + 4, device="cuda")
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(X=flat[1:1 + 8 * 64].view(8, 64))))
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(W=flat[1:1 + 4 * 64].view(4, 64))))


def test_conv_gemm_rejects_rows_shorter_than_cin(ctx):
    # ldx < Cin would take the kernel's clamped loads past the last row of X; ldw must hold whole float4s and cover taps * Cin
    x = cases.f32(np.zeros((16, 32)))
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(X=x, T_in=8)))
    _raises_invalid(ctx, lambda: ops.conv1d_f32(ctx, x, _small()["W"], cases.y_buf(8, 4), Cin=64, T_in=8))
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(ldw=66, W=cases.f32(np.zeros((4, 66))))))
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(ldw=32)))


def test_conv_gemm_rejects_a_pad_beyond_the_row_arithmetic(ctx):
    # the kernel subtracts pad in 32-bit row arithmetic; a negative pad only crops and stays valid
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(pad=-(2 ** 31 - 8))))
    _raises_invalid(ctx, lambda: ops.conv1d_f32(ctx, _small()["X"], _small()["W"], cases.y_buf(8, 4), Cin=64, pad=2 ** 31 - 8))
    d = _small(pad=-3, T_out=5, M=5)
    out = ops.conv_gemm_f32(ctx, 1, **d)
    assert np.array_equal(out[5:], d["Y"][5:]) and np.abs(out[:5] - d["X"][3:8].astype(np.float64) @ d["W"].astype(np.float64).T).max() < 1e-4


def test_conv_gemm_rejects_noise_without_residual(ctx):
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **_small(noise=cases.f32(np.zeros(8)))))


def test_conv_gemm_rejects_overlapping_stacked_sequences(ctx):
    d = _small(X=cases.f32(np.zeros((16, 64))), Y=cases.y_buf(16, 4), n_seq=2, x_seq_step=7, y_seq_step=8, seq_len=np.asarray([8, 8], np.int32))
    _raises_invalid(ctx, lambda: ops.conv_gemm_f32(ctx, 1, **d))


def _attn_small():
    qkv = torch.zeros((8, 3 * 64 + 2), device="cuda")
    return qkv, np.zeros((8, 64), np.float32)


def test_attention_rejects_strides_that_are_no_multiple_of_four(ctx):
    qkv, out = _attn_small()
    _raises_invalid(ctx, lambda: ops.attention_f32(ctx, qkv[:, :64], qkv[:, 64:128], qkv[:, 128:192], out, 1, 8, 1))
    _raises_invalid(ctx, lambda: ops.attention_f32_ex(ctx, qkv[:, :64], qkv[:, 64:128], qkv[:, 128:192], out, 1, 8, 1))


def test_attention_rejects_positional_keys_without_biases(ctx):
    q = np.zeros((8, 64), np.float32)
    _raises_invalid(ctx, lambda: ops.attention_f32_ex(ctx, q, q, q, q.copy(), 1, 8, 1, p=q))
    _raises_invalid(ctx, lambda: ops.attention_f32_ex(ctx, q, q, q, q.copy(), 1, 8, 1, p=q, bias_u=q[:1]))
    _raises_invalid(ctx, lambda: ops.attention_f32_ex(ctx, q, q, q, q.copy(), 0, 8, 1))
