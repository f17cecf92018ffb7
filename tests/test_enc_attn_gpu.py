"""mia_op_attention_h64 (csrc/attention.hip, the Whisper encoder's head-dim-64 flash attention) against an fp64 softmax(q k^T / 8) v of the
same 16-bit-rounded inputs (tests/_enc_attn_ref.py; the cases are in tests/_enc_attn_cases.py and tests/test_enc_attn_ref.py proves on the
CPU that the spiked ones reach the lazy-rescale paths they name and that each comparison here can fail).

The kernel's tiles: a workgroup owns 128 queries of one (clip, head), four waves of 32, and walks the keys in tiles of 64; the last,
partial tile is a separate instantiation that masks keys >= T.  A query's softmax reference point moves only when a tile's maximum is
more than 2^8 above it, decided per lane under a wave-wide ballot.

Bound, per element (_enc_attn_ref.attention_bound): 2^-8 (bf16) | 2^-11 (f16) of the largest |v| of the element's (b, h) -- half an ulp per
rounded P on a convex combination of v -- plus 1 ulp of the output type at |ref| + that term.  The same bound holds the spiked cases,
whose scores reach 38 log2 units: no term for the fp32 score sum was needed (its size is worked out in attention_bound).

Measured on the MI355X (worst error / bound, bf16 / f16): edges 0.28 / 0.31 (both at T = 2, H = 3; T >= 31: 0.08 .. 0.19), strides and
padding 0.14 / 0.11; spiked: three_moves 0.31 / 0.29, large_p 0.19 / 0.13, one_lane 0.11 / 0.26, underflow 0.28 / 0.27, tail_move
0.14 / 0.26, plateau 0.30 / 0.42.  Every repeated call was bit-identical, and every clip of a stack equal to its own B = 1 call."""
import numpy as np
import pytest

import _enc_attn_cases as cases
import _enc_attn_ref as ref

pytestmark = pytest.mark.gpu


def _dtype(kind):
    import mlx_swift_audio_amd as m
    return {"bf16": m.BF16, "f16": m.F16}[kind]


@pytest.fixture(scope="module")
def edge_refs():
    """(B, T, H, kind) -> (inputs, reference, vmax), computed once per case and left unchanged"""
    cache = {}

    def get(B, T, H, kind):
        key = (B, T, H, kind)
        if key not in cache:
            qkv = cases.edge_inputs(B, T, H)
            out, vmax = ref.attention_ref(*qkv, B, T, H, kind)
            cache[key] = (qkv, out, vmax)
        return cache[key]
    return get


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("B,T,H", cases.EDGES)
def test_attention_h64_edges(ctx, edge_refs, B, T, H, kind):
    """Every row of `out` starts as NaN: a query block the remap of blockIdx.x skipped (a non-bijective remap), or a wave that took its
    rows for out of range, leaves them so.  At H = 3 V^T carries one more key tile than the kernel may read, filled with NaN.  A clip's
    rows do not depend on the stack it sits in."""
    from mlx_swift_audio_amd import ops
    (q, k, v), want, vmax = edge_refs(B, T, H, kind)
    kw = dict(fill=np.nan, dtype=_dtype(kind))
    if H == 3:
        kw.update(Tpad=(T + 63) // 64 * 64 + 64, pad_fill=np.nan)
    got = ops.attention_h64(ctx, q, k, v, B, T, H, **kw)
    assert got.shape == (B * T, H * 64) and np.isfinite(got).all()
    err, bound = np.abs(got - want), ref.attention_bound(want, vmax, kind, B, T, H)
    print(f"attn64 edges {kind} B={B} T={T} H={H}: max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(got, ops.attention_h64(ctx, q, k, v, B, T, H, **kw))                 # deterministic
    for b in range(B if B > 1 else 0):
        rows = slice(b * T, (b + 1) * T)
        assert np.array_equal(got[rows], ops.attention_h64(ctx, q[rows], k[rows], v[rows], 1, T, H, **kw)), f"clip {b}"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_attention_h64_strides_and_padding(ctx, kind):
    """ld_qk = 2D + 8 with NaN in the padding columns, ld_out = D + 4 with a sentinel in its padding columns, Tpad = 192 > align_up(T, 64)
    with V^T columns [100, 128) zero (the model's contract: they are read under a zero weight) and [128, 192) NaN (never read)."""
    from mlx_swift_audio_amd import ops
    s = cases.STRIDES
    B, T, H = s["B"], s["T"], s["H"]
    D = H * 64
    q, k, v = cases.random_qkv(B, T, H, 31)
    got = ops.attention_h64(ctx, q, k, v, B, T, H, Tpad=s["Tpad"], ld_qk=s["ld_qk"], ld_out=s["ld_out"], fill=-3.0, pad_fill=np.nan,
                            dtype=_dtype(kind))
    assert got.shape == (B * T, s["ld_out"])
    assert (got[:, D:] == -3.0).all()
    want, vmax = ref.attention_ref(q, k, v, B, T, H, kind)
    assert np.isfinite(got[:, :D]).all()
    err, bound = np.abs(got[:, :D] - want), ref.attention_bound(want, vmax, kind, B, T, H)
    print(f"attn64 strides {kind}: worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all()
    plain = ops.attention_h64(ctx, q, k, v, B, T, H, dtype=_dtype(kind))
    assert np.array_equal(got[:, :D], plain)                                                   # the strides change addresses, not values


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("name", sorted(cases.spiked_cases()))
def test_attention_h64_spiked(ctx, name, kind):
    from mlx_swift_audio_amd import ops
    c = cases.spiked_cases()[name]
    got = ops.attention_h64(ctx, c.q, c.k, c.v, c.B, c.T, c.H, fill=np.nan, dtype=_dtype(kind))
    want, vmax = ref.attention_ref(c.q, c.k, c.v, c.B, c.T, c.H, kind)
    assert np.isfinite(got).all()
    err, bound = np.abs(got - want), ref.attention_bound(want, vmax, kind, c.B, c.T, c.H)
    print(f"attn64 spiked {name} {kind} ({c.claim}): worst err/bound {(err / bound).max():.3f}, at query {c.query} {(err / bound)[c.query].max():.3f}")
    assert (err <= bound).all()
    assert np.array_equal(got, ops.attention_h64(ctx, c.q, c.k, c.v, c.B, c.T, c.H, fill=np.nan, dtype=_dtype(kind)))


def test_attention_h64_rejects_bad_arguments(ctx):
    """refused by the host-side checks, before anything is copied or launched"""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    T, H, D = 8, 1, 64
    qk, vt, out = np.zeros((T, 2 * D + 8), np.uint16), np.zeros((H, 64, 128), np.uint16), np.zeros((T, D + 4), np.uint16)

    def call(qk_p=qk.ctypes.data, ld_qk=2 * D, vt_p=vt.ctypes.data, out_p=out.ctypes.data, ld_out=D, B=1, T=T, H=H, Tpad=64, dtype=m.BF16):
        return ctx.lib.mia_op_attention_h64(ctx.h, qk_p, ld_qk, vt_p, out_p, ld_out, B, T, H, Tpad, dtype, m._lib.MEM_HOST)

    ctx.check(call())                                                     # the baseline the refusals vary is accepted
    ctx.check(call(ld_qk=2 * D + 8, ld_out=D + 4, Tpad=128))
    for bad in (dict(Tpad=96), dict(Tpad=0), dict(T=65, Tpad=64), dict(ld_qk=2 * D + 4), dict(ld_out=D + 2), dict(ld_qk=2 * D - 8),
                dict(ld_out=D - 4), dict(dtype=m.F32), dict(qk_p=None), dict(vt_p=None), dict(out_p=None), dict(B=0), dict(T=0), dict(H=0),
                dict(H=2)):                                               # (H = 2: both strides then fail to cover the row)
        with pytest.raises(m.MiaError) as e:
            ctx.check(call(**bad))
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, bad
    assert not out.any()
