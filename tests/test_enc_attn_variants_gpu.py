"""The kernel forms of the Whisper encoder's attention (csrc/attention.hip; ops.ATT_VARIANTS) against each other and against the fp64
softmax of tests/_enc_attn_ref.py.

Every form keeps, per query, the key-tile order, the raw-max softmax, the lazy-rescale rule and the fp32 accumulation of the
register-staged 128-query kernel ("reg128", the form every earlier test ran), so the raw 16-bit outputs must be EQUAL, not close; each
form's output also passes the bound tests/test_enc_attn_gpu.py applies (_enc_attn_ref.attention_bound, unchanged).

Shapes: B = 2, H = 3 -- every grid here (nqb * 6) is not a multiple of 8, so the XCD remap's remainder branch runs -- and T at one
tile and tail-only (1, 63, 64, 65), two tiles with a 128-query block just full / just over (128, 129), three tiles, where the 3-slot
LDS-DMA ring wraps (191, 192, 193), a 256-query block just full / just over with the last wave's second query block empty or holding
one row (255, 256, 257), and 449: a ring that wraps twice, with a tail.

The buffers live on the device with 64 guard rows behind `out`; `out` and the guard rows start as a NaN bit pattern no arithmetic
produces, so a row or column the kernel must not write is found by its bits."""
import numpy as np
import pytest
import torch

import _enc_attn_cases as cases
import _enc_attn_ref as ref

pytestmark = pytest.mark.gpu

B, H = 2, 3
T_ALL = [1, 63, 64, 65, 128, 129, 191, 192, 193, 255, 256, 257, 449]
GUARD = 64
BIG = 3.0e4          # a large finite pad value (both 16-bit types hold it)


def _dtype(kind):
    import mlx_swift_audio_amd as m
    return {"bf16": m.BF16, "f16": m.F16}[kind]


def _align64(T):
    return (T + 63) // 64 * 64


@pytest.fixture(scope="module")
def refs():
    """(T, kind) -> (inputs, fp64 reference, vmax): computed once per case and left unchanged"""
    cache = {}

    def get(T, kind):
        if (T, kind) not in cache:
            qkv = cases.random_qkv(B, T, H, 7000 + T)
            out, vmax = ref.attention_ref(*qkv, B, T, H, kind)
            cache[(T, kind)] = (qkv, out, vmax)
        return cache[(T, kind)]
    return get


def _run(ctx, qkv, T, kind, variant, Tpad=None, ld_qk=None, ld_out=None, pad_fill=0.0, B=B, H=H):
    """one kernel form on device buffers; returns the raw output [B*T, ld_out] as uint16 after checking that the guard rows behind it and
    the pad columns still hold the sentinel"""
    from mlx_swift_audio_amd import ops
    dt, D = _dtype(kind), H * 64
    Tpad = _align64(T) if Tpad is None else Tpad
    ld_qk = 2 * D if ld_qk is None else ld_qk
    ld_out = D if ld_out is None else ld_out
    qk, vt = ops.enc_attention_buffers(*qkv, B, T, H, Tpad, ld_qk, pad_fill, dt)
    d_qk = torch.from_numpy(qk.view(np.int16)).cuda()
    d_vt = torch.from_numpy(vt.view(np.int16)).cuda()
    d_out = torch.from_numpy(np.full((B * T + GUARD, ld_out), cases.SENTINEL, np.uint16).view(np.int16)).cuda()
    ops.attention_h64_device_variant(ctx, d_qk, d_vt, d_out, B, T, H, Tpad, ld_qk, ld_out, dt, variant)
    got = d_out.cpu().numpy().view(np.uint16)
    assert (got[B * T:] == cases.SENTINEL).all(), "rows behind the last query were written"
    assert (got[:B * T, D:] == cases.SENTINEL).all(), "pad columns of out were written"
    return got[:B * T]


def _check_oracle(bits, want, vmax, T, kind, what):
    from mlx_swift_audio_amd import ops
    got = ops.from_bits16(np.ascontiguousarray(bits[:, :H * 64]), _dtype(kind))
    assert np.isfinite(got).all(), what
    err, bound = np.abs(got - want), ref.attention_bound(want, vmax, kind, B, T, H)
    print(f"attn64 variants {what} {kind} T={T}: worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), what


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("T", T_ALL)
def test_variants_bit_equal_and_within_bound(ctx, refs, T, kind):
    from mlx_swift_audio_amd import ops
    qkv, want, vmax = refs(T, kind)
    base = _run(ctx, qkv, T, kind, ops.ATT_REG128)
    _check_oracle(base, want, vmax, T, kind, "reg128")
    for name, variant in ops.ATT_VARIANTS.items():
        got = _run(ctx, qkv, T, kind, variant)
        assert np.array_equal(got, base), f"{name} differs from reg128 in {(got != base).sum()} elements"
        _check_oracle(got, want, vmax, T, kind, name)
    assert np.array_equal(_run(ctx, qkv, T, kind, -1), base), "the form the encoder launches at this shape"


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("T", [65, 193, 257])
def test_variants_wider_vt_and_pad_values(ctx, refs, T, kind):
    """Tpad = align64(T) + 64: the extra V^T key tile is never read, whether it (and nothing else the kernel may read) holds a large
    finite value or zero; V^T columns [T, align64(T)) are zero by the model's contract and the keys there are masked."""
    from mlx_swift_audio_amd import ops
    qkv, want, vmax = refs(T, kind)
    base = _run(ctx, qkv, T, kind, ops.ATT_REG128)
    for name, variant in ops.ATT_VARIANTS.items():
        big = _run(ctx, qkv, T, kind, variant, Tpad=_align64(T) + 64, pad_fill=BIG)
        zero = _run(ctx, qkv, T, kind, variant, Tpad=_align64(T) + 64, pad_fill=0.0)
        assert np.array_equal(big, zero), name
        assert np.array_equal(big, base), name
        _check_oracle(big, want, vmax, T, kind, name + " Tpad+64")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("T", [129, 449])
def test_variants_row_strides(ctx, refs, T, kind):
    """ld_qk = 2 H 64 + 8 (pad columns hold a large finite value), ld_out = H 64 + 4 (pad columns keep the sentinel: _run checks)"""
    from mlx_swift_audio_amd import ops
    qkv, want, vmax = refs(T, kind)
    D = H * 64
    base = _run(ctx, qkv, T, kind, ops.ATT_REG128)
    for name, variant in ops.ATT_VARIANTS.items():
        got = _run(ctx, qkv, T, kind, variant, ld_qk=2 * D + 8, ld_out=D + 4, pad_fill=BIG)
        assert np.array_equal(got[:, :D], base), name
        _check_oracle(got, want, vmax, T, kind, name + " strided")


def test_long_stack_where_the_launcher_takes_the_q64_form(ctx):
    """B = 8, H = 15, T = 1025: ceil(T / 256) * H * B = 600 workgroups of the 64-query form, the shape class at which
    mia_enc_attention_launch itself (variant -1) chooses it; 17 key tiles with a one-key tail, the last query block holding one row.
    Bits only: the fp64 reference of this size belongs to the whole-model tests."""
    from mlx_swift_audio_amd import ops
    Bl, Hl, T = 8, 15, 1025
    qkv = cases.random_qkv(Bl, T, Hl, 99)
    base = _run(ctx, qkv, T, "bf16", ops.ATT_REG128, B=Bl, H=Hl)
    assert (base != cases.SENTINEL).all()
    for name, variant in list(ops.ATT_VARIANTS.items()) + [("launcher's choice", -1)]:
        assert np.array_equal(_run(ctx, qkv, T, "bf16", variant, B=Bl, H=Hl), base), name


def test_variant_out_of_range_is_refused(ctx):
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    qkv = cases.random_qkv(1, 8, 1, 3)
    for bad in (-2, len(ops.ATT_VARIANTS)):
        with pytest.raises(m.MiaError) as e:
            ops.attention_h64_bits(ctx, *qkv, 1, 8, 1, variant=bad)
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT
