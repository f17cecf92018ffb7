"""mia_op_linear_epi: the two special store layouts of csrc/gemm.hip -- MIA_EPI_QKV_VT (q | k rows + V transposed per head, the operands
of the encoder attention) and MIA_EPI_HEADMAJOR (cross-attention K / V) -- on every tile variant, against an fp64 x @ w.T + bias scattered
by the layout formulas (tests/_enc_attn_ref.epilogue_ref; tests/test_enc_attn_ref.py shows that a wrong layout leaves the bound).

What the shapes reach (tests/_enc_attn_cases.QKV_SHAPES): in the 256^2 kernels (variants 2 and 4) a tile that lies wholly in the V third
runs with swapped MFMA operands and stores 8 bytes along t; a tile that straddles the k | V boundary (odd H) or holds q | k | V at once
(H = 1) falls back to the per-element scatter of epilogue_store; ldy % 8 == 0 takes the 8-phase kernel's row-staged 16-byte stores for q | k
tiles, ldy = 2D + 4 its 8-byte ones.

Value check: `got` is the 16-bit rounding of something inside the fp32 band tests/test_ops_gpu.py holds this GEMM to (2e-4 + 1e-4 |ref|),
i.e. the band plus half an ulp.  Layout check, exact: y and vt start as a NaN bit pattern no arithmetic produces; every V^T column t >= T
and every y column >= 2D keeps it, every other element lost it.

Measured on the MI355X (worst error / bound over all variants and shapes, bf16 / f16): QKV_VT q | k 0.96 / 0.76, V^T 0.96 / 0.76,
HEADMAJOR 0.95 / 0.75; the chained pair: GEMM 0.96 / 0.76, attention 0.32 / 0.36 (T = 100) and 0.28 / 0.29 (T = 36).  The GEMM figures
are the output's own rounding: half an ulp is nearly all of the bound (at |ref| in [4, 8) half a bf16 ulp is 1.56e-2, the fp32 band 1e-3),
so a ratio near 1 is what a correctly rounded result gives and says little about the fp32 value; the layout checks are exact."""
import numpy as np
import pytest
import torch          # before the library is loaded: the chained test shares the device with torch, whose HIP runtime has to come first

import _enc_attn_cases as cases
import _enc_attn_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = cases.SENTINEL


def _dtype(kind):
    import mlx_swift_audio_amd as m
    return {"bf16": m.BF16, "f16": m.F16}[kind]


def _check_values(tag, got, want, mask, kind):
    assert np.isfinite(got[mask]).all(), tag
    err, bound = np.abs(got[mask] - want[mask]), ref.epilogue_bound(want[mask], kind)
    print(f"{tag}: max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}")
    assert (err <= bound).all(), tag


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("B,T,H,K", cases.QKV_SHAPES)
def test_qkv_vt_epilogue(ctx, B, T, H, K, variant, kind):
    from mlx_swift_audio_amd import ops
    D, M = H * 64, B * T
    x, w, bias = cases.gemm_inputs(M, 3 * D, K)
    t64 = (T + 63) // 64 * 64
    for ldy, Tpad in [(2 * D + 4, t64), (2 * D + 4, t64 + 64), (2 * D, t64)]:
        y0 = np.full((M, ldy), SENTINEL, np.uint16)
        vt0 = np.full((B, H, 64, Tpad), SENTINEL, np.uint16)
        yb, vb, y, vt = ops.linear_epi(ctx, x, w, bias, y0, vt0, epi=ops.EPI_QKV_VT, T=T, H=H, Tpad=Tpad, ldy=ldy, dtype=_dtype(kind), variant=variant)
        ry, rvt, ym, vm = ref.epilogue_ref(x, w, bias, kind, "qkv_vt", B, T, H, Tpad=Tpad, ldy=ldy)
        assert (vb[..., T:] == SENTINEL).all(), "a V^T column t >= T was written"
        assert (yb[:, 2 * D:] == SENTINEL).all(), "a y column >= 2D was written"
        assert (yb[:, :2 * D] != SENTINEL).all() and (vb[..., :T] != SENTINEL).all(), "an in-range element was not written"
        assert np.array_equal(yb != SENTINEL, ym) and np.array_equal(vb != SENTINEL, vm)
        tag = f"qkv_vt {kind} variant {variant} B={B} T={T} H={H} K={K} ldy={ldy} Tpad={Tpad}"
        _check_values(tag + " q|k", y, ry, ym, kind)
        _check_values(tag + " V^T", vt, rvt, vm, kind)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("variant", cases.VARIANTS)
@pytest.mark.parametrize("B,T,H,K", cases.HEADMAJOR_SHAPES)
def test_headmajor_epilogue(ctx, B, T, H, K, variant, kind):
    from mlx_swift_audio_amd import ops
    x, w, bias = cases.gemm_inputs(B * T, H * 64, K)
    y0 = np.full((B, H, T, 64), SENTINEL, np.uint16)
    yb, _, y, _ = ops.linear_epi(ctx, x, w, bias, y0, None, epi=ops.EPI_HEADMAJOR, T=T, H=H, dtype=_dtype(kind), variant=variant)
    want, _, mask, _ = ref.epilogue_ref(x, w, bias, kind, "headmajor", B, T, H)
    assert (yb != SENTINEL).all(), "an element was not written"
    _check_values(f"headmajor {kind} variant {variant} B={B} T={T} H={H} K={K}", y, want, mask, kind)


def test_linear_epi_rejects_bad_arguments(ctx):
    """refused by mia_gemm_check or by the hook's own size checks, before anything is copied or launched"""
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import ops
    B, T, H, K = 1, 8, 1, 64
    x, w, bias = cases.gemm_inputs(B * T, 3 * H * 64, K)
    y0, vt0 = np.full((B * T, 128), SENTINEL, np.uint16), np.full((B, H, 64, 64), SENTINEL, np.uint16)
    ok = dict(epi=ops.EPI_QKV_VT, T=T, H=H, Tpad=64)
    yb, vb, _, _ = ops.linear_epi(ctx, x, w, bias, y0, vt0, **ok)                 # the baseline the refusals vary is accepted
    assert (yb != SENTINEL).all() and (vb[..., :T] != SENTINEL).all()
    for bad in (dict(T=2), dict(T=6, Tpad=64), dict(N=2 * H * 64), dict(H=2), dict(Tpad=4), dict(Tpad=66), dict(out_f32=True), dict(batch=2),
                dict(T=3), dict(ldy=124), dict(ldy=130), dict(epi=0), dict(epi=3), dict(variant=5)):
        with pytest.raises(m.MiaError) as e:
            ops.linear_epi(ctx, x, w, bias, y0, vt0, **{**ok, **bad})
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, bad
    hx, hw, hb = cases.gemm_inputs(8, 64, 64)
    hy = np.full((1, 1, 8, 64), SENTINEL, np.uint16)
    assert (ops.linear_epi(ctx, hx, hw, hb, hy, None, epi=ops.EPI_HEADMAJOR, T=8, H=1)[0] != SENTINEL).all()
    for bad in (dict(H=2), dict(T=3), dict(out_f32=True), dict(batch=2)):
        with pytest.raises(m.MiaError) as e:
            ops.linear_epi(ctx, hx, hw, hb, hy, None, **{**dict(epi=ops.EPI_HEADMAJOR, T=8, H=1), **bad})
        assert e.value.code == m._lib.ERR_INVALID_ARGUMENT, bad
    with pytest.raises(m.MiaError):                                               # QKV_VT without its second destination
        ops.linear_epi(ctx, x, w, bias, y0, None, **ok)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_qkv_gemm_then_attention_on_device(ctx, kind):
    """The encoder's pair end to end in device memory, as whisper_encode.hip runs it: V^T is zeroed once at allocation and never again; the
    QKV_VT GEMM fills q | k and V^T columns [0, T); the attention reads them.  The GEMM's outputs are held to epilogue_bound, and the
    attention to attention_bound against the fp64 reference FED THE GEMM'S OWN 16-bit q / k / v (so the bound needs no term for their
    rounding).  Then the same buffers take a shorter pass, T = 36: the GEMM leaves the first pass's V^T columns [36, 100) as they are, the
    attention reads [36, 64) of them under zero weights -- stale but finite, which is all the kernel needs -- and must not read further."""
    from mlx_swift_audio_amd import ops
    dtype = _dtype(kind)
    B, H, K, Tpad = 2, 2, 128, 128
    D = H * 64
    ld_qk, ld_out = 2 * D + 8, D + 4
    x, w, bias = cases.gemm_inputs(B * 100, 3 * D, K)

    def dev16(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()

    def host16(t):
        return t.cpu().numpy().view(np.uint16)

    dw, db = dev16(ops.bits16(w, dtype)), torch.from_numpy(bias).cuda()
    qk = dev16(np.zeros((B * 100, ld_qk), np.uint16))
    vt = dev16(np.zeros((B, H, 64, Tpad), np.uint16))                             # zeroed once
    stale = None
    for T in (100, 36):
        M = B * T
        dx = dev16(ops.bits16(x[:M], dtype))
        out = dev16(np.full((M, ld_out), SENTINEL, np.uint16))
        ops.linear_epi_device(ctx, dx, dw, db, qk, vt, M=M, N=3 * D, K=K, epi=ops.EPI_QKV_VT, T=T, H=H, Tpad=Tpad, ldy=ld_qk, dtype=dtype)
        ops.attention_h64_device(ctx, qk, vt, out, B, T, H, Tpad, ld_qk, ld_out, dtype)
        qkb, vtb, outb = host16(qk).reshape(-1)[:M * ld_qk].reshape(M, ld_qk), host16(vt), host16(out)
        ry, rvt, ym, vm = ref.epilogue_ref(x[:M], w, bias, kind, "qkv_vt", B, T, H, Tpad=Tpad, ldy=ld_qk)
        _check_values(f"chained {kind} T={T} q|k", ops.from_bits16(qkb, dtype), ry, ym, kind)
        _check_values(f"chained {kind} T={T} V^T", ops.from_bits16(vtb, dtype), rvt, vm, kind)
        if stale is None:
            assert not vtb[..., T:].any() and not qkb[:, 2 * D:].any()           # never written: still the allocation's zeros
            stale = vtb.copy()
        else:
            assert np.array_equal(vtb[..., T:], stale[..., T:]) and stale[..., T:100].any() and not vtb[..., 100:].any()
        q16, k16 = ops.from_bits16(qkb[:, :D], dtype), ops.from_bits16(qkb[:, D:2 * D], dtype)
        v16 = ops.from_bits16(np.ascontiguousarray(vtb[..., :T].transpose(0, 3, 1, 2)).reshape(M, D), dtype)
        want, vmax = ref.attention_ref(q16, k16, v16, B, T, H, kind)
        got = ops.from_bits16(outb, dtype)
        assert (outb[:, D:] == SENTINEL).all() and np.isfinite(got[:, :D]).all()
        err, bound = np.abs(got[:, :D] - want), ref.attention_bound(want, vmax, kind, B, T, H)
        print(f"chained {kind} T={T} attention: worst err/bound {(err / bound).max():.3f}")
        assert (err <= bound).all()
