"""CPU checks of what tests/test_enc_attn_gpu.py and tests/test_gemm_epilogues_gpu.py rest on (no GPU):
  * the fp64 attention reference equals torch's scaled_dot_product_attention;
  * every spiked case has the structure it claims, by the plain restatement of the kernel's reference-point rule (tile_rule);
  * every comparison can fail: each deliberately wrong reference leaves the bound of the case built to see it by at least 100 x, in both
    16-bit types, when the right reference (rounded to the type, as a perfect kernel would store it) stands in for the kernel."""
import numpy as np
import pytest

import _enc_attn_cases as cases
import _enc_attn_ref as ref

HEAD, D0 = cases.HEAD, cases.D0


def _rule(case, kind="bf16"):
    cols = case.cols()
    return ref.tile_rule(ref.round16(case.q[:, cols], kind), ref.round16(case.k[:, cols], kind))


def test_constants_read_from_the_kernel():
    assert ref.kernel_constants() == (64, 8.0)


@pytest.mark.parametrize("B,T,H", [(1, 1, 1), (2, 65, 3), (1, 257, 2)])
def test_reference_equals_torch_sdpa(B, T, H):
    import torch
    q, k, v = cases.random_qkv(B, T, H, 3)
    out, vmax = ref.attention_ref(q, k, v, B, T, H, "f16")
    tq, tk, tv = (torch.from_numpy(ref.round16(a, "f16")).reshape(B, T, H, 64).transpose(1, 2) for a in (q, k, v))
    want = torch.nn.functional.scaled_dot_product_attention(tq, tk, tv).transpose(1, 2).reshape(B * T, H * 64).numpy()
    assert want.dtype == np.float64
    assert np.abs(out - want).max() <= 1e-12
    assert vmax.shape == (B, H) and np.isclose(vmax.max(), np.abs(ref.round16(v, "f16")).max())


@pytest.mark.parametrize("name", sorted(cases.spiked_cases()))
def test_tiled_walk_equals_plain_softmax(name):
    """the online softmax under the lazy rule is the same function (so `no_rescale` differs from it by the missing rescale alone)"""
    c = cases.spiked_cases()[name]
    cols = c.cols()
    qh, kh, vh = (ref.round16(a[:, cols], "bf16") for a in (c.q, c.k, c.v))
    plain = ref.attention_ref(c.q, c.k, c.v, 1, c.T, 2, "bf16")[0][:, cols]
    assert np.abs(ref._tiled(qh, kh, vh) - plain).max() <= 1e-12


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_spiked_cases_are_what_they_claim(kind):
    """All decisions the claims rest on are at least half a log2 unit away from the threshold, so the kernel's fp32 scores decide alike."""
    cs = cases.spiked_cases()
    assert all(c.T <= 321 for c in cs.values())

    r = _rule(cs["three_moves"], kind)
    i = cs["three_moves"].query
    assert r["moved"][i, 0] and r["moved"][i, 1:].sum() >= 3                                   # (a)
    assert r["margin"][i].min() > 0.5

    r = _rule(cs["large_p"], kind)
    i = cs["large_p"].query
    assert not r["moved"][i, 1:].any() and 7.0 <= r["log2p"][i].max() < 8.0                   # (b)
    assert r["margin"][i, 1:].min() > 0.25 and r["log2p"][i].max() - 7.0 > 0.25

    r = _rule(cs["one_lane"], kind)
    i = cs["one_lane"].query
    wave = slice(i // 32 * 32, i // 32 * 32 + 32)
    assert i // 128 == 1 and (i % 128) // 32 == 1                                              # block 1, wave 1
    tiles = [j for j in range(1, r["moved"].shape[1]) if r["moved"][wave, j].sum() == 1]       # (c)
    assert tiles == [2] and r["moved"][i, 2]
    assert r["margin"][wave].min() > 0.5

    c = cs["underflow"]
    r = _rule(c, kind)
    i = c.query
    cc = ref.SCALE * np.log2(np.e)
    assert r["raw"][i, :64].max() == r["raw"][i].max()                                         # (d)
    assert (r["raw"][i, :64].max() - r["raw"][i, 64:].max()) * cc > 24.0 + 8.0
    assert not r["moved"][i, 1:].any()

    c = cs["tail_move"]
    r = _rule(c, kind)
    i = c.query
    assert c.T % 64 != 0 and r["moved"][i, -1] and not r["moved"][i, 1:-1].any()               # (e)
    assert r["margin"][i].min() > 0.5
    assert int(np.argmax(r["raw"][i])) == c.T - 1                                              # ... on the last key

    c = cs["plateau"]
    r = _rule(c, kind)
    top = np.sort(r["raw"][c.query])[::-1]
    assert np.ptp(top[1:9]) == 0.0 and 3.0 < top[0] - top[1] < 5.0 and (top[1] - top[9]) * cc > 10.0


# wrong reference -> the case that has to see it
SEES = {"drop_last_key": "tail_move", "swap23_v": "large_p", "no_rescale": "three_moves", "scale_twice": "large_p", "scale_none": "plateau"}


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("wrong", sorted(SEES))
def test_every_attention_comparison_can_fail(wrong, kind):
    c = cases.spiked_cases()[SEES[wrong]]
    good, vmax = ref.attention_ref(c.q, c.k, c.v, 1, c.T, 2, kind)
    kernel = ref.round16(good, kind)                                  # what a perfect kernel stores
    assert (np.abs(kernel - good) <= ref.attention_bound(good, vmax, kind, 1, c.T, 2)).all()
    bad = ref.attention_ref(c.q, c.k, c.v, 1, c.T, 2, kind, wrong=wrong)[0]
    ratio = np.abs(kernel - bad) / ref.attention_bound(bad, vmax, kind, 1, c.T, 2)
    i = c.query
    print(f"{wrong} on {c.name} {kind}: err/bound {ratio[i].max():.0f} at query {i}, column {int(np.argmax(ratio[i]))}")
    assert ratio[i, HEAD * 64 + D0] >= 100.0


@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("wrong", ["tpad_is_t", "hd_swapped"])
def test_every_epilogue_comparison_can_fail(wrong, kind):
    B, T, H, K = cases.QKV_SHAPES[1]
    x, w, bias = cases.gemm_inputs(B * T, 3 * H * 64, K)
    y, vt, ym, vm = ref.epilogue_ref(x, w, bias, kind, "qkv_vt", B, T, H, Tpad=128, ldy=2 * H * 64 + 4)
    assert ym.sum() == B * T * 2 * H * 64 and vm.sum() == B * T * H * 64 and not vm[..., T:].any() and not ym[:, 2 * H * 64:].any()
    assert (np.abs(ref.round16(vt, kind) - vt) <= ref.epilogue_bound(vt, kind)).all()
    bad = ref.epilogue_ref(x, w, bias, kind, "qkv_vt", B, T, H, Tpad=128, ldy=2 * H * 64 + 4, wrong=wrong)[1]
    assert (np.abs(ref.round16(vt, kind) - bad) / ref.epilogue_bound(bad, kind)).max() >= 100.0
    if wrong == "hd_swapped":
        B, T, H, K = cases.HEADMAJOR_SHAPES[0]
        x, w, bias = cases.gemm_inputs(B * T, H * 64, K)
        good = ref.epilogue_ref(x, w, bias, kind, "headmajor", B, T, H)[0]
        bad = ref.epilogue_ref(x, w, bias, kind, "headmajor", B, T, H, wrong=wrong)[0]
        assert good.shape == (B, H, T, 64)
        assert (np.abs(ref.round16(good, kind) - bad) / ref.epilogue_bound(bad, kind)).max() >= 100.0


def test_epilogue_reference_layout_by_hand():
    """the scatter formulas of gemm.hip, element by element on a small shape"""
    B, T, H, K, Tpad, ldy = 2, 4, 2, 64, 8, 2 * 128 + 4
    x, w, bias = cases.gemm_inputs(B * T, 3 * H * 64, K)
    full = ref.round16(x, "f16") @ ref.round16(w, "f16").T + bias.astype(np.float64)
    y, vt, _, _ = ref.epilogue_ref(x, w, bias, "f16", "qkv_vt", B, T, H, Tpad=Tpad, ldy=ldy)
    hm = ref.epilogue_ref(x, w[:H * 64], bias[:H * 64], "f16", "headmajor", B, T, H)[0].ravel()
    flat = vt.ravel()
    for b in range(B):
        for t in range(T):
            m = b * T + t
            assert np.array_equal(y[m, :2 * H * 64], full[m, :2 * H * 64])
            for h in range(H):
                for d in range(64):
                    assert flat[((b * H + h) * 64 + d) * Tpad + t] == full[m, 2 * H * 64 + h * 64 + d]
                    assert hm[((b * H + h) * T + t) * 64 + d] == full[m, h * 64 + d]
