"""Resource guard for the Mimi encode kernels (no GPU needed: hipcc cross-compiles gfx950): each kernel of mimi_encode_kernels.hip is
found once, compiles without spills or scratch and keeps its static LDS within the 160 KB of a CU; the chain-stage kernel also stays
within the 168 VGPRs of three waves per SIMD (its dynamic LDS, the [32][dq + 4] residual tile, is bounded to 64 KB by its launcher)."""
from test_mimi_resources import _clean, _kernels

ENCODE_KERNELS = ("mimi_edge_rows", "mimi_rvq_stage", "mimi_rvq_finish")


def test_mimi_encode_kernels_compile_without_spills_and_fit_lds():
    res = _kernels("mimi_encode_kernels.hip")
    for k in ENCODE_KERNELS:
        found = [(n, r) for n, r in res.items() if k in n]
        assert len(found) == 1, (k, sorted(res))
        _clean(*found[0])
        if k == "mimi_rvq_stage":
            assert found[0][1]["vgpr_count"] <= 168, found[0]
