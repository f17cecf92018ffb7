"""Resource guards of the top-k / top-p sampler kernels of lm_sample_topk.hip (no GPU needed: hipcc cross-compiles gfx950): no kernel spills
registers or uses private memory, and the finishing kernel's static LDS is within what its comment states (16.2 KB)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("tk_hist0", "tk_level", "tk_gather", "tk_finish")


def _resources():
    import shutil
    import subprocess
    import tempfile

    import pytest
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "lm_sample_topk.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    res = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if any(k in name for k in KERNELS):
            res[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                         for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")}
    return res


def test_no_kernel_spills_or_uses_private_memory():
    res = _resources()
    names = sorted(res)
    assert len(names) == 8, names                                  # tk_hist0, tk_level<1..3>, tk_gather, tk_finish<64 | 256 | 1024>
    for want in KERNELS:
        assert any(want in n for n in names), (want, names)
    for n, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
    finish = [r for n, r in res.items() if "tk_finish" in n]
    assert len(finish) == 3
    for r in finish:
        assert r["group_segment_fixed_size"] <= 16600, r           # at 1024 threads: pairs 8 KB + values 4 KB + ids 4 KB + scan scratch
        assert r["vgpr_count"] <= 128, r                           # 1024 threads = 4 waves per SIMD: 512 / 4
    for n, r in res.items():
        if "tk_finish" not in n:
            assert r["group_segment_fixed_size"] <= 8 * 257 * 4 + 8192 + 256, (n, r)     # the histogram copies, or the gather's list
