"""Resource guards of audio_trim.hip (no GPU needed: hipcc cross-compiles gfx950): neither kernel spills registers or uses private
memory, and the static LDS of both is a few hundred bytes."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "audio_trim.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    res = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                     for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")}
    return res


def test_no_kernel_spills_or_uses_private_memory():
    res = _resources()
    names = sorted(res)
    assert len(names) == 2, names
    for want in ("frame_energy_kernel", "bounds_finish_kernel"):
        assert any(want in n for n in names), (want, names)
    for n, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
        assert r["group_segment_fixed_size"] <= 1024, (n, r)
    finish = next(r for n, r in res.items() if "bounds_finish_kernel" in n)
    assert finish["vgpr_count"] <= 128, finish                    # 1024 threads = 4 waves per SIMD: 512 / 4
