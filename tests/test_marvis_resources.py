"""Resource guard for the Marvis kernels (no GPU needed: hipcc cross-compiles gfx950): the masked embedding sum, the frame sampler and the
frame bookkeeping of marvis_kernels.hip compile without spills or scratch and keep their static LDS within the 160 KB of a CU (the
sampler's sort keys are dynamic LDS: at most 64 KB on top, for a row of 8192)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel name -> instances (the two 16-bit types, or one)
MARVIS_KERNELS = {"mv_embed_rows": 2, "mv_sample": 1, "mv_frame_end": 2}


def _kernels(src):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", src), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    res = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
                     for key in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")}
    return res


def test_marvis_kernels_compile_without_spills_and_fit_lds():
    res = _kernels("marvis_kernels.hip")
    assert len(res) == sum(MARVIS_KERNELS.values()), sorted(res)
    for k, n in MARVIS_KERNELS.items():
        found = [(name, r) for name, r in res.items() if k in name]
        assert len(found) == n, (k, sorted(res))
        for name, r in found:
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
            assert r["group_segment_fixed_size"] + (64 * 1024 if k == "mv_sample" else 0) <= 160 * 1024, (name, r)
    sample = next(r for name, r in res.items() if "mv_sample" in name)
    assert sample["vgpr_count"] <= 128, sample          # 1024 threads: one workgroup must fit a CU's register file (512 VGPRs per SIMD lane / 4 waves)
