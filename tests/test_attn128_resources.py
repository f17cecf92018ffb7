"""Resource guard for attn128.hip (no GPU needed: hipcc cross-compiles gfx950): both instantiations compile without VGPR spills or
scratch and keep their static LDS within the 160 KB of a CU.  No register ceiling yet: the kernel runs one workgroup per CU's worth of
registers today (332 VGPRs, LABNOTES.md), and which occupancy it wants has not been measured."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_attn128_compiles_without_spills_and_fits_lds():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "attn128.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    found = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "attn128_kernel" not in name:
            continue
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        found.append(name)
        assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") <= 160 * 1024, name
        assert get("vgpr_count") <= 512, name
    assert len(found) == 2, found          # bf16 and f16
