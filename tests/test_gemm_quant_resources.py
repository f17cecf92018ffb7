"""Resource guard for gemm_quant.hip (no GPU needed: hipcc cross-compiles gfx950): every instantiation -- bf16 / f16 x 4 / 6 / 8 bits x
1 / 2 / 4 row tiles per wave, eighteen in all -- compiles without VGPR or SGPR spills and without a private segment (zero scratch
bytes), and uses no LDS at all: a workgroup is one wave that holds its activation rows as MFMA fragments, and the launch adds none."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_gemm_quant_compiles_without_scratch_and_without_lds():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mlx-swift-audio_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "gemm_quant.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    src = open(os.path.join(csrc, "gemm_quant.hip")).read()
    assert len(re.findall(r"dim3\(64\), 0, s, a\)", src)) == 3 and "__shared__" not in src      # every launch: one wave, no dynamic LDS
    found = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "gemm_quant_k" not in name:
            continue
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        found.append(name)
        print(name, "vgpr", get("vgpr_count"), "agpr", get("agpr_count"), "lds", get("group_segment_fixed_size"))
        assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") == 0, name
        assert get("vgpr_count") <= 512, name
    assert len(found) == 18, found          # (bf16, f16) x (4, 6, 8 bit) x (1, 2, 4 row tiles)
