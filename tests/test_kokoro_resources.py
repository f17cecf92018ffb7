"""Resource guard for the Kokoro kernels (no GPU needed: hipcc cross-compiles gfx950): every kernel of kokoro_kernels.hip compiles
without spilled registers or private segment and keeps its static LDS within the 160 KB of a CU.  Only the resource metadata of the
assembly is read.  (Kokoro adds no instantiation of the tap GEMM: AdaIN is materialised, so codec_kernels.hip is what it was.)"""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# kernel name -> instances
KOKORO_KERNELS = {"kokoro_style_rows": 1, "kokoro_inorm_partial": 1, "kokoro_inorm_final": 1, "kokoro_adain_act": 2, "kokoro_pool": 1,
                  "kokoro_pack": 1, "kokoro_curve_cols": 1, "kokoro_phase_scan": 1, "kokoro_source": 1, "kokoro_stft": 1,
                  "kokoro_istft_frames": 1, "kokoro_overlap_add": 1}


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


def test_kokoro_kernels_compile_without_spills_and_fit_lds():
    res = _kernels("kokoro_kernels.hip")
    assert len(res) == sum(KOKORO_KERNELS.values()), sorted(res)
    for k, n in KOKORO_KERNELS.items():
        found = [(name, r) for name, r in res.items() if k in name]
        assert len(found) == n, (k, sorted(res))
        for name, r in found:
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
            assert r["group_segment_fixed_size"] <= 160 * 1024, (name, r)
