"""Resource guards of speaker_features.hip (no GPU needed: hipcc cross-compiles gfx950): no kernel spills VGPRs, and the LDS the FFT
workgroup asks for -- its static part from the code object plus the dynamic float2 [kFftBlock] buffer the launcher requests -- stays
within the 160 KB a gfx950 workgroup can have."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "speaker_features.hip")).read()


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
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "speaker_features.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    res = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1))
                     for k in ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")}
    return res


def test_no_kernel_spills_and_fft_lds_fits():
    res = _resources()
    names = sorted(res)
    for want in ("seg_stats_kernel", "speaker_gain_kernel", "speaker_scale_kernel", "pitch_frames_kernel", "seg_finish_kernel"):
        assert any(want in n for n in names), (want, names)
    fft = [n for n in names if "fft_kernel" in n]
    assert len(fft) == 6, fft                                  # whole / step 1 / step 2, each with the centroid and the spectrum epilogue
    for n, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (n, r)
    log2 = int(re.search(r"constexpr int kFftBlockLog2 = (\d+)", SRC).group(1))
    assert re.search(r"size_t fft_lds\(int log2n\) \{ return sizeof\(float2\) << log2n; \}", SRC)
    for n in fft:
        assert res[n]["vgpr_count"] <= 128, (n, res[n])       # 1024 threads = 4 waves per SIMD: 512 / 4
        assert res[n]["group_segment_fixed_size"] + (8 << log2) <= 160 * 1024, (n, res[n])

