"""Resource guard for the Mimi kernels (no GPU needed: hipcc cross-compiles gfx950): the five kernels of mimi_kernels.hip and the three
tap-GEMM instantiations that carry the ELU prologue and the tanh-form GELU compile without spills or scratch, keep their static LDS
within the 160 KB of a CU and stay within the 168 VGPRs of three waves per SIMD.  There is no 128 x 128 tile among them: the plain one
sits at exactly 168 VGPRs and the additions took it to 324, so those launches run on the 128 x 64 tile (codec_kernels.hip)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MIMI_KERNELS = ("mimi_embed", "mimi_upsample", "mimi_qkv_finish", "mimi_window_attn", "mimi_conv_out1")


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


def _clean(name, r):
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
    assert r["group_segment_fixed_size"] <= 160 * 1024, (name, r)


def test_mimi_kernels_compile_without_spills_and_fit_lds():
    res = _kernels("mimi_kernels.hip")
    for k in MIMI_KERNELS:
        found = [(n, r) for n, r in res.items() if k in n]
        assert len(found) == 1, (k, sorted(res))
        _clean(*found[0])


def test_elu_gelu_tap_gemm_instantiations():
    res = _kernels("codec_kernels.hip")
    plain = {n: r for n, r in res.items() if "conv_gemm_f32" in n and "Lb0EEEv" in n}
    mimi = {n: r for n, r in res.items() if "conv_gemm_f32" in n and "Lb1EEEv" in n}
    assert len(plain) == 4 and len(mimi) == 3, sorted(res)
    assert not [n for n in mimi if "conv_gemm_f32ILi2ELi2ELi1E" in n]
    for n, r in mimi.items():
        _clean(n, r)
        assert r["vgpr_count"] <= 168, (n, r)
