"""Resource guards for every kernel of csrc/attention.hip (no GPU needed: hipcc cross-compiles gfx950; the method of
tests/test_kernel_resources.py, whose <= 168 VGPR guard on the 128-query kernels stays where it is).

No kernel may spill or use scratch: a spill's reload inside the tile loop brings its own s_waitcnt vmcnt(0), which drains the LDS-DMA
ring the counted waits keep in flight.  The 64-query-per-wave kernel is allowed the whole 256-register budget of two waves per SIMD, and
its LDS must let two workgroups share a CU (160 KB): it is launched with no dynamic LDS, so the static size is the whole of it."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "attention.hip")
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), SRC, "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    res = {}
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {f: int(re.search(r"\." + f + r":\s+(\d+)", blk).group(1)) for f in FIELDS}
    return res


def test_every_attention_kernel_is_compiled_in_both_types(kernels):
    for stem, count in (("enc_attention_kernel", 4), ("enc_attn_q64_kernel", 2)):      # 128 queries: two stagings; x {bf16, f16}
        names = [k for k in kernels if stem in k]
        assert len(names) == count, sorted(kernels)
        assert sum("BF16" in k for k in names) == count // 2, names


def test_no_attention_kernel_spills_or_uses_scratch(kernels):
    assert kernels
    for name, r in kernels.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


def test_q64_kernel_fits_two_workgroups_per_cu(kernels):
    ks = {k: r for k, r in kernels.items() if "enc_attn_q64_kernel" in k}
    assert ks and not any("enc_attention_kernel" in k for k in ks), sorted(kernels)
    launch = open(SRC).read()
    assert re.search(r"hipLaunchKernelGGL\(\(enc_attn_q64_kernel<E>\), g256, block, 0, s,", launch), "the q64 launch must pass no dynamic LDS"
    for name, r in ks.items():
        assert r["vgpr_count"] <= 256, (name, r)
        assert r["group_segment_fixed_size"] <= 80 * 1024, (name, r)


def test_ring_kernels_hold_three_slots(kernels):
    """the LDS-DMA forms stage into three 16 KB slots (K | V^T); the register-staged form keeps its two"""
    sizes = sorted({r["group_segment_fixed_size"] for r in kernels.values()})
    assert sizes == [32 * 1024, 48 * 1024], sizes
