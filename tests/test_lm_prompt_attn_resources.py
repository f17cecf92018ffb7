"""Resource guard for lm_prefill_attn.hip (no GPU needed: hipcc cross-compiles gfx950): every instantiation -- bf16 / f16 x head dim
64 / 128 x 4 / 2 / 1 query heads per workgroup, twelve in all -- compiles without VGPR or SGPR spills and without a private segment, and
its LDS (all static: two K + V^T buffers, 32 KB at head dim 64, 64 KB at 128; the launch adds none) stays within the 160 KB of a CU."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_lm_prefill_attn_compiles_without_spills_and_fits_lds():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    csrc = os.path.join(ROOT, "mlx-swift-audio_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(csrc, "lm_prefill_attn.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    launch_lds = 0                                            # lm_prefill_attn_launch passes no dynamic LDS
    assert re.search(r"lm_prefill_attn_kernel<TT, DD, GG>\), grid, block, 0, s,", open(os.path.join(csrc, "lm_prefill_attn.hip")).read())
    found = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "lm_prefill_attn_kernel" not in name:
            continue
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
        found.append(name)
        print(name, "vgpr", get("vgpr_count"), "agpr", get("agpr_count"), "lds", get("group_segment_fixed_size"))
        assert get("vgpr_spill_count") == 0 and get("sgpr_spill_count") == 0 and get("private_segment_fixed_size") == 0, name
        assert get("group_segment_fixed_size") + launch_lds <= 160 * 1024, name
        assert get("vgpr_count") <= 512, name
    assert len(found) == 12, found          # (bf16, f16) x (64, 128) x (4, 2, 1)
