"""Resource guard of the packed Whisper step kernels (no GPU needed: hipcc cross-compiles gfx950): no variant of dec_skinny_fq may spill
to scratch, the at-most-16-row variants (the reference's own batch sizes) must keep 3 waves per SIMD (<= 168 registers), the 32-row
one-tile variants 2 waves (<= 256), and the four-tile logits variant must fit the 512 registers of a lone wave.  LDS is the cross-wave
reduction alone: (NW - 1) x 2 KB at one tile per wave."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "mlx-swift-audio_amd", "csrc", "skinny_frag_quant.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        text = open(out).read()
    res = []
    for blk in re.findall(r"- \.agpr_count:.*?\.wavefront_size", text, re.S):
        def num(key):
            return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        m = re.search(r"dec_skinny_fqI\d+\w+?Li(\d)ELi(\d)ELi(\d)ELb(\d)ELi(\d)E", name)
        if m:
            mode, nt, nw, m16, planes = map(int, m.groups())
            res.append(dict(name=name, mode=mode, nt=nt, nw=nw, m16=m16, planes=planes, regs=num("vgpr_count"), spill=num("vgpr_spill_count"),
                            scratch=num("private_segment_fixed_size"), lds=num("group_segment_fixed_size")))
    return res


def test_every_variant_is_there_and_none_spills(kernels):
    # 2 storage types x (SK_OUT16, SK_PARTIAL, SK_QKV: 5 wave counts x 2 row counts x 2 widths; SK_OUTF32: 5 x 2 at <= 16 rows + 2 four-tile)
    assert len(kernels) == 2 * (3 * 5 * 2 * 2 + 5 * 2 + 2), len(kernels)
    for k in kernels:
        assert k["spill"] == 0 and k["scratch"] == 0, k
        assert k["lds"] == (k["nw"] - 1) * k["nt"] * 2048, k


def test_register_budgets(kernels):
    for k in kernels:
        if k["nt"] == 4:
            assert k["nw"] == 1 and k["regs"] <= 512, k
        elif k["m16"]:
            assert k["regs"] <= 168, k            # 3 waves per SIMD
        else:
            assert k["regs"] <= 256, k            # 2 waves per SIMD
