"""The staging rule of the C ABI lives in csrc/host_io.h alone: no other file of csrc/ spells the memory kinds, the header's `int mem`
entry points are all found, the GPU parity module names every one of them, and the check itself can fail."""
import glob
import os
import re

from _abi_header import mem_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlx-swift-audio_amd", "csrc")
HEADER = open(os.path.join(ROOT, "include", "mia.h")).read()
KINDS = re.compile(r"\bMIA_MEM_(?:HOST|DEVICE)\b")


def offenders(sources: dict) -> list:
    """'file:line: text' for every line outside host_io.h that names a memory kind; sources: {file name: text}."""
    return [f"{name}:{i}: {line.strip()}" for name, text in sorted(sources.items()) if name != "host_io.h"
            for i, line in enumerate(text.splitlines(), 1) if KINDS.search(line)]


def _csrc():
    files = glob.glob(os.path.join(CSRC, "*"))
    assert len(files) > 50
    return {os.path.basename(f): open(f).read() for f in files}


def test_memory_kinds_are_named_in_host_io_only():
    src = _csrc()
    assert offenders(src) == []
    assert "MIA_MEM_HOST" in src["host_io.h"] and "MIA_MEM_DEVICE" in src["host_io.h"]


def test_check_can_fail():
    clean = {"a.hip": "HostIo io(ctx, mem);\nif (io.host()) return 1;\n", "host_io.h": "mem == MIA_MEM_HOST"}
    assert offenders(clean) == []
    stray = dict(clean, **{"b.hip": "int f(int mem) {\n  if (mem == MIA_MEM_HOST) return 1;\n  return 0;\n}\n"})
    assert offenders(stray) == ["b.hip:2: if (mem == MIA_MEM_HOST) return 1;"]
    forced = dict(clean, **{"c.hip": "return whisper_decode(w, &o, nullptr, MIA_MEM_DEVICE);  // forced device mode\n"})
    assert [o.split(":")[0] for o in offenders(forced)] == ["c.hip"]


def test_every_mem_entry_point_is_found():
    names = mem_entry_points(HEADER)
    assert len(names) == len(re.findall(r"int mem\)", HEADER)) == 40
    assert len(set(names)) == len(names)
    assert "mia_snac_decode_batch" in names and "mia_op_fsmn_add" in names and "mia_synchronize" not in names
    assert mem_entry_points("int mia_a(mia_ctx* ctx, int mem);\nint mia_b(int mem, int x);\n/* int mia_c(int mem); */") == ["mia_a"]


def test_gpu_parity_module_names_every_entry_point():
    doc = open(os.path.join(ROOT, "tests", "test_host_io_gpu.py")).read().split('"""')[1]
    missing = [n for n in mem_entry_points(HEADER) if not re.search(rf"\b{n}\b", doc)]
    assert missing == []
