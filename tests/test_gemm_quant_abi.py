"""mia_op_gemm_quant and the LM / Marvis entry points of the packed prompt pass are declared in include/mia.h, listed in the ctypes table
with the header's types and exported by the built library; the descriptor of include/mia_gemm_quant.h (mia.h only declares its type) and
its ctypes mirror agree field for field; the Python surface is there (no GPU needed)."""
import ctypes as C
import os
import re

from _abi_header import parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mia.h")).read()
DESC_HEADER = open(os.path.join(ROOT, "include", "mia_gemm_quant.h")).read()
ENTRY_POINTS = {
    "mia_op_gemm_quant": ("i32", ["ptr", "ptr"]),
    "mia_lm_set_prompt_weights": ("i32", ["ptr", "i32"]),
    "mia_lm_release_dense": ("i32", ["ptr"]),
    "mia_lm_weight_bytes": ("i32", ["ptr", "ptr", "ptr"]),
    "mia_marvis_use_packed_prompt": ("i32", ["ptr", "i32"]),
    "mia_marvis_release_dense": ("i32", ["ptr"]),
}
FIELDS = [("A", "ptr", 0), ("lda", "i64", 0), ("wfrag", "ptr", 0), ("stfrag", "ptr", 0), ("bits", "i32", 0), ("C", "ptr", 0), ("ldc", "i64", 0),
          ("R", "ptr", 0), ("ldr", "i64", 0), ("M", "i32", 0), ("N", "i32", 0), ("K", "i32", 0), ("dtype", "i32", 0)]


def _desc_fields():
    """The fields of `struct mia_gemm_quant_desc { ... };`, read with the header parser (which takes the typedef form)."""
    text, n = re.subn(r"struct\s+mia_gemm_quant_desc\s*\{(.*?)\}\s*;", r"typedef struct {\1} mia_gemm_quant_desc;", DESC_HEADER, flags=re.S)
    assert n == 1
    text = re.sub(r'^\s*#.*$', " ", text, flags=re.M)
    return parse(text)[1]["mia_gemm_quant_desc"]


def test_header_declares_the_entry_points():
    functions, structs = parse(HEADER)
    for name, sig in ENTRY_POINTS.items():
        assert functions.get(name) == sig, name
    assert re.search(r"typedef\s+struct\s+mia_gemm_quant_desc\s+mia_gemm_quant_desc\s*;", HEADER) and "mia_gemm_quant_desc" not in structs
    assert _desc_fields() == FIELDS


def test_descriptor_mirror_matches_the_header_field_for_field():
    from mlx_swift_audio_amd import _abi
    kind = {C.c_void_p: "ptr", C.c_int64: "i64", C.c_int: "i32"}
    assert [(f, kind[t], 0) for f, t in _abi.GemmQuantDesc._fields_] == _desc_fields()
    # natural alignment, as the C compiler lays it out: bits and the four trailing ints pad to 8
    assert C.sizeof(_abi.GemmQuantDesc) == 88
    assert _abi.GemmQuantDesc.C.offset == 40 and _abi.GemmQuantDesc.M.offset == 72


def test_table_lists_them_and_the_library_exports_them():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import _abi
    lib = m._lib.load()
    for name in ENTRY_POINTS:
        assert name in _abi.PROTOTYPES, name
        assert getattr(lib, name).argtypes is not None, name
    assert "mia_gemm_quant_desc" not in _abi.STRUCTS


def test_python_surface():
    import inspect

    import mlx_swift_audio_amd  # noqa: F401
    from mlx_swift_audio_amd import lm, marvis, ops, outetts
    for f in ("set_prompt_weights", "release_dense", "weight_bytes"):
        assert callable(getattr(lm.CausalLM, f))
    for f in ("use_packed_prompt", "release_dense"):
        assert callable(getattr(marvis.MarvisModel, f))
    assert callable(ops.gemm_quant)
    # nothing is switched on by default: the keyword forwards only when given
    assert inspect.signature(outetts.OuteTTS.__init__).parameters["packed_prompt"].default is None
    assert inspect.signature(lm.OrpheusTTS.__init__).parameters["packed_prompt"].default is None
