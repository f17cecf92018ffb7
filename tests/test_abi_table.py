"""The ctypes table of mlx_swift_audio_amd/_abi.py against include/mia.h: every function, argument, return type, struct field and
array length; that the check itself can fail; that the loaded library carries the table; and that nothing else declares prototypes."""
import glob
import os
import re

import pytest

from _abi_header import compare, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mia.h")).read()
STRUCT_NAMES = {"mia_conv_gemm_desc", "mia_skinny_desc", "mia_whisper_dims", "mia_tensor_view", "mia_decode_opts", "mia_snac_config",
                "mia_dac_config", "mia_dac_encoder_config", "mia_lm_config", "mia_lm_sampler", "mia_ras_params", "mia_sensevoice_config",
                "mia_s3_config", "mia_hift_config", "mia_flow_config"}


def _abi():
    import mlx_swift_audio_amd as m   # noqa: F401
    from mlx_swift_audio_amd import _abi
    return _abi


def test_table_matches_header():
    abi = _abi()
    assert compare(HEADER, abi.PROTOTYPES, abi.STRUCTS) == []


def test_header_parse_floor():
    functions, structs = parse(HEADER)
    assert len(functions) >= 128
    assert set(structs) == STRUCT_NAMES
    assert structs["mia_skinny_desc"][10:16] == [(n, "i32", 0) for n in ("M", "N", "K", "S", "mode", "dtype")]   # one multi-declarator line
    assert ("shape", "i64", 4) in structs["mia_tensor_view"] and ("name", "str", 0) in structs["mia_tensor_view"]
    assert functions["mia_version"] == ("str", []) and functions["mia_dp_available"] == ("i32", [])
    assert functions["mia_op_skinny_gemm"] == ("i32", ["ptr", "struct:mia_skinny_desc"])


def _sub(pattern, repl):
    text, n = re.subn(pattern, repl, HEADER)
    assert n == 1, pattern
    return text


DOCTORED = {
    "argument dropped": ("mia_flow_inference_batch", lambda: _sub(r"float\* const\* mel, int mem\);", "float* const* mel);")),
    "int64_t lda -> int": ("mia_op_linear", lambda: _sub(r"(mia_op_linear\(mia_ctx\* ctx, const void\* x, )int64_t lda", r"\1int lda")),
    "handle returned as int": ("mia_lm_load", lambda: _sub(r"mia_lm\* mia_lm_load\(", "int mia_lm_load(")),
    "fields swapped": ("mia_decode_opts", lambda: _sub(r"int32_t n_initial;(\s*)int32_t per_clip_initial;",
                                                       r"int32_t per_clip_initial;\1int32_t n_initial;")),
    "shape[4] -> shape[3]": ("mia_tensor_view", lambda: _sub(r"int64_t shape\[4\];", "int64_t shape[3];")),
    "function added": ("mia_new_entry", lambda: _sub(r"(int mia_synchronize\(mia_ctx\* ctx\);)", r"\1 int mia_new_entry(mia_ctx* ctx, int x);")),
}


@pytest.mark.parametrize("case", sorted(DOCTORED))
def test_check_can_fail(case):
    abi = _abi()
    name, doctor = DOCTORED[case]
    found = compare(doctor(), abi.PROTOTYPES, abi.STRUCTS)
    assert found and all(s.startswith(name + ":") for s in found), found


def test_unknown_type_is_an_error():
    with pytest.raises(ValueError, match="closed set"):
        parse(_sub(r"int mia_synchronize\(mia_ctx\* ctx\);", "int mia_synchronize(mia_ctx* ctx, size_t n);"))
    with pytest.raises(ValueError, match="closed set"):
        parse(_sub(r"int64_t shape\[4\];", "unsigned shape[4];"))


def test_loaded_library_carries_the_table():
    import mlx_swift_audio_amd as m
    abi = _abi()
    lib = m._lib.load()
    assert m._lib.load() is lib
    for name, (restype, argtypes) in abi.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert list(fn.argtypes) == argtypes, name


def test_stale_library_fails_at_load():
    class Stale:
        _name = "libmia.so"

        def __getattr__(self, name):
            if name == "mia_op_skinny_gemm":
                raise AttributeError(name)
            return type("Fn", (), {})()
    with pytest.raises(ImportError, match="mia_op_skinny_gemm"):
        _abi().apply(Stale())


def test_prototypes_live_in_one_place():
    files = [f for d in ("mlx-swift-audio_amd", "tools", "tests") for f in glob.glob(os.path.join(ROOT, d, "*.py"))]
    assert len(files) > 100
    allowed = {os.path.join(ROOT, "mlx-swift-audio_amd", "_abi.py"), os.path.join(ROOT, "tests", "_abi_header.py")}
    assign = re.compile(r"\.(?:argtypes|restype)\s*=(?!=)")
    flag = re.compile(r"""["']_\w+_declared["']|\._\w+_declared\b""")
    bad = []
    for f in sorted(set(files) - allowed):
        for i, line in enumerate(open(f), 1):
            if assign.search(line) or flag.search(line):
                bad.append(f"{os.path.relpath(f, ROOT)}:{i}: {line.strip()}")
    assert bad == []
