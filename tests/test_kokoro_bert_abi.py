"""mia_kokoro_bert_config of include/mia_kokoro.h against its ctypes mirror, field for field (no GPU needed).  The entry points
themselves are covered by test_abi_table.py (header against the ctypes table) and test_abi_symbols.py (header against the library)."""
import ctypes as C
import os
import re

from _abi_header import parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_mirror_matches_the_header_field_for_field():
    from mlx_swift_audio_amd import _abi
    text = open(os.path.join(ROOT, "include", "mia_kokoro.h")).read()
    text, n = re.subn(r"struct\s+mia_kokoro_bert_config\s*\{(.*?)\}\s*;", r"typedef struct {\1} mia_kokoro_bert_config;", text, flags=re.S)
    fields = parse(re.sub(r'^\s*#.*$', " ", text, flags=re.M))[1]["mia_kokoro_bert_config"]
    assert n == 1 and all(t is C.c_int for _, t in _abi.KokoroBertConfig._fields_)
    assert [(f, "i32", 0) for f, _ in _abi.KokoroBertConfig._fields_] == fields
    assert [f for f, _, _ in fields] == ["vocab", "embed", "hidden", "heads", "intermediate", "n_layers", "max_positions", "type_vocab", "out_dim"]
    assert C.sizeof(_abi.KokoroBertConfig) == 4 * len(fields)
