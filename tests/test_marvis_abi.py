"""The Marvis entry points are declared in include/mia.h, listed in the ctypes table with the header's types, and exported by the built
library; the configuration record of include/mia_marvis.h (mia.h only declares its type) and its ctypes mirror agree field for field
(no GPU needed)."""
import ctypes as C
import os
import re

from _abi_header import parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mia.h")).read()
CONFIG_HEADER = open(os.path.join(ROOT, "include", "mia_marvis.h")).read()
ENTRY_POINTS = {
    "mia_marvis_load": ("ptr", ["ptr", "ptr", "struct:mia_tensor_view", "i32", "i32", "ptr"]),
    "mia_marvis_free": ("void", ["ptr"]),
    "mia_marvis_reset": ("i32", ["ptr"]),
    "mia_marvis_set_debug": ("i32", ["ptr", "i32"]),
    "mia_marvis_set_batch": ("i32", ["ptr", "i32"]),
    "mia_marvis_generate_batch": ("i32", ["ptr", "ptr", "ptr", "ptr", "i32", "i32", "f32", "f32", "i32", "ptr", "ptr", "ptr"]),
    "mia_marvis_frame": ("i32", ["ptr", "ptr", "ptr", "i32", "i32", "f32", "f32", "ptr", "ptr", "ptr", "ptr"]),
    "mia_marvis_generate": ("i32", ["ptr", "ptr", "ptr", "i32", "i32", "f32", "f32", "i32", "ptr", "ptr", "ptr"]),
    "mia_sample_top_p_ascending": ("i32", ["ptr", "ptr", "i32", "f32", "f32", "f32", "ptr", "ptr", "ptr"]),
}


def _config_fields():
    """The fields of `struct mia_marvis_config { ... };`, read with the header parser (which takes the typedef form)."""
    text, n = re.subn(r"struct\s+mia_marvis_config\s*\{(.*?)\}\s*;", r"typedef struct {\1} mia_marvis_config;", CONFIG_HEADER, flags=re.S)
    assert n == 1
    text = re.sub(r'^\s*#.*$', " ", text, flags=re.M)
    return parse(text)[1]["mia_marvis_config"]


def test_header_declares_the_entry_points():
    functions, structs = parse(HEADER)
    for name, sig in ENTRY_POINTS.items():
        assert functions.get(name) == sig, (name, functions.get(name))
    assert re.search(r"typedef\s+struct\s+mia_marvis_config\s+mia_marvis_config\s*;", HEADER) and "mia_marvis_config" not in structs
    assert "unpinned" in HEADER.split("Marvis TTS (CSM)")[1].split("Fun-ASR audio half")[0]      # the sampler rule says what it is restated from
    fields = [f for f, _, _ in _config_fields()]
    for f in ("text_vocab", "audio_vocab", "n_codebooks", "max_ctx", "bb_hidden", "bb_head_dim", "dec_hidden", "dec_head_dim", "rope_llama3", "rope_factor",
              "attention_bias", "mlp_bias"):
        assert f in fields, f


def test_config_mirror_matches_the_header_field_for_field():
    from mlx_swift_audio_amd import _abi
    kinds = {C.c_int: "i32", C.c_float: "f32"}
    mirror = [(f, kinds[t], 0) for f, t in _abi.MarvisConfig._fields_]          # flat 4-byte scalars only
    assert mirror == _config_fields()
    assert C.sizeof(_abi.MarvisConfig) == 4 * len(mirror)


def test_table_lists_them_and_the_library_exports_them():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import _abi
    lib = m._lib.load()
    for name in ENTRY_POINTS:
        assert name in _abi.PROTOTYPES, name
        assert getattr(lib, name).argtypes is not None, name
    assert "mia_marvis_config" not in _abi.STRUCTS


def test_python_surface():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import checkpoint, marvis, synthetic
    assert m.MarvisModel and m.MarvisConfig and m.MarvisTTS
    assert set(synthetic.MARVIS_CONFIGS) == {"marvis-micro", "marvis-micro128", "marvis-csm-1b"}
    for f in ("load", "frame", "generate", "generate_batch", "set_batch", "reset", "close", "set_debug"):
        assert callable(getattr(m.MarvisModel, f))
    for f in ("generate", "generate_streaming"):
        assert callable(getattr(m.MarvisTTS, f))
    assert callable(checkpoint.sanitize_marvis) and callable(synthetic.marvis_weights) and callable(marvis.tokenize_start)
    c = marvis._c_config(synthetic.MARVIS_CONFIGS["marvis-micro128"])
    assert (c.text_vocab, c.audio_vocab, c.n_codebooks, c.max_ctx, c.dec_heads, c.dec_head_dim, c.rope_llama3, c.rope_old_ctx) == (300, 67, 5, 96, 1, 128, 1, 8192.0)
