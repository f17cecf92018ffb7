"""The Mimi entry points are declared in include/mia.h, listed in the ctypes table with the header's types, and exported by the built
library; the configuration record of include/mia_mimi.h (mia.h only declares its type) and its ctypes mirror agree field for field
(no GPU needed)."""
import ctypes as C
import os
import re

from _abi_header import parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mia.h")).read()
CONFIG_HEADER = open(os.path.join(ROOT, "include", "mia_mimi.h")).read()
ENTRY_POINTS = {
    "mia_mimi_load": ("ptr", ["ptr", "ptr", "struct:mia_tensor_view", "i32"]),
    "mia_mimi_free": ("void", ["ptr"]),
    "mia_mimi_output_len": ("i64", ["ptr", "i64"]),
    "mia_mimi_decode": ("i32", ["ptr", "ptr", "i32", "i64", "ptr", "i64", "ptr", "i32"]),
    "mia_mimi_stream_create": ("ptr", ["ptr"]),
    "mia_mimi_stream_free": ("void", ["ptr"]),
    "mia_mimi_stream_reset": ("i32", ["ptr"]),
    "mia_mimi_stream_decode": ("i32", ["ptr", "ptr", "i32", "i64", "ptr", "i64", "ptr", "i32"]),
}


def _config_fields():
    """The fields of `struct mia_mimi_config { ... };`, read with the header parser (which takes the typedef form)."""
    text, n = re.subn(r"struct\s+mia_mimi_config\s*\{(.*?)\}\s*;", r"typedef struct {\1} mia_mimi_config;", CONFIG_HEADER, flags=re.S)
    assert n == 1
    text = re.sub(r'^\s*#.*$', " ", text, flags=re.M)
    return parse(text)[1]["mia_mimi_config"]


def test_header_declares_the_entry_points():
    functions, structs = parse(HEADER)
    for name, sig in ENTRY_POINTS.items():
        assert functions.get(name) == sig, name
    assert re.search(r"typedef\s+struct\s+mia_mimi_config\s+mia_mimi_config\s*;", HEADER) and "mia_mimi_config" not in structs
    fields = [f for f, _, _ in _config_fields()]
    for f in ("nq", "bins", "quantizer_dim", "upsample_stride", "seanet_ratios", "d_model", "n_heads", "n_layers", "dim_feedforward", "context",
              "kv_repeat", "gating", "layer_norm", "max_period"):
        assert f in fields, f


def test_config_mirror_matches_the_header_field_for_field():
    from mlx_swift_audio_amd import _abi
    mirror = []
    for f, t in _abi.MimiConfig._fields_:
        assert t is C.c_int or (hasattr(t, "_length_") and t._type_ is C.c_int), (f, t)          # int32 scalars and arrays only
        mirror.append((f, "i32", getattr(t, "_length_", 0)))
    assert mirror == _config_fields()
    assert C.sizeof(_abi.MimiConfig) == 4 * (len(mirror) + 7)          # seanet_ratios[8] counts once above


def test_table_lists_them_and_the_library_exports_them():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import _abi
    lib = m._lib.load()
    for name in ENTRY_POINTS:
        assert name in _abi.PROTOTYPES, name
        assert getattr(lib, name).argtypes is not None, name
    assert "mia_mimi_config" not in _abi.STRUCTS


def test_python_surface():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import synthetic
    from mlx_swift_audio_amd.mimi import mimi_202407
    assert m.MimiCodec and m.MimiStream and m.MimiConfig
    cfg = mimi_202407(32)
    assert cfg == synthetic.MIMI_CONFIGS["mimi_202407"] and cfg.samples_per_frame == 1920 and cfg.quantizer_nq == 32
    assert set(synthetic.MIMI_CONFIGS) == {"mimi_micro", "mimi_micro_ctx250", "mimi_202407"}
    assert synthetic.MIMI_CONFIGS["mimi_micro"].transformer.context == 6 and synthetic.MIMI_CONFIGS["mimi_micro_ctx250"].transformer.context == 250
    for f in ("decode", "new_stream", "load", "output_len"):
        assert callable(getattr(m.MimiCodec, f))
    for f in ("decode_frames", "reset", "close"):
        assert callable(getattr(m.MimiStream, f))
