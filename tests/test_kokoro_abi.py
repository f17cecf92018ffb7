"""The Kokoro entry points are declared in include/mia.h, listed in the ctypes table with the header's types, and exported by the built
library; the configuration record of include/mia_kokoro.h (mia.h only declares its type) and its ctypes mirror agree field for field
(no GPU needed)."""
import ctypes as C
import os
import re

from _abi_header import parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "mia.h")).read()
CONFIG_HEADER = open(os.path.join(ROOT, "include", "mia_kokoro.h")).read()
ENTRY_POINTS = {
    "mia_kokoro_load": ("ptr", ["ptr", "ptr", "struct:mia_tensor_view", "i32"]),
    "mia_kokoro_free": ("void", ["ptr"]),
    "mia_kokoro_output_len": ("i64", ["ptr", "i64"]),
    "mia_kokoro_f0n": ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "i32"]),
    "mia_kokoro_source": ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "i32"]),
    "mia_kokoro_generate": ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "i32"]),
    "mia_kokoro_decode": ("i32", ["ptr", "ptr", "i32", "ptr", "ptr", "ptr", "ptr", "ptr", "i32"]),
    "mia_op_instance_norm": ("i32", ["ptr", "ptr", "i64", "i64", "i32", "ptr", "ptr"]),
}


def _config_fields():
    text, n = re.subn(r"struct\s+mia_kokoro_config\s*\{(.*?)\}\s*;", r"typedef struct {\1} mia_kokoro_config;", CONFIG_HEADER, flags=re.S)
    assert n == 1
    text = re.sub(r'^\s*#.*$', " ", text, flags=re.M)
    return parse(text)[1]["mia_kokoro_config"]


def test_header_declares_the_entry_points():
    functions, structs = parse(HEADER)
    for name, sig in ENTRY_POINTS.items():
        assert functions.get(name) == sig, (name, functions.get(name))
    assert re.search(r"typedef\s+struct\s+mia_kokoro_config\s+mia_kokoro_config\s*;", HEADER) and "mia_kokoro_config" not in structs
    fields = [f for f, _, _ in _config_fields()]
    for f in ("dim_in", "style_dim", "hidden", "asr_res_dim", "pred_dim", "up_initial", "up_rates", "up_kernels", "res_kernels", "dilations",
              "n_fft", "hop", "n_harmonics", "voiced_threshold", "sample_rate"):
        assert f in fields, f


def test_config_mirror_matches_the_header_field_for_field():
    from mlx_swift_audio_amd import _abi
    mirror = []
    for f, t in _abi.KokoroConfig._fields_:
        assert t is C.c_int or (hasattr(t, "_length_") and t._type_ is C.c_int), (f, t)
        mirror.append((f, "i32", getattr(t, "_length_", 0)))
    assert mirror == _config_fields()
    assert C.sizeof(_abi.KokoroConfig) == 4 * (len(mirror) + 4 * 3)          # four arrays of 4 count once above


def test_table_lists_them_and_the_library_exports_them():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import _abi
    lib = m._lib.load()
    for name in ENTRY_POINTS:
        assert name in _abi.PROTOTYPES, name
        assert getattr(lib, name).argtypes is not None, name
    assert "mia_kokoro_config" not in _abi.STRUCTS


def test_python_surface():
    import mlx_swift_audio_amd as m
    from mlx_swift_audio_amd import checkpoint, synthetic
    from mlx_swift_audio_amd.kokoro import KOKORO_CONFIGS, KokoroDecoder
    assert m.KokoroDecoder is KokoroDecoder and m.KokoroConfig
    assert set(KOKORO_CONFIGS) == {"kokoro_82m", "kokoro_micro"}
    big, micro = KOKORO_CONFIGS["kokoro_82m"], KOKORO_CONFIGS["kokoro_micro"]
    assert (big.dim_in, big.style_dim, big.hidden, big.asr_res_dim, big.up_initial, big.pred_dim) == (512, 128, 1024, 64, 512, 512)
    assert big.upsample_scale == micro.upsample_scale == 300
    assert (micro.dim_in + 2, micro.hidden + micro.asr_res_dim + 2) == (66, 130)
    for f in ("load", "f0n", "source", "generate", "decode", "__call__", "output_len", "close"):
        assert callable(getattr(KokoroDecoder, f))
    w = synthetic.kokoro_weights(micro, 3)
    assert w["decoder.generator.ups.0.weight_v"].shape == (64, 20, 32) and w["decoder.decode.3.pool.weight_v"].shape == (130, 3, 1)
    assert not any(k.startswith("predictor.") for k in synthetic.kokoro_weights(micro, 3, predictor=False))
    # sanitize_kokoro: the checkpoint's [Cout][Cin][K] layouts back to what the synthetic weights hold; foreign keys are dropped
    raw = {k: (v.transpose(0, 2, 1) if v.ndim == 3 and ("weight_v" in k or (k.endswith(".weight") and "fc." not in k and "l_linear" not in k)) else v)
           for k, v in w.items()}
    raw["bert.embeddings.word_embeddings.weight"] = w["decoder.F0_conv.bias"]
    raw["predictor.lstm.weight_ih_l0"] = w["decoder.F0_conv.bias"]
    back = checkpoint.sanitize_kokoro(raw)
    assert set(back) == set(w)
    for k in w:
        assert back[k].shape == w[k].shape and (back[k] == w[k]).all(), k
