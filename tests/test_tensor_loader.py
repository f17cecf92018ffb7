"""The models' tensor lookup (csrc/tensor_loader.h) and the host's 16-bit conversions (csrc/host_convert.h) are pure host code: a
stand-alone program with its own main includes the header, never uploads anything, and prints what every lookup case returns (or
writes what every conversion gives to a file).  No GPU needed (hipcc only supplies the HIP headers)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mlx-swift-audio_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

PROGRAM = r"""
#include <cstdio>
#include "tensor_loader.h"

static mia_tensor_view view(const char* name, int dtype, int ndim, int64_t a, int64_t b, const void* data) {
  mia_tensor_view v{};
  v.name = name; v.dtype = dtype; v.ndim = ndim; v.shape[0] = a; v.shape[1] = b; v.data = data;
  return v;
}

static void report(const char* what, TensorLoader L, const char* name, std::initializer_list<int64_t> shp) {
  std::vector<float> out;
  const bool ok = L.f32(name, out, shp);
  printf("%s: %d n=%zu err=[%s]", what, ok ? 1 : 0, out.size(), L.err.c_str());
  for (float x : out) printf(" %g", x);
  printf("\n");
}

int main() {
  static const float six[6] = {1, 2, 3, 4, 5, 6};
  static const uint16_t half[6] = {};
  const mia_tensor_view t[] = {
      view("w", MIA_F32, 2, 2, 3, six),
      view("nodata", MIA_F32, 2, 2, 3, nullptr),
      view(nullptr, MIA_F32, 2, 2, 3, six),
      view("h", MIA_F16, 2, 2, 3, half),
  };
  TensorLoader L;
  L.index(t, 4);
  printf("indexed: %zu has_w=%d has_nodata=%d\n", L.by_name.size(), L.has("w") ? 1 : 0, L.has("nodata") ? 1 : 0);
  report("found", L, "w", {2, 3});
  report("missing", L, "absent", {2, 3});
  report("null data", L, "nodata", {2, 3});
  report("wrong dtype", L, "h", {2, 3});
  report("wrong rank", L, "w", {6});
  report("wrong rank 3", L, "w", {2, 3, 1});
  report("wrong dim", L, "w", {2, 4});
  report("same count", L, "w", {3, 2});
  {  // the first error wins, and a later success does not clear it
    std::vector<float> out;
    L.f32("absent", out, {1});
    L.f32("w", out, {3, 2});
    const bool ok = L.f32("w", out, {2, 3});
    printf("first error: %d err=[%s]\n", ok ? 1 : 0, L.err.c_str());
  }
  {
    TensorLoader F; F.index(t, 4);
    const mia_tensor_view* v = F.find("w");
    printf("find: %d ndim=%d shape0=%lld err=[%s]\n", v == &t[0] ? 1 : 0, v ? v->ndim : -1, v ? (long long)v->shape[0] : -1ll, F.err.c_str());
    printf("find absent: %d nodata: %d err=[%s]\n", F.find("absent") ? 1 : 0, F.find("nodata") ? 1 : 0, F.err.c_str());
  }
  return 0;
}
"""

EXPECTED = """\
indexed: 2 has_w=1 has_nodata=0
found: 1 n=6 err=[] 1 2 3 4 5 6
missing: 0 n=0 err=[missing tensor 'absent']
null data: 0 n=0 err=[missing tensor 'nodata']
wrong dtype: 0 n=0 err=[tensor 'h' must be float32]
wrong rank: 0 n=0 err=[tensor 'w' has an unexpected shape]
wrong rank 3: 0 n=0 err=[tensor 'w' has an unexpected shape]
wrong dim: 0 n=0 err=[tensor 'w' has an unexpected shape]
same count: 0 n=0 err=[tensor 'w' has an unexpected shape]
first error: 1 err=[missing tensor 'absent']
find: 1 ndim=2 shape0=2 err=[]
find absent: 0 nodata: 0 err=[]
"""


def _run(tmp_path, name, program, *args):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    src = tmp_path / (name + ".cpp")
    src.write_text(program)
    exe = tmp_path / name
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return subprocess.run([str(exe), *args], check=True, capture_output=True, text=True, timeout=60).stdout


def test_tensor_loader_lookup(tmp_path):
    assert _run(tmp_path, "loader_cases", PROGRAM).splitlines() == EXPECTED.splitlines()


# ---- read(): F32, F16 or BF16 sources; the status code kept beside err -------------------------------------------------------------------
READ_PROGRAM = r"""
#include <cstdio>
#include "tensor_loader.h"

static mia_tensor_view view(const char* name, int dtype, int ndim, int64_t a, int64_t b, const void* data) {
  mia_tensor_view v{};
  v.name = name; v.dtype = dtype; v.ndim = ndim; v.shape[0] = a; v.shape[1] = b; v.data = data;
  return v;
}

static void report(const char* what, TensorLoader L, const char* name, std::initializer_list<int64_t> shp) {
  std::vector<float> out;
  const bool ok = L.read(name, out, shp);
  printf("%s: %d n=%zu code=%d err=[%s]", what, ok ? 1 : 0, out.size(), L.code, L.err.c_str());
  for (float x : out) printf(" %g", x);
  printf("\n");
}

int main() {
  static const float six[6] = {1, 2, 3, 4, 5, 6};
  static const uint16_t half[6] = {0x3c00, 0x4000, 0x4200, 0x4400, 0x4500, 0x4600};
  static const uint16_t brain[6] = {0x3f80, 0x4000, 0x4040, 0x4080, 0x40a0, 0x40c0};
  static const uint32_t words[6] = {};
  const mia_tensor_view t[] = {
      view("w", MIA_F32, 2, 2, 3, six), view("h", MIA_F16, 2, 2, 3, half), view("b", MIA_BF16, 2, 2, 3, brain),
      view("u", MIA_U32, 2, 2, 3, words), view("nodata", MIA_F16, 2, 2, 3, nullptr),
  };
  TensorLoader L;
  L.index(t, 5);
  printf("codes: ok=%d invalid=%d oom=%d device=%d\n", MIA_OK, MIA_ERR_INVALID_ARGUMENT, MIA_ERR_OUT_OF_MEMORY, MIA_ERR_DEVICE);
  report("f32 source", L, "w", {2, 3});
  report("f16 source", L, "h", {2, 3});
  report("bf16 source", L, "b", {2, 3});
  report("u32 source", L, "u", {2, 3});
  report("missing", L, "absent", {2, 3});
  report("null data", L, "nodata", {2, 3});
  report("wrong shape f16", L, "h", {3, 2});
  report("wrong rank bf16", L, "b", {6});
  printf("optional: has_absent=%d has_h=%d err=[%s] code=%d\n", L.has("absent") ? 1 : 0, L.has("h") ? 1 : 0, L.err.c_str(), L.code);
  {  // f32() on a 16-bit source still refuses it, with its own text
    TensorLoader F = L;
    std::vector<float> out;
    const bool ok = F.f32("b", out, {2, 3});
    printf("f32 of bf16: %d code=%d err=[%s]\n", ok ? 1 : 0, F.code, F.err.c_str());
  }
  {  // the first error wins, text and code, whatever kind the later ones are; a later success does not clear it
    TensorLoader F = L;
    std::vector<float> out;
    F.read("u", out, {2, 3});
    F.read("absent", out, {1});
    F.fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed");
    F.fail(MIA_ERR_DEVICE, "hipMemcpy failed");
    const bool ok = F.read("h", out, {2, 3});
    printf("first error: %d code=%d err=[%s]\n", ok ? 1 : 0, F.code, F.err.c_str());
  }
  {  // what a refused allocation and a failed copy are recorded as
    TensorLoader A = L, B = L;
    A.fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed"); A.fail(MIA_ERR_DEVICE, "hipMemcpy failed");
    B.fail(MIA_ERR_DEVICE, "hipMemcpy failed"); B.fail(MIA_ERR_INVALID_ARGUMENT, "missing tensor 'x'");
    printf("allocation: code=%d err=[%s]\ncopy: code=%d err=[%s]\n", A.code, A.err.c_str(), B.code, B.err.c_str());
  }
  return 0;
}
"""

READ_EXPECTED = """\
codes: ok=0 invalid=-1 oom=-4 device=-5
f32 source: 1 n=6 code=0 err=[] 1 2 3 4 5 6
f16 source: 1 n=6 code=0 err=[] 1 2 3 4 5 6
bf16 source: 1 n=6 code=0 err=[] 1 2 3 4 5 6
u32 source: 0 n=0 code=-1 err=[tensor 'u' must be float32, float16 or bfloat16]
missing: 0 n=0 code=-1 err=[missing tensor 'absent']
null data: 0 n=0 code=-1 err=[missing tensor 'nodata']
wrong shape f16: 0 n=0 code=-1 err=[tensor 'h' has an unexpected shape]
wrong rank bf16: 0 n=0 code=-1 err=[tensor 'b' has an unexpected shape]
optional: has_absent=0 has_h=1 err=[] code=0
f32 of bf16: 0 code=-1 err=[tensor 'b' must be float32]
first error: 1 code=-1 err=[tensor 'u' must be float32, float16 or bfloat16]
allocation: code=-4 err=[hipMalloc failed]
copy: code=-5 err=[hipMemcpy failed]
"""


def test_tensor_loader_read_and_status(tmp_path):
    assert _run(tmp_path, "read_cases", READ_PROGRAM).splitlines() == READ_EXPECTED.splitlines()


# ---- the four conversions, against numpy (f16) and torch (bf16) ---------------------------------------------------------------------------
LOW_HALVES = (0x0000, 0x0001, 0x0fff, 0x1000, 0x1001, 0x1fff, 0x2000, 0x3000, 0x7fff, 0x8000, 0x8001, 0xefff, 0xf000, 0xffff)

CONVERT_PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "host_convert.h"

int main(int argc, char** argv) {
  static const uint32_t low[] = {%s};
  const int n_low = (int)(sizeof(low) / sizeof(low[0]));
  FILE* f = fopen(argv[1], "wb");
  if (!f) return 1;
  std::vector<uint16_t> bf, hf;                         // [65536][n_low] each
  for (uint32_t hi = 0; hi < 65536; ++hi)
    for (int j = 0; j < n_low; ++j) {
      const uint32_t u = (hi << 16) | low[j];
      float x; memcpy(&x, &u, 4);
      bf.push_back(f32_to_bf16(x)); hf.push_back(f32_to_f16(x));
    }
  std::vector<float> wide_h, wide_b;                    // [65536] each
  for (uint32_t v = 0; v < 65536; ++v) { wide_h.push_back(f16_to_f32((uint16_t)v)); wide_b.push_back(bf16_to_f32((uint16_t)v)); }
  fwrite(bf.data(), 2, bf.size(), f); fwrite(hf.data(), 2, hf.size(), f);
  fwrite(wide_h.data(), 4, wide_h.size(), f); fwrite(wide_b.data(), 4, wide_b.size(), f);
  return fclose(f) == 0 ? 0 : 1;
}
""" % ", ".join(hex(v) for v in LOW_HALVES)


def test_host_conversions_match_numpy_and_torch(tmp_path):
    """Every high half x the listed low halves (917 504 floats): a non-NaN input rounds to what numpy (float16) and torch (bfloat16)
    give, bit for bit, and a NaN stays a NaN in both formats; all 65 536 patterns of either 16-bit format widen to what numpy / torch
    widen them to (NaN patterns: to a NaN)."""
    import torch
    path = tmp_path / "converted.bin"
    _run(tmp_path, "convert_cases", CONVERT_PROGRAM, str(path))
    n = 65536 * len(LOW_HALVES)
    raw = np.fromfile(path, np.uint8)
    assert raw.size == 2 * n * 2 + 2 * 65536 * 4
    got_bf, got_hf = raw[:2 * n].view(np.uint16), raw[2 * n:4 * n].view(np.uint16)
    wide_h, wide_b = raw[4 * n:4 * n + 4 * 65536].view(np.uint32), raw[4 * n + 4 * 65536:].view(np.uint32)
    bits = ((np.arange(65536, dtype=np.uint32) << 16)[:, None] | np.asarray(LOW_HALVES, np.uint32)[None, :]).reshape(-1)
    x = bits.view(np.float32)
    nan = np.isnan(x)
    assert nan.sum() == 2 * 127 * len(LOW_HALVES) + 2 * (len(LOW_HALVES) - 1)       # every NaN high half, and 0x7f80 / 0xff80 with a low half set
    with np.errstate(over="ignore"):
        want_hf = x.astype(np.float16).view(np.uint16)
    want_bf = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    np.testing.assert_array_equal(got_hf[~nan], want_hf[~nan])
    np.testing.assert_array_equal(got_bf[~nan], want_bf[~nan])
    assert np.isnan(got_hf[nan].view(np.float16)).all()
    assert (((got_bf[nan] & 0x7f80) == 0x7f80) & ((got_bf[nan] & 0x007f) != 0)).all()
    pat = np.arange(65536, dtype=np.uint16)
    for got, want in ((wide_h, pat.view(np.float16).astype(np.float32)),
                      (wide_b, torch.from_numpy(pat.view(np.int16)).view(torch.bfloat16).to(torch.float32).numpy())):
        is_nan = np.isnan(want)
        np.testing.assert_array_equal(got[~is_nan], want.view(np.uint32)[~is_nan])
        assert np.isnan(got.view(np.float32)[is_nan]).all()
