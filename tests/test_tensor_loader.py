"""The fp32 models' tensor lookup (csrc/tensor_loader.h) is pure host code: a stand-alone program with its own main includes the
header, never uploads anything, and prints what every lookup case returns.  No GPU needed (hipcc only supplies the HIP headers)."""
import os
import subprocess

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


def test_tensor_loader_lookup(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    src = tmp_path / "loader_cases.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "loader_cases"
    subprocess.run([HIPCC, "-std=c++17", "-O1", "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout
    assert out.splitlines() == EXPECTED.splitlines()
