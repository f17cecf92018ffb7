// tensor_loader.h -- name -> host tensor lookup with shape checks and upload: the one loader of every model.  Each model puts its own
// helpers in a struct on top of it (whisper_load.hip, lm_load.hip, sensevoice.hip, the fp32 models).  The first error is kept in `err`
// with its status in `code`; later ones are dropped.  The host's 16-bit conversions live in host_convert.h.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/mia.h"
#include "host_convert.h"

#define MIA_HIDDEN __attribute__((visibility("hidden")))      // new members stay out of the library's dynamic symbols

struct TensorLoader {
  std::vector<void*>* allocs = nullptr;      // every device allocation is appended here (freed by the owner)
  std::map<std::string, const mia_tensor_view*> by_name;
  std::string err;
  int code = MIA_OK;                         // status of `err`: INVALID_ARGUMENT (lookup, dtype, shape), OUT_OF_MEMORY (hipMalloc), DEVICE (copy)

  MIA_HIDDEN bool fail(int c, const std::string& m) { if (err.empty()) { err = m; code = c; } return false; }
  // a view without a name or without data is not indexed: asking for it reports "missing tensor"
  void index(const mia_tensor_view* tensors, int n) {
    for (int i = 0; i < n; ++i) if (tensors[i].name && tensors[i].data) by_name[tensors[i].name] = &tensors[i];
  }
  bool has(const std::string& n) const { return by_name.count(n) != 0; }       // optional tensors: ask first
  MIA_HIDDEN const mia_tensor_view* find(const std::string& n) const { auto it = by_name.find(n); return it == by_name.end() ? nullptr : it->second; }
  // the tensor as fp32 from an F32 source (f32), or from an F32, F16 or BF16 source (read); the shape must match exactly
  bool f32(const std::string& n, std::vector<float>& out, std::initializer_list<int64_t> shp) { return get(n, out, shp, false); }
  MIA_HIDDEN bool read(const std::string& n, std::vector<float>& out, std::initializer_list<int64_t> shp) { return get(n, out, shp, true); }
  MIA_HIDDEN void* alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes + 64) != hipSuccess) { fail(MIA_ERR_OUT_OF_MEMORY, "hipMalloc failed"); return nullptr; }
    allocs->push_back(p);
    return p;
  }
  // bytes as they are (tables that are not floats), and the fp32 form of it
  MIA_HIDDEN void* put(const void* host, size_t bytes) {
    void* p = alloc(bytes);
    if (p && hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) fail(MIA_ERR_DEVICE, "hipMemcpy failed");
    return p;
  }
  float* up(const std::vector<float>& v) { return (float*)put(v.data(), v.size() * 4); }
  // the values rounded to dtype (MIA_F16, else bf16)
  MIA_HIDDEN void* up16(const std::vector<float>& v, int dtype) {
    std::vector<uint16_t> q(v.size());
    if (dtype == MIA_F16) for (size_t i = 0; i < v.size(); ++i) q[i] = f32_to_f16(v[i]);
    else for (size_t i = 0; i < v.size(); ++i) q[i] = f32_to_bf16(v[i]);
    return put(q.data(), q.size() * 2);
  }

 private:
  MIA_HIDDEN bool get(const std::string& n, std::vector<float>& out, std::initializer_list<int64_t> shp, bool any_float) {
    const mia_tensor_view* t = find(n);
    if (!t) return fail(MIA_ERR_INVALID_ARGUMENT, "missing tensor '" + n + "'");
    if (t->dtype != MIA_F32 && !(any_float && (t->dtype == MIA_F16 || t->dtype == MIA_BF16)))
      return fail(MIA_ERR_INVALID_ARGUMENT, "tensor '" + n + (any_float ? "' must be float32, float16 or bfloat16" : "' must be float32"));
    int64_t numel = 1; bool ok = t->ndim == (int)shp.size(); int i = 0;
    for (int64_t s : shp) { if (ok && t->shape[i] != s) ok = false; numel *= s; ++i; }
    if (!ok) return fail(MIA_ERR_INVALID_ARGUMENT, "tensor '" + n + "' has an unexpected shape");
    if (t->dtype == MIA_F32) { out.assign((const float*)t->data, (const float*)t->data + numel); return true; }
    const uint16_t* p = (const uint16_t*)t->data;
    out.resize(numel);
    if (t->dtype == MIA_F16) for (int64_t k = 0; k < numel; ++k) out[k] = f16_to_f32(p[k]);
    else for (int64_t k = 0; k < numel; ++k) out[k] = bf16_to_f32(p[k]);
    return true;
  }
};
