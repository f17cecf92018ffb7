// host_io.h -- the one staging rule of the entry points that take `int mem` ("One staging rule").  A HostIo lives for one call.
// Device mode hands the caller's pointers through and adds nothing to the stream.  Host mode queues the copies on the ctx stream, and the
// call returns -- through finish() or through any early `return` -- only when no copy that touches the caller's memory or this call's
// own stack is pending.  The first failed HIP call is kept and returned by finish(); later ones are dropped.  Sizes are in bytes.
#pragma once
#include "mia_internal.h"

// the workspace carving rule: every block starts on a 256-byte boundary
struct Carve {
  size_t bytes = 0;
  size_t add(size_t n) { const size_t off = bytes; bytes += align_up(n, 256); return off; }
  // the ctx workspace holding the carve; false when it cannot be allocated (an empty carve, all-device operands, needs none)
  bool workspace(mia_ctx* ctx, char*& ws) const { ws = bytes ? (char*)mia_workspace(ctx, bytes) : nullptr; return ws || !bytes; }
};

class HostIo {
 public:
  HostIo(mia_ctx* ctx, int mem) : ctx_(ctx), mem_(mem) {}
  static HostIo device(mia_ctx* ctx) { return HostIo(ctx, MIA_MEM_DEVICE); }     // internal calls on device pointers
  static HostIo host(mia_ctx* ctx) { return HostIo(ctx, MIA_MEM_HOST); }         // entry points whose pointers are host memory by contract
  static bool valid(int mem) { return mem == MIA_MEM_HOST || mem == MIA_MEM_DEVICE; }
  HostIo(const HostIo&) = delete;
  ~HostIo() { if (pending_) (void)hipStreamSynchronize(ctx_->stream); }           // a return before finish(): it already carries its own error

  int mem() const { return mem_; }                                                // as given: a forwarded call validates it in its own place
  bool host() const { return mem_ == MIA_MEM_HOST; }
  size_t staged(size_t bytes) const { return host() ? bytes : 0; }                 // staging an operand needs: none in device mode

  // an input: the caller's pointer (device), or `stage` behind a queued upload (host)
  template <class T> const T* in(const T* p, void* stage, size_t bytes) {
    if (!p || !host()) return p;
    copy(stage, p, bytes, hipMemcpyHostToDevice);
    return (const T*)stage;
  }
  // an output: the caller's pointer (device), or `stage`, downloaded by finish() (host)
  template <class T> T* out(T* p, void* stage, size_t bytes) {
    if (!p || !host()) return p;
    outs_.push_back({p, stage, bytes});
    return (T*)stage;
  }
  // an operand the kernel updates in place: bytes it does not write survive the round trip
  template <class T> T* inout(T* p, void* stage, size_t bytes) { in(p, stage, bytes); return out(p, stage, bytes); }
  // a table built by the library on this call's stack or heap, uploaded in either mode: the call must not return before it is read
  template <class T> const T* table(const T* host_array, void* stage, size_t bytes) {
    copy(stage, host_array, bytes, hipMemcpyHostToDevice);
    return (const T*)stage;
  }
  // the way back: device data into an array of the library's own, in either mode (read it after finish())
  void fetch(void* host_array, const void* dev, size_t bytes) { copy(host_array, dev, bytes, hipMemcpyDeviceToHost); }
  // a copy the entry point queues itself in either mode (into a handle's buffer, 2-D): the kind of it, and its status
  hipMemcpyKind from_caller() { pending_ |= host(); return host() ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice; }
  hipMemcpyKind to_caller() { pending_ |= host(); return host() ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice; }
  void check(hipError_t e) { if (err_ == hipSuccess) err_ = e; }

  // queue the downloads in the order out() was called, wait once if a copy touching host memory was queued, report the first error.
  // May be called more than once (per clip of a loop).
  int finish() {
    for (const Out& o : outs_) copy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost);
    outs_.clear();
    if (pending_) check(hipStreamSynchronize(ctx_->stream));
    pending_ = false;
    const hipError_t e = err_;
    err_ = hipSuccess;
    return e == hipSuccess ? MIA_OK : mia_fail(ctx_, MIA_ERR_DEVICE, "host/device copy failed: %s", hipGetErrorString(e));
  }

 private:
  struct Out { void* host; const void* dev; size_t bytes; };
  void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    if (!bytes) return;
    pending_ = true;
    check(hipMemcpyAsync(dst, src, bytes, kind, ctx_->stream));
  }
  mia_ctx* ctx_;
  int mem_;
  bool pending_ = false;
  hipError_t err_ = hipSuccess;
  std::vector<Out> outs_;
};
