// mia_internal.h -- shared host-side plumbing for the HIP layer (context, workspace, error handling).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/mia.h"

// One cache for the context's device tables ("One table cache"): a record per (owner, a, b) holds the device pointers of one
// set, in the order they were given to mia_tables_build, and a few host ints of the owner's choosing.  Records never move, a failed
// build registers nothing, and mia_destroy frees them all.
enum { MIA_TAB_LOGMEL, MIA_TAB_S3GEN_MEL, MIA_TAB_FUNASR, MIA_TAB_SPEAKER, MIA_TAB_RESAMPLE };
struct mia_table_key { int owner, a, b; };          // a, b: what tells an owner's sets apart (0 for a singleton)
struct mia_table_src {
  const void* host; size_t bytes;
  template <class T> mia_table_src(const std::vector<T>& v) : host(v.data()), bytes(v.size() * sizeof(T)) {}
};
struct mia_tables {
  mia_table_key key;
  void* dev[4];
  int meta[4];
};

struct mia_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  // grow-only scratch arena in HBM (never freed between calls: no hipMalloc on the hot path)
  void* ws = nullptr;
  size_t ws_bytes = 0;
  std::deque<mia_tables> tables;     // a deque: push_back leaves the records where they are
  // optional HIP-event profiling of kernel classes (mia_profile_*): bench.py's roofline figures come from here
  bool prof_on = false;
  struct ProfRec { int cls; hipEvent_t start, stop; double work; };
  std::vector<ProfRec> prof;
  std::vector<hipEvent_t> ev_pool;
  // data-parallel exchange (dp.hip): one RCCL communicator per context, collectives run on the context's stream
  void* dp_comm = nullptr;
  int dp_rank = 0, dp_world = 0, dp_plan_items = -1;
  void* dp_buf = nullptr;
  size_t dp_buf_bytes = 0;
};

enum { MIA_PROF_LOGMEL = 0, MIA_PROF_ENC_GEMM = 1, MIA_PROF_ENC_ATTN = 2, MIA_PROF_ENC_NORM = 3, MIA_PROF_DECODE = 4,
       MIA_PROF_CROSSKV_GEMM = 5, MIA_PROF_MEL_GATHER = 6, MIA_PROF_FSMN = 7,
       MIA_PROF_DECODE_KEPT = 8,      // the decode passes whose step kept the layer weights cache-resident (whisper_decode.hip: dec_cache_policy)
       MIA_PROF_NCLASSES = 9 };

// RAII-less helpers: if profiling is on, bracket the launches between begin/end with events on the ctx stream
int mia_prof_begin(mia_ctx* ctx, int cls, double work);   // returns record index or -1
void mia_prof_end(mia_ctx* ctx, int rec);

inline int mia_fail(mia_ctx* ctx, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

#define MIA_HIP(ctx, expr)                                                                      \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return mia_fail((ctx), MIA_ERR_DEVICE, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                      __FILE__, __LINE__);                                                      \
  } while (0)

#define MIA_CHECK_ARG(ctx, cond, ...)                                   \
  do {                                                                  \
    if (!(cond)) return mia_fail((ctx), MIA_ERR_INVALID_ARGUMENT, __VA_ARGS__); \
  } while (0)

// Ensure the ctx workspace holds at least `bytes`; returns nullptr on failure (ctx->err set).
void* mia_workspace(mia_ctx* ctx, size_t bytes);

// Grow-only device buffer of a handle: make p hold at least n elements (+ 64 B of slack), keeping it when it already does.  The old
// buffer is freed behind a stream synchronisation, and p / cap are cleared BEFORE the allocation, so that a failed one leaves an empty
// buffer on record and the next call allocates again instead of launching on a null pointer.  Contents are not carried over.
template <class P>
static int mia_grow(mia_ctx* ctx, P*& p, size_t& cap, size_t n, const char* msg) {
  if (n <= cap) return MIA_OK;
  (void)hipStreamSynchronize(ctx->stream);
  if (p) (void)hipFree(p);
  p = nullptr; cap = 0;
  if (hipMalloc((void**)&p, n * sizeof(P) + 64) != hipSuccess) { p = nullptr; return mia_fail(ctx, MIA_ERR_OUT_OF_MEMORY, "%s", msg); }
  cap = n;
  return MIA_OK;
}

inline size_t mia_dtype_size(int dt) { return dt == MIA_F32 ? 4 : 2; }

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// The set under `key`, or nullptr when it has not been built.
const mia_tables* mia_tables_find(const mia_ctx* ctx, mia_table_key key);
// Allocate one device buffer per source, upload them on ctx->stream as it is now, wait, and register the set (at most 4 sources and 4
// meta ints).  On any failure every allocation of this call is freed, nothing is registered and the next call builds again.
int mia_tables_build(mia_ctx* ctx, mia_table_key key, std::initializer_list<mia_table_src> src, std::initializer_list<int> meta, const mia_tables** out);

#include "host_io.h"   // HostIo, Carve: the staging rule of every entry point that takes `int mem`
