// Private host-side helpers shared by the translation units of libcoxgraph_hip.so: status mapping, the device guard, the owners of
// device memory, pinned memory, streams and events, and argument checks.  Every unit includes this header (it brings cox_internal.hpp along) and defines none of it
// itself.  Everything is inline: the units are linked into one shared object.
#pragma once
#include <cmath>

#include "cox_internal.hpp"

#define COX_TRY(expr)              \
  do {                             \
    int st_ = (expr);              \
    if (st_ != COX_OK) return st_; \
  } while (0)

// COX_* status of a HIP call; a failure also clears the per-thread sticky error, so that the next check sees its own errors only
static inline int cox_hip_status(hipError_t e) {
  if (e == hipSuccess) return COX_OK;
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? COX_ERR_OUT_OF_MEMORY : COX_ERR_NO_DEVICE;
}

static inline int device_present() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return COX_ERR_NO_DEVICE;
  }
  return COX_OK;
}

// count elements of device memory (one element for a count of 0); *p is null after a failure.  Silent.
template <class T>
inline int dev_alloc(T** p, size_t count) {
  *p = nullptr;
  const int st = cox_hip_status(hipMalloc(reinterpret_cast<void**>(p), (count ? count : 1) * sizeof(T)));
  if (st != COX_OK) *p = nullptr;
  return st;
}

template <class T>
inline void dev_free(T** p) {
  if (*p) (void)hipFree(*p);
  *p = nullptr;
}

// The pointer form of DevBuf::grow, for a buffer kept as a pointer and a capacity: room for need elements, a no-op when it has
// them, otherwise a new buffer (contents are not kept).  After a failure *p is null and *cap is 0.
template <class T>
inline int dev_grow(T** p, u64* cap, u64 need) {
  if (need <= *cap) return COX_OK;
  dev_free(p);
  *cap = 0;
  COX_TRY(dev_alloc(p, need));
  *cap = need;
  return COX_OK;
}

// The owning types.  All are move-only and start out null; their destructors release what they hold, tolerate null and do not set
// the device (the owner of a handle does that before it deletes the handle) or synchronise.
#define COX_MOVE_ONLY(Type)                  \
  Type() = default;                          \
  Type(const Type&) = delete;                \
  Type& operator=(const Type&) = delete;     \
  Type(Type&& o) noexcept { swap(o); }       \
  Type& operator=(Type&& o) noexcept {       \
    Type t(static_cast<Type&&>(o));          \
    swap(t);                                 \
    return *this;                            \
  }

// device memory (or, Pinned, page-locked host memory) for cap elements
template <class T, bool Pinned = false>
struct DevBuf {
  T* p = nullptr;
  u64 cap = 0;
  COX_MOVE_ONLY(DevBuf)
  ~DevBuf() { reset(); }
  void swap(DevBuf& o) {
    T* const q = p;
    const u64 c = cap;
    p = o.p, cap = o.cap;
    o.p = q, o.cap = c;
  }
  void reset() {
    if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr, cap = 0;
  }
  // count elements (one element for a count of 0), whatever it held before; null after a failure.  Silent.
  int alloc(size_t count) {
    reset();
    const size_t bytes = (count ? count : 1) * sizeof(T);
    void* q = nullptr;
    COX_TRY(cox_hip_status(Pinned ? hipHostMalloc(&q, bytes, hipHostMallocDefault) : hipMalloc(&q, bytes)));
    p = static_cast<T*>(q), cap = count;
    return COX_OK;
  }
  // room for need elements: a no-op when it has them, otherwise a new buffer (contents are not kept); null, cap 0 after a failure
  int grow(u64 need) { return need <= cap ? COX_OK : alloc(need); }
  operator T*() const { return p; }
  T* release() {  // the caller owns the buffer from here on
    T* q = p;
    p = nullptr, cap = 0;
    return q;
  }
};
template <class T>
using PinnedBuf = DevBuf<T, true>;

struct Stream {  // non-blocking
  hipStream_t s = nullptr;
  COX_MOVE_ONLY(Stream)
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  void swap(Stream& o) {
    hipStream_t t = s;
    s = o.s, o.s = t;
  }
  int create() {
    const int st = cox_hip_status(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    if (st != COX_OK) s = nullptr;
    return st;
  }
  operator hipStream_t() const { return s; }
};

struct Event {
  hipEvent_t e = nullptr;
  COX_MOVE_ONLY(Event)
  ~Event() {
    if (e) (void)hipEventDestroy(e);
  }
  void swap(Event& o) {
    hipEvent_t t = e;
    e = o.e, o.e = t;
  }
  int create(bool timing) {
    const int st = cox_hip_status(timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (st != COX_OK) e = nullptr;
    return st;
  }
  operator hipEvent_t() const { return e; }
};

struct EventPair {  // two timing events around a stretch of one stream
  Event a, b;
  int create() {
    COX_TRY(a.create(true));
    return b.create(true);
  }
  hipError_t begin(hipStream_t s) { return hipEventRecord(a, s); }
  hipError_t end(hipStream_t s) { return hipEventRecord(b, s); }
  // false, with the sticky error cleared, when the events cannot be read (not created, not recorded, not complete)
  bool elapsed_ms(double* ms) const {
    float f = 0.0f;
    if (!a.e || !b.e || hipEventElapsedTime(&f, a, b) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    *ms = static_cast<double>(f);
    return true;
  }
};

static inline bool finite_all(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}
