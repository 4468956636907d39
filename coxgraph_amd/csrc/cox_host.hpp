// Private host-side helpers shared by the translation units of libcoxgraph_hip.so: status mapping, the device guard, device
// allocation and argument checks.  Every unit includes this header (it brings cox_internal.hpp along) and defines none of it
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

// room for need elements in a buffer that holds *cap: a no-op when it has them, otherwise a new buffer (contents are not
// kept).  After a failure *p is null and *cap is 0.
template <class T>
inline int dev_grow(T** p, u64* cap, u64 need) {
  if (need <= *cap) return COX_OK;
  dev_free(p);
  *cap = 0;
  COX_TRY(dev_alloc(p, need));
  *cap = need;
  return COX_OK;
}

template <class T>
struct DevBuf {  // frees on scope exit
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { dev_free(&p); }
  int alloc(size_t count) { return dev_alloc(&p, count); }
  T* release() {  // the caller owns the buffer from here on
    T* q = p;
    p = nullptr;
    return q;
  }
};

static inline bool finite_all(const float* v, int n) {
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}
