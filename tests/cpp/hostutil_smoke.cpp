// coxgraph_amd/csrc/cox_host.hpp on its own, compiled as HIP: the status mapping, the device guard, dev_alloc / dev_grow, the owning types
// (DevBuf, PinnedBuf, Stream, Event, EventPair) and finite_all.
//   hostutil_smoke      the checks that need no device; where there is none, the failure paths as well.  Prints "device" or
//                       "no-device" for the mode it found.
//   hostutil_smoke gpu  needs a device: the growth sequence 0 -> 16 -> 16 -> 17 -> 4 elements in device and in pinned memory, release at
//                       scope exit, swap, and a timed memset on a stream
// Exit code 0 = all good.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "../../coxgraph_amd/csrc/cox_host.hpp"

static int g_failures = 0;
// What hipGetLastError() answers when nothing of ours is pending, taken before the first helper runs: hipSuccess with a device.
// Without one the runtime cannot initialise and the query itself answers hipErrorNoDevice, on every call, so "the sticky error
// is cleared" reads there as "the answer is the untouched process's".
static hipError_t g_quiet = hipSuccess;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                       \
    }                                                                     \
  } while (0)

static int try_returns(int st) {
  COX_TRY(st);
  return -1000;  // reached only for COX_OK
}

static void check_finite_all() {
  const float bad[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity()};
  float v[7];
  for (int n : {1, 3, 7}) {
    for (int i = 0; i < n; ++i) v[i] = 0.5f * static_cast<float>(i) - 1.0f;
    CHECK(finite_all(v, n));
    for (float b : bad)
      for (int at : {0, n / 2, n - 1}) {
        const float keep = v[at];
        v[at] = b;
        CHECK(!finite_all(v, n));
        CHECK(finite_all(v, at));  // everything before the bad value is fine
        v[at] = keep;
      }
  }
  CHECK(finite_all(bad, 0));
  CHECK(finite_all(nullptr, 0));
  const float edge[] = {std::numeric_limits<float>::max(), -std::numeric_limits<float>::max(), std::numeric_limits<float>::denorm_min(), -0.0f};
  CHECK(finite_all(edge, 4));
}

static void check_status_mapping() {
  CHECK(cox_hip_status(hipSuccess) == COX_OK);
  CHECK(cox_hip_status(hipErrorOutOfMemory) == COX_ERR_OUT_OF_MEMORY);
  CHECK(cox_hip_status(hipErrorNoDevice) == COX_ERR_NO_DEVICE);
  CHECK(cox_hip_status(hipErrorInvalidValue) == COX_ERR_NO_DEVICE);
  CHECK(hipGetLastError() == g_quiet);
  CHECK(try_returns(COX_OK) == -1000);
  CHECK(try_returns(COX_ERR_OUT_OF_MEMORY) == COX_ERR_OUT_OF_MEMORY);
}

// need <= cap touches nothing, with a device or without; moves and swaps hand over p and cap and leave the source null
template <class Buf>
static void check_noop_growth_of() {
  Buf buf;
  CHECK(buf.grow(0) == COX_OK);
  CHECK(buf.p == nullptr && buf.cap == 0);
  float* const fake = reinterpret_cast<float*>(0x1000);  // never dereferenced and never freed: grow must leave it alone
  buf.p = fake, buf.cap = 8;
  CHECK(buf.grow(0) == COX_OK && buf.p == fake && buf.cap == 8);
  CHECK(buf.grow(8) == COX_OK && buf.p == fake && buf.cap == 8);
  Buf moved(static_cast<Buf&&>(buf));
  CHECK(moved.p == fake && moved.cap == 8 && buf.p == nullptr && buf.cap == 0);
  Buf other;
  float* const fake2 = reinterpret_cast<float*>(0x2000);
  other.p = fake2, other.cap = 3;
  moved.swap(other);
  CHECK(moved.p == fake2 && moved.cap == 3 && other.p == fake && other.cap == 8);
  buf = static_cast<Buf&&>(other);  // into an empty one: nothing to free
  CHECK(buf.p == fake && buf.cap == 8 && other.p == nullptr && other.cap == 0);
  CHECK(buf.release() == fake && buf.p == nullptr && buf.cap == 0);
  CHECK(moved.release() == fake2 && moved.p == nullptr && moved.cap == 0);
  CHECK(hipGetLastError() == g_quiet);
}  // every destructor here sees null
static void check_noop_growth() {
  float* p = nullptr;
  u64 cap = 0;
  CHECK(dev_grow(&p, &cap, 0) == COX_OK);
  CHECK(p == nullptr && cap == 0);
  float* const fake = reinterpret_cast<float*>(0x1000);  // never dereferenced and never freed: dev_grow must leave it alone
  p = fake, cap = 8;
  CHECK(dev_grow(&p, &cap, 0) == COX_OK && p == fake && cap == 8);
  CHECK(dev_grow(&p, &cap, 8) == COX_OK && p == fake && cap == 8);
  CHECK(hipGetLastError() == g_quiet);
  check_noop_growth_of<DevBuf<float>>();
  check_noop_growth_of<PinnedBuf<float>>();
}

static void check_without_device() {
  CHECK(g_quiet == hipSuccess || g_quiet == hipErrorNoDevice);
  CHECK(device_present() == COX_ERR_NO_DEVICE);
  CHECK(hipGetLastError() == g_quiet);
  float* p = nullptr;
  u64 cap = 0;
  CHECK(dev_grow(&p, &cap, 16) == COX_ERR_NO_DEVICE);
  CHECK(p == nullptr && cap == 0);
  CHECK(hipGetLastError() == g_quiet);
  {
    DevBuf<float> grown;
    CHECK(grown.grow(16) == COX_ERR_NO_DEVICE);
    CHECK(grown.p == nullptr && grown.cap == 0);
    CHECK(hipGetLastError() == g_quiet);
    PinnedBuf<float> pinned;
    CHECK(pinned.grow(16) == COX_ERR_NO_DEVICE && pinned.p == nullptr && pinned.cap == 0);
    CHECK(hipGetLastError() == g_quiet);
    CHECK(pinned.alloc(0) == COX_ERR_NO_DEVICE && pinned.p == nullptr && pinned.cap == 0);
    CHECK(hipGetLastError() == g_quiet);
    Stream stream;
    CHECK(stream.create() == COX_ERR_NO_DEVICE && stream.s == nullptr);
    CHECK(hipGetLastError() == g_quiet);
    Event timing, plain;
    CHECK(timing.create(true) == COX_ERR_NO_DEVICE && timing.e == nullptr);
    CHECK(plain.create(false) == COX_ERR_NO_DEVICE && plain.e == nullptr);
    CHECK(hipGetLastError() == g_quiet);
    EventPair pair;
    CHECK(pair.create() == COX_ERR_NO_DEVICE && pair.a.e == nullptr && pair.b.e == nullptr);
    double ms = -1.0;
    CHECK(!pair.elapsed_ms(&ms) && ms == -1.0);
    CHECK(hipGetLastError() == g_quiet);
  }  // nothing was made: the destructors touch nothing
  CHECK(hipGetLastError() == g_quiet);
  double* q = reinterpret_cast<double*>(0x1000);
  CHECK(dev_alloc(&q, 4) == COX_ERR_NO_DEVICE && q == nullptr);
  CHECK(hipGetLastError() == g_quiet);
  CHECK(dev_alloc(&q, 0) == COX_ERR_NO_DEVICE && q == nullptr);
  CHECK(hipGetLastError() == g_quiet);
  dev_free(&q);  // null: nothing to do
  CHECK(q == nullptr);
  {
    DevBuf<u32> buf;
    CHECK(buf.alloc(16) == COX_ERR_NO_DEVICE && buf.p == nullptr && buf.cap == 0);
    CHECK(hipGetLastError() == g_quiet);
    CHECK(buf.alloc(0) == COX_ERR_NO_DEVICE && buf.p == nullptr && buf.cap == 0);
    CHECK(hipGetLastError() == g_quiet);
    CHECK(buf.release() == nullptr);
  }  // the destructor of an empty buffer frees nothing
  CHECK(hipGetLastError() == g_quiet);
}

struct Chunk {  // large, so that a granularity the allocator may round to cannot hide one element more
  unsigned char bytes[1 << 20];
};
static size_t allocation_bytes(const void* p) {
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  CHECK(hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) == hipSuccess);
  CHECK(base == p);
  return size;
}

// the address belongs to no allocation any more (the query's error is cleared)
static void check_released(const void* p) {
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  CHECK(hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess);
  (void)hipGetLastError();
}

static void check_with_device() {
  CHECK(device_present() == COX_OK);
  Chunk* p = nullptr;
  u64 cap = 0;
  CHECK(dev_grow(&p, &cap, 16) == COX_OK);  // 0 -> 16: allocates
  CHECK(p != nullptr && cap == 16);
  const size_t bytes16 = p ? allocation_bytes(p) : 0;
  CHECK(bytes16 >= 16 * sizeof(Chunk) && bytes16 < 17 * sizeof(Chunk));
  Chunk* const first = p;
  CHECK(dev_grow(&p, &cap, 16) == COX_OK);  // 16 -> 16: nothing
  CHECK(p == first && cap == 16);
  CHECK(dev_grow(&p, &cap, 17) == COX_OK);  // 16 -> 17: a new buffer (which may sit at the old address)
  CHECK(p != nullptr && cap == 17);
  CHECK(p && allocation_bytes(p) >= 17 * sizeof(Chunk));
  CHECK(p && hipMemset(p + 16, 0x5A, sizeof(Chunk)) == hipSuccess);  // the last element is there
  Chunk* const third = p;
  CHECK(dev_grow(&p, &cap, 4) == COX_OK);  // 17 -> 4: nothing, buffers never shrink
  CHECK(p == third && cap == 17);
  CHECK(p && allocation_bytes(p) >= 17 * sizeof(Chunk));
  dev_free(&p);
  CHECK(p == nullptr);
  const void* old_dev = nullptr;
  {
    DevBuf<Chunk> buf;
    CHECK(buf.grow(16) == COX_OK);  // 0 -> 16: allocates
    CHECK(buf.p != nullptr && buf.cap == 16);
    const size_t bytes16 = buf.p ? allocation_bytes(buf.p) : 0;
    CHECK(bytes16 >= 16 * sizeof(Chunk) && bytes16 < 17 * sizeof(Chunk));
    Chunk* const first = buf.p;
    CHECK(buf.grow(16) == COX_OK);  // 16 -> 16: nothing
    CHECK(buf.p == first && buf.cap == 16);
    CHECK(buf.grow(17) == COX_OK);  // 16 -> 17: a new buffer (which may sit at the old address)
    CHECK(buf.p != nullptr && buf.cap == 17);
    CHECK(buf.p && allocation_bytes(buf.p) >= 17 * sizeof(Chunk));
    CHECK(buf.p && hipMemset(buf.p + 16, 0x5A, sizeof(Chunk)) == hipSuccess);  // the last element is there
    Chunk* const third = buf.p;
    CHECK(buf.grow(4) == COX_OK);  // 17 -> 4: nothing, buffers never shrink
    CHECK(buf.p == third && buf.cap == 17);
    CHECK(buf.p && allocation_bytes(buf.p) >= 17 * sizeof(Chunk));
    old_dev = buf.p;
  }
  if (old_dev) check_released(old_dev);
  {
    PinnedBuf<Chunk> buf;  // the same sequence in pinned host memory
    CHECK(buf.grow(16) == COX_OK && buf.p != nullptr && buf.cap == 16);
    Chunk* const first = buf.p;
    CHECK(buf.grow(16) == COX_OK && buf.p == first && buf.cap == 16);
    CHECK(buf.grow(17) == COX_OK && buf.p != nullptr && buf.cap == 17);
    if (buf.p) {
      std::memset(buf.p + 16, 0x5A, sizeof(Chunk));  // the last element is there, and the host may write it
      CHECK(buf.p[16].bytes[sizeof(Chunk) - 1] == 0x5A);
    }
    Chunk* const third = buf.p;
    CHECK(buf.grow(4) == COX_OK && buf.p == third && buf.cap == 17);
  }
  {
    DevBuf<u32> a, b;  // swapped buffers keep their contents
    CHECK(a.alloc(1) == COX_OK && b.alloc(1) == COX_OK);
    const u32 wa = 0xA5A5A5A5u, wb = 0x12345678u;
    CHECK(hipMemcpy(a.p, &wa, sizeof(u32), hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(b.p, &wb, sizeof(u32), hipMemcpyHostToDevice) == hipSuccess);
    u32* const pa = a.p;
    a.swap(b);
    CHECK(b.p == pa && a.cap == 1 && b.cap == 1);
    u32 ra = 0, rb = 0;
    CHECK(hipMemcpy(&ra, a.p, sizeof(u32), hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(&rb, b.p, sizeof(u32), hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(ra == wb && rb == wa);
    DevBuf<u32> c(static_cast<DevBuf<u32>&&>(a));
    CHECK(a.p == nullptr && a.cap == 0 && c.cap == 1);
    CHECK(hipMemcpy(&ra, c.p, sizeof(u32), hipMemcpyDeviceToHost) == hipSuccess && ra == wb);
  }
  {
    Stream stream;
    EventPair timed;
    Event plain;
    DevBuf<u32> word;
    CHECK(stream.create() == COX_OK && stream.s != nullptr);
    CHECK(timed.create() == COX_OK && plain.create(false) == COX_OK && plain.e != nullptr);
    CHECK(word.alloc(1) == COX_OK);
    double ms = -1.0;
    CHECK(!timed.elapsed_ms(&ms));  // nothing recorded yet
    CHECK(hipGetLastError() == hipSuccess);
    CHECK(timed.begin(stream) == hipSuccess);
    CHECK(hipMemsetAsync(word.p, 0, sizeof(u32), stream) == hipSuccess);
    CHECK(timed.end(stream) == hipSuccess);
    CHECK(hipStreamSynchronize(stream) == hipSuccess);
    CHECK(timed.elapsed_ms(&ms) && std::isfinite(ms) && ms >= 0.0);
  }
  {
    DevBuf<u32> buf;
    CHECK(buf.alloc(0) == COX_OK && buf.p != nullptr);  // a count of 0 is one element
    CHECK(buf.p && hipMemset(buf.p, 0, sizeof(u32)) == hipSuccess);
    u32* const held = buf.release();
    CHECK(buf.p == nullptr && held != nullptr);
    u32* mine = held;
    dev_free(&mine);
    DevBuf<float> scoped;
    CHECK(scoped.alloc(1000) == COX_OK && scoped.p != nullptr);
  }
  CHECK(hipDeviceSynchronize() == hipSuccess);
  CHECK(g_quiet == hipSuccess && hipGetLastError() == hipSuccess);
}

int main(int argc, char** argv) {
  const bool want_gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
  g_quiet = hipGetLastError();
  check_finite_all();
  check_status_mapping();
  check_noop_growth();
  const bool have_device = device_present() == COX_OK;
  if (want_gpu) {
    if (!have_device) {
      std::fprintf(stderr, "hostutil_smoke gpu: no device\n");
      return 2;
    }
    check_with_device();
  } else if (!have_device) {
    check_without_device();
  }
  std::printf("%s\n", have_device ? "device" : "no-device");
  if (g_failures) std::fprintf(stderr, "%d check(s) failed\n", g_failures);
  return g_failures ? 1 : 0;
}
