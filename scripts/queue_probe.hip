// Which streams of one process share a hardware queue?  
//
//   hipcc --offload-arch=gfx950 -O2 -o queue_probe scripts/queue_probe.hip
//   queue_probe N            N non-blocking streams created back to back after the null stream has been used (as a torch host has)
//   queue_probe N before     ... after N other streams were created and destroyed (an integrator that came and went before)
//   queue_probe N after      ... and N more created behind them and destroyed again (bench.py's clock ramp: a second integrator dropped)
//
// For every pair of streams (the null stream included) two independent kernels of one workgroup each spin on wall_clock64() for
// about 200 us.  Each writes down when it started and ended; two kernels whose intervals overlap ran side by side (`|`), two that
// did not ran back to back (`B`): their streams share a queue, or queues that one pipe serves in turn.  The number of hardware
// queues is the runtime's (GPU_MAX_HW_QUEUES, 4 when unset); the probe leaves the environment alone and prints what it found.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(x)                                                                            \
  do {                                                                                      \
    const hipError_t e_ = (x);                                                              \
    if (e_ != hipSuccess) {                                                                 \
      std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      std::exit(2);                                                                         \
    }                                                                                       \
  } while (0)

// one workgroup; out[0] = first tick, out[1] = last tick.  Bounded by an iteration count as well, so that it ends whatever the clock does.
__global__ void k_spin(unsigned long long ticks, unsigned long long* out) {
  const unsigned long long t0 = wall_clock64();
  unsigned long long t = t0;
  for (unsigned it = 0; it < 4000000u && t - t0 < ticks; ++it) t = wall_clock64();
  if (threadIdx.x == 0) {
    out[0] = t0;
    out[1] = t;
  }
}

int main(int argc, char** argv) {
  const int n = argc > 1 ? std::atoi(argv[1]) : 4;
  const char* mode = argc > 2 ? argv[2] : "";
  if (n < 1 || n > 16) {
    std::fprintf(stderr, "usage: queue_probe N [before|after]   (1 <= N <= 16)\n");
    return 2;
  }
  int khz = 0;
  CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, 0));
  if (khz <= 0) khz = 100000;
  const unsigned long long ticks = 200ull * static_cast<unsigned long long>(khz) / 1000ull;  // 200 us
  unsigned long long* d_out = nullptr;
  unsigned long long h[4];
  CHECK(hipMalloc(&d_out, sizeof(h)));
  CHECK(hipMemset(d_out, 0, sizeof(h)));
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, nullptr, ticks / 20, d_out);  // the null stream first, as a torch host uses it
  CHECK(hipDeviceSynchronize());

  auto create = [](int count) {
    std::vector<hipStream_t> s(count);
    for (hipStream_t& x : s) CHECK(hipStreamCreateWithFlags(&x, hipStreamNonBlocking));
    return s;
  };
  auto destroy = [](std::vector<hipStream_t>& s) {
    for (hipStream_t x : s) CHECK(hipStreamDestroy(x));
    s.clear();
  };
  if (std::strcmp(mode, "before") == 0) {
    std::vector<hipStream_t> gone = create(n);
    for (hipStream_t x : gone) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, x, ticks / 20, d_out);
    CHECK(hipDeviceSynchronize());
    destroy(gone);
  }
  std::vector<hipStream_t> st = create(n);
  if (std::strcmp(mode, "after") == 0) {
    std::vector<hipStream_t> gone = create(n);
    for (hipStream_t x : gone) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, x, ticks / 20, d_out);
    CHECK(hipDeviceSynchronize());
    destroy(gone);
  }
  st.insert(st.begin(), nullptr);  // index 0: the null stream
  const int m = n + 1;
  for (hipStream_t x : st) hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, x, ticks / 20, d_out);  // every stream once, untimed
  CHECK(hipDeviceSynchronize());

  std::vector<char> rel(static_cast<size_t>(m) * m, '.');
  std::vector<double> both_us(static_cast<size_t>(m) * m, 0.0);
  for (int i = 0; i < m; ++i) {
    for (int j = i + 1; j < m; ++j) {
      int side = 0;
      double span = 0.0;
      for (int rep = 0; rep < 3; ++rep) {  // three times, the second and third in the other order of launch
        const int a = (rep & 1) ? j : i, b = (rep & 1) ? i : j;
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st[a], ticks, d_out);
        hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, st[b], ticks, d_out + 2);
        CHECK(hipStreamSynchronize(st[a]));
        CHECK(hipStreamSynchronize(st[b]));
        CHECK(hipMemcpy(h, d_out, sizeof(h), hipMemcpyDeviceToHost));
        const bool overlap = h[2] < h[1] && h[0] < h[3];
        side += overlap ? 1 : 0;
        const unsigned long long lo = h[0] < h[2] ? h[0] : h[2], hi = h[1] > h[3] ? h[1] : h[3];
        span += static_cast<double>(hi - lo) * 1000.0 / khz / 3.0;
      }
      rel[i * m + j] = rel[j * m + i] = side == 3 ? '|' : side == 0 ? 'B' : '?';
      both_us[i * m + j] = both_us[j * m + i] = span;
    }
  }
  const char* q = std::getenv("GPU_MAX_HW_QUEUES");
  std::printf("queue_probe: %d streams%s%s, GPU_MAX_HW_QUEUES=%s, wall clock %d kHz, two kernels of %.0f us each\n", n, mode[0] ? " " : "", mode,
              q ? q : "(unset)", khz, static_cast<double>(ticks) * 1000.0 / khz);
  std::printf("  ('|' side by side, 'B' back to back, '?' differed between three tries; 0 = the null stream, 1.. in creation order)\n     ");
  for (int j = 0; j < m; ++j) std::printf("%3d", j);
  std::printf("\n");
  for (int i = 0; i < m; ++i) {
    std::printf("  %3d", i);
    for (int j = 0; j < m; ++j) std::printf("  %c", rel[i * m + j]);
    std::printf("\n");
  }
  // streams that ran back to back with one another, as groups (the queues, if the relation is what it should be)
  std::vector<int> group(m);
  for (int i = 0; i < m; ++i) group[i] = i;
  for (int i = 0; i < m; ++i)
    for (int j = i + 1; j < m; ++j)
      if (rel[i * m + j] == 'B') {
        const int g = group[j], to = group[i];
        for (int k = 0; k < m; ++k)
          if (group[k] == g) group[k] = to;
      }
  std::printf("  groups:");
  int n_groups = 0;
  for (int g = 0; g < m; ++g) {
    bool any = false;
    for (int k = 0; k < m; ++k)
      if (group[k] == g) {
        std::printf("%s%d", any ? "," : " {", k);
        any = true;
      }
    if (any) {
      std::printf("}");
      ++n_groups;
    }
  }
  double lo_side = 1e30, hi_side = 0, lo_back = 1e30, hi_back = 0;
  for (int i = 0; i < m; ++i)
    for (int j = i + 1; j < m; ++j) {
      const double v = both_us[i * m + j];
      if (rel[i * m + j] == '|') lo_side = v < lo_side ? v : lo_side, hi_side = v > hi_side ? v : hi_side;
      if (rel[i * m + j] == 'B') lo_back = v < lo_back ? v : lo_back, hi_back = v > hi_back ? v : hi_back;
    }
  std::printf("   -> %d groups\n  first start to last end of a pair: side by side %.0f-%.0f us, back to back %.0f-%.0f us\n", n_groups, hi_side ? lo_side : 0.0, hi_side,
              hi_back ? lo_back : 0.0, hi_back);
  st.erase(st.begin());
  destroy(st);
  CHECK(hipFree(d_out));
  return 0;
}
