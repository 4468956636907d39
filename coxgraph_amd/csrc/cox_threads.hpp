// The integrator's host threads: the submission thread that enqueues the layer-update half of every frame, and the helpers of the
// bounce copy of pageable inputs.  Host code only (the submission thread binds its device; the copy helpers never touch HIP).
#pragma once
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// ---- submission thread ------------------------------------------------------------------------------------------------
// At 5 cm a frame is 24 launches plus a dozen event operations, and on a box with slow host cores the caller's thread, not
// the GPU, would set the frame rate.  The caller's thread enqueues ray generation (stages H, P, M) and returns; this thread
// enqueues the layer update (T, R, U) of the same frame behind it (at most one frame behind: the per-slot events it records are
// waited for by the caller's thread three and six frames later).
struct Submitter {
  std::thread th;
  std::mutex m;
  std::condition_variable cv_job, cv_done;
  std::deque<std::function<int()>> q;
  uint64_t posted = 0, finished = 0;
  int status = COX_OK;  // first error of a job; reported (and cleared) by the next drain
  bool stop = false;
  bool ready = false;  // the thread has bound its device
  int device = 0;
  void run() {
    (void)hipSetDevice(device);
    (void)hipGetLastError();
    {
      std::lock_guard<std::mutex> lk(m);
      ready = true;
    }
    cv_done.notify_all();
    for (;;) {
      std::function<int()> job;
      {
        std::unique_lock<std::mutex> lk(m);
        cv_job.wait(lk, [&] { return stop || !q.empty(); });
        if (q.empty()) return;
        job = std::move(q.front());
        q.pop_front();
      }
      const int st = job();
      {
        std::lock_guard<std::mutex> lk(m);
        if (st != COX_OK && status == COX_OK) status = st;
        finished += 1;
      }
      cv_done.notify_all();
    }
  }
  void post(std::function<int()> job) {
    {
      std::lock_guard<std::mutex> lk(m);
      q.push_back(std::move(job));
      posted += 1;
    }
    cv_job.notify_one();
  }
  // returns when at most `outstanding` posted jobs have not been enqueued completely
  void wait_outstanding(uint64_t outstanding) {
    std::unique_lock<std::mutex> lk(m);
    cv_done.wait(lk, [&] { return posted - finished <= outstanding; });
  }
  int take_status() {
    std::lock_guard<std::mutex> lk(m);
    const int st = status;
    status = COX_OK;
    return st;
  }
};
// Pageable host inputs go through a pinned bounce buffer, and that CPU copy (4.9 MB per 640 x 480 cloud) is the caller's thread's:
// 0.35 ms with one core -- 2 800 frames/s however fast the GPU is.  A few helper threads take a share each (COX_COPY_THREADS, default 3
// beside the caller; 0: the caller alone).  They never touch HIP.
struct CopyPool {
  struct Part {
    void* dst;
    const void* src;
    size_t bytes;
  };
  std::vector<std::thread> th;
  std::mutex m;
  std::condition_variable cv_job, cv_done;
  std::vector<Part> parts;  // one per helper, bytes == 0: nothing to do
  uint64_t generation = 0;
  uint32_t pending = 0;
  bool stop = false;
  explicit CopyPool(int n) {
    parts.resize(static_cast<size_t>(n));
    for (int k = 0; k < n; ++k) th.emplace_back([this, k] { run(k); });
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    cv_job.notify_all();
    for (std::thread& t : th) t.join();
  }
  void run(int k) {
    uint64_t seen = 0;
    for (;;) {
      Part p;
      {
        std::unique_lock<std::mutex> lk(m);
        cv_job.wait(lk, [&] { return stop || generation != seen; });
        if (stop) return;
        seen = generation;
        p = parts[static_cast<size_t>(k)];
      }
      if (p.bytes) memcpy(p.dst, p.src, p.bytes);
      {
        std::lock_guard<std::mutex> lk(m);
        pending -= 1;
      }
      cv_done.notify_one();
    }
  }
  // dst <- src, split between the helpers and the calling thread; returns when all of it is there
  void copy(void* dst, const void* src, size_t bytes) {
    const size_t n = th.size() + 1;
    const size_t share = ((bytes / n) + 63) & ~static_cast<size_t>(63);
    if (th.empty() || bytes < (1u << 18)) {
      memcpy(dst, src, bytes);
      return;
    }
    size_t off = 0;
    {
      std::lock_guard<std::mutex> lk(m);
      for (size_t k = 0; k < th.size(); ++k) {
        const size_t b = std::min(share, bytes - off);
        parts[k] = Part{static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, b};
        off += b;
      }
      pending = static_cast<uint32_t>(th.size());
      generation += 1;
    }
    cv_job.notify_all();
    if (off < bytes) memcpy(static_cast<char*>(dst) + off, static_cast<const char*>(src) + off, bytes - off);
    std::unique_lock<std::mutex> lk(m);
    cv_done.wait(lk, [&] { return pending == 0; });
  }
};
