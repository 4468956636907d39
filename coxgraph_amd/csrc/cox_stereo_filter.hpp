// MI355X (gfx950): the two filters on the disparity image of dense stereo, DESIGN.md section 7n steps 7a (3 x 3 median over the
// valid values) and 7b (speckle filter: connected components of the 4-neighbour graph whose links are |a - b| <= range16, the ones
// of at most `window` pixels invalidated).  tests/stereo_filter_ref.py restates both in numpy and these kernels owe it every bit.
// Included by cox_stereo.hip (the matcher) and by cox_selftest.hip (cox_selftest_stereo_filters), which launch the kernels through
// the same two functions, stf_launch_median and stf_launch_speckle; everything is static, each unit gets its own copies.
//
//   k_stf_median         7a: 32 x 8 pixels per workgroup from an LDS tile with a one-pixel apron, a 9-element sorting network
//   k_stf_label_local    7b: union-find of one 32 x 8 tile in LDS; every pixel leaves with parent = the tile-local root, as a global index
//   k_stf_label_border       one thread per pixel on a tile's left or upper border unites it with its neighbour across the border
//   k_stf_label_flatten      every pixel finds its root: parent becomes the label image; sizes are added onto the roots
//   k_stf_apply              components of at most `window` pixels become invalid
//
// Why nothing here can spin.  parent[i] <= i holds at all times: the local pass writes the least index of a pixel's tile-local
// component, a union only ever lowers a ROOT's parent with an atomic min to a smaller index, and the flatten pass replaces a
// parent by an ancestor.  A find therefore descends strictly and ends after at most i steps, and it stops at the first parent that
// is not smaller than its pixel, so that no value it could ever read sends it out of the array or in a circle.  A union's retry
// happens only when the atomic min found that somebody else had already lowered the root, to a strictly smaller index, with which
// it goes on: every retry starts from a strictly smaller pixel.  No loop waits for a value another workgroup has yet to write, there
// is no grid barrier and no cooperative launch; the passes are separated by stream order alone, and within a pass parents go
// through relaxed agent-scope atomics.  Every other loop is bounded by a compile-time constant.
// Every index is formed from w, h <= 2^15, so w * h <= 2^30 fits a u32 with 0xFFFFFFFF left over for "no label".
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cox_stf {

typedef uint16_t u16;
typedef uint32_t u32;

constexpr int kThreads = 256;
constexpr int kTileW = 32, kTileH = 8;  // the tile of k_stf_median and of k_stf_label_local: one thread per pixel
constexpr u16 kInvalid = 0xFFFF;
constexpr u32 kNoLabel = 0xFFFFFFFFu;
// the counters of a filtered frame, in the order of cox_stereo_filter_stats
constexpr int kCntMedianChanged = 0, kCntComponents = 1, kCntSpeckleComponents = 2, kCntSpecklePixels = 3, kCntWords = 4;

static_assert(kTileW * kTileH == kThreads, "one thread per pixel of a tile");

// ---- 7a --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void stf_cswap(u32& a, u32& b) {
  const u32 lo = min(a, b), hi = max(a, b);
  a = lo, b = hi;
}

// `out` takes 7a of `in`; `out2_or_null` takes the same image again.  Never in place.
static __global__ void __launch_bounds__(kThreads) k_stf_median(const u16* __restrict__ in, int w, int h, u16* __restrict__ out,
                                                                u16* __restrict__ out2_or_null, u32* __restrict__ counters) {
  constexpr int TW = kTileW + 2, TH = kTileH + 2;
  __shared__ u16 tile[TH][TW];
  __shared__ u32 block_changed;
  const int bx = blockIdx.x * kTileW, by = blockIdx.y * kTileH;
  if (threadIdx.x == 0) block_changed = 0;
  for (int t = threadIdx.x; t < TW * TH; t += kThreads) {
    const int ty = t / TW, tx = t - ty * TW;
    const int gx = bx + tx - 1, gy = by + ty - 1;
    // outside the image: invalid, read only by pixels 7a does not apply to anyway
    tile[ty][tx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? in[static_cast<size_t>(gy) * w + gx] : kInvalid;
  }
  __syncthreads();
  const int lx = threadIdx.x % kTileW, ly = threadIdx.x / kTileW;
  const int x = bx + lx, y = by + ly;
  const bool inside = x < w && y < h;
  bool changed = false;
  if (inside) {
    const u32 own = tile[ly + 1][lx + 1];
    u32 res = own;
    if (own != kInvalid && x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
      u32 v[9];
#pragma unroll
      for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) v[3 * dy + dx] = tile[ly + dy][lx + dx];
      int n = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) n += v[k] != kInvalid;
      // a sorting network of 25 exchanges in 7 layers: ascending, so the invalid values (0xFFFF, above every valid one) come last
      stf_cswap(v[0], v[3]), stf_cswap(v[1], v[7]), stf_cswap(v[2], v[5]), stf_cswap(v[4], v[8]);
      stf_cswap(v[0], v[7]), stf_cswap(v[2], v[4]), stf_cswap(v[3], v[8]), stf_cswap(v[5], v[6]);
      stf_cswap(v[0], v[2]), stf_cswap(v[1], v[3]), stf_cswap(v[4], v[5]), stf_cswap(v[7], v[8]);
      stf_cswap(v[1], v[4]), stf_cswap(v[3], v[6]), stf_cswap(v[5], v[7]);
      stf_cswap(v[0], v[1]), stf_cswap(v[2], v[4]), stf_cswap(v[3], v[5]), stf_cswap(v[6], v[8]);
      stf_cswap(v[2], v[3]), stf_cswap(v[4], v[5]), stf_cswap(v[6], v[7]);
      stf_cswap(v[1], v[2]), stf_cswap(v[3], v[4]), stf_cswap(v[5], v[6]);
      const int rank = (n - 1) / 2;  // n >= 1 (the pixel itself): 0 .. 4
#pragma unroll
      for (int k = 0; k < 5; ++k) res = rank == k ? v[k] : res;  // selects, not an indexed register array
      changed = res != own;
    }
    const size_t i = static_cast<size_t>(y) * w + x;
    out[i] = static_cast<u16>(res);
    if (out2_or_null) out2_or_null[i] = static_cast<u16>(res);
  }
  // through LDS: one global atomic per workgroup
  if (changed) atomicAdd(&block_changed, 1u);
  __syncthreads();
  if (threadIdx.x == 0 && block_changed) atomicAdd(&counters[kCntMedianChanged], block_changed);
}

// ---- 7b --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool stf_linked(u32 a, u32 b, int range16) {
  return a != kInvalid && b != kInvalid && abs(static_cast<int>(a) - static_cast<int>(b)) <= range16;
}

// the union-find, over LDS (workgroup scope) or global memory (agent scope)
template <int SCOPE>
__device__ __forceinline__ u32 stf_find(u32* parent, u32 i) {
  for (;;) {
    const u32 p = __hip_atomic_load(&parent[i], __ATOMIC_RELAXED, SCOPE);
    if (p >= i) return i;  // p == i: a root; p > i never happens, and could not lead anywhere if it did
    i = p;                 // strictly smaller
  }
}

template <int SCOPE>
__device__ __forceinline__ void stf_union(u32* parent, u32 a, u32 b) {
  for (;;) {
    a = stf_find<SCOPE>(parent, a);
    b = stf_find<SCOPE>(parent, b);
    if (a == b) return;
    if (a < b) {
      const u32 t = a;
      a = b, b = t;
    }
    // a > b: a root, as far as this thread has seen, takes the smaller root as its parent
    const u32 old = __hip_atomic_fetch_min(&parent[a], b, __ATOMIC_RELAXED, SCOPE);
    if (old >= a) return;  // a was a root
    a = old;               // somebody lowered it first, to old < a: what a belonged to is united with b from there
  }
}

static __global__ void __launch_bounds__(kThreads) k_stf_label_local(const u16* __restrict__ d, int w, int h, int range16, u32* __restrict__ parent,
                                                                     u32* __restrict__ size) {
  __shared__ u16 val[kThreads];
  __shared__ u32 lab[kThreads];
  const int t = threadIdx.x, lx = t % kTileW, ly = t / kTileW;
  const int bx = blockIdx.x * kTileW, by = blockIdx.y * kTileH;
  const int x = bx + lx, y = by + ly;
  const bool inside = x < w && y < h;
  const size_t i = static_cast<size_t>(y) * w + x;
  const u32 v = inside ? d[i] : kInvalid;
  val[t] = static_cast<u16>(v);
  lab[t] = static_cast<u32>(t);
  __syncthreads();
  // tile-local indices order as the global ones do, so the least local index of a component is its least global index in the tile
  if (v != kInvalid) {
    if (lx > 0 && stf_linked(v, val[t - 1], range16)) stf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, t, t - 1);
    if (ly > 0 && stf_linked(v, val[t - kTileW], range16)) stf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, t, t - kTileW);
  }
  __syncthreads();
  if (!inside) return;
  u32 p = kNoLabel;
  if (v != kInvalid) {
    const u32 r = stf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, t);
    p = static_cast<u32>(by + static_cast<int>(r / kTileW)) * static_cast<u32>(w) + static_cast<u32>(bx + static_cast<int>(r % kTileW));
  }
  parent[i] = p;
  size[i] = 0;
}

// vertical borders first (n_vertical = (tiles across - 1) * h pixels, column by column), then the horizontal ones, row by row
static __global__ void __launch_bounds__(kThreads) k_stf_label_border(const u16* __restrict__ d, int w, int h, int range16, u32 n_vertical, u32 n_total,
                                                                      u32* parent) {
  u32 t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= n_total) return;
  int x, y, xn, yn;
  if (t < n_vertical) {
    x = (static_cast<int>(t / static_cast<u32>(h)) + 1) * kTileW, y = static_cast<int>(t % static_cast<u32>(h));
    xn = x - 1, yn = y;
  } else {
    t -= n_vertical;
    y = (static_cast<int>(t / static_cast<u32>(w)) + 1) * kTileH, x = static_cast<int>(t % static_cast<u32>(w));
    xn = x, yn = y - 1;
  }
  if (x >= w || y >= h) return;  // (cannot happen: the counts are formed from the same w and h)
  const u32 i = static_cast<u32>(y) * static_cast<u32>(w) + static_cast<u32>(x), j = static_cast<u32>(yn) * static_cast<u32>(w) + static_cast<u32>(xn);
  if (stf_linked(d[i], d[j], range16)) stf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, i, j);
}

static __global__ void __launch_bounds__(kThreads) k_stf_label_flatten(const u16* __restrict__ d, u32 n_px, u32* parent, u32* size,
                                                                       u32* __restrict__ counters) {
  __shared__ u32 block_roots;
  if (threadIdx.x == 0) block_roots = 0;
  __syncthreads();
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  const bool valid = i < n_px && d[i] != kInvalid;
  u32 r = kNoLabel;
  if (valid) {
    r = stf_find<__HIP_MEMORY_SCOPE_AGENT>(parent, i);
    // an ancestor in place of the parent: parent[i] <= i still holds, and roots do not move in this pass
    __hip_atomic_store(&parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // sizes: the lanes that share the root of the wave's first valid lane add once, together; a wave mostly lies in one component
  const unsigned long long valid_lanes = __ballot(valid);
  if (valid_lanes) {
    const int lane = threadIdx.x & 63, lead = __ffsll(valid_lanes) - 1;
    const u32 r_lead = __shfl(r, lead);
    const unsigned long long same = __ballot(valid && r == r_lead);
    if (lane == lead)
      atomicAdd(&size[r_lead], static_cast<u32>(__popcll(same)));
    else if (valid && r != r_lead)
      atomicAdd(&size[r], 1u);
  }
  if (valid && r == i) atomicAdd(&block_roots, 1u);
  __syncthreads();
  if (threadIdx.x == 0 && block_roots) atomicAdd(&counters[kCntComponents], block_roots);
}

static __global__ void __launch_bounds__(kThreads) k_stf_apply(const u16* __restrict__ d, const u32* __restrict__ labels, const u32* __restrict__ size,
                                                               u32 n_px, u32 window, u16* __restrict__ out, u16* __restrict__ out2_or_null,
                                                               u32* __restrict__ counters) {
  __shared__ u32 block_counts[2];
  if (threadIdx.x < 2) block_counts[threadIdx.x] = 0;
  __syncthreads();
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n_px) {
    u32 v = d[i];
    if (v != kInvalid) {
      const u32 r = labels[i];
      if (size[r] <= window) {
        v = kInvalid;
        atomicAdd(&block_counts[1], 1u);
        if (r == i) atomicAdd(&block_counts[0], 1u);
      }
    }
    out[i] = static_cast<u16>(v);
    if (out2_or_null) out2_or_null[i] = static_cast<u16>(v);
  }
  __syncthreads();
  if (threadIdx.x < 2 && block_counts[threadIdx.x]) atomicAdd(&counters[kCntSpeckleComponents + threadIdx.x], block_counts[threadIdx.x]);
}

// ---- the launches ------------------------------------------------------------------------------------------------------------------
// the ranges of cox_stereo_filter_config
static inline bool stf_config_ok(int median_size, int window, int range16, u32 reserved) {
  return (median_size == 0 || median_size == 3) && window >= 0 && range16 >= 0 && range16 <= 0xFFFE && reserved == 0;
}

// w, h in 1 .. 2^15.  counters: kCntWords words, zeroed by the caller in stream order before.
static inline void stf_launch_median(const u16* in, int w, int h, u16* out, u16* out2_or_null, u32* counters, hipStream_t s) {
  const dim3 grid(static_cast<u32>((w + kTileW - 1) / kTileW), static_cast<u32>((h + kTileH - 1) / kTileH));
  k_stf_median<<<grid, kThreads, 0, s>>>(in, w, h, out, out2_or_null, counters);
}

// parent, size: w * h words each; parent holds the labels afterwards.  0 <= range16 <= 0xFFFE, 1 <= window <= 2^31 - 1.
static inline void stf_launch_speckle(const u16* in, int w, int h, int window, int range16, u32* parent, u32* size, u16* out, u16* out2_or_null,
                                      u32* counters, hipStream_t s) {
  const u32 tiles_x = static_cast<u32>((w + kTileW - 1) / kTileW), tiles_y = static_cast<u32>((h + kTileH - 1) / kTileH);
  const u32 n_px = static_cast<u32>(w) * static_cast<u32>(h), px_groups = (n_px + kThreads - 1) / kThreads;
  k_stf_label_local<<<dim3(tiles_x, tiles_y), kThreads, 0, s>>>(in, w, h, range16, parent, size);
  const u32 n_vertical = (tiles_x - 1) * static_cast<u32>(h), n_total = n_vertical + (tiles_y - 1) * static_cast<u32>(w);  // < 2 w h / 8
  if (n_total) k_stf_label_border<<<(n_total + kThreads - 1) / kThreads, kThreads, 0, s>>>(in, w, h, range16, n_vertical, n_total, parent);
  k_stf_label_flatten<<<px_groups, kThreads, 0, s>>>(in, n_px, parent, size, counters);
  k_stf_apply<<<px_groups, kThreads, 0, s>>>(in, parent, size, n_px, static_cast<u32>(window), out, out2_or_null, counters);
}

}  // namespace cox_stf
