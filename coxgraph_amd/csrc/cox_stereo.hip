// MI355X (gfx950): dense stereo, a raw 8-bit pair to a depth image.  DESIGN.md section 7n is the specification (steps R and 1-8);
// tests/stereo_ref.py restates it in numpy and this file owes it every bit.
//
// One frame, all on the handle's one stream, no host read:
//   k_st_remap    x2   step 1: one thread per pixel, 5-bit bilinear weights; the left one also writes the mask
//   k_st_census   x2   step 2: 32 x 8 pixels per workgroup from an LDS tile with a 4 x 3 apron; bit 63 of a word says "has a census"
//   k_st_path<K>  x4|8 steps 3-4: ONE WAVE WALKS ONE PATH LINE.  Lane l holds the K = D / 64 consecutive disparities l K .. l K + K - 1
//                      of L(q, .) in registers from step to step; the d +- 1 neighbours of a lane's first and last disparity come
//                      from the lanes next to it and min_k L(q, k) is a wave reduction, both as DPP moves; costs are formed on
//                      the fly from the census words, which are loaded a step ahead.  The first direction stores S, the others add into it: the directions run one
//                      after the other on the stream, so the read-modify-write needs no atomics.
//   k_st_winner        steps 5 and 7: one wave per pixel reads S(x, y, .) contiguously
//   k_st_right         dR of step 6: one wave per right pixel
//   k_st_depth         steps 6 and 8, the disparity image, rgba and the counts
//
// With a filter switched on (include/coxgraph_hip_stereo_filter.h; both are off until cox_stereo_set_filters) the tail of the chain is
//   k_st_depth<false>  step 6 alone: the disparity before the filters, rgba, the two rejection counts
//   stf_launch_median  step 7a and stf_launch_speckle step 7b, of cox_stereo_filter.hpp, whichever is on
//   k_st_step8         step 8 on the filtered disparity: depth and its two counts
// still one stream, a fixed chain, no allocation and no host read.  With both off the chain above is untouched.
//
// Every loop is bounded by a launch-time constant (the length of a line, K); no kernel waits for another workgroup; a wave of
// a path kernel never diverges: the line, its length and every branch on them are wave-uniform, lanes differ in data only.
// Every index is formed in size_t from values checked at create: w, h <= 2^15 and w * h * D <= 2^31.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>

#include "../../include/coxgraph_hip_stereo_filter.h"
#include "cox_host.hpp"
#include "cox_stereo_filter.hpp"

namespace {

typedef unsigned long long ull;
typedef uint16_t u16;
typedef uint8_t u8;

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWavesPerGroup = kThreads / kWave;
constexpr int kCensusW = 32, kCensusH = 8, kApronX = 4, kApronY = 3;  // the tile of k_st_census: 256 threads
constexpr ull kHasCensus = 1ull << 63;
constexpr int kNoCensusCost = 62;
constexpr int kAbsent = 1 << 14;  // above every L + P1 (L <= 62 + 255)
constexpr int kDepthPixelsPerThread = 4;  // k_st_depth
constexpr int kPathSets = 4;              // k_st_path: register sets of step inputs, loaded kPathSets - 1 steps ahead
constexpr int kStages = 5;        // remap, census, paths, winner, depth
// the counters of a frame
constexpr int kCntValid = 0, kCntUnique = 1, kCntLr = 2, kCntDepth = 3, kCntWords = 4;
// k_st_winner's word per pixel: d16 in bits 0-15, d0 in bits 16-24, bit 31: rejected by uniqueness
constexpr u32 kWinUniqueBit = 1u << 31;

// ---- step 1 ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_st_remap(const u8* __restrict__ in, const float* __restrict__ map_xy, int w, int h,
                                                       u8* __restrict__ out, u8* __restrict__ mask_or_null) {
  const size_t n = static_cast<size_t>(w) * h;
  const size_t i = static_cast<size_t>(blockIdx.x) * kThreads + threadIdx.x;
  if (i >= n) return;
  if (map_xy == nullptr) {
    out[i] = in[i];
    if (mask_or_null) mask_or_null[i] = 0;
    return;
  }
  const float mx = map_xy[2 * i], my = map_xy[2 * i + 1];
  const float fx = floorf(mx * 32.0f + 0.5f), fy = floorf(my * 32.0f + 0.5f);
  // in-source: 0 <= ix <= 32 (w - 1), which is x0 + 1 <= w - 1, or x0 = w - 1 with ax = 0; NaN and infinities fail the comparisons
  const bool inside = isfinite(mx) && isfinite(my) && fx >= 0.0f && fx <= static_cast<float>(32 * (w - 1)) && fy >= 0.0f &&
                      fy <= static_cast<float>(32 * (h - 1));
  u32 v = 0;
  if (inside) {
    const int ix = static_cast<int>(fx), iy = static_cast<int>(fy);
    const int x0 = ix >> 5, ax = ix & 31, y0 = iy >> 5, ay = iy & 31;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);  // weight 0 where clamped
    const u32 a = in[static_cast<size_t>(y0) * w + x0], b = in[static_cast<size_t>(y0) * w + x1];
    const u32 c = in[static_cast<size_t>(y1) * w + x0], d = in[static_cast<size_t>(y1) * w + x1];
    v = (a * (32 - ax) * (32 - ay) + b * ax * (32 - ay) + c * (32 - ax) * ay + d * ax * ay + 512u) >> 10;
  }
  out[i] = static_cast<u8>(v);
  if (mask_or_null) mask_or_null[i] = inside ? 0 : 1;
}

// ---- step 2 ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_st_census(const u8* __restrict__ img, int w, int h, ull* __restrict__ census) {
  constexpr int TW = kCensusW + 2 * kApronX, TH = kCensusH + 2 * kApronY;
  __shared__ u8 tile[TH][TW];
  const int bx = blockIdx.x * kCensusW, by = blockIdx.y * kCensusH;
  for (int t = threadIdx.x; t < TW * TH; t += kThreads) {
    const int ty = t / TW, tx = t - ty * TW;
    const int gx = bx + tx - kApronX, gy = by + ty - kApronY;
    // outside the image: 0, read only by pixels that have no census anyway
    tile[ty][tx] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? img[static_cast<size_t>(gy) * w + gx] : static_cast<u8>(0);
  }
  __syncthreads();
  const int lx = threadIdx.x % kCensusW, ly = threadIdx.x / kCensusW;
  const int x = bx + lx, y = by + ly;
  if (x >= w || y >= h) return;
  ull word = 0;
  if (x >= kApronX && x < w - kApronX && y >= kApronY && y < h - kApronY) {
    const u8 centre = tile[ly + kApronY][lx + kApronX];
    int bit = 0;
#pragma unroll
    for (int dy = 0; dy < 2 * kApronY + 1; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2 * kApronX + 1; ++dx) {
        if (dy == kApronY && dx == kApronX) continue;
        word |= static_cast<ull>(tile[ly + dy][lx + dx] < centre) << bit;
        ++bit;
      }
    word |= kHasCensus;
  }
  census[static_cast<size_t>(y) * w + x] = word;
}

// ---- steps 3-4 ---------------------------------------------------------------------------------------------------------------------
// Cross-lane moves in the VALU (DPP), not through the LDS crossbar: the min over a line's disparities and the d +- 1 neighbours
// are on the chain of dependent steps of a path, where six ds_bpermute round trips per step were most of a step's time.
// A lane whose source does not exist (lane 0 of a shift up, lane 63 of a shift down) keeps `old`.
template <int kCtrl>
__device__ __forceinline__ int dpp(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, kCtrl, 0xf, 0xf, false);
}
constexpr int kDppRowRor = 0x120;   // + n: rotate right by n within each row of 16 lanes
constexpr int kDppWaveShl1 = 0x130; // lane l takes lane l + 1
constexpr int kDppWaveShr1 = 0x138; // lane l takes lane l - 1

// the minimum over the 64 lanes, in every lane; all 64 lanes must be active
__device__ __forceinline__ int wave_min(int v) {
  v = min(v, dpp<kDppRowRor + 1>(v, v));
  v = min(v, dpp<kDppRowRor + 2>(v, v));
  v = min(v, dpp<kDppRowRor + 4>(v, v));
  v = min(v, dpp<kDppRowRor + 8>(v, v));  // every lane: the minimum of its row
  return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// a lane's K sums of S, moved as one word: (pixel * D + lane * K) * 2 bytes is a multiple of 2 K
template <int K>
struct alignas(2 * K) SumVec {
  u16 v[K];
};

// what one step of a path reads from memory: nothing of it depends on the chain
template <int K>
struct StepInput {
  ull left;        // cL(p)
  ull right[K];    // cR(x - d, y) for the lane's K disparities; 0 (no census) where x - d < 0
  SumVec<K> sum;   // S(p, .) as the directions before this one left it
};

// Every load is unconditional (addresses are clamped, values selected afterwards): the compiler then counts exactly how many loads
// are in flight and a step waits for its own input only, not for the input of the step after it.
template <int K, bool FIRST>
__device__ __forceinline__ void load_step(StepInput<K>& in, const ull* __restrict__ cl, const ull* __restrict__ cr, const u16* S, int w, int x, int y,
                                          int d_lo) {
  const size_t row = static_cast<size_t>(y) * w;
  in.left = cl[row + x];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int xr = x - d_lo - k;
    const ull v = cr[row + max(xr, 0)];
    in.right[k] = xr >= 0 ? v : 0ull;
  }
  if (!FIRST) in.sum = *reinterpret_cast<const SumVec<K>*>(S + (row + x) * (K * kWave) + d_lo);
}

// steps 3-4 at one pixel: L(q, .) and its minimum m become L(p, .) and its minimum; S(p, .) takes L(p, .)
template <int K, bool FIRST>
__device__ __forceinline__ void path_step(const StepInput<K>& in, int p1, int p2, int (&L)[K], int& m, u16* S, int w, int x, int y, int d_lo) {
  int C[K];
#pragma unroll
  for (int k = 0; k < K; ++k) C[k] = ((in.left & in.right[k]) >> 63) ? __popcll(in.left ^ in.right[k]) : kNoCensusCost;
  const int below = dpp<kDppWaveShr1>(kAbsent, L[K - 1]);  // L(q, d_lo - 1); absent below d = 0
  const int above = dpp<kDppWaveShl1>(kAbsent, L[0]);      // L(q, d_lo + K); absent above d = D - 1
  int Ln[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int lo = k == 0 ? below : L[k - 1];
    const int hi = k == K - 1 ? above : L[k + 1];
    Ln[k] = C[k] + min(min(L[k], m + p2), min(lo, hi) + p1) - m;
  }
  int mine = Ln[0];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    L[k] = Ln[k];
    mine = min(mine, Ln[k]);
  }
  m = wave_min(mine);
  SumVec<K> out;
#pragma unroll
  for (int k = 0; k < K; ++k) out.v[k] = static_cast<u16>(FIRST ? L[k] : in.sum.v[k] + L[k]);
  *reinterpret_cast<SumVec<K>*>(S + (static_cast<size_t>(y) * w + x) * (K * kWave) + d_lo) = out;  // one store of 2 K bytes
}

// FIRST: the first direction of a frame stores S, the others add into it
template <int K, bool FIRST>
__global__ void __launch_bounds__(kThreads) k_st_path(const ull* __restrict__ cl, const ull* __restrict__ cr, int w, int h, int dx, int dy, int p1,
                                                      int p2, u16* S) {
  const int lane = threadIdx.x & (kWave - 1);
  // wave-uniform from here to the loop bound
  const int line = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x) * kWavesPerGroup + static_cast<int>(threadIdx.x >> 6));
  int x0, y0, n_lines;
  if (dy == 0) {  // horizontal: one line per row
    n_lines = h;
    x0 = dx > 0 ? 0 : w - 1;
    y0 = line;
  } else if (dx == 0) {  // vertical: one line per column
    n_lines = w;
    x0 = line;
    y0 = dy > 0 ? 0 : h - 1;
  } else {  // diagonal: lines start on the row the path enters by (w of them), then on the column it enters by (h - 1)
    n_lines = w + h - 1;
    if (line < w) {
      x0 = line;
      y0 = dy > 0 ? 0 : h - 1;
    } else {
      x0 = dx > 0 ? 0 : w - 1;
      y0 = dy > 0 ? line - w + 1 : h - 1 - (line - w + 1);
    }
  }
  if (line >= n_lines) return;  // the whole wave
  const int nx = dx > 0 ? w - x0 : (dx < 0 ? x0 + 1 : w + h);
  const int ny = dy > 0 ? h - y0 : (dy < 0 ? y0 + 1 : w + h);
  const int len = min(nx, ny);  // >= 1: the pixels (x0 + i dx, y0 + i dy), i < len, are the line

  const int d_lo = lane * K;
  // L = 0 and m = 0 in front of the line make the first step's L(p, d) = C(p, d): min(0, P2, P1) - 0 = 0
  int L[K];
#pragma unroll
  for (int k = 0; k < K; ++k) L[k] = 0;
  int m = 0;
  // A step's input is loaded kPathSets - 1 steps ahead, into the register set the step before that has finished with: a line is one
  // wave on its SIMD, nothing else hides the latency, and a step is shorter than a trip to memory.  kPathSets steps per turn of the
  // loop, so that no set is ever copied (a copy would wait for the load).  The steps after the last one load the last pixel again
  // (clamped) into sets nobody reads.
  StepInput<K> in[kPathSets];
#pragma unroll
  for (int j = 0; j < kPathSets - 1; ++j) {
    const int ij = min(j, len - 1);
    load_step<K, FIRST>(in[j], cl, cr, S, w, x0 + ij * dx, y0 + ij * dy, d_lo);
  }
  for (int i = 0; i < len; i += kPathSets) {
#pragma unroll
    for (int j = 0; j < kPathSets; ++j) {
      if (i + j >= len) return;  // the whole wave
      const int ia = min(i + j + kPathSets - 1, len - 1);
      load_step<K, FIRST>(in[(j + kPathSets - 1) % kPathSets], cl, cr, S, w, x0 + ia * dx, y0 + ia * dy, d_lo);
      path_step<K, FIRST>(in[j], p1, p2, L, m, S, w, x0 + (i + j) * dx, y0 + (i + j) * dy, d_lo);
    }
  }
}

// ---- steps 5 and 7 -----------------------------------------------------------------------------------------------------------------
// lane l reads disparities l, l + 64, ...: contiguous across the wave
template <int K>
__global__ void __launch_bounds__(kThreads) k_st_winner(const u16* __restrict__ S, u32 n_px, int uniqueness, u32* __restrict__ win) {
  constexpr int D = K * kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const u32 pix = blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (pix >= n_px) return;  // the whole wave
  const u16* s = S + static_cast<size_t>(pix) * D;
  int v[K];
  int key = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = s[k * kWave + lane];
    key = min(key, (v[k] << 16) | (k * kWave + lane));  // the lowest S, then the lowest d: first wins
  }
  key = wave_min(key);
  const int d0 = key & 0xffff, m0 = key >> 16;
  bool beaten = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int d = k * kWave + lane;
    beaten = beaten || (abs(d - d0) > 1 && v[k] * (100 - uniqueness) < m0 * 100);
  }
  const bool rejected = __any(beaten);
  if (lane == 0) {
    int d16 = 16 * d0;
    if (d0 > 0 && d0 < D - 1) {
      const int sm = s[d0 - 1], sp = s[d0 + 1];
      const int den = max(sm + sp - 2 * m0, 1);
      const int num = (sm - sp) * 16 + den;
      d16 += num / (2 * den);  // truncates toward zero
    }
    win[pix] = static_cast<u32>(d16) | (static_cast<u32>(d0) << 16) | (rejected ? kWinUniqueBit : 0u);
  }
}

// dR of step 6: one wave per right pixel
template <int K>
__global__ void __launch_bounds__(kThreads) k_st_right(const u16* __restrict__ S, int w, u32 n_px, u16* __restrict__ d_right) {
  constexpr int D = K * kWave;
  const int lane = threadIdx.x & (kWave - 1);
  const u32 pix = blockIdx.x * kWavesPerGroup + (threadIdx.x >> 6);
  if (pix >= n_px) return;  // the whole wave
  const int xr = static_cast<int>(pix % static_cast<u32>(w));
  int key = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int d = k * kWave + lane;
    if (xr + d < w) key = min(key, (static_cast<int>(S[(static_cast<size_t>(pix) + d) * D + d]) << 16) | d);
  }
  key = wave_min(key);  // d = 0 is always there
  if (lane == 0) d_right[pix] = static_cast<u16>(key & 0xffff);
}

// ---- steps 6 and 8 -----------------------------------------------------------------------------------------------------------------
// STEP8 false: step 6 alone, for a frame whose disparity goes through the filters first (depth is not touched, nor its two counts)
template <bool STEP8>
__global__ void __launch_bounds__(kThreads) k_st_depth(const u32* __restrict__ win, const u16* __restrict__ d_right, const ull* __restrict__ cl,
                                                       const u8* __restrict__ mask, const u8* __restrict__ rect_left, int w, u32 n_px, int lr_max_diff,
                                                       float fB16, float min_depth, float max_depth, float* __restrict__ depth,
                                                       u8* __restrict__ rgba_or_null, u16* __restrict__ disparity, u16* __restrict__ disparity_user_or_null,
                                                       u32* __restrict__ counters) {
  __shared__ u32 block_counts[kCntWords];
  if (threadIdx.x < kCntWords) block_counts[threadIdx.x] = 0;
  __syncthreads();
  u32 n_valid = 0, n_unique = 0, n_lr = 0, n_depth = 0;
  for (int j = 0; j < kDepthPixelsPerThread; ++j) {
    const size_t pix64 = (static_cast<size_t>(blockIdx.x) * kDepthPixelsPerThread + j) * kThreads + threadIdx.x;
    if (pix64 >= n_px) break;
    const u32 pix = static_cast<u32>(pix64);
    const u32 wd = win[pix];
    const int d16 = wd & 0xffff, d0 = (wd >> 16) & 0x1ff;
    const bool usable = (cl[pix] >> 63) != 0 && mask[pix] == 0;
    const bool rej_unique = (wd & kWinUniqueBit) != 0;
    bool rej_lr = false;
    if (lr_max_diff >= 0) {
      const int x = static_cast<int>(pix % static_cast<u32>(w));
      rej_lr = x - d0 < 0 || abs(static_cast<int>(d_right[pix - d0]) - d0) > lr_max_diff;
    }
    const bool valid = usable && !rej_unique && !rej_lr && d16 > 0;
    if (STEP8) {
      float z = __builtin_nanf("");
      if (valid) {
        const float zz = fB16 / static_cast<float>(d16);
        if (zz < min_depth || zz > max_depth)
          ++n_depth;
        else
          z = zz, ++n_valid;
      }
      depth[pix] = z;
    }
    n_unique += usable && rej_unique;
    n_lr += usable && !rej_unique && rej_lr;
    const u16 dv = valid ? static_cast<u16>(d16) : static_cast<u16>(0xffff);
    disparity[pix] = dv;
    if (disparity_user_or_null) disparity_user_or_null[pix] = dv;
    if (rgba_or_null) {
      const u32 g = rect_left[pix];
      reinterpret_cast<u32*>(rgba_or_null)[pix] = g | (g << 8) | (g << 16) | 0xff000000u;
    }
  }
  // through LDS: one global atomic per workgroup and counter (one per wave took as long as the rest of the kernel)
  if (n_valid) atomicAdd(&block_counts[kCntValid], n_valid);
  if (n_unique) atomicAdd(&block_counts[kCntUnique], n_unique);
  if (n_lr) atomicAdd(&block_counts[kCntLr], n_lr);
  if (n_depth) atomicAdd(&block_counts[kCntDepth], n_depth);
  __syncthreads();
  if (threadIdx.x < kCntWords && block_counts[threadIdx.x]) atomicAdd(&counters[threadIdx.x], block_counts[threadIdx.x]);
}

// step 8 alone, on the disparity image the filters left
__global__ void __launch_bounds__(kThreads) k_st_step8(const u16* __restrict__ disparity, u32 n_px, float fB16, float min_depth, float max_depth,
                                                       float* __restrict__ depth, u32* __restrict__ counters) {
  __shared__ u32 block_counts[2];
  if (threadIdx.x < 2) block_counts[threadIdx.x] = 0;
  __syncthreads();
  u32 n_valid = 0, n_depth = 0;
  for (int j = 0; j < kDepthPixelsPerThread; ++j) {
    const size_t pix = (static_cast<size_t>(blockIdx.x) * kDepthPixelsPerThread + j) * kThreads + threadIdx.x;
    if (pix >= n_px) break;
    const int d16 = disparity[pix];
    float z = __builtin_nanf("");
    if (d16 != 0xffff) {
      const float zz = fB16 / static_cast<float>(d16);
      if (zz < min_depth || zz > max_depth)
        ++n_depth;
      else
        z = zz, ++n_valid;
    }
    depth[pix] = z;
  }
  if (n_valid) atomicAdd(&block_counts[0], n_valid);
  if (n_depth) atomicAdd(&block_counts[1], n_depth);
  __syncthreads();
  if (threadIdx.x == 0 && block_counts[0]) atomicAdd(&counters[kCntValid], block_counts[0]);
  if (threadIdx.x == 1 && block_counts[1]) atomicAdd(&counters[kCntDepth], block_counts[1]);
}

// ---- step R (host) -----------------------------------------------------------------------------------------------------------------
struct V3 {
  double x, y, z;
};
V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 normalized(V3 a) {
  const double n = std::sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return V3{a.x / n, a.y / n, a.z / n};
}

// unit quaternion (w >= 0 branch first) of a rotation matrix, row-major
void quaternion_of(const double M[9], float q[4]) {
  const double tr = M[0] + M[4] + M[8];
  double w, x, y, z;
  if (tr > 0.0) {
    const double s = std::sqrt(tr + 1.0) * 2.0;
    w = 0.25 * s, x = (M[7] - M[5]) / s, y = (M[2] - M[6]) / s, z = (M[3] - M[1]) / s;
  } else if (M[0] > M[4] && M[0] > M[8]) {
    const double s = std::sqrt(1.0 + M[0] - M[4] - M[8]) * 2.0;
    w = (M[7] - M[5]) / s, x = 0.25 * s, y = (M[1] + M[3]) / s, z = (M[2] + M[6]) / s;
  } else if (M[4] > M[8]) {
    const double s = std::sqrt(1.0 + M[4] - M[0] - M[8]) * 2.0;
    w = (M[2] - M[6]) / s, x = (M[1] + M[3]) / s, y = 0.25 * s, z = (M[5] + M[7]) / s;
  } else {
    const double s = std::sqrt(1.0 + M[8] - M[0] - M[4]) * 2.0;
    w = (M[3] - M[1]) / s, x = (M[2] + M[6]) / s, y = (M[5] + M[7]) / s, z = 0.25 * s;
  }
  const double n = std::sqrt(w * w + x * x + y * y + z * z) * (w < 0.0 ? -1.0 : 1.0);
  q[0] = static_cast<float>(w / n), q[1] = static_cast<float>(x / n), q[2] = static_cast<float>(y / n), q[3] = static_cast<float>(z / n);
}

bool config_ok(const cox_stereo_config& c) {
  if (c.n_disparities != 64 && c.n_disparities != 128 && c.n_disparities != 256) return false;
  if (c.n_paths != 4 && c.n_paths != 8) return false;
  if (c.p1 < 0 || c.p1 > c.p2 || c.p2 > 255) return false;
  if (c.uniqueness_percent < 0 || c.uniqueness_percent > 99) return false;
  if (std::isnan(c.min_depth_m) || std::isnan(c.max_depth_m) || c.min_depth_m < 0.0f || c.max_depth_m < c.min_depth_m) return false;
  return c.reserved == 0;
}

bool filter_config_ok(const cox_stereo_filter_config& c) {
  return cox_stf::stf_config_ok(c.median_size, c.speckle_window, c.speckle_range16, c.reserved);
}

}  // namespace

struct cox_stereo {
  int device = 0;
  int w = 0, h = 0;
  cox_stereo_config cfg{};
  float fB16 = 0.0f;
  bool have_maps = false, have_frame = false, timed = false;
  Stream stream;
  Event ev_in, ev_read;  // the producer's work so far; the frame has read its inputs
  Event ev_t[kStages + 1];
  DevBuf<float> d_map0, d_map1;
  DevBuf<u8> d_in_left, d_in_right;  // staging of cox_stereo_compute
  DevBuf<u8> d_rect_left, d_rect_right, d_mask;
  DevBuf<ull> d_census_left, d_census_right;
  DevBuf<u16> d_S, d_right, d_disparity;
  DevBuf<u32> d_win, d_counters;
  DevBuf<float> d_depth;  // outputs of cox_stereo_compute before they go to the host
  DevBuf<u8> d_rgba;
  PinnedBuf<u32> h_counters;
  // the filters on the disparity (coxgraph_hip_stereo_filter.h): nothing below exists until one is switched on
  cox_stereo_filter_config fcfg{0, 0, 16, 0};
  bool filter_bufs = false;
  bool last_filtered = false, last_labelled = false;  // of the last frame
  const u16* last_median = nullptr;                   // where the last frame left the image after 7a
  DevBuf<u16> f_raw, f_median;
  DevBuf<u32> f_parent, f_size, f_counters;
  PinnedBuf<u32> h_fcounters;
  Event ev_f[3];  // behind step 6, behind 7a, behind 7b

  int acquire(size_t n_px) {
    COX_TRY(stream.create());
    COX_TRY(ev_in.create(false));
    COX_TRY(ev_read.create(false));
    for (Event& e : ev_t) COX_TRY(e.create(true));
    if (have_maps) {
      COX_TRY(d_map0.alloc(2 * n_px));
      COX_TRY(d_map1.alloc(2 * n_px));
    }
    COX_TRY(d_in_left.alloc(n_px));
    COX_TRY(d_in_right.alloc(n_px));
    COX_TRY(d_rect_left.alloc(n_px));
    COX_TRY(d_rect_right.alloc(n_px));
    COX_TRY(d_mask.alloc(n_px));
    COX_TRY(d_census_left.alloc(n_px));
    COX_TRY(d_census_right.alloc(n_px));
    COX_TRY(d_S.alloc(n_px * static_cast<size_t>(cfg.n_disparities)));
    COX_TRY(d_right.alloc(n_px));
    COX_TRY(d_disparity.alloc(n_px));
    COX_TRY(d_win.alloc(n_px));
    COX_TRY(d_counters.alloc(kCntWords));
    COX_TRY(d_depth.alloc(n_px));
    COX_TRY(d_rgba.alloc(4 * n_px));
    return h_counters.alloc(kCntWords);
  }
  // nothing of it exists until a filter is switched on; what a failed attempt got stays for the next one
  int acquire_filters(size_t n_px) {
    for (Event& e : ev_f)
      if (!e) COX_TRY(e.create(true));
    if (!f_raw) COX_TRY(f_raw.alloc(n_px));
    if (!f_median) COX_TRY(f_median.alloc(n_px));
    if (!f_parent) COX_TRY(f_parent.alloc(n_px));
    if (!f_size) COX_TRY(f_size.alloc(n_px));
    if (!f_counters) COX_TRY(f_counters.alloc(cox_stf::kCntWords));
    if (!h_fcounters) COX_TRY(h_fcounters.alloc(cox_stf::kCntWords));
    return COX_OK;
  }
};

namespace {

size_t n_px_of(const cox_stereo* H) { return static_cast<size_t>(H->w) * H->h; }

template <int K>
int launch_paths_and_winner(cox_stereo* H) {
  static const int kDirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, 1}, {1, -1}, {-1, -1}};
  const int w = H->w, h = H->h;
  const u32 n_px = static_cast<u32>(n_px_of(H));
  hipStream_t s = H->stream;
  for (int i = 0; i < H->cfg.n_paths; ++i) {
    const int dx = kDirs[i][0], dy = kDirs[i][1];
    const int n_lines = dy == 0 ? h : (dx == 0 ? w : w + h - 1);
    const u32 groups = static_cast<u32>((n_lines + kWavesPerGroup - 1) / kWavesPerGroup);
    if (i == 0)
      k_st_path<K, true><<<groups, kThreads, 0, s>>>(H->d_census_left, H->d_census_right, w, h, dx, dy, H->cfg.p1, H->cfg.p2, H->d_S);
    else
      k_st_path<K, false><<<groups, kThreads, 0, s>>>(H->d_census_left, H->d_census_right, w, h, dx, dy, H->cfg.p1, H->cfg.p2, H->d_S);
  }
  COX_HIP(hipEventRecord(H->ev_t[3], s));
  const u32 wave_groups = (n_px + kWavesPerGroup - 1) / kWavesPerGroup;
  k_st_winner<K><<<wave_groups, kThreads, 0, s>>>(H->d_S, n_px, H->cfg.uniqueness_percent, H->d_win);
  if (H->cfg.lr_max_diff >= 0) k_st_right<K><<<wave_groups, kThreads, 0, s>>>(H->d_S, w, n_px, H->d_right);
  COX_HIP(hipEventRecord(H->ev_t[4], s));
  return COX_OK;
}

// one frame from device images; the stream already orders behind their producer, and ev_t[0] is recorded
int enqueue_frame(cox_stereo* H, const u8* left, const u8* right, float* depth, u8* rgba_or_null, u16* disparity_or_null, bool signal_read) {
  const int w = H->w, h = H->h;
  const u32 n_px = static_cast<u32>(n_px_of(H));
  const u32 px_groups = (n_px + kThreads - 1) / kThreads;
  hipStream_t s = H->stream;
  COX_HIP(hipMemsetAsync(H->d_counters, 0, sizeof(u32) * kCntWords, s));
  k_st_remap<<<px_groups, kThreads, 0, s>>>(left, H->have_maps ? H->d_map0 : nullptr, w, h, H->d_rect_left, H->d_mask);
  k_st_remap<<<px_groups, kThreads, 0, s>>>(right, H->have_maps ? H->d_map1 : nullptr, w, h, H->d_rect_right, nullptr);
  if (signal_read) COX_HIP(hipEventRecord(H->ev_read, s));
  COX_HIP(hipEventRecord(H->ev_t[1], s));
  const dim3 census_grid(static_cast<u32>((w + kCensusW - 1) / kCensusW), static_cast<u32>((h + kCensusH - 1) / kCensusH));
  k_st_census<<<census_grid, kThreads, 0, s>>>(H->d_rect_left, w, h, H->d_census_left);
  k_st_census<<<census_grid, kThreads, 0, s>>>(H->d_rect_right, w, h, H->d_census_right);
  COX_HIP(hipEventRecord(H->ev_t[2], s));
  switch (H->cfg.n_disparities) {
    case 64: COX_TRY(launch_paths_and_winner<1>(H)); break;
    case 128: COX_TRY(launch_paths_and_winner<2>(H)); break;
    default: COX_TRY(launch_paths_and_winner<4>(H)); break;
  }
  const u32 depth_groups = (n_px + kThreads * kDepthPixelsPerThread - 1) / (kThreads * kDepthPixelsPerThread);
  const bool median = H->fcfg.median_size == 3, speckle = H->fcfg.speckle_window > 0;
  if (!median && !speckle) {
    k_st_depth<true><<<depth_groups, kThreads, 0, s>>>(H->d_win, H->d_right, H->d_census_left, H->d_mask, H->d_rect_left, w, n_px, H->cfg.lr_max_diff,
                                                    H->fB16, H->cfg.min_depth_m, H->cfg.max_depth_m, depth, rgba_or_null, H->d_disparity,
                                                    disparity_or_null, H->d_counters);
  } else {
    // steps 6, 7a, 7b, 8: the last stage that is on writes the final image, for cox_stereo_download and for the caller
    COX_HIP(hipMemsetAsync(H->f_counters, 0, sizeof(u32) * cox_stf::kCntWords, s));
    k_st_depth<false><<<depth_groups, kThreads, 0, s>>>(H->d_win, H->d_right, H->d_census_left, H->d_mask, H->d_rect_left, w, n_px, H->cfg.lr_max_diff,
                                                     H->fB16, H->cfg.min_depth_m, H->cfg.max_depth_m, nullptr, rgba_or_null, H->f_raw, nullptr,
                                                     H->d_counters);
    COX_HIP(hipEventRecord(H->ev_f[0], s));
    const u16* image = H->f_raw;
    if (median) {
      u16* out = speckle ? H->f_median : H->d_disparity;
      cox_stf::stf_launch_median(image, w, h, out, speckle ? nullptr : disparity_or_null, H->f_counters, s);
      image = out;
    }
    H->last_median = image;
    COX_HIP(hipEventRecord(H->ev_f[1], s));
    if (speckle)
      cox_stf::stf_launch_speckle(image, w, h, H->fcfg.speckle_window, H->fcfg.speckle_range16, H->f_parent, H->f_size, H->d_disparity, disparity_or_null,
                                  H->f_counters, s);
    COX_HIP(hipEventRecord(H->ev_f[2], s));
    k_st_step8<<<depth_groups, kThreads, 0, s>>>(H->d_disparity, n_px, H->fB16, H->cfg.min_depth_m, H->cfg.max_depth_m, depth, H->d_counters);
  }
  COX_HIP(hipGetLastError());
  H->last_filtered = median || speckle;
  H->last_labelled = speckle;
  H->have_frame = true;
  return COX_OK;
}

}  // namespace

extern "C" {

void cox_stereo_config_default(cox_stereo_config* cfg) {
  if (!cfg) return;
  cfg->n_disparities = 128;
  cfg->n_paths = 8;
  cfg->p1 = 7;
  cfg->p2 = 86;
  cfg->uniqueness_percent = 10;
  cfg->lr_max_diff = 1;
  cfg->min_depth_m = 0.0f;
  cfg->max_depth_m = INFINITY;
  cfg->reserved = 0;
}

int cox_stereo_rectify_maps(const cox_stereo_calibration* calib, int w, int h, double scale, float* map0_xy, float* map1_xy, float K_rect[4],
                            float* baseline_m, float T_c0_rect[7]) {
  if (!calib || !map0_xy || !map1_xy || !K_rect || !baseline_m || !T_c0_rect) return COX_ERR_INVALID_ARG;
  if (w < 1 || h < 1 || w > COX_STEREO_MAX_SIDE || h > COX_STEREO_MAX_SIDE || !std::isfinite(scale) || !(scale > 0.0)) return COX_ERR_INVALID_ARG;
  for (const cox_stereo_camera& c : calib->cam)
    if (c.camera_model != 0 || c.distortion_model != 0) return COX_ERR_UNSUPPORTED;
  for (const cox_stereo_camera& c : calib->cam)
    for (int i = 0; i < 4; ++i)
      if (!std::isfinite(c.intrinsics[i]) || !std::isfinite(c.distortion_coeffs[i]) || (i < 2 && !(c.intrinsics[i] > 0.0))) return COX_ERR_INVALID_ARG;
  const double* T = calib->T_cn_cnm1;
  for (int i = 0; i < 12; ++i)
    if (!std::isfinite(T[i])) return COX_ERR_INVALID_ARG;
  const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  const V3 t{T[3], T[7], T[11]};
  // b = -R^T t: cam1's centre in cam0
  const V3 b{-(R[0] * t.x + R[3] * t.y + R[6] * t.z), -(R[1] * t.x + R[4] * t.y + R[7] * t.z), -(R[2] * t.x + R[5] * t.y + R[8] * t.z)};
  const double B = std::sqrt(b.x * b.x + b.y * b.y + b.z * b.z);
  if (!(B > 0.0)) return COX_ERR_INVALID_ARG;
  const V3 e1{b.x / B, b.y / B, b.z / B};
  const V3 zm = normalized(V3{0.0 + R[6], 0.0 + R[7], 1.0 + R[8]});  // (0, 0, 1) + R^T (0, 0, 1)
  const V3 e2 = normalized(cross(zm, e1));
  const V3 e3 = cross(e1, e2);
  const double Rr[9] = {e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, e3.x, e3.y, e3.z};  // cam0 -> rect
  for (double v : Rr)
    if (!std::isfinite(v)) return COX_ERR_INVALID_ARG;
  const cox_stereo_camera &c0 = calib->cam[0], &c1 = calib->cam[1];
  const double f = scale * (c0.intrinsics[0] + c0.intrinsics[1] + c1.intrinsics[0] + c1.intrinsics[1]) / 4.0;
  const double cx = (c0.intrinsics[2] + c1.intrinsics[2]) / 2.0, cy = (c0.intrinsics[3] + c1.intrinsics[3]) / 2.0;
  double M0[9], M1[9];  // M0 = Rr^T, M1 = R Rr^T
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M0[3 * i + j] = Rr[3 * j + i];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) M1[3 * i + j] = (R[3 * i] * M0[j] + R[3 * i + 1] * M0[3 + j]) + R[3 * i + 2] * M0[6 + j];
  const double nan = std::nan("");
  for (int cam = 0; cam < 2; ++cam) {
    const double* M = cam == 0 ? M0 : M1;
    const cox_stereo_camera& c = calib->cam[cam];
    const double k1 = c.distortion_coeffs[0], k2 = c.distortion_coeffs[1], p1 = c.distortion_coeffs[2], p2 = c.distortion_coeffs[3];
    float* out = cam == 0 ? map0_xy : map1_xy;
    for (int v = 0; v < h; ++v)
      for (int u = 0; u < w; ++u) {
        const double rx = (u - cx) / f, ry = (v - cy) / f;
        const double px = (M[0] * rx + M[1] * ry) + M[2], py = (M[3] * rx + M[4] * ry) + M[5], pz = (M[6] * rx + M[7] * ry) + M[8];
        double mx = nan, my = nan;
        if (pz > 0.0) {
          const double x = px / pz, y = py / pz, r2 = x * x + y * y;
          const double rad = 1.0 + k1 * r2 + k2 * r2 * r2;
          const double xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x);
          const double yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y;
          mx = c.intrinsics[0] * xd + c.intrinsics[2];
          my = c.intrinsics[1] * yd + c.intrinsics[3];
        }
        float* o = out + 2 * (static_cast<size_t>(v) * w + u);
        o[0] = static_cast<float>(mx);
        o[1] = static_cast<float>(my);
      }
  }
  K_rect[0] = K_rect[1] = static_cast<float>(f);
  K_rect[2] = static_cast<float>(cx);
  K_rect[3] = static_cast<float>(cy);
  *baseline_m = static_cast<float>(B);
  quaternion_of(M0, T_c0_rect);
  T_c0_rect[4] = T_c0_rect[5] = T_c0_rect[6] = 0.0f;
  return COX_OK;
}

int cox_stereo_create(int device, int w, int h, const cox_stereo_config* cfg, const float* map0_xy, const float* map1_xy, const float K_rect[4],
                      float baseline_m, cox_stereo_t** out) {
  COX_ENTRY_NO_DRAIN();
  if (out) *out = nullptr;
  COX_TRY(device_present());
  int n_dev = 0;
  COX_HIP(hipGetDeviceCount(&n_dev));
  if (!out || !K_rect || device < 0 || device >= n_dev) return COX_ERR_INVALID_ARG;
  if (w < 1 || h < 1 || w > COX_STEREO_MAX_SIDE || h > COX_STEREO_MAX_SIDE) return COX_ERR_INVALID_ARG;
  cox_stereo_config c;
  cox_stereo_config_default(&c);
  if (cfg) c = *cfg;
  if (!config_ok(c)) return COX_ERR_INVALID_ARG;
  const ull n_px = static_cast<ull>(w) * static_cast<ull>(h);
  if (n_px * static_cast<ull>(c.n_disparities) > COX_STEREO_MAX_COST_CELLS) return COX_ERR_INVALID_ARG;
  if ((map0_xy == nullptr) != (map1_xy == nullptr)) return COX_ERR_INVALID_ARG;
  if (!std::isfinite(K_rect[0]) || !(K_rect[0] > 0.0f) || !std::isfinite(baseline_m) || !(baseline_m > 0.0f)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(device));
  cox_stereo* H = new (std::nothrow) cox_stereo();
  if (!H) return COX_ERR_OUT_OF_MEMORY;
  H->device = device;
  H->w = w;
  H->h = h;
  H->cfg = c;
  H->fB16 = static_cast<float>(static_cast<double>(K_rect[0]) * static_cast<double>(baseline_m) * 16.0);
  H->have_maps = map0_xy != nullptr;
  bool ok = H->acquire(n_px) == COX_OK;
  if (ok && H->have_maps) {
    ok = hipMemcpyAsync(H->d_map0, map0_xy, sizeof(float) * 2 * n_px, hipMemcpyHostToDevice, H->stream) == hipSuccess;
    ok = ok && hipMemcpyAsync(H->d_map1, map1_xy, sizeof(float) * 2 * n_px, hipMemcpyHostToDevice, H->stream) == hipSuccess;
    ok = ok && hipStreamSynchronize(H->stream) == hipSuccess;  // the caller's arrays are free again
  }
  if (!ok) {
    (void)hipGetLastError();
    delete H;
    return COX_ERR_OUT_OF_MEMORY;
  }
  *out = H;
  return COX_OK;
}

void cox_stereo_destroy(cox_stereo_t* H) {
  if (!H) return;
  COX_ENTRY_NO_DRAIN();
  (void)hipSetDevice(H->device);
  if (H->stream) (void)hipStreamSynchronize(H->stream);  // nothing of this matcher is in flight after this
  delete H;
}

int cox_stereo_compute_dev(cox_stereo_t* H, const uint8_t* left_dev, const uint8_t* right_dev, float* depth_dev, uint8_t* rgba_dev_or_null,
                           uint16_t* disparity_dev_or_null, void* producer_stream) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !left_dev || !right_dev || !depth_dev) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->device));
  hipStream_t producer = static_cast<hipStream_t>(producer_stream);
  COX_HIP(hipEventRecord(H->ev_in, producer));
  COX_HIP(hipStreamWaitEvent(H->stream, H->ev_in, 0));
  COX_HIP(hipEventRecord(H->ev_t[0], H->stream));
  const int st = enqueue_frame(H, left_dev, right_dev, depth_dev, rgba_dev_or_null, disparity_dev_or_null, true);
  if (st != COX_OK) return st;
  COX_HIP(hipEventRecord(H->ev_t[5], H->stream));
  H->timed = true;
  COX_HIP(hipStreamWaitEvent(producer, H->ev_read, 0));
  return COX_OK;
}

int cox_stereo_compute(cox_stereo_t* H, const uint8_t* left, const uint8_t* right, float* depth, uint8_t* rgba_or_null, uint16_t* disparity_or_null) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !left || !right || !depth) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->device));
  const size_t n_px = n_px_of(H);
  hipStream_t s = H->stream;
  COX_HIP(hipEventRecord(H->ev_t[0], s));
  // the staging buffers are single: in stream order behind the frame that read them last
  COX_HIP(hipMemcpyAsync(H->d_in_left, left, n_px, hipMemcpyHostToDevice, s));
  COX_HIP(hipMemcpyAsync(H->d_in_right, right, n_px, hipMemcpyHostToDevice, s));
  COX_TRY(enqueue_frame(H, H->d_in_left, H->d_in_right, H->d_depth, rgba_or_null ? H->d_rgba.p : nullptr, nullptr, false));
  COX_HIP(hipMemcpyAsync(depth, H->d_depth, sizeof(float) * n_px, hipMemcpyDeviceToHost, s));
  if (rgba_or_null) COX_HIP(hipMemcpyAsync(rgba_or_null, H->d_rgba, 4 * n_px, hipMemcpyDeviceToHost, s));
  if (disparity_or_null) COX_HIP(hipMemcpyAsync(disparity_or_null, H->d_disparity, sizeof(u16) * n_px, hipMemcpyDeviceToHost, s));
  COX_HIP(hipEventRecord(H->ev_t[5], s));
  H->timed = true;
  return COX_OK;
}

void* cox_stereo_stream(cox_stereo_t* H) { return H ? static_cast<void*>(H->stream) : nullptr; }

int cox_stereo_sync(cox_stereo_t* H) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->device));
  COX_HIP(hipStreamSynchronize(H->stream));
  return COX_OK;
}

int cox_stereo_last_stats(cox_stereo_t* H, cox_stereo_stats* out) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !out) return COX_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!H->have_frame) return COX_OK;
  COX_HIP(hipSetDevice(H->device));
  COX_HIP(hipMemcpyAsync(H->h_counters, H->d_counters, sizeof(u32) * kCntWords, hipMemcpyDeviceToHost, H->stream));
  COX_HIP(hipStreamSynchronize(H->stream));
  out->n_valid_pixels = H->h_counters.p[kCntValid];
  out->n_rejected_uniqueness = H->h_counters.p[kCntUnique];
  out->n_rejected_lr = H->h_counters.p[kCntLr];
  out->n_rejected_depth = H->h_counters.p[kCntDepth];
  if (H->timed) {
    double* stage[kStages] = {&out->remap_ms, &out->census_ms, &out->paths_ms, &out->winner_ms, &out->depth_ms};
    float t = 0.0f;
    for (int k = 0; k < kStages; ++k)
      if (hipEventElapsedTime(&t, H->ev_t[k], H->ev_t[k + 1]) == hipSuccess) *stage[k] = t;
    if (hipEventElapsedTime(&t, H->ev_t[0], H->ev_t[kStages]) == hipSuccess) out->frame_ms = t;
    if (H->last_filtered) {  // steps 6 and 8 lie on either side of the filters
      float t6 = 0.0f, t8 = 0.0f;
      if (hipEventElapsedTime(&t6, H->ev_t[kStages - 1], H->ev_f[0]) == hipSuccess && hipEventElapsedTime(&t8, H->ev_f[2], H->ev_t[kStages]) == hipSuccess)
        out->depth_ms = static_cast<double>(t6) + static_cast<double>(t8);
    }
    (void)hipGetLastError();
  }
  return COX_OK;
}

int cox_stereo_download(cox_stereo_t* H, int which, void* buf, uint64_t cap_bytes) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !buf || !H->have_frame) return COX_ERR_INVALID_ARG;
  const size_t n_px = n_px_of(H);
  const void* src = nullptr;
  size_t bytes = 0;
  switch (which) {
    case COX_STEREO_RECT_LEFT: src = H->d_rect_left, bytes = n_px; break;
    case COX_STEREO_RECT_RIGHT: src = H->d_rect_right, bytes = n_px; break;
    case COX_STEREO_COST_SUM: src = H->d_S, bytes = sizeof(u16) * n_px * static_cast<size_t>(H->cfg.n_disparities); break;
    case COX_STEREO_DISPARITY: src = H->d_disparity, bytes = sizeof(u16) * n_px; break;
    default: return COX_ERR_INVALID_ARG;
  }
  if (cap_bytes < bytes) return COX_ERR_BUFFER_TOO_SMALL;
  COX_HIP(hipSetDevice(H->device));
  COX_HIP(hipMemcpyAsync(buf, src, bytes, hipMemcpyDeviceToHost, H->stream));
  COX_HIP(hipStreamSynchronize(H->stream));
  return COX_OK;
}

// ---- the filters on the disparity (coxgraph_hip_stereo_filter.h) ------------------------------------------------------------------
void cox_stereo_filter_config_default(cox_stereo_filter_config* cfg) {
  if (!cfg) return;
  cfg->median_size = 0;
  cfg->speckle_window = 0;
  cfg->speckle_range16 = 16;
  cfg->reserved = 0;
}

int cox_stereo_set_filters(cox_stereo_t* H, const cox_stereo_filter_config* cfg) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  cox_stereo_filter_config c;
  cox_stereo_filter_config_default(&c);
  if (cfg) c = *cfg;
  if (!filter_config_ok(c)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->device));
  COX_HIP(hipStreamSynchronize(H->stream));
  if ((c.median_size != 0 || c.speckle_window > 0) && !H->filter_bufs) {
    if (H->acquire_filters(n_px_of(H)) != COX_OK) return COX_ERR_OUT_OF_MEMORY;  // the setting does not change
    H->filter_bufs = true;
  }
  H->fcfg = c;
  return COX_OK;
}

int cox_stereo_get_filters(cox_stereo_t* H, cox_stereo_filter_config* out) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !out) return COX_ERR_INVALID_ARG;
  *out = H->fcfg;
  return COX_OK;
}

int cox_stereo_filter_last_stats(cox_stereo_t* H, cox_stereo_filter_stats* out) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !out) return COX_ERR_INVALID_ARG;
  std::memset(out, 0, sizeof(*out));
  if (!H->have_frame) return COX_OK;
  COX_HIP(hipSetDevice(H->device));
  if (!H->last_filtered) {
    COX_HIP(hipStreamSynchronize(H->stream));
    return COX_OK;
  }
  COX_HIP(hipMemcpyAsync(H->h_fcounters, H->f_counters, sizeof(u32) * cox_stf::kCntWords, hipMemcpyDeviceToHost, H->stream));
  COX_HIP(hipStreamSynchronize(H->stream));
  out->n_median_changed = H->h_fcounters.p[cox_stf::kCntMedianChanged];
  out->n_components = H->h_fcounters.p[cox_stf::kCntComponents];
  out->n_speckle_components = H->h_fcounters.p[cox_stf::kCntSpeckleComponents];
  out->n_speckle_pixels = H->h_fcounters.p[cox_stf::kCntSpecklePixels];
  float t = 0.0f;
  if (hipEventElapsedTime(&t, H->ev_f[0], H->ev_f[1]) == hipSuccess) out->median_ms = t;
  if (hipEventElapsedTime(&t, H->ev_f[1], H->ev_f[2]) == hipSuccess) out->speckle_ms = t;
  (void)hipGetLastError();
  return COX_OK;
}

int cox_stereo_filter_download(cox_stereo_t* H, int which, void* buf, uint64_t cap_bytes) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !buf || !H->have_frame || !H->last_filtered) return COX_ERR_INVALID_ARG;
  const size_t n_px = n_px_of(H);
  const void* src = nullptr;
  size_t bytes = 0;
  switch (which) {
    case COX_STEREO_FILTER_DISPARITY_RAW: src = H->f_raw, bytes = sizeof(u16) * n_px; break;
    case COX_STEREO_FILTER_DISPARITY_MEDIAN: src = H->last_median, bytes = sizeof(u16) * n_px; break;
    case COX_STEREO_FILTER_LABELS:
      if (!H->last_labelled) return COX_ERR_INVALID_ARG;
      src = H->f_parent, bytes = sizeof(u32) * n_px;
      break;
    default: return COX_ERR_INVALID_ARG;
  }
  if (cap_bytes < bytes) return COX_ERR_BUFFER_TOO_SMALL;
  COX_HIP(hipSetDevice(H->device));
  COX_HIP(hipMemcpyAsync(buf, src, bytes, hipMemcpyDeviceToHost, H->stream));
  COX_HIP(hipStreamSynchronize(H->stream));
  return COX_OK;
}

}  // extern "C"
