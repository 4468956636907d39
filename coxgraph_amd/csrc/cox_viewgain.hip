// MI355X (gfx950): scoring candidate views behind include/coxgraph_hip_gain.h -- which voxels would a ray-casting sensor see from
// each of a batch of poses, each voxel once per view, and what are they worth?
//
//   k_vg_prep     one workgroup per view: the view's pose, and the box of voxel indices its samples can reach.  A sample's voxel
//                 index is a monotone function of the sample's coordinate, and that coordinate (o + d * dir, one multiply and one
//                 add) is monotone in d, so on every axis the index of a sample lies between the indices of o and of
//                 o + ray_length * dir: the box over all rays of those two is exact, no sample falls outside it.  Zeroes the
//                 view's counters.
//   k_vg_march    one lane per ray, one wave per 8 x 8 tile of the ray grid, the grid over (view, tile): one launch covers a chunk
//                 of views.  A ray steps one sample at a time, keeps the pool index of the last block it resolved (one hash look-up
//                 per block crossed), loads only the distance and weight words, and ends behind its first occupied voxel.  "Each
//                 voxel once per view" is a per-view bitmap over the box: the lane whose atomicOr flips a voxel's bit owns it --
//                 classifies it, values it, does the frontier look-ups.  A plain load that shows the bit set skips the atomic (bits
//                 never clear, a stale 0 only costs the atomic).  Owners' contributions are summed across the wave, then one
//                 atomic per wave and counter.  All sums are integers: a record does not depend on which lane got where first.
//   k_vg_finish   the records from the counters.
//   k_vg_compact  cox_viewgain_visible: a running scan over the bitmap's words; ascending bit order is ascending (z, y, x).
//
// Bitmap words, counters and what the march reads (layer, rays, view boxes) live in allocations of their own: the atomics run at
// the memory side and drop their line from L2.  Rules and arithmetic: DESIGN.md section 7j.  The float expressions are those of
// tests/cpp/viewgain_reference.cpp, one by one.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/coxgraph_hip_gain.h"
#include "cox_host.hpp"
#include "cox_interp.hpp"

using namespace cox;

namespace {

typedef unsigned long long ull;

constexpr int kThreads = 256;          // 4 waves, one 8 x 8 tile each
constexpr int kCompactThreads = 1024;  // one workgroup walks the bitmap
constexpr int kIdxLimit = 1 << 24;     // voxel indices of in-range samples lie in [-2^24, 2^24)
constexpr u32 kViewEmpty = 1u;         // the origin is not finite or outside the index range: no sample
constexpr u32 kViewOverflow = 2u;      // the box does not fit the view's share of the workspace
constexpr float kMaxSteps = 1048576.0f;  // samples a ray may take (ray_length / step)
constexpr u64 kMaxViews = 1ull << 24;
// counters of a view: 128 B, a line of their own
enum : int { C_VISIBLE = 0, C_FREE, C_OCCUPIED, C_COUNTED, C_UNKNOWN, C_FRONTIER, C_Q32, C_SAMPLES, C_OUTSIDE, C_WORDS = 16 };
// totals of a call
enum : int { T_SAMPLES = 0, T_OVERFLOW, T_OUTSIDE, T_WORDS = 4 };
enum : u32 { S_FREE = 0, S_OCCUPIED = 1, S_UNKNOWN = 2 };

struct GainParams {
  int w, h;
  u32 tiles_x, tiles_per_view;
  float min_range, ray_length, step, min_weight, surface_distance;
  float frontier_weight, new_weight, min_impact, ray_angle_xy;  // ray_angle_x * ray_angle_y
  int accurate, surface_frontiers, use_box;
  float box_min[3], box_max[3];
  u32 max_dim;     // a view's box may be this long on an axis
  u64 slot_words;  // bitmap words per view
};

struct ViewInfo {  // 64 B
  float q[4], o[3];
  int lo[3];
  u32 dim[3];
  u32 flags;
  u32 pad[2];
};

__device__ __forceinline__ F3 rotate(const float q[4], F3 v) { return quat_rotate(q[0], q[1], q[2], q[3], v); }

__device__ __forceinline__ bool coord_in_range(const LayerView& L, float p) { return index_in_range(p * L.block_size_inv); }  // false for NaN, +-inf

__device__ __forceinline__ bool block_in_range(int b) { return b >= -kIdxBias && b < kIdxBias; }

// rule 3 for voxel v of pool block `pool` (kInvalid: unallocated); the weight too when the block exists
__device__ __forceinline__ u32 voxel_state(const LayerView& L, const GainParams& P, u32 pool, int vx, int vy, int vz, float* weight) {
  if (pool == kInvalid) return S_UNKNOWN;
  const u32* vox = voxel_ptr(L, pool, vx, vy, vz);
  const float d = __uint_as_float(vox[0]), w = __uint_as_float(vox[1]);
  *weight = w;
  if (!(w > P.min_weight)) return S_UNKNOWN;
  return d <= P.surface_distance ? S_OCCUPIED : S_FREE;
}

__device__ __forceinline__ float centre_coord(const LayerView& L, int b, int v) {  // the free-points expression
  return static_cast<float>(b) * L.block_size + (static_cast<float>(v) + 0.5f) * L.voxel_size;
}

__device__ __forceinline__ bool centre_in_box(const LayerView& L, const GainParams& P, const int b[3], const int v[3]) {
  bool in = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float c = centre_coord(L, b[k], v[k]);
    in = in && !(c < P.box_min[k]) && !(c > P.box_max[k]);
  }
  return in;
}

// rule 5, unknown voxel (b, v) whose block has pool index `pool`: does a neighbour make it a frontier?
__device__ __forceinline__ bool is_frontier(const LayerView& L, const GainParams& P, int bx, int by, int bz, int vx, int vy, int vz, u32 pool) {
  // strictly inside an unallocated block every neighbour is unallocated too
  if (pool == kInvalid && vx >= 1 && vx <= 14 && vy >= 1 && vy <= 14 && vz >= 1 && vz <= 14) return false;
  int cbx = bx, cby = by, cbz = bz;  // the last block resolved
  u32 cpool = pool;
#pragma unroll 1
  for (int i = 0; i < 27; ++i) {
    const int dx = i % 3 - 1, dy = (i / 3) % 3 - 1, dz = i / 9 - 1;
    const int axes = (dx != 0) + (dy != 0) + (dz != 0);
    if (axes == 0 || (!P.accurate && axes != 1)) continue;
    int nx = vx + dx, ny = vy + dy, nz = vz + dz, nbx = bx, nby = by, nbz = bz;
    if (nx < 0) nx += 16, --nbx;
    if (nx > 15) nx -= 16, ++nbx;
    if (ny < 0) ny += 16, --nby;
    if (ny > 15) ny -= 16, ++nby;
    if (nz < 0) nz += 16, --nbz;
    if (nz > 15) nz -= 16, ++nbz;
    if (nbx != cbx || nby != cby || nbz != cbz) {
      cbx = nbx, cby = nby, cbz = nbz;
      cpool = (block_in_range(nbx) && block_in_range(nby) && block_in_range(nbz)) ? HtPool{L}(nbx, nby, nbz) : kInvalid;
    }
    float w = 0.0f;
    const u32 s = voxel_state(L, P, cpool, nx, ny, nz, &w);
    if (P.surface_frontiers ? s == S_OCCUPIED : s != S_UNKNOWN) return true;
  }
  return false;
}

// rule 5 for a visible voxel of state s: its class (COX_VG_*), its value, and for an occupied voxel that counts its fixed-point impact
__device__ __forceinline__ u32 voxel_value(const LayerView& L, const GainParams& P, const float o[3], const int b[3], const int v[3], u32 pool, u32 s,
                                           float weight, float* value, bool* counted, u64* q32) {
  *counted = false;
  *value = 0.0f;
  *q32 = 0;
  if (s == S_FREE) return COX_VG_FREE;
  if (s == S_OCCUPIED) {
    const float dx = centre_coord(L, b[0], v[0]) - o[0], dy = centre_coord(L, b[1], v[1]) - o[1], dz = centre_coord(L, b[2], v[2]) - o[2];
    const float z = sqrtf(dx * dx + dy * dy + dz * dz);
    const float a = 2.0f * atan2f(L.voxel_size, 2.0f * z);
    const float nw = a * a / P.ray_angle_xy / (z * z);
    const float imp = nw / (nw + weight);
    if (imp > P.min_impact) {  // false for NaN
      *counted = true;
      *value = imp;
      *q32 = static_cast<u64>(static_cast<double>(imp) * 4294967296.0);
    }
    return COX_VG_OCCUPIED;
  }
  if (P.frontier_weight > 0.0f && is_frontier(L, P, b[0], b[1], b[2], v[0], v[1], v[2], pool)) {
    *value = P.frontier_weight;
    return COX_VG_FRONTIER;
  }
  *value = P.new_weight;
  return COX_VG_UNKNOWN;
}

// ---- the box of a view -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_vg_prep(LayerView L, GainParams P, const float* __restrict__ rays, const float* __restrict__ poses,
                                                       ViewInfo* __restrict__ info, ull* __restrict__ counters) {
  const u32 view = blockIdx.x, tid = threadIdx.x;
  __shared__ int red[6][kThreads / 64];
  float T[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) T[k] = poses[7ull * view + k];
  if (tid < C_WORDS) counters[static_cast<size_t>(view) * C_WORDS + tid] = 0ull;
  const float o[3] = {T[4], T[5], T[6]};
  const bool have_origin = coord_in_range(L, o[0]) && coord_in_range(L, o[1]) && coord_in_range(L, o[2]);  // uniform
  int lo[3] = {kIdxLimit, kIdxLimit, kIdxLimit}, hi[3] = {-kIdxLimit, -kIdxLimit, -kIdxLimit};
  if (have_origin) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      int b, v;
      locate(L, o[k], &b, &v);
      lo[k] = hi[k] = 16 * b + v;
    }
    const u32 n_rays = static_cast<u32>(P.w) * static_cast<u32>(P.h);
    for (u32 i = tid; i < n_rays; i += kThreads) {
      const F3 dg = rotate(T, F3{rays[3ull * i], rays[3ull * i + 1], rays[3ull * i + 2]});
      const float dir[3] = {dg.x, dg.y, dg.z};
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float e = o[k] + P.ray_length * dir[k];
        if (coord_in_range(L, e)) {
          int b, v;
          locate(L, e, &b, &v);
          const int g = 16 * b + v;
          lo[k] = g < lo[k] ? g : lo[k];
          hi[k] = g > hi[k] ? g : hi[k];
        } else {  // the ray leaves the index range (or is not finite): whatever it reaches before that
          lo[k] = -kIdxLimit;
          hi[k] = kIdxLimit - 1;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int a = lo[k], b = hi[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const int a2 = __shfl_xor(a, off), b2 = __shfl_xor(b, off);
      a = a2 < a ? a2 : a;
      b = b2 > b ? b2 : b;
    }
    if ((tid & 63u) == 0u) red[k][tid >> 6] = a, red[3 + k][tid >> 6] = b;
  }
  __syncthreads();
  if (tid == 0) {
    ViewInfo I{};
#pragma unroll
    for (int k = 0; k < 4; ++k) I.q[k] = T[k];
    I.flags = have_origin ? 0u : kViewEmpty;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      I.o[k] = o[k];
      int a = red[k][0], b = red[3 + k][0];
      for (int wv = 1; wv < kThreads / 64; ++wv) {
        a = red[k][wv] < a ? red[k][wv] : a;
        b = red[3 + k][wv] > b ? red[3 + k][wv] : b;
      }
      I.lo[k] = a;
      const u32 dim = have_origin ? static_cast<u32>(b - a) + 1u : 0u;
      I.dim[k] = dim;
      if (dim > P.max_dim) I.flags |= kViewOverflow;
    }
    info[view] = I;
  }
}

// ---- the march ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_vg_march(LayerView L, GainParams P, const float* __restrict__ rays, const ViewInfo* __restrict__ info,
                                                        u32* __restrict__ bitmap, ull* __restrict__ counters, u32 view_base, u32 n_views) {
  const u32 lane = threadIdx.x & 63u;
  const u32 wave = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);  // the same for every lane of a wave
  if (wave >= n_views * P.tiles_per_view) return;
  const u32 slot = wave / P.tiles_per_view, tile = wave % P.tiles_per_view;
  const ViewInfo I = info[view_base + slot];
  if (I.flags) return;
  u32* const bm = bitmap + static_cast<size_t>(slot) * P.slot_words;
  const int u = static_cast<int>((tile % P.tiles_x) * 8u + (lane & 7u)), v = static_cast<int>((tile / P.tiles_x) * 8u + (lane >> 3));
  u32 n_vis = 0, n_free = 0, n_occ = 0, n_cnt = 0, n_unk = 0, n_fro = 0, n_smp = 0, n_out = 0;
  u64 q32 = 0;
  if (u < P.w && v < P.h) {
    const size_t ri = 3ull * (static_cast<size_t>(v) * static_cast<size_t>(P.w) + static_cast<size_t>(u));
    const F3 dg = rotate(I.q, F3{rays[ri], rays[ri + 1], rays[ri + 2]});
    const float o[3] = {I.o[0], I.o[1], I.o[2]}, dir[3] = {dg.x, dg.y, dg.z};
    int lb[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF};  // the block resolved last (no block has this index)
    u32 lpool = kInvalid;
    for (u32 k = 0;; ++k) {
      const float d = static_cast<float>(k) * P.step;
      if (!(d < P.ray_length)) break;
      if (d < P.min_range) continue;
      float p[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) p[c] = o[c] + d * dir[c];
      if (!point_in_range(L, p)) break;  // left the index range (or NaN)
      ++n_smp;
      int b[3], vv[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) locate(L, p[c], &b[c], &vv[c]);
      if (b[0] != lb[0] || b[1] != lb[1] || b[2] != lb[2]) {
        lb[0] = b[0], lb[1] = b[1], lb[2] = b[2];
        lpool = HtPool{L}(b[0], b[1], b[2]);
      }
      float weight = 0.0f;
      const u32 s = voxel_state(L, P, lpool, vv[0], vv[1], vv[2], &weight);
      if (!P.use_box || centre_in_box(L, P, b, vv)) {
        const u32 rx = static_cast<u32>(16 * b[0] + vv[0] - I.lo[0]), ry = static_cast<u32>(16 * b[1] + vv[1] - I.lo[1]),
                  rz = static_cast<u32>(16 * b[2] + vv[2] - I.lo[2]);
        if (rx < I.dim[0] && ry < I.dim[1] && rz < I.dim[2]) {
          const u64 bit = (static_cast<u64>(rz) * I.dim[1] + ry) * I.dim[0] + rx;
          u32* const word = bm + (bit >> 5);
          const u32 mask = 1u << (static_cast<u32>(bit) & 31u);
          bool owner = false;
          if (!(*word & mask)) owner = !(atomicOr(word, mask) & mask);
          if (owner) {
            float value;
            bool counted;
            u64 q;
            const u32 cls = voxel_value(L, P, o, b, vv, lpool, s, weight, &value, &counted, &q);
            ++n_vis;
            n_free += cls == COX_VG_FREE;
            n_occ += cls == COX_VG_OCCUPIED;
            n_cnt += counted;
            n_unk += cls >= COX_VG_UNKNOWN;
            n_fro += cls == COX_VG_FRONTIER;
            q32 += q;
          }
        } else {
          ++n_out;  // cannot happen (see k_vg_prep); reported, never written through
        }
      }
      if (s == S_OCCUPIED) break;
    }
  }
  // one atomic per wave and counter
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    n_vis += __shfl_xor(n_vis, off);
    n_free += __shfl_xor(n_free, off);
    n_occ += __shfl_xor(n_occ, off);
    n_cnt += __shfl_xor(n_cnt, off);
    n_unk += __shfl_xor(n_unk, off);
    n_fro += __shfl_xor(n_fro, off);
    n_smp += __shfl_xor(n_smp, off);
    n_out += __shfl_xor(n_out, off);
    q32 += static_cast<u64>(__shfl_xor(static_cast<ull>(q32), off));
  }
  if (lane == 0u) {
    ull* c = counters + static_cast<size_t>(view_base + slot) * C_WORDS;
    if (n_vis) atomicAdd(c + C_VISIBLE, static_cast<ull>(n_vis));
    if (n_free) atomicAdd(c + C_FREE, static_cast<ull>(n_free));
    if (n_occ) atomicAdd(c + C_OCCUPIED, static_cast<ull>(n_occ));
    if (n_cnt) atomicAdd(c + C_COUNTED, static_cast<ull>(n_cnt));
    if (n_unk) atomicAdd(c + C_UNKNOWN, static_cast<ull>(n_unk));
    if (n_fro) atomicAdd(c + C_FRONTIER, static_cast<ull>(n_fro));
    if (q32) atomicAdd(c + C_Q32, static_cast<ull>(q32));
    if (n_smp) atomicAdd(c + C_SAMPLES, static_cast<ull>(n_smp));
    if (n_out) atomicAdd(c + C_OUTSIDE, static_cast<ull>(n_out));
  }
}

// ---- the records -------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) k_vg_finish(GainParams P, const ViewInfo* __restrict__ info, const ull* __restrict__ counters, u32 n_views,
                                                         cox_view_gain* __restrict__ out, ull* __restrict__ totals) {
  const u32 view = blockIdx.x * kThreads + threadIdx.x;
  if (view >= n_views) return;
  const ull* c = counters + static_cast<size_t>(view) * C_WORDS;
  cox_view_gain r;
  r.surface_gain_q32 = c[C_Q32];
  r.n_visible = static_cast<u32>(c[C_VISIBLE]);
  r.n_free = static_cast<u32>(c[C_FREE]);
  r.n_occupied = static_cast<u32>(c[C_OCCUPIED]);
  r.n_surface_counted = static_cast<u32>(c[C_COUNTED]);
  r.n_unknown = static_cast<u32>(c[C_UNKNOWN]);
  r.n_frontier = static_cast<u32>(c[C_FRONTIER]);
  r.surface_gain = static_cast<double>(r.surface_gain_q32) / 4294967296.0;
  r.gain = r.surface_gain + static_cast<double>(P.frontier_weight) * static_cast<double>(r.n_frontier) +
           static_cast<double>(P.new_weight) * static_cast<double>(r.n_unknown - r.n_frontier);
  const bool bad = (info[view].flags & kViewOverflow) != 0u || c[C_OUTSIDE] != 0ull;
  if (bad) r.gain = r.surface_gain = __longlong_as_double(0x7FF8000000000000ll);
  out[view] = r;
  if (totals) {
    if (c[C_SAMPLES]) atomicAdd(totals + T_SAMPLES, c[C_SAMPLES]);
    if (info[view].flags & kViewOverflow) atomicAdd(totals + T_OVERFLOW, 1ull);
    if (c[C_OUTSIDE]) atomicAdd(totals + T_OUTSIDE, 1ull);
  }
}

// ---- the visible set in (z, y, x) order ----------------------------------------------------------------------------------------
// One workgroup walks the bitmap 1024 words at a time with a running offset.  The outputs (any may be null) are written below cap;
// *n_out gets the size of the set either way.
__global__ void __launch_bounds__(kCompactThreads) k_vg_compact(LayerView L, GainParams P, const ViewInfo* __restrict__ info, const u32* __restrict__ bm,
                                                                 u64 cap, int* __restrict__ xyz, uint8_t* __restrict__ cls_out,
                                                                 float* __restrict__ value_out, ull* __restrict__ n_out) {
  __shared__ u32 wave_sum[kCompactThreads / 64];
  const ViewInfo I = info[0];
  const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const u64 n_bits = I.flags ? 0ull : static_cast<u64>(I.dim[0]) * I.dim[1] * I.dim[2];
  const u64 n_words = (n_bits + 31) >> 5;
  const bool emit = cap != 0 && (xyz || cls_out || value_out);
  const float o[3] = {I.o[0], I.o[1], I.o[2]};
  u64 base = 0;
  for (u64 w0 = 0; w0 < n_words; w0 += kCompactThreads) {
    const u64 w = w0 + tid;
    u32 bits = w < n_words ? bm[w] : 0u;
    const u32 cnt = __popc(bits);
    u32 incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const u32 t = __shfl_up(incl, off);
      if (lane >= static_cast<u32>(off)) incl += t;
    }
    if (lane == 63u) wave_sum[wave] = incl;
    __syncthreads();
    u32 before = 0, total = 0;
    for (u32 k = 0; k < kCompactThreads / 64; ++k) {
      before += k < wave ? wave_sum[k] : 0u;
      total += wave_sum[k];
    }
    if (emit) {
      u64 at = base + before + (incl - cnt);
      while (bits) {
        const u32 j = static_cast<u32>(__ffs(bits)) - 1u;
        bits &= bits - 1u;
        if (at < cap) {
          const u64 bit = (w << 5) + j;
          const u64 plane = static_cast<u64>(I.dim[0]) * I.dim[1];
          const int g[3] = {I.lo[0] + static_cast<int>(bit % I.dim[0]), I.lo[1] + static_cast<int>((bit % plane) / I.dim[0]),
                            I.lo[2] + static_cast<int>(bit / plane)};
          const int b[3] = {g[0] >> 4, g[1] >> 4, g[2] >> 4}, v[3] = {g[0] & 15, g[1] & 15, g[2] & 15};
          const u32 pool = HtPool{L}(b[0], b[1], b[2]);
          float weight = 0.0f, value;
          bool counted;
          u64 q;
          const u32 s = voxel_state(L, P, pool, v[0], v[1], v[2], &weight);
          const u32 cls = voxel_value(L, P, o, b, v, pool, s, weight, &value, &counted, &q);
          if (xyz) xyz[3 * at] = g[0], xyz[3 * at + 1] = g[1], xyz[3 * at + 2] = g[2];
          if (cls_out) cls_out[at] = static_cast<uint8_t>(cls);
          if (value_out) value_out[at] = value;
        }
        ++at;
      }
    }
    base += total;
    __syncthreads();  // wave_sum is rewritten by the next strip
  }
  if (tid == 0) *n_out = base;
}

bool config_ok(const cox_viewgain_config& c, float voxel_size) {
  if (c.w <= 0 || c.h <= 0 || static_cast<u64>(c.w) * static_cast<u64>(c.h) > 0x7FFFFFFFull) return false;
  if (!finite_all(c.K, 4) || c.K[0] == 0.0f || c.K[1] == 0.0f) return false;
  const float scalars[] = {c.min_range,         c.ray_length,  c.ray_step,    c.min_weight, c.surface_distance, c.frontier_voxel_weight, c.new_voxel_weight,
                           c.min_impact_factor, c.ray_angle_x, c.ray_angle_y};
  if (!finite_all(scalars, 10)) return false;
  if (!(c.ray_length > c.min_range) || c.min_range < 0.0f || c.ray_step < 0.0f) return false;
  if (!(c.ray_angle_x * c.ray_angle_y > 0.0f)) return false;
  const float step = c.ray_step == 0.0f ? voxel_size : c.ray_step;
  if (!(c.ray_length / step <= kMaxSteps)) return false;  // float(k) stays exact and the march ends
  if (c.use_box) {
    if (!finite_all(c.box_min, 3) || !finite_all(c.box_max, 3)) return false;
    for (int k = 0; k < 3; ++k)
      if (c.box_min[k] > c.box_max[k]) return false;
  }
  return true;
}

}  // namespace

struct cox_viewgain {
  cox_layer* layer = nullptr;
  cox_viewgain_config cfg;
  GainParams P;
  u64 workspace_bytes = 0, slot_bytes = 0;
  Stream stream;
  EventPair ev;
  DevBuf<float> d_rays;  // [h][w][3] dir_C
  DevBuf<u32> d_bitmap;
  DevBuf<ViewInfo> d_info;
  DevBuf<ull> d_counters;
  DevBuf<ull> d_totals;   // T_WORDS, then the visible set's size
  DevBuf<float> d_poses;  // staging of the host entry points
  DevBuf<cox_view_gain> d_out;

  int acquire(const std::vector<float>& rays) {
    COX_TRY(stream.create());
    COX_TRY(ev.create());
    COX_TRY(d_rays.alloc(rays.size()));
    COX_TRY(d_totals.alloc(T_WORDS + 1));
    return cox_hip_status(hipMemcpy(d_rays, rays.data(), rays.size() * sizeof(float), hipMemcpyHostToDevice));
  }
};

namespace {

// prep, (clear, march) per chunk, finish -- enqueued on s.  totals may be null.
int enqueue_views(cox_viewgain* H, const float* poses_dev, u64 n, cox_view_gain* out_dev, ull* totals, hipStream_t s, u64* n_chunks) {
  const GainParams& P = H->P;
  if (H->slot_bytes == 0 || H->slot_bytes > H->workspace_bytes) return COX_ERR_OUT_OF_MEMORY;
  u64 per_chunk = H->workspace_bytes / H->slot_bytes;
  // tiles of a chunk fit the launch grid
  const u64 grid_cap = (0x7FFFFFFFull / P.tiles_per_view);
  if (per_chunk > grid_cap) per_chunk = grid_cap;
  if (per_chunk > n) per_chunk = n;
  if (per_chunk == 0) return COX_ERR_INVALID_ARG;  // more tiles in one view than a grid holds
  COX_TRY(H->d_bitmap.grow(per_chunk * P.slot_words));
  COX_TRY(H->d_info.grow(n));
  COX_TRY(H->d_counters.grow(n * C_WORDS));
  const LayerView V = layer_view(H->layer);  // read on every call: a layer that grew has new buffers
  cox_layer_wait_writes(H->layer, s);        // frames still in flight on the layer
  hipLaunchKernelGGL(k_vg_prep, dim3(static_cast<u32>(n)), dim3(kThreads), 0, s, V, P, H->d_rays, poses_dev, H->d_info, H->d_counters);
  u64 chunks = 0;
  for (u64 base = 0; base < n; base += per_chunk, ++chunks) {
    const u64 nv = n - base < per_chunk ? n - base : per_chunk;
    COX_HIP(hipMemsetAsync(H->d_bitmap, 0, nv * H->slot_bytes, s));
    const u64 waves = nv * P.tiles_per_view;
    hipLaunchKernelGGL(k_vg_march, dim3(static_cast<u32>((waves + kThreads / 64 - 1) / (kThreads / 64))), dim3(kThreads), 0, s, V, P, H->d_rays, H->d_info,
                       H->d_bitmap, H->d_counters, static_cast<u32>(base), static_cast<u32>(nv));
  }
  if (out_dev)
    hipLaunchKernelGGL(k_vg_finish, dim3(static_cast<u32>((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, P, H->d_info, H->d_counters,
                       static_cast<u32>(n), out_dev, totals);
  COX_HIP(hipGetLastError());
  if (n_chunks) *n_chunks = chunks;
  return COX_OK;
}

}  // namespace

extern "C" {

void cox_viewgain_config_default(cox_viewgain_config* cfg) {
  if (!cfg) return;
  cfg->w = 35, cfg->h = 96;
  cfg->K[0] = 64.0f, cfg->K[1] = 64.0f, cfg->K[2] = 17.0f, cfg->K[3] = 48.0f;
  cfg->min_range = 0.0f, cfg->ray_length = 5.0f;
  cfg->ray_step = 0.0f;
  cfg->min_weight = 0.0f;
  cfg->surface_distance = 0.0f;
  cfg->frontier_voxel_weight = 1.0f, cfg->new_voxel_weight = 0.0f, cfg->min_impact_factor = 0.01f;
  cfg->ray_angle_x = 0.002454f, cfg->ray_angle_y = 0.002681f;
  cfg->accurate_frontiers = 1, cfg->surface_frontiers = 1;
  cfg->use_box = 0;
  for (int k = 0; k < 3; ++k) cfg->box_min[k] = cfg->box_max[k] = 0.0f;
  cfg->workspace_bytes = 0;
}

int cox_viewgain_create(cox_layer_t* layer, const cox_viewgain_config* cfg, cox_viewgain_t** out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!layer || !out) return COX_ERR_INVALID_ARG;
  cox_viewgain_config c;
  if (cfg)
    c = *cfg;
  else
    cox_viewgain_config_default(&c);
  if (!config_ok(c, layer->voxel_size)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(layer->device));
  cox_viewgain* H = new (std::nothrow) cox_viewgain();
  if (!H) return COX_ERR_OUT_OF_MEMORY;
  H->layer = layer;
  H->cfg = c;
  GainParams& P = H->P;
  P.w = c.w, P.h = c.h;
  P.tiles_x = static_cast<u32>((c.w + 7) / 8);
  P.tiles_per_view = P.tiles_x * static_cast<u32>((c.h + 7) / 8);
  P.min_range = c.min_range, P.ray_length = c.ray_length;
  P.step = c.ray_step == 0.0f ? layer->voxel_size : c.ray_step;
  P.min_weight = c.min_weight, P.surface_distance = c.surface_distance;
  P.frontier_weight = c.frontier_voxel_weight, P.new_weight = c.new_voxel_weight, P.min_impact = c.min_impact_factor;
  P.ray_angle_xy = c.ray_angle_x * c.ray_angle_y;
  P.accurate = c.accurate_frontiers != 0, P.surface_frontiers = c.surface_frontiers != 0, P.use_box = c.use_box != 0;
  for (int k = 0; k < 3; ++k) P.box_min[k] = c.box_min[k], P.box_max[k] = c.box_max[k];
  // A view's share of the workspace: the cube of voxels within ray_length of the origin's voxel, with 0.1 % for a quaternion that is
  // only nearly of unit length and 4 voxels for rounding (near the edge of the index range a coordinate's ulp is up to 2 voxels).
  const double reach = std::ceil(static_cast<double>(c.ray_length) * 1.001 / static_cast<double>(layer->voxel_size)) + 4.0;
  if (reach < static_cast<double>(kIdxLimit)) {
    const u64 dim = 2 * static_cast<u64>(reach) + 1;
    P.max_dim = static_cast<u32>(dim);
    P.slot_words = (((dim * dim * dim + 31) / 32) + 31) / 32 * 32;  // whole 128-byte lines
  } else {  // no workspace holds this: every evaluation reports COX_ERR_OUT_OF_MEMORY
    P.max_dim = 0;
    P.slot_words = 0;
  }
  H->slot_bytes = P.slot_words * sizeof(u32);
  H->workspace_bytes = c.workspace_bytes ? c.workspace_bytes : (256ull << 20);
  // rule 1: the ray table
  const size_t n_rays = static_cast<size_t>(c.w) * static_cast<size_t>(c.h);
  std::vector<float> rays(3 * n_rays);
  for (int v = 0; v < c.h; ++v)
    for (int u = 0; u < c.w; ++u) {
      const float x = (static_cast<float>(u) - c.K[2]) / c.K[0];
      const float y = (static_cast<float>(v) - c.K[3]) / c.K[1];
      const float n = std::sqrt(x * x + y * y + 1.0f);
      float* r = &rays[3 * (static_cast<size_t>(v) * c.w + u)];
      r[0] = x / n, r[1] = y / n, r[2] = 1.0f / n;
    }
  if (H->acquire(rays) != COX_OK) {
    cox_viewgain_destroy(H);
    return COX_ERR_NO_DEVICE;
  }
  *out = H;
  return COX_OK;
}

void cox_viewgain_destroy(cox_viewgain_t* H) {
  if (!H) return;
  (void)hipSetDevice(H->layer->device);
  if (H->stream) (void)hipStreamSynchronize(H->stream);
  delete H;
}

uint64_t cox_viewgain_view_bytes(const cox_viewgain_t* H) { return H ? H->slot_bytes : 0; }

int cox_viewgain_evaluate(cox_viewgain_t* H, const float* T_G_C, uint64_t n_views, cox_view_gain* out, cox_viewgain_stats* stats) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n_views == 0) return COX_OK;
  if (!T_G_C || !out || n_views > kMaxViews) return COX_ERR_INVALID_ARG;
  for (u64 i = 0; i < n_views; ++i)
    if (!finite_all(T_G_C + 7 * i, 7)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->layer->device));
  COX_TRY(H->d_poses.grow(7 * n_views));
  COX_TRY(H->d_out.grow(n_views));
  hipStream_t s = H->stream;
  COX_HIP(hipMemcpyAsync(H->d_poses, T_G_C, sizeof(float) * 7 * n_views, hipMemcpyHostToDevice, s));
  COX_HIP(hipMemsetAsync(H->d_totals, 0, T_WORDS * sizeof(ull), s));
  COX_HIP(H->ev.begin(s));
  u64 n_chunks = 0;
  COX_TRY(enqueue_views(H, H->d_poses, n_views, H->d_out, H->d_totals, s, &n_chunks));
  COX_HIP(H->ev.end(s));
  ull totals[T_WORDS] = {0, 0, 0, 0};
  COX_HIP(hipMemcpyAsync(totals, H->d_totals, sizeof(totals), hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  if (totals[T_OUTSIDE]) return COX_ERR_INTERNAL;
  if (totals[T_OVERFLOW]) return COX_ERR_OUT_OF_MEMORY;
  COX_HIP(hipMemcpy(out, H->d_out, sizeof(cox_view_gain) * n_views, hipMemcpyDeviceToHost));
  if (stats) {
    if (!H->ev.elapsed_ms(&stats->kernel_ms)) stats->kernel_ms = 0.0;
    stats->n_samples = totals[T_SAMPLES];
    stats->n_chunks = n_chunks;
  }
  return COX_OK;
}

int cox_viewgain_evaluate_dev(cox_viewgain_t* H, const float* poses_dev, uint64_t n_views, cox_view_gain* out_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n_views == 0) return COX_OK;
  if (!poses_dev || !out_dev || n_views > kMaxViews || (reinterpret_cast<uintptr_t>(out_dev) & 7u)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->layer->device));
  return enqueue_views(H, poses_dev, n_views, out_dev, nullptr, static_cast<hipStream_t>(hip_stream), nullptr);
}

int cox_viewgain_visible(cox_viewgain_t* H, const float T_G_C[7], uint64_t cap, int32_t* voxel_xyz, uint8_t* cls, float* value, uint64_t* n) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H || !T_G_C || !n || !finite_all(T_G_C, 7)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->layer->device));
  COX_TRY(H->d_poses.grow(7));
  hipStream_t s = H->stream;
  COX_HIP(hipMemcpyAsync(H->d_poses, T_G_C, sizeof(float) * 7, hipMemcpyHostToDevice, s));
  COX_TRY(enqueue_views(H, H->d_poses, 1, nullptr, nullptr, s, nullptr));
  const LayerView V = layer_view(H->layer);
  ull* d_n = H->d_totals + T_WORDS;
  hipLaunchKernelGGL(k_vg_compact, dim3(1), dim3(kCompactThreads), 0, s, V, H->P, H->d_info, H->d_bitmap, 0ull, nullptr, nullptr, nullptr, d_n);
  ull total = 0;
  COX_HIP(hipMemcpyAsync(&total, d_n, sizeof(ull), hipMemcpyDeviceToHost, s));
  ViewInfo info;
  ull counters[C_WORDS];
  COX_HIP(hipMemcpyAsync(&info, H->d_info, sizeof(ViewInfo), hipMemcpyDeviceToHost, s));
  COX_HIP(hipMemcpyAsync(counters, H->d_counters, sizeof(counters), hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  if (counters[C_OUTSIDE]) return COX_ERR_INTERNAL;
  if (info.flags & kViewOverflow) return COX_ERR_OUT_OF_MEMORY;
  *n = total;
  const bool want = voxel_xyz || cls || value;
  if (!want || total == 0) return COX_OK;
  if (cap < total) return COX_ERR_BUFFER_TOO_SMALL;
  // one staging allocation: xyz | value | cls
  const size_t b_xyz = voxel_xyz ? 12 * total : 0, b_val = value ? 4 * total : 0, b_cls = cls ? total : 0;
  DevBuf<uint8_t> buf;
  COX_TRY(buf.alloc(b_xyz + b_val + b_cls));
  int* d_xyz = voxel_xyz ? reinterpret_cast<int*>(buf.p) : nullptr;
  float* d_val = value ? reinterpret_cast<float*>(buf.p + b_xyz) : nullptr;
  uint8_t* d_cls = cls ? buf.p + b_xyz + b_val : nullptr;
  hipLaunchKernelGGL(k_vg_compact, dim3(1), dim3(kCompactThreads), 0, s, V, H->P, H->d_info, H->d_bitmap, static_cast<u64>(total), d_xyz, d_cls, d_val, d_n);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && voxel_xyz) e = hipMemcpyAsync(voxel_xyz, d_xyz, b_xyz, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && value) e = hipMemcpyAsync(value, d_val, b_val, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess && cls) e = hipMemcpyAsync(cls, d_cls, b_cls, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  return cox_hip_status(e);
}

}  // extern "C"
