// MI355X (gfx950): the voxel-projective integrator of a pinhole depth camera.  DESIGN.md section 7m is the specification (the rule
// of one frame, steps 1-9); tests/cpp/depthfuse_reference.cpp restates it on the CPU and this file owes it every bit.
//
// One frame:
//   candidates  (host)  a box of block indices around the frustum, x fastest: ascending candidate = ascending packed key
//   k_df_valid          step 1's count of valid pixels
//   k_df_select         one workgroup per candidate: conservative cull, one table lookup, steps 2-6 and step 7's first line per
//                       voxel until the first hit; two flags per candidate (touched, new) and the pool index of an existing block
//   scans               exclusive_scan_u32 (cox_sort.hpp) of the two flags; k_df_compact lists the touched candidates
//   host read           n_touched, n_new, the layer's block count and error word, one copy into pinned memory; the pool grows here
//   k_df_update         one workgroup per touched block: a new block takes pool slot nb0 + rank and enters the table; steps 2-7
//
// Every device loop is bounded by a launch-time constant (16 voxels per thread, the table's probe bound, grid strides); no
// kernel waits for another workgroup.  Every grid and buffer is sized on the host from the candidate count, which is checked
// against COX_DEPTHFUSE_MAX_CANDIDATES before anything is enqueued.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/coxgraph_hip_depthfuse.h"
#include "../../include/coxgraph_hip_selftest.h"
#include "cox_host.hpp"
#include "cox_sort.hpp"

using namespace cox;

namespace {

typedef unsigned long long ull;

constexpr int kDfThreads = 256;
constexpr int kDfSlices = kVoxelsPerBlock / kDfThreads;  // 16 voxels per thread
constexpr int kMaxImageSide = 1 << 15;
constexpr size_t kBlockWords = static_cast<size_t>(kVoxelsPerBlock) * kWordsPerVoxel;
// device control block: u32 n_touched, n_new, then (8-byte aligned) u64 valid pixels, updated voxels, coloured voxels
constexpr int kCtlTouched = 0, kCtlNew = 1, kCtlValid64 = 2, kCtlUpdated64 = 4, kCtlColoured64 = 6, kCtlWords = 8;
// behind them, for the host read: the layer's block count and error word as k_df_compact found them
constexpr int kHostNb = kCtlWords, kHostErr = kCtlWords + 1, kHostWords = kCtlWords + 2;

// one frame's constants, by value per launch
struct DfParams {
  float iqw, iqx, iqy, iqz, itx, ity, itz;  // T_C_G = (q*, -rotate(q*, t)), formed on the host in float32
  float fx, fy, cx, cy, u_hi, v_hi;         // u_hi = float(w) - 0.5f
  float voxel_size, trunc, max_weight, min_depth, max_depth, gap;
  int w, h, scheme, carving, const_weight, dropoff;
  int lo_x, lo_y, lo_z;                     // the candidate box
  u32 dim_x, dim_y;
  // the cull: block radius, the four side planes through the camera centre (unit normals (n?x, 0 | n?x, n?z) pointing inwards)
  float radius, pl_x0, pl_z0, pl_x1, pl_z1, pl_y2, pl_z2, pl_y3, pl_z3;
};

struct DfObs {
  float sdf, uw;
  int pu, pv;  // the nearest pixel (colour)
};

__device__ __forceinline__ bool valid_depth(float d) { return isfinite(d) && d > 0.0f; }

// step 2's transform: ((c + w uv) + q.vec x uv) + t'
__device__ __forceinline__ F3 to_camera(const DfParams& P, F3 c) {
  return quat_transform(P.iqw, P.iqx, P.iqy, P.iqz, F3{P.itx, P.ity, P.itz}, c);
}

// step 4
__device__ __forceinline__ bool depth_lookup(const DfParams& P, const float* __restrict__ depth, float u, float v, float* D, int* pu, int* pv) {
  int un = static_cast<int>(floorf(u + 0.5f)), vn = static_cast<int>(floorf(v + 0.5f));
  un = min(max(un, 0), P.w - 1);
  vn = min(max(vn, 0), P.h - 1);
  *pu = un;
  *pv = vn;
  const float nearest = depth[static_cast<size_t>(vn) * P.w + un];
  const int u0 = static_cast<int>(floorf(u)), v0 = static_cast<int>(floorf(v));
  const bool cell = P.scheme != 0 && u0 >= 0 && v0 >= 0 && u0 + 1 <= P.w - 1 && v0 + 1 <= P.h - 1;
  if (!cell) {
    *D = nearest;
    return valid_depth(nearest);
  }
  const float a = depth[static_cast<size_t>(v0) * P.w + u0], b = depth[static_cast<size_t>(v0) * P.w + u0 + 1];
  const float c = depth[static_cast<size_t>(v0 + 1) * P.w + u0], d = depth[static_cast<size_t>(v0 + 1) * P.w + u0 + 1];
  const bool oa = valid_depth(a), ob = valid_depth(b), oc = valid_depth(c), od = valid_depth(d);
  const int n_ok = static_cast<int>(oa) + static_cast<int>(ob) + static_cast<int>(oc) + static_cast<int>(od);
  float mn = INFINITY, mx = -INFINITY;
  if (oa) mn = std_min(mn, a), mx = std_max(mx, a);
  if (ob) mn = std_min(mn, b), mx = std_max(mx, b);
  if (oc) mn = std_min(mn, c), mx = std_max(mx, c);
  if (od) mn = std_min(mn, d), mx = std_max(mx, d);
  if (P.scheme == 1) {
    if (n_ok == 0) return false;
    *D = mn;
    return true;
  }
  if (P.scheme == 3 && n_ok != 0 && mx - mn > P.gap) {
    *D = mn;
    return true;
  }
  if (n_ok != 4) {
    *D = nearest;
    return valid_depth(nearest);
  }
  const float du = u - static_cast<float>(u0), dv = v - static_cast<float>(v0);
  *D = (a * (1.0f - dv) + c * dv) * (1.0f - du) + (b * (1.0f - dv) + d * dv) * du;
  return true;
}

// steps 2-6 of global voxel (gx, gy, gz): false when the rule skips it before step 7
__device__ __forceinline__ bool observe(const DfParams& P, const float* __restrict__ depth, int gx, int gy, int gz, DfObs* o) {
  // step 2
  const F3 c{center_coord(gx, P.voxel_size), center_coord(gy, P.voxel_size), center_coord(gz, P.voxel_size)};
  const F3 q = to_camera(P, c);
  const float z = q.z;
  if (!(P.min_depth <= z && z <= P.max_depth)) return false;
  // step 3
  const float u = P.fx * (q.x / z) + P.cx;
  const float v = P.fy * (q.y / z) + P.cy;
  if (!(-0.5f <= u && u < P.u_hi && -0.5f <= v && v < P.v_hi)) return false;
  // step 4
  float D;
  if (!depth_lookup(P, depth, u, v, &D, &o->pu, &o->pv)) return false;
  // step 5
  const float norm = sqrtf((q.x * q.x + q.y * q.y) + q.z * q.z);
  const float sdf = (D - z) * (norm / z);
  if (sdf < -P.trunc) return false;
  if (!P.carving && sdf > P.trunc) return false;
  // step 6 (update_weight without the sparsity factor)
  float uw = P.const_weight ? 1.0f : 1.0f / (D * D);
  if (P.dropoff && sdf < -P.voxel_size) {
    uw = uw * (P.trunc + sdf) / (P.trunc - P.voxel_size);
    uw = std_max(uw, 0.0f);
  }
  o->sdf = sdf;
  o->uw = uw;
  return true;
}

__device__ __forceinline__ void candidate_block(const DfParams& P, u32 cand, int* bx, int* by, int* bz) {
  const u32 x = cand % P.dim_x, r = cand / P.dim_x;
  *bx = P.lo_x + static_cast<int>(x);
  *by = P.lo_y + static_cast<int>(r % P.dim_y);
  *bz = P.lo_z + static_cast<int>(r / P.dim_y);
}

// May only drop a block that the rule cannot touch: the voxel centres lie within `radius` of the block's centre, and a voxel the
// rule takes has min_depth <= z <= max_depth and projects between the image borders.  The margin carries the float32 error of
// step 2 (a few ulp of the coordinates that enter it), the planes are widened by half a pixel on the host.
__device__ __forceinline__ bool culled(const DfParams& P, int bx, int by, int bz) {
  const float bs = 16.0f * P.voxel_size;
  const F3 c{(static_cast<float>(bx) + 0.5f) * bs, (static_cast<float>(by) + 0.5f) * bs, (static_cast<float>(bz) + 0.5f) * bs};
  const F3 q = to_camera(P, c);
  const float mag = ((fabsf(c.x) + fabsf(c.y)) + fabsf(c.z)) + ((fabsf(P.itx) + fabsf(P.ity)) + fabsf(P.itz));
  const float r = P.radius + 1e-5f * mag;
  if (q.z + r < P.min_depth || q.z - r > P.max_depth) return true;
  if (P.pl_x0 * q.x + P.pl_z0 * q.z < -r) return true;
  if (P.pl_x1 * q.x + P.pl_z1 * q.z < -r) return true;
  if (P.pl_y2 * q.y + P.pl_z2 * q.z < -r) return true;
  if (P.pl_y3 * q.y + P.pl_z3 * q.z < -r) return true;
  return false;
}

// ---- step 1 ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kDfThreads) k_df_valid(const float* __restrict__ depth, u32 n_px, u32* __restrict__ ctl) {
  __shared__ u32 part[kDfThreads / 64];
  u32 mine = 0;
  for (u32 i = blockIdx.x * kDfThreads + threadIdx.x; i < n_px; i += gridDim.x * kDfThreads) mine += valid_depth(depth[i]) ? 1u : 0u;
  mine = wave_sum_u32(mine);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u32 tot = (part[0] + part[1]) + (part[2] + part[3]);
    if (tot) atomicAdd(reinterpret_cast<ull*>(ctl + kCtlValid64), static_cast<ull>(tot));
  }
}

// ---- selection -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kDfThreads) k_df_select(DfParams P, const float* __restrict__ depth, const u32* __restrict__ voxels,
                                                          const u64* __restrict__ ht_keys, const u32* __restrict__ ht_vals, u32 ht_mask, const u32* __restrict__ d_nblocks,
                                                          u32 capacity, u32 n_cand, u32* __restrict__ touched, u32* __restrict__ is_new, u32* __restrict__ pool_of) {
  __shared__ u32 s_pool;
  const u32 cand = blockIdx.x;
  if (cand >= n_cand) return;
  int bx, by, bz;
  candidate_block(P, cand, &bx, &by, &bz);
  if (culled(P, bx, by, bz)) {  // workgroup-uniform
    if (threadIdx.x == 0) touched[cand] = 0u, is_new[cand] = 0u, pool_of[cand] = kInvalid;
    return;
  }
  if (threadIdx.x == 0) {
    u32 pool = kInvalid;
    const u32 slot = ht_find(ht_keys, ht_mask, pack_key(bx, by, bz));
    if (slot != kInvalid) pool = ht_vals[slot];
    const u32 nb0 = min(*d_nblocks, capacity);
    s_pool = pool < nb0 ? pool : kInvalid;  // (a key that an exhausted frame of another writer left without storage counts as missing)
  }
  __syncthreads();
  const u32 pool = s_pool;
  const u32* blk = pool != kInvalid ? voxels + static_cast<size_t>(pool) * kBlockWords : nullptr;
  int any = 0;
  for (int s = 0; s < kDfSlices; ++s) {
    const u32 lin = static_cast<u32>(s) * kDfThreads + threadIdx.x;
    const int gx = bx * kVps + static_cast<int>(lin & 15u), gy = by * kVps + static_cast<int>((lin >> 4) & 15u), gz = bz * kVps + static_cast<int>(lin >> 8);
    DfObs o;
    int hit = 0;
    if (observe(P, depth, gx, gy, gz, &o)) {
      const float w0 = blk ? __uint_as_float(blk[3 * lin + 1]) : 0.0f;
      const float nw = w0 + o.uw;
      hit = (nw < kEps) ? 0 : 1;  // step 7's first line
    }
    any = __syncthreads_or(hit);
    if (any) break;
  }
  if (threadIdx.x == 0) {
    touched[cand] = any ? 1u : 0u;
    is_new[cand] = (any && pool == kInvalid) ? 1u : 0u;
    pool_of[cand] = pool;
  }
}

// the touched candidates, in candidate order; and the two words of the layer that the host read wants next to the totals
__global__ void __launch_bounds__(kDfThreads) k_df_compact(const u32* __restrict__ touched, const u32* __restrict__ scan_t, u32 n_cand, u32* __restrict__ list,
                                                           const u32* __restrict__ d_nblocks, const u32* __restrict__ d_err, u32* __restrict__ ctl) {
  const u32 i = blockIdx.x * kDfThreads + threadIdx.x;
  if (i == 0) ctl[kHostNb] = *d_nblocks, ctl[kHostErr] = *d_err;
  if (i < n_cand && touched[i]) list[scan_t[i]] = i;
}

// ---- update ----------------------------------------------------------------------------------------------------------
// rank_new: the exclusive scan of is_new; a block is new iff pool_of says it has no storage (every listed candidate is touched)
__global__ void __launch_bounds__(kDfThreads) k_df_update(DfParams P, const float* __restrict__ depth, const uint8_t* __restrict__ rgba, u32* __restrict__ voxels,
                                                          u64* __restrict__ ht_keys, u32* __restrict__ ht_vals, u32 ht_mask, u64* __restrict__ block_keys,
                                                          u32 nb0, u32 nb1, u32 capacity, u32 n_touched, const u32* __restrict__ list,
                                                          const u32* __restrict__ rank_new, const u32* __restrict__ pool_of, u32* __restrict__ ctl,
                                                          u32* __restrict__ d_nblocks, u32* __restrict__ h_nblocks, u32* __restrict__ d_err) {
  __shared__ u32 part[2 * (kDfThreads / 64)];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    *d_nblocks = nb1;
    *h_nblocks = nb1;
  }
  const u32 j = blockIdx.x;
  if (j >= n_touched) return;
  const u32 cand = list[j];
  int bx, by, bz;
  candidate_block(P, cand, &bx, &by, &bz);
  u32 pool = pool_of[cand];
  if (pool == kInvalid) {
    pool = nb0 + rank_new[cand];
    if (pool >= nb1 || pool >= capacity) {  // cannot happen: the host has sized the pool for nb1 blocks
      if (threadIdx.x == 0) atomicOr(d_err, kErrPool);
      return;
    }
    if (threadIdx.x == 0) {  // the pool's tail is zero; nobody looks this key up during this kernel
      const u64 key = pack_key(bx, by, bz);
      block_keys[pool] = key;
      bool fresh;
      const u32 slot = ht_insert(ht_keys, ht_mask, key, &fresh);
      if (slot == kInvalid)
        atomicOr(d_err, kErrTable);
      else
        ht_vals[slot] = pool;
    }
  } else if (pool >= nb0) {
    return;
  }
  u32* blk = voxels + static_cast<size_t>(pool) * kBlockWords;
  u32 n_upd = 0, n_col = 0;
  for (int s = 0; s < kDfSlices; ++s) {
    const u32 lin = static_cast<u32>(s) * kDfThreads + threadIdx.x;  // consecutive lanes, consecutive voxels
    const int gx = bx * kVps + static_cast<int>(lin & 15u), gy = by * kVps + static_cast<int>((lin >> 4) & 15u), gz = bz * kVps + static_cast<int>(lin >> 8);
    DfObs o;
    if (!observe(P, depth, gx, gy, gz, &o)) continue;
    // step 7 (update_voxel; the colour only with an image)
    u32* word = blk + 3 * lin;
    const float d0 = __uint_as_float(word[0]), w0 = __uint_as_float(word[1]);
    const float nw = w0 + o.uw;
    if (nw < kEps) continue;
    const float nsdf = (o.sdf * o.uw + d0 * w0) / nw;
    if (rgba != nullptr && fabsf(o.sdf) < P.trunc) {
      const uint8_t* px = rgba + 4 * (static_cast<size_t>(o.pv) * P.w + o.pu);
      const u32 colour = static_cast<u32>(px[3]) | (static_cast<u32>(px[2]) << 8) | (static_cast<u32>(px[1]) << 16) | (static_cast<u32>(px[0]) << 24);
      word[2] = blend_colors(word[2], w0, colour, o.uw);
      ++n_col;
    }
    word[0] = __float_as_uint((nsdf > 0.0f) ? std_min(P.trunc, nsdf) : std_max(-P.trunc, nsdf));
    word[1] = __float_as_uint(std_min(P.max_weight, nw));
    ++n_upd;
  }
  n_upd = wave_sum_u32(n_upd);
  n_col = wave_sum_u32(n_col);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n_upd, part[4 + (threadIdx.x >> 6)] = n_col;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u32 upd = (part[0] + part[1]) + (part[2] + part[3]), col = (part[4] + part[5]) + (part[6] + part[7]);
    if (upd) atomicAdd(reinterpret_cast<ull*>(ctl + kCtlUpdated64), static_cast<ull>(upd));
    if (col) atomicAdd(reinterpret_cast<ull*>(ctl + kCtlColoured64), static_cast<ull>(col));
  }
}

// ---- host: the candidate box and the cull's planes ---------------------------------------------------------------------
int check_config(const cox_depthfuse_config& c, float voxel_size) {
  const bool pos_finite = std::isfinite(c.truncation_distance) && c.truncation_distance > 0.0f && std::isfinite(c.max_weight) && c.max_weight > 0.0f &&
                          std::isfinite(c.min_depth_m) && c.min_depth_m > 0.0f && std::isfinite(c.max_depth_m) && c.max_depth_m > 0.0f &&
                          std::isfinite(c.adaptive_gap_m) && c.adaptive_gap_m > 0.0f;
  if (!pos_finite) return COX_ERR_INVALID_ARG;
  if (c.interpolation_scheme < 0 || c.interpolation_scheme > 3) return COX_ERR_INVALID_ARG;
  if (c.use_weight_dropoff && !(c.truncation_distance > voxel_size)) return COX_ERR_INVALID_ARG;
  return COX_OK;
}

int check_frame_args(const float T[7], int w, int h, const float K[4]) {
  if (!T || !K || w < 1 || h < 1 || w > kMaxImageSide || h > kMaxImageSide) return COX_ERR_INVALID_ARG;
  if (!finite_all(T, 7) || !finite_all(K, 4) || !(K[0] > 0.0f) || !(K[1] > 0.0f)) return COX_ERR_INVALID_ARG;
  return COX_OK;
}

struct Box {
  int32_t lo[3];
  u32 dims[3];
  u64 count;
};

// The eight corners of the min_depth and max_depth planes along the rays through the image's outer borders, in the layer's frame
// (float64), widened by one block each way.
int candidate_box(float voxel_size, const cox_depthfuse_config& c, const float T[7], int w, int h, const float K[4], Box* out) {
  const double qw = T[0], qx = T[1], qy = T[2], qz = T[3];
  const double R[3][3] = {{1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)},
                          {2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)},
                          {2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)}};
  const double ax[2] = {(-0.5 - K[2]) / K[0], (w - 0.5 - K[2]) / K[0]}, ay[2] = {(-0.5 - K[3]) / K[1], (h - 0.5 - K[3]) / K[1]};
  const double zs[2] = {c.min_depth_m, c.max_depth_m};
  double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (double z : zs)
    for (double a : ax)
      for (double b : ay) {
        const double p[3] = {a * z, b * z, z};
        for (int k = 0; k < 3; ++k) {
          const double g = (R[k][0] * p[0] + R[k][1] * p[1] + R[k][2] * p[2]) + T[4 + k];
          mn[k] = std::min(mn[k], g), mx[k] = std::max(mx[k], g);
        }
      }
  const double bs = 16.0 * static_cast<double>(voxel_size);
  u64 count = 1;
  for (int k = 0; k < 3; ++k) {
    const double lo = std::floor(mn[k] / bs) - 1.0, hi = std::floor(mx[k] / bs) + 1.0;
    if (!std::isfinite(lo) || !std::isfinite(hi)) return COX_ERR_INVALID_ARG;
    if (lo < -static_cast<double>(kIdxBias) || hi >= static_cast<double>(kIdxBias)) return COX_ERR_INDEX_RANGE;
    out->lo[k] = static_cast<int32_t>(lo);
    out->dims[k] = static_cast<u32>(hi - lo) + 1u;
    count *= out->dims[k];  // three factors below 2^21 each: checked against the cap before the next one could overflow
    if (count > COX_DEPTHFUSE_MAX_CANDIDATES) return COX_ERR_INVALID_ARG;
  }
  out->count = count;
  return COX_OK;
}

// inward unit normal (nx, nz) of the plane x = a z (sign +1: the half space x >= a z; -1: x <= a z)
void side_plane(double a, double sign, float* nx, float* nz) {
  const double len = std::sqrt(1.0 + a * a);
  *nx = static_cast<float>(sign / len);
  *nz = static_cast<float>(-sign * a / len);
}

}  // namespace

struct cox_depthfuse {
  int device = 0;
  cox_layer* layer = nullptr;
  cox_depthfuse_config cfg{};
  Stream stream;
  Event ev_in, ev_read;  // the producer's work so far; the frame has read its images
  Event ev_t[4];         // selection begin / end, update begin / end
  DevBuf<u32> d_ctl;     // kHostWords
  PinnedBuf<u32> h_ctl;  // kHostWords
  // per candidate, sized by the largest frame so far
  u64 cand_cap = 0;
  DevBuf<u32> d_touched, d_scan_t, d_new, d_pool_of, d_list, d_sums;
  // staging of host images
  DevBuf<float> d_depth;
  DevBuf<uint8_t> d_rgba;

  int acquire() {
    COX_TRY(stream.create());
    COX_TRY(ev_in.create(false));
    COX_TRY(ev_read.create(false));
    for (Event& e : ev_t) COX_TRY(e.create(true));
    COX_TRY(d_ctl.alloc(kHostWords));
    return h_ctl.alloc(kHostWords);
  }
  cox_depthfuse_stats last{};
  bool pending = false;   // the last frame's counters are still on the device
  bool timed[2] = {false, false};
};

namespace {

int grow_candidates(cox_depthfuse* H, u64 n) {
  if (n <= H->cand_cap) return COX_OK;
  COX_HIP(hipStreamSynchronize(H->stream));
  DevBuf<u32>* const per_candidate[] = {&H->d_touched, &H->d_scan_t, &H->d_new, &H->d_pool_of, &H->d_list};
  for (DevBuf<u32>* q : per_candidate) q->reset();
  H->d_sums.reset();
  H->cand_cap = 0;
  const u64 cap = std::min<u64>(std::max<u64>(n, 4096), COX_DEPTHFUSE_MAX_CANDIDATES);
  bool ok = true;
  for (DevBuf<u32>* q : per_candidate) ok = ok && q->alloc(cap) == COX_OK;
  ok = ok && H->d_sums.alloc(scan_num_blocks(static_cast<u32>(cap)) + 1) == COX_OK;
  if (!ok) return COX_ERR_OUT_OF_MEMORY;
  H->cand_cap = cap;
  return COX_OK;
}

// counters of the last frame -> H->last; everything of this handle has run when this returns
int settle(cox_depthfuse* H) {
  COX_HIP(hipSetDevice(H->device));
  if (!H->pending) {
    COX_HIP(hipStreamSynchronize(H->stream));
    return COX_OK;
  }
  COX_HIP(hipMemcpyAsync(H->h_ctl, H->d_ctl, sizeof(u32) * kCtlWords, hipMemcpyDeviceToHost, H->stream));
  COX_HIP(hipStreamSynchronize(H->stream));
  ull v64[3];
  memcpy(v64, H->h_ctl + kCtlValid64, sizeof(v64));
  H->last.n_valid_pixels = v64[0];
  H->last.n_updated_voxels = v64[1];
  H->last.n_coloured_voxels = v64[2];
  double ms = 0.0;
  for (int k = 0; k < 2; ++k) {
    float t = 0.0f;
    if (H->timed[k] && hipEventElapsedTime(&t, H->ev_t[2 * k], H->ev_t[2 * k + 1]) == hipSuccess) ms += t;
  }
  (void)hipGetLastError();
  H->last.kernel_ms = ms;
  H->pending = false;
  return COX_OK;
}

// one frame from device images; the stream already orders behind their producer
int frame(cox_depthfuse* H, const Box& box, const float T[7], const float* depth, const uint8_t* rgba, int w, int h, const float K[4]) {
  cox_layer* L = H->layer;
  hipStream_t s = H->stream;
  const cox_depthfuse_config& c = H->cfg;
  COX_TRY(settle(H));  // the control block is single: the frame before this one is done with it
  H->last = cox_depthfuse_stats{};
  H->timed[0] = H->timed[1] = false;
  const u32 n_cand = static_cast<u32>(box.count);

  DfParams P;
  memset(&P, 0, sizeof(P));
  {  // T_C_G = (q*, -rotate(q*, t)) in float32, A.1's order
    const float q[4] = {T[0], -T[1], -T[2], -T[3]};
    const float qv[3] = {q[1], q[2], q[3]}, v[3] = {T[4], T[5], T[6]};
    float uv[3] = {qv[1] * v[2] - qv[2] * v[1], qv[2] * v[0] - qv[0] * v[2], qv[0] * v[1] - qv[1] * v[0]};
    for (int k = 0; k < 3; ++k) uv[k] = uv[k] + uv[k];
    const float cr[3] = {qv[1] * uv[2] - qv[2] * uv[1], qv[2] * uv[0] - qv[0] * uv[2], qv[0] * uv[1] - qv[1] * uv[0]};
    float r[3];
    for (int k = 0; k < 3; ++k) r[k] = (v[k] + q[0] * uv[k]) + cr[k];
    P.iqw = q[0], P.iqx = q[1], P.iqy = q[2], P.iqz = q[3];
    P.itx = -r[0], P.ity = -r[1], P.itz = -r[2];
  }
  P.fx = K[0], P.fy = K[1], P.cx = K[2], P.cy = K[3];
  P.u_hi = static_cast<float>(w) - 0.5f, P.v_hi = static_cast<float>(h) - 0.5f;
  P.voxel_size = L->voxel_size, P.trunc = c.truncation_distance, P.max_weight = c.max_weight;
  P.min_depth = c.min_depth_m, P.max_depth = c.max_depth_m, P.gap = c.adaptive_gap_m;
  P.w = w, P.h = h, P.scheme = c.interpolation_scheme, P.carving = c.voxel_carving_enabled, P.const_weight = c.use_const_weight, P.dropoff = c.use_weight_dropoff;
  P.lo_x = box.lo[0], P.lo_y = box.lo[1], P.lo_z = box.lo[2];
  P.dim_x = box.dims[0], P.dim_y = box.dims[1];
  {
    // the voxel centres of a block lie within 7.5 voxels per axis of its centre; the planes half a pixel (and 1e-5 of the
    // coordinates that enter u) outside the image's borders
    P.radius = static_cast<float>(7.5 * std::sqrt(3.0) * static_cast<double>(L->voxel_size) * 1.001);
    const double pm_u = 0.5 + 1e-5 * (std::fabs(static_cast<double>(K[2])) + w), pm_v = 0.5 + 1e-5 * (std::fabs(static_cast<double>(K[3])) + h);
    side_plane((-0.5 - pm_u - K[2]) / K[0], 1.0, &P.pl_x0, &P.pl_z0);
    side_plane((w - 0.5 + pm_u - K[2]) / K[0], -1.0, &P.pl_x1, &P.pl_z1);
    side_plane((-0.5 - pm_v - K[3]) / K[1], 1.0, &P.pl_y2, &P.pl_z2);
    side_plane((h - 0.5 + pm_v - K[3]) / K[1], -1.0, &P.pl_y3, &P.pl_z3);
  }

  // the layer: its other writers first (a projective integrator may settle, and grow the layer, in here), then its buffers
  const bool foreign = cox_layer_order_writer(L, H);
  COX_TRY(grow_candidates(H, n_cand));
  if (foreign) cox_layer_wait_writes(L, s);
  ++L->frame_id;  // a frame of the layer like any other writer's (ht_stamp and ht_ord are the ray casters' and stay as they are)

  COX_HIP(hipMemsetAsync(H->d_ctl, 0, sizeof(u32) * kCtlWords, s));
  COX_HIP(hipEventRecord(H->ev_t[0], s));
  const u32 n_px = static_cast<u32>(w) * static_cast<u32>(h);
  // (few workgroups: each ends in one atomic on the same counter)
  hipLaunchKernelGGL(k_df_valid, dim3(std::min<u32>((n_px + kDfThreads - 1) / kDfThreads, 128u)), dim3(kDfThreads), 0, s, depth, n_px, H->d_ctl);
  // frames of other writers may still be in flight ahead of this one on the device, so the selection reads the layer's block
  // count where it runs, from d_nblocks; the host learns it with the flags (nb0 below)
  hipLaunchKernelGGL(k_df_select, dim3(n_cand), dim3(kDfThreads), 0, s, P, depth, L->voxels, L->ht_keys, L->ht_vals, L->ht_cap - 1, L->d_nblocks, static_cast<u32>(L->capacity), n_cand,
                     H->d_touched, H->d_new, H->d_pool_of);
  const ScanWorkspace ws{H->d_sums};
  exclusive_scan_u32(H->d_touched, H->d_scan_t, nullptr, n_cand, n_cand, H->d_ctl + kCtlTouched, ws, s);
  exclusive_scan_u32(H->d_new, H->d_new, nullptr, n_cand, n_cand, H->d_ctl + kCtlNew, ws, s);
  hipLaunchKernelGGL(k_df_compact, dim3((n_cand + kDfThreads - 1) / kDfThreads), dim3(kDfThreads), 0, s, H->d_touched, H->d_scan_t, n_cand, H->d_list,
                     L->d_nblocks, L->d_err, H->d_ctl);
  COX_HIP(hipEventRecord(H->ev_t[1], s));
  H->timed[0] = true;
  COX_HIP(hipGetLastError());
  // the frame's single host read
  COX_HIP(hipMemcpyAsync(H->h_ctl, H->d_ctl, sizeof(u32) * kHostWords, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  if (H->h_ctl.p[kHostErr]) return err_bits_to_status(H->h_ctl.p[kHostErr]);  // no frame onto a layer in error
  const u32 n_touched = H->h_ctl.p[kCtlTouched], n_new = H->h_ctl.p[kCtlNew];
  if (n_touched > n_cand || n_new > n_touched) return COX_ERR_INTERNAL;
  const u32 nb0 = static_cast<u32>(std::min<u64>(H->h_ctl.p[kHostNb], L->capacity));
  const u64 nb1 = static_cast<u64>(nb0) + n_new;
  if (nb1 > L->capacity) {
    if (!L->auto_grow) return COX_ERR_POOL_EXHAUSTED;  // nothing was written
    const int st = cox_internal_layer_reserve(L, std::max<u64>(2 * L->capacity, nb1));  // device-wide sync; pool indices stay
    if (st != COX_OK) return st == COX_ERR_OUT_OF_MEMORY ? COX_ERR_POOL_EXHAUSTED : st;
  }
  ull v64 = 0;
  memcpy(&v64, H->h_ctl + kCtlValid64, sizeof(v64));
  H->last.n_valid_pixels = v64;
  H->last.n_candidate_blocks = n_cand;
  H->last.n_touched_blocks = n_touched;
  H->last.n_new_blocks = n_new;
  H->pending = true;
  if (n_touched) {
    // (the layer's buffers are read here, after the reserve: its generation may have moved)
    COX_HIP(hipEventRecord(H->ev_t[2], s));
    hipLaunchKernelGGL(k_df_update, dim3(n_touched), dim3(kDfThreads), 0, s, P, depth, rgba, L->voxels, L->ht_keys, L->ht_vals, L->ht_cap - 1, L->block_keys, nb0,
                       static_cast<u32>(nb1), static_cast<u32>(L->capacity), n_touched, H->d_list, H->d_new, H->d_pool_of, H->d_ctl, L->d_nblocks, L->h_nblocks,
                       L->d_err);
    COX_HIP(hipEventRecord(H->ev_t[3], s));
    H->timed[1] = true;
    COX_HIP(hipGetLastError());
  }
  COX_HIP(hipEventRecord(L->last_write, s));
  L->has_write = true;
  return COX_OK;
}

// the frame's candidate box, or the status it is refused with before anything is enqueued (the statistics then say that nothing
// happened)
int box_or_refuse(cox_depthfuse* H, const float T[7], int w, int h, const float K[4], Box* box) {
  const int st = candidate_box(H->layer->voxel_size, H->cfg, T, w, h, K, box);
  if (st != COX_OK) {
    (void)settle(H);
    H->last = cox_depthfuse_stats{};
  }
  return st;
}

}  // namespace

extern "C" {

void cox_depthfuse_config_default(cox_depthfuse_config* cfg) {
  if (!cfg) return;
  memset(cfg, 0, sizeof(*cfg));
  cfg->truncation_distance = 0.1f;
  cfg->max_weight = 10000.0f;
  cfg->min_depth_m = 0.1f;
  cfg->max_depth_m = 5.0f;
  cfg->voxel_carving_enabled = 1;
  cfg->use_const_weight = 0;
  cfg->use_weight_dropoff = 1;
  cfg->interpolation_scheme = 3;
  cfg->adaptive_gap_m = 0.5f;
  cfg->reserved = 0;
}

int cox_selftest_depthfuse_box(float voxel_size, const cox_depthfuse_config* cfg_in, const float T[7], int w, int height, const float K[4], int32_t lo[3],
                                uint32_t dims[3]) {
  if (!lo || !dims || !(voxel_size > 0.0f) || !std::isfinite(voxel_size)) return COX_ERR_INVALID_ARG;
  cox_depthfuse_config cfg;
  if (cfg_in)
    cfg = *cfg_in;
  else
    cox_depthfuse_config_default(&cfg);
  COX_TRY(check_config(cfg, voxel_size));
  COX_TRY(check_frame_args(T, w, height, K));
  Box box;
  COX_TRY(candidate_box(voxel_size, cfg, T, w, height, K, &box));
  for (int k = 0; k < 3; ++k) lo[k] = box.lo[k], dims[k] = box.dims[k];
  return COX_OK;
}

int cox_depthfuse_create(cox_layer_t* layer, const cox_depthfuse_config* cfg_in, cox_depthfuse_t** out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!layer || !out) return COX_ERR_INVALID_ARG;
  cox_depthfuse_config cfg;
  if (cfg_in)
    cfg = *cfg_in;
  else
    cox_depthfuse_config_default(&cfg);
  COX_TRY(check_config(cfg, layer->voxel_size));
  COX_HIP(hipSetDevice(layer->device));
  cox_depthfuse* H = new (std::nothrow) cox_depthfuse();
  if (!H) return COX_ERR_OUT_OF_MEMORY;
  H->layer = layer;
  H->device = layer->device;
  H->cfg = cfg;
  if (H->acquire() != COX_OK) {
    cox_depthfuse_destroy(H);
    return COX_ERR_NO_DEVICE;
  }
  memset(H->h_ctl, 0, sizeof(u32) * kHostWords);
  *out = H;
  return COX_OK;
}

void cox_depthfuse_destroy(cox_depthfuse_t* H) {
  if (!H) return;
  (void)hipSetDevice(H->device);
  if (H->stream) (void)hipStreamSynchronize(H->stream);  // nothing of this integrator is in flight after this
  delete H;
}

int cox_depthfuse_integrate_dev(cox_depthfuse_t* H, const float T[7], const float* depth_dev, const uint8_t* rgba_dev, int w, int height, const float K[4],
                                void* producer_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H || !depth_dev) return COX_ERR_INVALID_ARG;
  COX_TRY(check_frame_args(T, w, height, K));
  Box box;
  COX_TRY(box_or_refuse(H, T, w, height, K, &box));
  COX_HIP(hipSetDevice(H->device));
  hipStream_t producer = static_cast<hipStream_t>(producer_stream);
  COX_HIP(hipEventRecord(H->ev_in, producer));
  COX_HIP(hipStreamWaitEvent(H->stream, H->ev_in, 0));
  const int st = frame(H, box, T, depth_dev, rgba_dev, w, height, K);
  // whatever the frame enqueued has read the images behind this point
  COX_HIP(hipEventRecord(H->ev_read, H->stream));
  COX_HIP(hipStreamWaitEvent(producer, H->ev_read, 0));
  return st;
}

int cox_depthfuse_integrate(cox_depthfuse_t* H, const float T[7], const float* depth, const uint8_t* rgba, int w, int height, const float K[4]) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H || !depth) return COX_ERR_INVALID_ARG;
  COX_TRY(check_frame_args(T, w, height, K));
  Box box;
  COX_TRY(box_or_refuse(H, T, w, height, K, &box));
  COX_HIP(hipSetDevice(H->device));
  const size_t n_px = static_cast<size_t>(w) * static_cast<size_t>(height);
  COX_HIP(hipStreamSynchronize(H->stream));  // the staging buffers are single: the frame that read them last is done
  COX_TRY(H->d_depth.grow(n_px));
  if (rgba) COX_TRY(H->d_rgba.grow(4 * n_px));
  COX_HIP(hipMemcpyAsync(H->d_depth, depth, sizeof(float) * n_px, hipMemcpyHostToDevice, H->stream));
  if (rgba) COX_HIP(hipMemcpyAsync(H->d_rgba, rgba, 4 * n_px, hipMemcpyHostToDevice, H->stream));
  return frame(H, box, T, H->d_depth, rgba ? H->d_rgba.p : nullptr, w, height, K);
}

int cox_depthfuse_sync(cox_depthfuse_t* H) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  COX_TRY(settle(H));
  u32 err = 0;
  COX_HIP(hipMemcpyAsync(H->h_ctl + kHostErr, H->layer->d_err, sizeof(u32), hipMemcpyDeviceToHost, H->stream));
  COX_HIP(hipStreamSynchronize(H->stream));
  err = H->h_ctl.p[kHostErr];
  return err_bits_to_status(err);
}

int cox_depthfuse_last_stats(cox_depthfuse_t* H, cox_depthfuse_stats* out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H || !out) return COX_ERR_INVALID_ARG;
  COX_TRY(settle(H));
  *out = H->last;
  return COX_OK;
}

int cox_depthfuse_pool_order(cox_depthfuse_t* H, int32_t* block_idx_xyz, uint64_t cap_blocks, uint64_t* n_blocks) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H || !n_blocks) return COX_ERR_INVALID_ARG;
  cox_layer* L = H->layer;
  COX_HIP(hipSetDevice(H->device));
  if (L->settle_writer && L->settle_ctx == L->last_writer) L->settle_writer(L->settle_ctx);
  COX_HIP(hipDeviceSynchronize());  // every writer of the layer, on whatever stream
  u32 nb = 0;
  COX_HIP(hipMemcpy(&nb, L->d_nblocks, sizeof(u32), hipMemcpyDeviceToHost));
  nb = static_cast<u32>(std::min<u64>(nb, L->capacity));
  *n_blocks = nb;
  if (cap_blocks < nb || (nb && !block_idx_xyz)) return COX_ERR_BUFFER_TOO_SMALL;
  if (nb == 0) return COX_OK;
  std::vector<u64> keys(nb);
  COX_HIP(hipMemcpy(keys.data(), L->block_keys, sizeof(u64) * nb, hipMemcpyDeviceToHost));
  for (u32 i = 0; i < nb; ++i) {
    int x, y, z;
    unpack_key(keys[i], &x, &y, &z);
    block_idx_xyz[3 * i] = x, block_idx_xyz[3 * i + 1] = y, block_idx_xyz[3 * i + 2] = z;
  }
  return COX_OK;
}

}  // extern "C"
