// MI355X (gfx950): point queries on TSDF / ESDF layers and the free-space cloud of an ESDF, behind include/coxgraph_hip_map.h.
//
// What a consumer of coxgraph's maps reads (MapServer, coxgraph/src/client/map_server.cpp:61-147, and the planners behind
// voxblox's EsdfMap / TsdfMap / Interpolator):
//
//   k_query<MODE, GRAD>  one lane per query, queries in input order, outputs coalesced.  The <= 8 blocks a query can touch
//                        (its 7 samples lie in voxels v0 - 1 .. v0 + 2 on each axis) are resolved once, up front, into a
//                        BlockCache of cox_interp.hpp (block_cache_fill's body, in place); a sample whose cell falls outside
//                        that set (float rounding) looks its block up afresh.  The samples are tri_sample / nearest_sample of
//                        the same header: each cell is interp_cell, 16 independent voxel loads.
//   k_free_count         createFreePointcloudFromEsdfLayer, pass 1: per block (download order) the voxels that pass
//   exclusive_scan_u32   block offsets (cox_sort.hpp)
//   k_free_write         pass 2: voxel centres + distances, linear voxel order inside a block
//
// Rules and arithmetic: DESIGN.md section 7e.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/coxgraph_hip_map.h"
#include "cox_host.hpp"
#include "cox_interp.hpp"
#include "cox_sort.hpp"

using namespace cox;

namespace {

// ---- the query kernel ------------------------------------------------------------------------------------------------------
constexpr int kQueryThreads = 256;

// One branch of the Interpolator (TRI: trilinear, else nearest) at p: distance + weight, and with GRAD the central differences
// of Interpolator::getGradient at p +- h e_i (h = voxel size), g_i = ((0 + d(p - h e_i) * -1) + d(p + h e_i)) / (2 h), valid
// when the block of p exists (own_block) and all six samples succeed.  The seven samples run in a loop that is not unrolled:
// one copy of the gather in the code, its 16 loads independent of each other; other waves hide the latency of the next one.
template <bool TRI, bool GRAD>
__device__ __forceinline__ void branch(const LayerView& L, const BlockCache& bc, const float p[3], bool own_block, bool* vd, bool* vg, float* d,
                                       float* w, float g[3]) {
  const float h = L.voxel_size, two_h = 2.0f * L.voxel_size;
  bool okg = GRAD && own_block;
  float acc = 0.0f;
  constexpr int ns = GRAD ? 7 : 1;
#pragma unroll 1
  for (int k = 0; k < ns; ++k) {
    if (k > 0 && !okg) break;
    const int axis = (k - 1) >> 1;
    const bool plus = ((k - 1) & 1) != 0;
    const float off = plus ? h : -h;
    // pos + offset: the zero components are added too
    const float s[3] = {k == 0 ? p[0] : (axis == 0 ? p[0] + off : p[0] + 0.0f), k == 0 ? p[1] : (axis == 1 ? p[1] + off : p[1] + 0.0f),
                        k == 0 ? p[2] : (axis == 2 ? p[2] + off : p[2] + 0.0f)};
    float dv = 0.0f, wv = 0.0f;
    const bool ok = TRI ? tri_sample(L, bc, s, &dv, &wv, k == 0) : nearest_sample(L, bc, s, &dv, &wv);
    if (k == 0) {
      *vd = ok;
      *d = dv;
      *w = wv;
    } else if (!ok) {
      okg = false;
    } else if (!plus) {
      acc = 0.0f + dv * -1.0f;
    } else {
      const float gi = (acc + dv) / two_h;
      g[0] = axis == 0 ? gi : g[0];
      g[1] = axis == 1 ? gi : g[1];
      g[2] = axis == 2 ? gi : g[2];
    }
  }
  *vg = okg;
}

// MODE: COX_QUERY_NEAREST / INTERPOLATE / ADAPTIVE
template <int MODE, bool GRAD>
__global__ void __launch_bounds__(kQueryThreads) k_query(LayerView L, const float* __restrict__ xyz, u64 n, float* __restrict__ dist,
                                                         float* __restrict__ weight, float* __restrict__ grad, uint8_t* __restrict__ status) {
  const u64 i = static_cast<u64>(blockIdx.x) * kQueryThreads + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  float sc[3];
  if (!block_scaled(L, p, sc)) {  // NaN, +-inf, beyond the packed keys
    if (status) status[i] = 0;
    return;
  }
  // the blocks of voxels g - r .. g + r around the voxel g that contains p: the samples reach g - 2 .. g + 2 (g - 1 .. g + 1
  // without a gradient), one more voxel on each side for rounding at block faces
  constexpr int r = GRAD ? 3 : (MODE == COX_QUERY_NEAREST ? 1 : 2);
  BlockCache bc{L, kNoBlocks};
  // block_cache_fill<r>'s body, kept in place: through the call ADAPTIVE without a gradient takes 66 VGPRs for 64 and loses a wave
  int span[3], b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    b[k] = grid_index(sc[k]);
    const int v = grid_index((p[k] - static_cast<float>(b[k]) * L.block_size) * L.voxel_size_inv);
    const int g = b[k] * 16 + (v > 15 ? 15 : (v < 0 ? 0 : v));
    bc.s.lo[k] = (g - r) >> 4;
    span[k] = ((g + r) >> 4) - bc.s.lo[k];
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int mx = (c >> 2) & 1, my = (c >> 1) & 1, mz = c & 1;
    if (mx <= span[0] && my <= span[1] && mz <= span[2]) {
      bc.s.pool[c] = HtPool{L}(bc.s.lo[0] + mx, bc.s.lo[1] + my, bc.s.lo[2] + mz);
      bc.s.have |= 1u << c;
    }
  }
  const bool own_block = !GRAD || bc(b[0], b[1], b[2]) != kInvalid;  // getGradient: getBlockPtrByCoordinates(pos)
  float d = 0.0f, w = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
  bool vd = false, vg = false;
  u32 st = 0;
  if (MODE != COX_QUERY_NEAREST) {
    branch<true, GRAD>(L, bc, p, own_block, &vd, &vg, &d, &w, g);
    if (MODE == COX_QUERY_INTERPOLATE) {
      st = (vd ? (COX_Q_VALUE | COX_Q_TRILINEAR) : 0u) | (vg ? COX_Q_GRADIENT : 0u);
    } else if (vd && (vg || !GRAD)) {  // getAdaptiveDistanceAndGradient: trilinear when distance and gradient both succeed
      st = COX_Q_VALUE | COX_Q_TRILINEAR | (GRAD ? COX_Q_GRADIENT : 0u);
    }
  }
  if (MODE == COX_QUERY_NEAREST || (MODE == COX_QUERY_ADAPTIVE && st == 0u)) {  // ... otherwise nearest distance and gradient
    branch<false, GRAD>(L, bc, p, own_block, &vd, &vg, &d, &w, g);
    st = (vd ? COX_Q_VALUE : 0u) | (vg ? COX_Q_GRADIENT : 0u);
  }
  if (status) status[i] = static_cast<uint8_t>(st);
  if (st & COX_Q_VALUE) {
    if (dist) dist[i] = d;
    if (weight) weight[i] = w;
  }
  if (GRAD && grad && (st & COX_Q_GRADIENT)) {
    grad[3 * i] = g[0];
    grad[3 * i + 1] = g[1];
    grad[3 * i + 2] = g[2];
  }
}

template <int MODE>
void launch_query_mode(bool want_gradient, const LayerView& V, const float* xyz, u64 n, float* dist, float* weight, float* grad, uint8_t* status,
                       hipStream_t s) {
  const dim3 grid(static_cast<u32>((n + kQueryThreads - 1) / kQueryThreads));
  if (want_gradient)
    hipLaunchKernelGGL((k_query<MODE, true>), grid, dim3(kQueryThreads), 0, s, V, xyz, n, dist, weight, grad, status);
  else
    hipLaunchKernelGGL((k_query<MODE, false>), grid, dim3(kQueryThreads), 0, s, V, xyz, n, dist, weight, static_cast<float*>(nullptr), status);
}

void launch_query(int mode, bool want_gradient, const LayerView& V, const float* xyz, u64 n, float* dist, float* weight, float* grad, uint8_t* status,
                  hipStream_t s) {
  if (mode == COX_QUERY_NEAREST)
    launch_query_mode<COX_QUERY_NEAREST>(want_gradient, V, xyz, n, dist, weight, grad, status, s);
  else if (mode == COX_QUERY_INTERPOLATE)
    launch_query_mode<COX_QUERY_INTERPOLATE>(want_gradient, V, xyz, n, dist, weight, grad, status, s);
  else
    launch_query_mode<COX_QUERY_ADAPTIVE>(want_gradient, V, xyz, n, dist, weight, grad, status, s);
}

int check_query_args(const cox_layer* L, const void* xyz, u64 n, int mode) {
  if (!L || (n > 0 && !xyz)) return COX_ERR_INVALID_ARG;
  if (mode != COX_QUERY_NEAREST && mode != COX_QUERY_INTERPOLATE && mode != COX_QUERY_ADAPTIVE) return COX_ERR_INVALID_ARG;
  if (n > (static_cast<u64>(0x7FFFFFFF) * kQueryThreads)) return COX_ERR_INVALID_ARG;  // grid size
  return COX_OK;
}

// ---- free-space cloud ------------------------------------------------------------------------------------------------------
constexpr int kFreeThreads = 256;

__device__ __forceinline__ bool free_voxel(const u32* vox, float min_distance) {
  const float w = __uint_as_float(vox[1]);
  return w > 0.0f && __uint_as_float(vox[0]) >= min_distance;  // EsdfVoxel::observed && distance >= min_distance
}

// one workgroup per block in download order: voxels that pass
__global__ void __launch_bounds__(kFreeThreads) k_free_count(const u32* __restrict__ voxels, const u32* __restrict__ order, float min_distance,
                                                             u32* __restrict__ counts) {
  __shared__ u32 lds[kFreeThreads / 64];
  const u32* blk = voxels + static_cast<size_t>(order[blockIdx.x]) * kVoxelsPerBlock * kWordsPerVoxel;
  u32 c = 0;
  for (u32 v = threadIdx.x; v < kVoxelsPerBlock; v += kFreeThreads) c += free_voxel(blk + 3 * v, min_distance) ? 1u : 0u;
  u32 total;
  (void)block_exclusive_scan<kFreeThreads / 64>(c, &total, lds);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one workgroup per block in download order: voxel centre origin + centerCoord, intensity = distance, linear voxel order
__global__ void __launch_bounds__(kFreeThreads) k_free_write(const u32* __restrict__ voxels, const u32* __restrict__ order, const u64* __restrict__ keys,
                                                             const u32* __restrict__ offsets, float min_distance, float voxel_size, float block_size,
                                                             float* __restrict__ xyz, float* __restrict__ intensity) {
  __shared__ u32 lds[kFreeThreads / 64];
  const u32 pool = order[blockIdx.x];
  const u32* blk = voxels + static_cast<size_t>(pool) * kVoxelsPerBlock * kWordsPerVoxel;
  int bx, by, bz;
  unpack_key(keys[pool], &bx, &by, &bz);
  const float ox = static_cast<float>(bx) * block_size, oy = static_cast<float>(by) * block_size, oz = static_cast<float>(bz) * block_size;
  u64 next = offsets[blockIdx.x];
  for (u32 v = threadIdx.x; v < kVoxelsPerBlock; v += kFreeThreads) {  // every thread runs all 16 rounds (the scan has barriers)
    const u32* vox = blk + 3 * v;
    const bool pass = free_voxel(vox, min_distance);
    u32 total;
    const u32 ex = block_exclusive_scan<kFreeThreads / 64>(pass ? 1u : 0u, &total, lds);
    if (pass) {
      const u64 o = next + ex;
      xyz[3 * o] = ox + center_coord(static_cast<int>(v & 15u), voxel_size);
      xyz[3 * o + 1] = oy + center_coord(static_cast<int>((v >> 4) & 15u), voxel_size);
      xyz[3 * o + 2] = oz + center_coord(static_cast<int>(v >> 8), voxel_size);
      intensity[o] = __uint_as_float(vox[0]);
    }
    next += total;
  }
}

}  // namespace

extern "C" {

int cox_layer_query(cox_layer_t* L, const float* xyz, uint64_t n, int mode, int want_gradient, float* distance, float* weight, float* gradient,
                     uint8_t* status) {
  COX_ENTRY();
  COX_TRY(device_present());
  COX_TRY(check_query_args(L, xyz, n, mode));
  if (n == 0) return COX_OK;
  COX_HIP(hipSetDevice(L->device));
  const bool grad = want_gradient != 0;
  // one staging allocation: xyz | distance | weight | gradient | status
  const size_t f_xyz = 3 * n, f_d = distance ? n : 0, f_w = weight ? n : 0, f_g = (grad && gradient) ? 3 * n : 0;
  const size_t floats = f_xyz + f_d + f_w + f_g;
  DevBuf<uint8_t> buf;
  COX_TRY(buf.alloc(floats * sizeof(float) + (status ? n : 0)));
  float* d_xyz = reinterpret_cast<float*>(buf.p);
  float* d_d = distance ? d_xyz + f_xyz : nullptr;
  float* d_w = weight ? d_xyz + f_xyz + f_d : nullptr;
  float* d_g = f_g ? d_xyz + f_xyz + f_d + f_w : nullptr;
  uint8_t* d_s = status ? buf.p + floats * sizeof(float) : nullptr;
  hipStream_t s = nullptr;
  cox_layer_wait_writes(L, s);  // frames still in flight on the layer
  COX_HIP(hipMemcpyAsync(d_xyz, xyz, sizeof(float) * f_xyz, hipMemcpyHostToDevice, s));
  if (f_d + f_w + f_g) COX_HIP(hipMemsetAsync(d_xyz + f_xyz, 0xFF, sizeof(float) * (f_d + f_w + f_g), s));  // NaN where nothing is written
  launch_query(mode, grad, layer_view(L), d_xyz, n, d_d, d_w, d_g, d_s, s);
  COX_HIP(hipGetLastError());
  if (distance) COX_HIP(hipMemcpyAsync(distance, d_d, sizeof(float) * n, hipMemcpyDeviceToHost, s));
  if (weight) COX_HIP(hipMemcpyAsync(weight, d_w, sizeof(float) * n, hipMemcpyDeviceToHost, s));
  if (f_g) COX_HIP(hipMemcpyAsync(gradient, d_g, sizeof(float) * f_g, hipMemcpyDeviceToHost, s));
  if (status) COX_HIP(hipMemcpyAsync(status, d_s, n, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  return COX_OK;
}

int cox_layer_query_dev(cox_layer_t* L, const float* xyz_dev, uint64_t n, int mode, int want_gradient, float* distance_dev, float* weight_dev,
                        float* gradient_dev, uint8_t* status_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  COX_TRY(check_query_args(L, xyz_dev, n, mode));
  if (n == 0) return COX_OK;
  COX_HIP(hipSetDevice(L->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  cox_layer_wait_writes(L, s);
  launch_query(mode, want_gradient != 0, layer_view(L), xyz_dev, n, distance_dev, weight_dev, gradient_dev, status_dev, s);
  COX_HIP(hipGetLastError());
  return COX_OK;
}

int cox_layer_free_points(cox_layer_t* L, float min_distance, float* xyz, float* intensity, uint64_t cap, uint64_t* n) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!L || !n) return COX_ERR_INVALID_ARG;
  *n = 0;
  COX_HIP(hipSetDevice(L->device));
  cox_layer_wait_writes(L, nullptr);
  COX_HIP(hipStreamSynchronize(nullptr));
  u32 nb = 0;
  COX_HIP(hipMemcpy(&nb, L->d_nblocks, sizeof(u32), hipMemcpyDeviceToHost));
  if (nb > L->capacity) nb = static_cast<u32>(L->capacity);
  if (nb == 0) return COX_OK;
  // blocks in (z, y, x) order, as cox_layer_download: the packed key orders that way
  std::vector<u64> keys(nb);
  COX_HIP(hipMemcpy(keys.data(), L->block_keys, sizeof(u64) * nb, hipMemcpyDeviceToHost));
  std::vector<u32> order(nb);
  for (u32 i = 0; i < nb; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return keys[a] < keys[b]; });
  DevBuf<u32> d_order, d_counts, d_offsets, d_total, d_sums;
  COX_TRY(d_order.alloc(nb));
  COX_TRY(d_counts.alloc(nb));
  COX_TRY(d_offsets.alloc(nb));
  COX_TRY(d_total.alloc(1));
  COX_TRY(d_sums.alloc(scan_num_blocks(nb)));
  COX_HIP(hipMemcpy(d_order.p, order.data(), sizeof(u32) * nb, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_free_count, dim3(nb), dim3(kFreeThreads), 0, nullptr, L->voxels, d_order.p, min_distance, d_counts.p);
  ScanWorkspace ws;
  ws.block_sums = d_sums.p;
  exclusive_scan_u32(d_counts.p, d_offsets.p, nullptr, nb, nb, d_total.p, ws, nullptr);
  u32 total = 0;
  COX_HIP(hipMemcpy(&total, d_total.p, sizeof(u32), hipMemcpyDeviceToHost));
  COX_HIP(hipGetLastError());
  *n = total;
  if (!xyz && !intensity) return COX_OK;  // size query
  if (cap < total) return COX_ERR_BUFFER_TOO_SMALL;
  if (total == 0) return COX_OK;
  DevBuf<float> d_xyz, d_int;
  COX_TRY(d_xyz.alloc(3ull * total));
  COX_TRY(d_int.alloc(total));
  hipLaunchKernelGGL(k_free_write, dim3(nb), dim3(kFreeThreads), 0, nullptr, L->voxels, d_order.p, L->block_keys, d_offsets.p, min_distance, L->voxel_size,
                     L->block_size, d_xyz.p, d_int.p);
  COX_HIP(hipGetLastError());
  if (xyz) COX_HIP(hipMemcpy(xyz, d_xyz.p, sizeof(float) * 3 * total, hipMemcpyDeviceToHost));
  if (intensity) COX_HIP(hipMemcpy(intensity, d_int.p, sizeof(float) * total, hipMemcpyDeviceToHost));
  return COX_OK;
}

}  // extern "C"
