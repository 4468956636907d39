// MI355X (gfx950): voxblox's mesher on the GPU -- MeshIntegrator::generateMesh, createConnectedMesh, generateVoxbloxMeshMsg.
//
// coxgraph's client publishes a mesh of every submap (SubmapVisuals::generateSubmapMesh + generateSubmapMeshMsg,
// coxgraph/src/client/map_server.cpp:119-150) and its server writes a global mesh of every submap moved by its optimised pose
// (coxgraph/src/server/visualizer/server_visualizer.cpp:20-142).  Here:
//
//   k_mesh_block<false>  one workgroup per allocated block in (z, y, x) order: the 17^3 corner samples (distance + validity) in
//                        LDS as k_mc_block stages them (cox_submap.hip), triangles per block
//   host                 offsets of the blocks that have triangles (the block list is sorted on the host anyway)
//   k_mesh_block<true>   one workgroup per block with triangles: corners + colour words in LDS; vertices in extractBlockMesh
//                        order, face normals, colour of the voxel that contains each vertex
//   k_mesh_msg           wire encoding + colour mode, one workgroup per block
//   k_mesh_transform     T p, R n in place
//   k_weld_*             createConnectedMesh: cell bounds, "first in mesh order wins" (atomicMin), scan, compaction
//
// Vertex positions are computed expression by expression as k_mc_block does, so they are bit-identical to the isosurface path.
// The rules that are recollection rather than reference code are listed in DESIGN.md section 7d ([U]).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/coxgraph_hip_mesh.h"
#include "cox_host.hpp"
#include "cox_mc_table.hpp"
#include "cox_sort.hpp"

using namespace cox;

namespace {

struct MeshView {
  const u32* voxels;
  const u64* ht_keys;
  const u32* ht_vals;
  u32 ht_mask;
  float voxel_size, voxel_size_inv, block_size, block_size_inv;
};

constexpr int kCorner = 17;                            // corner samples per axis of one block's cubes
constexpr int kCorners = kCorner * kCorner * kCorner;  // 4913

// cube sequence number within a block (MeshIntegrator::extractBlockMesh order) -> lower-corner voxel; as in cox_submap.hip
__device__ __forceinline__ void cube_of_seq(u32 seq, int* x, int* y, int* z) {
  if (seq < 3375u) {  // inside: x outer, y, z inner, each 0..14
    *x = static_cast<int>(seq / 225u);
    *y = static_cast<int>((seq / 15u) % 15u);
    *z = static_cast<int>(seq % 15u);
  } else if (seq < 3631u) {  // max X plane: z outer, y inner, each 0..15
    const u32 s = seq - 3375u;
    *x = 15;
    *z = static_cast<int>(s / 16u);
    *y = static_cast<int>(s % 16u);
  } else if (seq < 3871u) {  // max Y plane: z outer 0..15, x inner 0..14
    const u32 s = seq - 3631u;
    *y = 15;
    *z = static_cast<int>(s / 15u);
    *x = static_cast<int>(s % 15u);
  } else {  // max Z plane: y outer 0..14, x inner 0..14
    const u32 s = seq - 3871u;
    *z = 15;
    *y = static_cast<int>(s / 15u);
    *x = static_cast<int>(s % 15u);
  }
}
__device__ __forceinline__ F3 mc_interpolate_vertex(F3 v1, F3 v2, float sdf1, float sdf2) {
  const float diff = sdf1 - sdf2;
  if (fabsf(diff) >= 1e-6f) {
    const float t = sdf1 / diff;
    return F3{v1.x + t * (v2.x - v1.x), v1.y + t * (v2.y - v1.y), v1.z + t * (v2.z - v1.z)};
  }
  return F3{0.5f * (v1.x + v2.x), 0.5f * (v1.y + v2.y), 0.5f * (v1.z + v2.z)};
}
__device__ __forceinline__ u32 mc_triangles(u32 cfg) {
  u32 n = 0;
  while (n < 16 && kMcTriangleTable[cfg][n] != -1) n += 3;
  return n / 3;
}

// Eigen normalized(): a / sqrt(squaredNorm) when that is > 0, else a unchanged (a degenerate triangle keeps its zero normal)
__device__ __forceinline__ F3 normalized3(F3 a) {
  const float z = dot3(a, a);
  if (z > 0.0f) {
    const float s = sqrtf(z);
    return F3{a.x / s, a.y / s, a.z / s};
  }
  return a;
}

// The rare vertex the staged samples cannot serve: its block through the hash, one voxel (weight and colour word) from HBM.
// l is clamped into the block by the caller; a block index beyond the packed keys names no block.
__device__ __forceinline__ u32 vertex_color_unstaged(const MeshView& L, const int bb[3], const int l[3], float min_weight, bool* missing) {
  u32 slot = kInvalid;
  if (bb[0] >= -kIdxBias && bb[0] < kIdxBias && bb[1] >= -kIdxBias && bb[1] < kIdxBias && bb[2] >= -kIdxBias && bb[2] < kIdxBias)
    slot = ht_find(L.ht_keys, L.ht_mask, pack_key(bb[0], bb[1], bb[2]));
  if (slot == kInvalid) {
    *missing = true;
    return 0u;
  }
  const u32 lin = static_cast<u32>(l[0]) | (static_cast<u32>(l[1]) << 4) | (static_cast<u32>(l[2]) << 8);
  const u32* vw = L.voxels + (static_cast<size_t>(L.ht_vals[slot]) * kVoxelsPerBlock + lin) * kWordsPerVoxel;
  return __uint_as_float(vw[1]) > min_weight ? vw[2] : 0u;
}

// MeshIntegrator::updateMeshColor for one vertex: the voxel that contains it (computeVoxelIndexFromCoordinates); outside the
// block, the block found by coordinates and the voxel clamped into it (getVoxelByCoordinates); missing only when that block does
// not exist.  Where a float coordinate resolves a voxel both are among the staged 17^3 samples (the containing voxel is a corner
// of the vertex's cube).  Hundreds of thousands of blocks out it does not: the vertex can round into a block below its own or
// into a voxel past the staged face, and vertex_color_unstaged serves it.
__device__ __forceinline__ u32 vertex_color(const MeshView& L, F3 v, const int b[3], const float o[3], const u32* nbr_pool, const u32* col,
                                            const unsigned char* ok, float min_weight, bool* missing) {
  const float p[3] = {v.x, v.y, v.z};
  int s[3];
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s[k] = grid_index((p[k] - o[k]) * L.voxel_size_inv);
    inside = inside && s[k] >= 0 && s[k] < kVps;
  }
  if (!inside) {
    int bb[3], l[3];
    u32 sel = 0;
    bool staged = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      bb[k] = grid_index(p[k] * L.block_size_inv);
      const int d = bb[k] - b[k];
      const float ob = static_cast<float>(bb[k]) * L.block_size;
      l[k] = grid_index((p[k] - ob) * L.voxel_size_inv);
      l[k] = l[k] < 0 ? 0 : (l[k] > kVps - 1 ? kVps - 1 : l[k]);
      s[k] = d * kVps + l[k];
      staged = staged && d >= 0 && d <= 1 && s[k] <= kVps;
      sel |= (d == 1 ? 1u : 0u) << k;
    }
    if (!staged) return vertex_color_unstaged(L, bb, l, min_weight, missing);
    if (nbr_pool[sel] == kInvalid) {
      *missing = true;
      return 0u;
    }
  }
  const u32 ci = static_cast<u32>(s[0] + kCorner * (s[1] + kCorner * s[2]));
  return ok[ci] ? col[ci] : 0u;  // getColorIfValid, else the default Color()
}

// One workgroup per block.  kWrite = false: blocks are all allocated blocks in (z, y, x) order, out = triangles per block.
// kWrite = true: blocks are the ones with triangles, vertices written from vert_begin[i] on.
template <bool kWrite>
__global__ void __launch_bounds__(256) k_mesh_block(MeshView L, const u32* __restrict__ pools, const u64* __restrict__ block_keys, float min_weight,
                                                    u32* __restrict__ block_tris, const u64* __restrict__ vert_begin, float* __restrict__ pos,
                                                    float* __restrict__ nrm, uint8_t* __restrict__ rgb, u32* __restrict__ n_missing) {
  __shared__ float sdf[kCorners];
  __shared__ u32 col[kWrite ? kCorners : 1];
  __shared__ unsigned char ok[kCorners];
  __shared__ u32 nbr_pool[8];
  __shared__ u32 scan_lds[4];
  const u32 i = blockIdx.x;
  const u32 pool = pools[i];
  int bx, by, bz;
  unpack_key(block_keys[pool], &bx, &by, &bz);
  if (threadIdx.x < 8) {
    const int dx = threadIdx.x & 1, dy = (threadIdx.x >> 1) & 1, dz = threadIdx.x >> 2;
    u32 p = pool;
    if (threadIdx.x != 0) {
      const u32 slot = ht_find(L.ht_keys, L.ht_mask, pack_key(bx + dx, by + dy, bz + dz));
      p = slot == kInvalid ? kInvalid : L.ht_vals[slot];
    }
    nbr_pool[threadIdx.x] = p;
  }
  __syncthreads();
  for (u32 c = threadIdx.x; c < kCorners; c += 256) {
    const u32 cx = c % kCorner, cy = (c / kCorner) % kCorner, cz = c / (kCorner * kCorner);
    const u32 sel = (cx == 16u ? 1u : 0u) | (cy == 16u ? 2u : 0u) | (cz == 16u ? 4u : 0u);
    const u32 p = nbr_pool[sel];
    float d = 0.0f;
    u32 cw = 0;
    bool valid = false;
    if (p != kInvalid) {
      const u32 lin = (cx & 15u) | ((cy & 15u) << 4) | ((cz & 15u) << 8);
      const u32* vw = L.voxels + (static_cast<size_t>(p) * kVoxelsPerBlock + lin) * kWordsPerVoxel;
      d = __uint_as_float(vw[0]);
      valid = __uint_as_float(vw[1]) > min_weight;  // utils::getSdfIfValid / getColorIfValid: weight <= min_weight is invalid
      if (kWrite) cw = vw[2];
    }
    sdf[c] = d;
    ok[c] = valid ? 1 : 0;
    if (kWrite) col[c] = cw;
  }
  __syncthreads();
  auto cube_config = [&](u32 seq, int* x, int* y, int* z) -> u32 {
    cube_of_seq(seq, x, y, z);
    u32 cfg = 0;
    bool all = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int ox = (c ^ (c >> 1)) & 1, oy = (c >> 1) & 1, oz = c >> 2;
      const u32 ci = static_cast<u32>((*x + ox) + kCorner * ((*y + oy) + kCorner * (*z + oz)));
      all = all && ok[ci] != 0;
      if (sdf[ci] < 0.0f) cfg |= 1u << c;
    }
    return all ? cfg : 0u;
  };
  if (!kWrite) {  // thread t counts the 16 consecutive cubes [16 t, 16 t + 16) of the block's sequence
    u32 mine = 0;
#pragma unroll 1
    for (u32 k = 0; k < 16; ++k) {
      int x, y, z;
      mine += mc_triangles(cube_config(threadIdx.x * 16u + k, &x, &y, &z));
    }
    u32 total;
    (void)block_exclusive_scan<4>(mine, &total, scan_lds);
    if (threadIdx.x == 0) block_tris[i] = total;
    return;
  }
  // Round k: thread t meshes cube 256 k + t; a block-wide scan per round puts the round's triangles in sequence order behind the
  // previous rounds'.  Neighbouring lanes then write neighbouring vertex ranges (coalesced stores), where sixteen consecutive
  // cubes per thread would scatter every store over up to 64 cache lines.
  const int b[3] = {bx, by, bz};
  const float o[3] = {static_cast<float>(bx) * L.block_size, static_cast<float>(by) * L.block_size, static_cast<float>(bz) * L.block_size};
  u64 round_base = vert_begin[i];
  u32 missing = 0;
#pragma unroll 1
  for (u32 k = 0; k < 16; ++k) {
    int x, y, z;
    const u32 cfg = cube_config(k * 256u + threadIdx.x, &x, &y, &z);
    u32 round_tris;
    const u32 off = block_exclusive_scan<4>(mc_triangles(cfg), &round_tris, scan_lds);
    u64 vi = round_base + 3ull * off;
    round_base += 3ull * round_tris;
    if (cfg == 0 || cfg == 255u) continue;
    const F3 base{o[0] + center_coord(x, L.voxel_size), o[1] + center_coord(y, L.voxel_size), o[2] + center_coord(z, L.voxel_size)};
    const signed char* row = kMcTriangleTable[cfg];
    for (int c = 0; c < 16 && row[c] != -1; c += 3) {
      F3 v[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int e = row[c + 2 - j];  // vertices are emitted as (col + 2, col + 1, col)
        const int a = kMcEdgePairs[e][0], bb = kMcEdgePairs[e][1];
        const int ax = (a ^ (a >> 1)) & 1, ay = (a >> 1) & 1, az = a >> 2;
        const int bxx = (bb ^ (bb >> 1)) & 1, byy = (bb >> 1) & 1, bzz = bb >> 2;
        const F3 va{base.x + static_cast<float>(ax) * L.voxel_size, base.y + static_cast<float>(ay) * L.voxel_size, base.z + static_cast<float>(az) * L.voxel_size};
        const F3 vb{base.x + static_cast<float>(bxx) * L.voxel_size, base.y + static_cast<float>(byy) * L.voxel_size, base.z + static_cast<float>(bzz) * L.voxel_size};
        const float sa = sdf[(x + ax) + kCorner * ((y + ay) + kCorner * (z + az))];
        const float sb = sdf[(x + bxx) + kCorner * ((y + byy) + kCorner * (z + bzz))];
        v[j] = mc_interpolate_vertex(va, vb, sa, sb);
      }
      // face normal over the emitted order: points to the positive (observed free) side, DESIGN.md section 7d
      const F3 n = normalized3(cross3(v[1] - v[0], v[2] - v[0]));
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        bool miss = false;
        const u32 cw = vertex_color(L, v[j], b, o, nbr_pool, col, ok, min_weight, &miss);
        missing += miss ? 1u : 0u;
        pos[3 * vi] = v[j].x;
        pos[3 * vi + 1] = v[j].y;
        pos[3 * vi + 2] = v[j].z;
        nrm[3 * vi] = n.x;
        nrm[3 * vi + 1] = n.y;
        nrm[3 * vi + 2] = n.z;
        rgb[3 * vi] = static_cast<uint8_t>(cw >> 24);  // wire word a | b << 8 | g << 16 | r << 24
        rgb[3 * vi + 1] = static_cast<uint8_t>(cw >> 16);
        rgb[3 * vi + 2] = static_cast<uint8_t>(cw >> 8);
        ++vi;
      }
    }
  }
  if (missing) atomicAdd(n_missing, missing);
}

// ---- colour modes (voxblox mesh_vis.h) and the wire encoding -----------------------------------------------------------
__device__ __forceinline__ uint8_t unit_to_byte(float u) {  // std::min(u, 1) * 255, truncated
  const float c = (u < 1.0f ? u : 1.0f) * 255.0f;
  return static_cast<uint8_t>(c > 0.0f ? static_cast<int>(c) : 0);
}
__device__ __forceinline__ uint16_t encode_coord(float p, float block_edge, int index) {
  const float q = (p / block_edge - static_cast<float>(index)) / (2.0f / 65535.0f);
  if (!(q > 0.0f)) return 0;
  if (q >= 65535.0f) return 65535;
  return static_cast<uint16_t>(q);
}

__global__ void __launch_bounds__(256) k_mesh_msg(const float* __restrict__ pos, const float* __restrict__ nrm, const uint8_t* __restrict__ rgb,
                                                  const int32_t* __restrict__ bidx, const u64* __restrict__ vbegin, float block_edge, int mode,
                                                  uint16_t* __restrict__ ox, uint16_t* __restrict__ oy, uint16_t* __restrict__ oz, uint8_t* __restrict__ orr,
                                                  uint8_t* __restrict__ og, uint8_t* __restrict__ ob) {
  const u32 blk = blockIdx.x;
  const int ix = bidx[3 * blk], iy = bidx[3 * blk + 1], iz = bidx[3 * blk + 2];
  const F3 l1 = normalized3(F3{0.8f, -0.2f, 0.7f}), l2 = normalized3(F3{-0.5f, 0.2f, 0.2f});
  for (u64 v = vbegin[blk] + threadIdx.x; v < vbegin[blk + 1]; v += 256) {
    ox[v] = encode_coord(pos[3 * v], block_edge, ix);
    oy[v] = encode_coord(pos[3 * v + 1], block_edge, iy);
    oz[v] = encode_coord(pos[3 * v + 2], block_edge, iz);
    const F3 n{nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]};
    uint8_t c[3] = {rgb[3 * v], rgb[3 * v + 1], rgb[3 * v + 2]};
    if (mode == COX_MESH_NORMALS) {
      const float f[3] = {n.x, n.y, n.z};
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = unit_to_byte(f[k] * 0.5f + 0.5f);
    } else if (mode == COX_MESH_GRAY) {
      c[0] = c[1] = c[2] = unit_to_byte(0.5f);
    } else if (mode == COX_MESH_LAMBERT || mode == COX_MESH_LAMBERT_COLOR) {
      const float d1 = std_max(dot3(n, l1), 0.0f), d2 = std_max(dot3(n, l2), 0.0f);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const float base = (mode == COX_MESH_LAMBERT) ? 0.5f : static_cast<float>(c[k]) / 255.0f;
        c[k] = unit_to_byte((d1 * base + d2 * base) + 0.2f);
      }
    }
    orr[v] = c[0];
    og[v] = c[1];
    ob[v] = c[2];
  }
}

struct Xf {
  float qw, qx, qy, qz, tx, ty, tz;
};
__device__ __forceinline__ F3 rotate_xf(const Xf& T, F3 v) { return quat_rotate(T.qw, T.qx, T.qy, T.qz, v); }
// in place when src == dst; otherwise a (moved) copy, colours included
__global__ void __launch_bounds__(256) k_mesh_transform(const float* __restrict__ pos_in, const float* __restrict__ nrm_in, const uint8_t* __restrict__ rgb_in,
                                                        u64 n, Xf T, int move, float* pos_out, float* nrm_out, uint8_t* rgb_out) {
  const u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n) return;
  F3 p{pos_in[3 * v], pos_in[3 * v + 1], pos_in[3 * v + 2]};
  F3 q{nrm_in[3 * v], nrm_in[3 * v + 1], nrm_in[3 * v + 2]};
  if (move) {
    p = rotate_xf(T, p);
    p = F3{p.x + T.tx, p.y + T.ty, p.z + T.tz};
    q = rotate_xf(T, q);
  }
  pos_out[3 * v] = p.x;
  pos_out[3 * v + 1] = p.y;
  pos_out[3 * v + 2] = p.z;
  nrm_out[3 * v] = q.x;
  nrm_out[3 * v + 1] = q.y;
  nrm_out[3 * v + 2] = q.z;
  if (rgb_out && rgb_out != rgb_in) {
    rgb_out[3 * v] = rgb_in[3 * v];
    rgb_out[3 * v + 1] = rgb_in[3 * v + 1];
    rgb_out[3 * v + 2] = rgb_in[3 * v + 2];
  }
}

// ---- createConnectedMesh -------------------------------------------------------------------------------------------------
// cell = round(double(p) * inv), the key k_iso_insert (cox_submap.hip) uses; lo / hi per axis first, so that the key can drop
// to 21 bits per axis relative to lo
__device__ __forceinline__ long long cell_of(float p, double inv) { return static_cast<long long>(round(static_cast<double>(p) * inv)); }
// grid-strided over a capped grid, reduced per workgroup: six 64-bit atomics per workgroup (per wave they serialised the kernel)
__global__ void __launch_bounds__(256) k_weld_bounds(const float* __restrict__ pos, u64 n, double inv, long long* __restrict__ lohi /*[6]*/) {
  __shared__ long long red[4][6];
  long long lo[3] = {LLONG_MAX, LLONG_MAX, LLONG_MAX}, hi[3] = {LLONG_MIN, LLONG_MIN, LLONG_MIN};
  for (u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x; v < n; v += static_cast<u64>(gridDim.x) * blockDim.x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long c = cell_of(pos[3 * v + k], inv);
      lo[k] = c < lo[k] ? c : lo[k];
      hi[k] = c > hi[k] ? c : hi[k];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long a = __shfl_xor(lo[k], off, 64), b = __shfl_xor(hi[k], off, 64);
      lo[k] = a < lo[k] ? a : lo[k];
      hi[k] = b > hi[k] ? b : hi[k];
    }
  }
  const u32 wave = threadIdx.x >> 6;
  if (lane_id() == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      red[wave][k] = lo[k];
      red[wave][3 + k] = hi[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    long long r = red[0][threadIdx.x];
    for (int w = 1; w < 4; ++w) {
      const long long q = red[w][threadIdx.x];
      r = (threadIdx.x < 3) ? (q < r ? q : r) : (q > r ? q : r);
    }
    if (threadIdx.x < 3) {
      if (r != LLONG_MAX) atomicMin(&lohi[threadIdx.x], r);
    } else if (r != LLONG_MIN) {
      atomicMax(&lohi[threadIdx.x], r);
    }
  }
}
__global__ void __launch_bounds__(256) k_weld_insert(const float* __restrict__ pos, u64 n, double inv, long long ox, long long oy, long long oz,
                                                     u64* __restrict__ keys, u32* __restrict__ first, u32 mask, u32* __restrict__ vslot, u32* d_err) {
  const u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const long long cx = cell_of(pos[3 * v], inv) - ox, cy = cell_of(pos[3 * v + 1], inv) - oy, cz = cell_of(pos[3 * v + 2], inv) - oz;
  vslot[v] = kInvalid;
  if (cx < 0 || cy < 0 || cz < 0 || cx >= (1 << 21) || cy >= (1 << 21) || cz >= (1 << 21)) {
    atomicOr(d_err, kErrRange);
    return;
  }
  const u64 key = static_cast<u64>(cx) | (static_cast<u64>(cy) << 21) | (static_cast<u64>(cz) << 42);
  bool fresh;
  const u32 slot = ht_insert(keys, mask, key, &fresh);
  if (slot == kInvalid) {
    atomicOr(d_err, kErrTable);
    return;
  }
  atomicMin(&first[slot], static_cast<u32>(v));
  vslot[v] = slot;
}
__global__ void __launch_bounds__(256) k_weld_flag(u64 n, const u32* __restrict__ first, const u32* __restrict__ vslot, u32* __restrict__ flag) {
  const u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const u32 slot = vslot[v];
  flag[v] = (slot != kInvalid && first[slot] == static_cast<u32>(v)) ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_weld_write(const float* __restrict__ pos, const float* __restrict__ nrm, const uint8_t* __restrict__ rgb, u64 n,
                                                    const u32* __restrict__ first, const u32* __restrict__ vslot, const u32* __restrict__ flag,
                                                    const u32* __restrict__ cidx, float* __restrict__ opos, float* __restrict__ onrm, uint8_t* __restrict__ orgb,
                                                    u32* __restrict__ otri) {
  const u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const u32 slot = vslot[v];
  if (slot == kInvalid) return;  // reported through d_err
  otri[v] = cidx[first[slot]];
  if (!flag[v]) return;
  const u64 c = cidx[v];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    opos[3 * c + k] = pos[3 * v + k];
    onrm[3 * c + k] = nrm[3 * v + k];
    orgb[3 * c + k] = rgb[3 * v + k];
  }
}

// a stream-ordered point behind every frame enqueued on the layer (the submission threads drained by COX_ENTRY)
int order_behind_frames(cox_layer* L) {
  COX_HIP(hipSetDevice(L->device));
  cox_layer_wait_writes(L, nullptr);
  COX_HIP(hipStreamSynchronize(nullptr));
  return COX_OK;
}

void free_meshlayer(cox_meshlayer* M) {
  if (!M) return;
  (void)hipSetDevice(M->device);
  delete M;
}
void free_meshconn(cox_meshconn* C) {
  if (!C) return;
  (void)hipSetDevice(C->device);
  delete C;
}

}  // namespace

extern "C" {

int cox_meshlayer_from_layer(cox_layer_t* L, float min_weight, cox_meshlayer_t** out, uint64_t* n_blocks, uint64_t* n_triangles) {
  COX_ENTRY();
  if (!L || !out) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  COX_TRY(order_behind_frames(L));
  u32 nb = 0;
  COX_HIP(hipMemcpy(&nb, L->d_nblocks, sizeof(u32), hipMemcpyDeviceToHost));
  if (nb > L->capacity) nb = static_cast<u32>(L->capacity);
  cox_meshlayer* M = new (std::nothrow) cox_meshlayer();
  if (!M) return COX_ERR_OUT_OF_MEMORY;
  M->device = L->device;
  M->voxel_size = L->voxel_size;
  M->block_edge = L->block_size;
  M->vertex_begin.assign(1, 0);
  auto fail = [&](int st) {
    free_meshlayer(M);
    return st;
  };
  if (nb > 0) {
    // blocks in (z, y, x) order: the packed key orders that way
    std::vector<u64> keys(nb);
    if (hipMemcpy(keys.data(), L->block_keys, sizeof(u64) * nb, hipMemcpyDeviceToHost) != hipSuccess) return fail(COX_ERR_NO_DEVICE);
    std::vector<u32> order(nb);
    for (u32 i = 0; i < nb; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return keys[a] < keys[b]; });
    DevBuf<u32> d_order, d_tris, d_missing;
    DevBuf<u64> d_begin;
    if (int st = d_order.alloc(nb)) return fail(st);
    if (int st = d_tris.alloc(nb)) return fail(st);
    if (int st = d_missing.alloc(1)) return fail(st);
    if (hipMemcpy(d_order.p, order.data(), sizeof(u32) * nb, hipMemcpyHostToDevice) != hipSuccess) return fail(COX_ERR_NO_DEVICE);
    const MeshView V{L->voxels, L->ht_keys, L->ht_vals, L->ht_cap - 1, L->voxel_size, L->voxel_size_inv, L->block_size, L->block_size_inv};
    EventPair t_count, t_fill;
    if (t_count.create() != COX_OK || t_fill.create() != COX_OK) return fail(COX_ERR_NO_DEVICE);
    (void)t_count.begin(nullptr);
    hipLaunchKernelGGL(k_mesh_block<false>, dim3(nb), dim3(256), 0, nullptr, V, d_order.p, L->block_keys, min_weight, d_tris.p,
                       static_cast<const u64*>(nullptr), static_cast<float*>(nullptr), static_cast<float*>(nullptr), static_cast<uint8_t*>(nullptr),
                       static_cast<u32*>(nullptr));
    (void)t_count.end(nullptr);
    std::vector<u32> tris(nb);
    if (hipMemcpy(tris.data(), d_tris.p, sizeof(u32) * nb, hipMemcpyDeviceToHost) != hipSuccess) return fail(COX_ERR_NO_DEVICE);
    // the blocks with triangles, their vertex ranges
    std::vector<u32> live;
    u64 nv = 0;
    for (u32 i = 0; i < nb; ++i) {
      if (!tris[i]) continue;
      live.push_back(order[i]);
      int x, y, z;
      unpack_key(keys[order[i]], &x, &y, &z);
      M->block_index.push_back(x);
      M->block_index.push_back(y);
      M->block_index.push_back(z);
      nv += 3ull * tris[i];
      M->vertex_begin.push_back(nv);
    }
    M->n_blocks = live.size();
    M->n_vertices = nv;
    if (nv > 0xFFFFFFF0ull) return fail(COX_ERR_UNSUPPORTED);
    if (M->n_blocks) {
      int st = COX_OK;
      DevBuf<float> pos, nrm;
      DevBuf<uint8_t> rgb;
      if (!st) st = pos.alloc(3 * nv);
      if (!st) st = nrm.alloc(3 * nv);
      if (!st) st = rgb.alloc(3 * nv);
      if (!st) st = d_begin.alloc(M->n_blocks);
      if (!st && hipMemcpy(d_order.p, live.data(), sizeof(u32) * live.size(), hipMemcpyHostToDevice) != hipSuccess) st = COX_ERR_NO_DEVICE;
      if (!st && hipMemcpy(d_begin.p, M->vertex_begin.data(), sizeof(u64) * M->n_blocks, hipMemcpyHostToDevice) != hipSuccess) st = COX_ERR_NO_DEVICE;
      if (!st && hipMemsetAsync(d_missing.p, 0, sizeof(u32), nullptr) != hipSuccess) st = COX_ERR_NO_DEVICE;
      if (st) return fail(st);
      (void)t_fill.begin(nullptr);
      hipLaunchKernelGGL(k_mesh_block<true>, dim3(static_cast<u32>(M->n_blocks)), dim3(256), 0, nullptr, V, d_order.p, L->block_keys, min_weight,
                         static_cast<u32*>(nullptr), d_begin.p, pos.p, nrm.p, rgb.p, d_missing.p);
      (void)t_fill.end(nullptr);
      u32 miss = 0;
      if (hipMemcpy(&miss, d_missing.p, sizeof(u32), hipMemcpyDeviceToHost) != hipSuccess) return fail(COX_ERR_NO_DEVICE);
      M->n_color_missing = miss;
      M->pos = pos.release();
      M->nrm = nrm.release();
      M->rgb = rgb.release();
      if (!t_fill.elapsed_ms(&M->kernel_ms[1])) return fail(COX_ERR_NO_DEVICE);
    }
    if (!t_count.elapsed_ms(&M->kernel_ms[0]) || hipGetLastError() != hipSuccess) return fail(COX_ERR_NO_DEVICE);
  }
  if (n_blocks) *n_blocks = M->n_blocks;
  if (n_triangles) *n_triangles = M->n_vertices / 3;
  *out = M;
  return COX_OK;
}

void cox_meshlayer_destroy(cox_meshlayer_t* M) { free_meshlayer(M); }

int cox_meshlayer_size(const cox_meshlayer_t* M, uint64_t* n_blocks, uint64_t* n_vertices, float* block_edge_length) {
  COX_ENTRY_NO_DRAIN();
  if (!M) return COX_ERR_INVALID_ARG;
  if (n_blocks) *n_blocks = M->n_blocks;
  if (n_vertices) *n_vertices = M->n_vertices;
  if (block_edge_length) *block_edge_length = M->block_edge;
  return COX_OK;
}

int cox_meshlayer_stats(const cox_meshlayer_t* M, uint64_t* n_color_missing, double kernel_ms[2]) {
  COX_ENTRY_NO_DRAIN();
  if (!M) return COX_ERR_INVALID_ARG;
  if (n_color_missing) *n_color_missing = M->n_color_missing;
  if (kernel_ms) {
    kernel_ms[0] = M->kernel_ms[0];
    kernel_ms[1] = M->kernel_ms[1];
  }
  return COX_OK;
}

int cox_meshlayer_download(const cox_meshlayer_t* M, int32_t* block_index, uint64_t* vertex_begin, float* xyz, float* normals, uint8_t* rgb,
                           uint64_t cap_blocks, uint64_t cap_vertices) {
  COX_ENTRY();
  if (!M) return COX_ERR_INVALID_ARG;
  if ((block_index || vertex_begin) && cap_blocks < M->n_blocks) return COX_ERR_BUFFER_TOO_SMALL;
  if ((xyz || normals || rgb) && cap_vertices < M->n_vertices) return COX_ERR_BUFFER_TOO_SMALL;
  if (block_index) std::copy(M->block_index.begin(), M->block_index.end(), block_index);
  if (vertex_begin) std::copy(M->vertex_begin.begin(), M->vertex_begin.end(), vertex_begin);
  if (M->n_vertices == 0) return COX_OK;
  COX_HIP(hipSetDevice(M->device));
  if (xyz) COX_HIP(hipMemcpy(xyz, M->pos, sizeof(float) * 3 * M->n_vertices, hipMemcpyDeviceToHost));
  if (normals) COX_HIP(hipMemcpy(normals, M->nrm, sizeof(float) * 3 * M->n_vertices, hipMemcpyDeviceToHost));
  if (rgb) COX_HIP(hipMemcpy(rgb, M->rgb, 3 * M->n_vertices, hipMemcpyDeviceToHost));
  return COX_OK;
}

int cox_meshlayer_data_dev(const cox_meshlayer_t* M, const float** xyz_dev, const float** normals_dev, const uint8_t** rgb_dev, uint64_t* n_vertices) {
  COX_ENTRY_NO_DRAIN();
  if (!M) return COX_ERR_INVALID_ARG;
  if (xyz_dev) *xyz_dev = M->pos;
  if (normals_dev) *normals_dev = M->nrm;
  if (rgb_dev) *rgb_dev = M->rgb;
  if (n_vertices) *n_vertices = M->n_vertices;
  return COX_OK;
}

int cox_meshlayer_transform(cox_meshlayer_t* M, const float T[7]) {
  COX_ENTRY();
  if (!M || !T) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  if (M->n_vertices == 0) return COX_OK;
  COX_HIP(hipSetDevice(M->device));
  const Xf X{T[0], T[1], T[2], T[3], T[4], T[5], T[6]};
  const u32 grid = static_cast<u32>((M->n_vertices + 255) / 256);
  hipLaunchKernelGGL(k_mesh_transform, dim3(grid), dim3(256), 0, nullptr, M->pos, M->nrm, M->rgb, M->n_vertices, X, 1, M->pos, M->nrm,
                     static_cast<uint8_t*>(nullptr));
  if (hipStreamSynchronize(nullptr) != hipSuccess || hipGetLastError() != hipSuccess) return COX_ERR_NO_DEVICE;
  M->transformed = true;
  return COX_OK;
}

int cox_meshlayer_msg(const cox_meshlayer_t* M, int color_mode, uint16_t* x, uint16_t* y, uint16_t* z, uint8_t* r, uint8_t* g, uint8_t* b,
                      uint64_t cap_vertices) {
  COX_ENTRY();
  if (!M || !x || !y || !z || !r || !g || !b || color_mode < COX_MESH_COLOR || color_mode > COX_MESH_LAMBERT_COLOR) return COX_ERR_INVALID_ARG;
  if (cap_vertices < M->n_vertices) return COX_ERR_BUFFER_TOO_SMALL;
  COX_TRY(device_present());
  const u64 nv = M->n_vertices;
  if (nv == 0) return COX_OK;
  COX_HIP(hipSetDevice(M->device));
  DevBuf<int32_t> bidx;
  DevBuf<u64> vbeg;
  DevBuf<uint16_t> xyz16;
  DevBuf<uint8_t> c8;
  COX_TRY(bidx.alloc(3 * M->n_blocks));
  COX_TRY(vbeg.alloc(M->n_blocks + 1));
  COX_TRY(xyz16.alloc(3 * nv));
  COX_TRY(c8.alloc(3 * nv));
  COX_HIP(hipMemcpy(bidx.p, M->block_index.data(), sizeof(int32_t) * 3 * M->n_blocks, hipMemcpyHostToDevice));
  COX_HIP(hipMemcpy(vbeg.p, M->vertex_begin.data(), sizeof(u64) * (M->n_blocks + 1), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_mesh_msg, dim3(static_cast<u32>(M->n_blocks)), dim3(256), 0, nullptr, M->pos, M->nrm, M->rgb, bidx.p, vbeg.p, M->block_edge,
                     color_mode, xyz16.p, xyz16.p + nv, xyz16.p + 2 * nv, c8.p, c8.p + nv, c8.p + 2 * nv);
  COX_HIP(hipMemcpy(x, xyz16.p, sizeof(uint16_t) * nv, hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(y, xyz16.p + nv, sizeof(uint16_t) * nv, hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(z, xyz16.p + 2 * nv, sizeof(uint16_t) * nv, hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(r, c8.p, nv, hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(g, c8.p + nv, nv, hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(b, c8.p + 2 * nv, nv, hipMemcpyDeviceToHost));
  return COX_OK;
}

int cox_meshlayer_connected(const cox_meshlayer_t* const* parts, const float* T_per_part, uint64_t n_parts, float proximity_threshold, cox_meshconn_t** out,
                            uint64_t* n_vertices, uint64_t* n_triangles) {
  COX_ENTRY();
  if (!out || (n_parts && !parts) || !(proximity_threshold > 0.0f)) return COX_ERR_INVALID_ARG;
  for (u64 p = 0; p < n_parts; ++p)
    if (!parts[p] || parts[p]->device != parts[0]->device) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  int dev = 0;
  if (n_parts) {
    dev = parts[0]->device;
  } else {
    COX_HIP(hipGetDevice(&dev));
  }
  COX_HIP(hipSetDevice(dev));
  u64 nv = 0;
  for (u64 p = 0; p < n_parts; ++p) nv += parts[p]->n_vertices;
  if (nv > 0x7FFFFFF0ull) return COX_ERR_UNSUPPORTED;
  cox_meshconn* C = new (std::nothrow) cox_meshconn();
  if (!C) return COX_ERR_OUT_OF_MEMORY;
  C->device = dev;
  auto fail = [&](int st) {
    free_meshconn(C);
    return st;
  };
  if (nv) {
    // 1. every part moved into one buffer, in part order
    DevBuf<float> pos, nrm;
    DevBuf<uint8_t> rgb;
    if (int st = pos.alloc(3 * nv)) return fail(st);
    if (int st = nrm.alloc(3 * nv)) return fail(st);
    if (int st = rgb.alloc(3 * nv)) return fail(st);
    u64 at = 0;
    for (u64 p = 0; p < n_parts; ++p) {
      const cox_meshlayer* M = parts[p];
      if (!M->n_vertices) continue;
      Xf X{1, 0, 0, 0, 0, 0, 0};
      const int move = T_per_part != nullptr;
      if (move) X = Xf{T_per_part[7 * p], T_per_part[7 * p + 1], T_per_part[7 * p + 2], T_per_part[7 * p + 3], T_per_part[7 * p + 4], T_per_part[7 * p + 5],
                       T_per_part[7 * p + 6]};
      hipLaunchKernelGGL(k_mesh_transform, dim3(static_cast<u32>((M->n_vertices + 255) / 256)), dim3(256), 0, nullptr, M->pos, M->nrm, M->rgb, M->n_vertices, X,
                         move, pos.p + 3 * at, nrm.p + 3 * at, rgb.p + 3 * at);
      at += M->n_vertices;
    }
    // 2. cell bounds -> origin of the 21-bit keys
    const double inv = 1.0 / static_cast<double>(proximity_threshold);
    const u32 grid = static_cast<u32>((nv + 255) / 256);
    DevBuf<long long> lohi;
    if (int st = lohi.alloc(6)) return fail(st);
    const long long init[6] = {LLONG_MAX, LLONG_MAX, LLONG_MAX, LLONG_MIN, LLONG_MIN, LLONG_MIN};
    if (hipMemcpy(lohi.p, init, sizeof(init), hipMemcpyHostToDevice) != hipSuccess) return fail(COX_ERR_NO_DEVICE);
    hipLaunchKernelGGL(k_weld_bounds, dim3(std::min<u32>(grid, 1024u)), dim3(256), 0, nullptr, pos.p, nv, inv, lohi.p);
    long long hl[6];
    if (hipMemcpy(hl, lohi.p, sizeof(hl), hipMemcpyDeviceToHost) != hipSuccess) return fail(COX_ERR_NO_DEVICE);
    for (int k = 0; k < 3; ++k)
      if (hl[3 + k] - hl[k] >= (1ll << 21)) return fail(COX_ERR_INDEX_RANGE);
    // 3. first vertex in mesh order per cell
    const u32 hcap = next_pow2(2 * nv);
    DevBuf<u64> hkeys;
    DevBuf<u32> first, vslot, flag, cidx, sums, misc;
    if (int st = hkeys.alloc(hcap)) return fail(st);
    if (int st = first.alloc(hcap)) return fail(st);
    if (int st = vslot.alloc(nv)) return fail(st);
    if (int st = flag.alloc(nv)) return fail(st);
    if (int st = cidx.alloc(nv)) return fail(st);
    if (int st = sums.alloc(scan_num_blocks(static_cast<u32>(nv)) + 2)) return fail(st);
    if (int st = misc.alloc(2)) return fail(st);  // [0] error bits, [1] connected vertices
    (void)hipMemsetAsync(hkeys.p, 0xFF, sizeof(u64) * hcap, nullptr);
    (void)hipMemsetAsync(first.p, 0xFF, sizeof(u32) * hcap, nullptr);
    (void)hipMemsetAsync(misc.p, 0, sizeof(u32) * 2, nullptr);
    hipLaunchKernelGGL(k_weld_insert, dim3(grid), dim3(256), 0, nullptr, pos.p, nv, inv, hl[0], hl[1], hl[2], hkeys.p, first.p, hcap - 1, vslot.p, misc.p);
    hipLaunchKernelGGL(k_weld_flag, dim3(grid), dim3(256), 0, nullptr, nv, first.p, vslot.p, flag.p);
    ScanWorkspace ws;
    ws.block_sums = sums.p;
    exclusive_scan_u32(flag.p, cidx.p, nullptr, static_cast<u32>(nv), static_cast<u32>(nv), misc.p + 1, ws, nullptr);
    u32 hm[2] = {0, 0};
    if (hipMemcpy(hm, misc.p, sizeof(hm), hipMemcpyDeviceToHost) != hipSuccess) return fail(COX_ERR_NO_DEVICE);
    if (hm[0]) return fail(err_bits_to_status(hm[0]));
    // 4. survivors compacted in mesh order, every vertex replaced by its survivor's index
    C->n_vertices = hm[1];
    C->n_triangles = nv / 3;
    DevBuf<float> opos, onrm;
    DevBuf<uint8_t> orgb;
    DevBuf<u32> otri;
    if (int st = opos.alloc(3ull * C->n_vertices)) return fail(st);
    if (int st = onrm.alloc(3ull * C->n_vertices)) return fail(st);
    if (int st = orgb.alloc(3ull * C->n_vertices)) return fail(st);
    if (int st = otri.alloc(nv)) return fail(st);
    hipLaunchKernelGGL(k_weld_write, dim3(grid), dim3(256), 0, nullptr, pos.p, nrm.p, rgb.p, nv, first.p, vslot.p, flag.p, cidx.p, opos.p, onrm.p, orgb.p, otri.p);
    if (hipStreamSynchronize(nullptr) != hipSuccess || hipGetLastError() != hipSuccess) return fail(COX_ERR_NO_DEVICE);
    C->pos = opos.release();
    C->nrm = onrm.release();
    C->rgb = orgb.release();
    C->tri = otri.release();
  }
  if (n_vertices) *n_vertices = C->n_vertices;
  if (n_triangles) *n_triangles = C->n_triangles;
  *out = C;
  return COX_OK;
}

void cox_meshconn_destroy(cox_meshconn_t* C) { free_meshconn(C); }

int cox_meshconn_size(const cox_meshconn_t* C, uint64_t* n_vertices, uint64_t* n_triangles) {
  COX_ENTRY_NO_DRAIN();
  if (!C) return COX_ERR_INVALID_ARG;
  if (n_vertices) *n_vertices = C->n_vertices;
  if (n_triangles) *n_triangles = C->n_triangles;
  return COX_OK;
}

int cox_meshconn_download(const cox_meshconn_t* C, float* xyz, float* normals, uint8_t* rgb, uint32_t* triangles, uint64_t cap_vertices, uint64_t cap_triangles) {
  COX_ENTRY();
  if (!C) return COX_ERR_INVALID_ARG;
  if ((xyz || normals || rgb) && cap_vertices < C->n_vertices) return COX_ERR_BUFFER_TOO_SMALL;
  if (triangles && cap_triangles < C->n_triangles) return COX_ERR_BUFFER_TOO_SMALL;
  if (C->n_vertices == 0 && C->n_triangles == 0) return COX_OK;
  COX_HIP(hipSetDevice(C->device));
  if (xyz && C->n_vertices) COX_HIP(hipMemcpy(xyz, C->pos, sizeof(float) * 3 * C->n_vertices, hipMemcpyDeviceToHost));
  if (normals && C->n_vertices) COX_HIP(hipMemcpy(normals, C->nrm, sizeof(float) * 3 * C->n_vertices, hipMemcpyDeviceToHost));
  if (rgb && C->n_vertices) COX_HIP(hipMemcpy(rgb, C->rgb, 3 * C->n_vertices, hipMemcpyDeviceToHost));
  if (triangles && C->n_triangles) COX_HIP(hipMemcpy(triangles, C->tri, sizeof(u32) * 3 * C->n_triangles, hipMemcpyDeviceToHost));
  return COX_OK;
}

}  // extern "C"
