// MI355X (gfx950): the clean-up of the global mesh that coxgraph's server leaves to Open3D
// (ServerVisualizer::getFinalGlobalMesh, coxgraph/src/server/visualizer/server_visualizer.cpp:67-86): duplicate / degenerate
// triangles and unreferenced vertices removed, Taubin smoothing, vertex clustering, vertex normals -- in place on a cox_meshconn.
//
//   clean      k_tri_canon -> 3-word stable LSD sort of the canonical triples -> k_tri_dupflag (neighbours in sorted order,
//              flags scattered back to mesh order) -> k_mark_used -> two scans -> k_compact_tris / k_compact_verts
//   smooth     k_emit_edges (6 directed edges per triangle) -> sort by (u, v) -> k_edge_flags -> scan -> k_csr_fill, then one
//              k_taubin_half launch per half-step between two position buffers (Jacobi)
//   cluster    k_bounds_f32 -> k_cells -> 3-word sort of the vertex indices by (z, y, x) cell -> k_cell_flags -> scan ->
//              k_cell_ids -> k_cluster_avg (one thread per cell, members in ascending input index) -> k_reindex -> clean
//   normals    stable sort of the 3 nt (vertex, corner) pairs by vertex -> k_rows -> k_vertex_normals
//
// Every result is deterministic: there is no float atomic, every float sum runs sequentially in one thread in a stated order
// (ascending neighbour, member or triangle index), and every sort is the stable LSD sort of cox_sort.hpp on key bits sized
// from the actual ranges.  The rules are recollection of Open3D, not reference code: DESIGN.md section 7h ([U]).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <utility>

#include "../../include/coxgraph_hip_mesh.h"
#include "cox_host.hpp"
#include "cox_sort.hpp"

using namespace cox;

namespace {

int finish() {  // every entry point is synchronous
  if (hipStreamSynchronize(nullptr) != hipSuccess || hipGetLastError() != hipSuccess) return COX_ERR_NO_DEVICE;
  return COX_OK;
}
inline dim3 grid_for(u64 n) { return dim3(static_cast<u32>(std::max<u64>(1, (n + 255) / 256))); }
#define COX_LAUNCH(kernel, n, ...) hipLaunchKernelGGL(kernel, grid_for(n), dim3(256), 0, nullptr, __VA_ARGS__)

// Eigen normalized(), as the mesher's face normal (cox_mesher.hip)
__device__ __forceinline__ F3 normalized3(F3 a) {
  const float z = dot3(a, a);
  if (z > 0.0f) {
    const float s = sqrtf(z);
    return F3{a.x / s, a.y / s, a.z / s};
  }
  return a;
}
__device__ __forceinline__ F3 load3(const float* p, u32 i) { return F3{p[3ull * i], p[3ull * i + 1], p[3ull * i + 2]}; }
__device__ __forceinline__ void store3(float* p, u32 i, F3 v) {
  p[3ull * i] = v.x;
  p[3ull * i + 1] = v.y;
  p[3ull * i + 2] = v.z;
}

// ---- a permutation sorted word by word (low word first), each pass the stable LSD sort of cox_sort.hpp ---------------------
__global__ void __launch_bounds__(256) k_iota(u32* __restrict__ v, u32 n) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) v[i] = static_cast<u32>(i);
}
__global__ void __launch_bounds__(256) k_gather(const u32* __restrict__ word, const u32* __restrict__ perm, u32* __restrict__ key, u32 n) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) key[i] = word[perm[i]];
}
struct PermSort {
  DevBuf<u32> key[2], val[2], counts, totals;
  SortWorkspace ws;
  u32 n = 0;
  int cur = 0;
  int init(u32 count) {  // the identity permutation of count elements
    n = count;
    for (int b = 0; b < 2; ++b) {
      COX_TRY(key[b].alloc(n));
      COX_TRY(val[b].alloc(n));
    }
    ws.tiles_cap = std::min<u32>(kRsMaxTiles, std::max<u32>(1, sort_num_tiles(n)));  // beyond kRsMaxTiles tiles the tile doubles
    COX_TRY(counts.alloc(sort_counts_words(ws.tiles_cap)));
    COX_TRY(totals.alloc(sort_totals_words()));
    ws.counts = counts.p;
    ws.totals = totals.p;
    COX_HIP(hipMemsetAsync(totals.p, 0, sizeof(u32) * sort_totals_words(), nullptr));  // every sort leaves it zero again
    COX_LAUNCH(k_iota, n, val[0].p, n);
    return COX_OK;
  }
  // stable sort of the permutation by word[element], values < 2^bits
  void by(const u32* word, int bits) {
    if (bits <= 0 || n == 0) return;
    COX_LAUNCH(k_gather, n, word, val[cur].p, key[cur].p, n);
    cur ^= radix_sort_pairs<11>(key[cur].p, val[cur].p, key[cur ^ 1].p, val[cur ^ 1].p, nullptr, n, n, bits, false, 0, ws, nullptr, nullptr);
  }
  const u32* perm() const { return val[cur].p; }
};
struct Scan {
  DevBuf<u32> sums;
  ScanWorkspace ws;
  int init(u32 n_max) {
    COX_TRY(sums.alloc(scan_num_blocks(n_max) + 2));
    ws.block_sums = sums.p;
    return COX_OK;
  }
  void run(const u32* in, u32* out, u32 n, u32* d_total) { exclusive_scan_u32(in, out, nullptr, n, n, d_total, ws, nullptr); }
};

// ---- clean -------------------------------------------------------------------------------------------------------------------
// canonical form: the rotation with the smallest index first (orientation kept); deg = two equal indices
__global__ void __launch_bounds__(256) k_tri_canon(const u32* __restrict__ tri, u32 nt, u32* __restrict__ c0, u32* __restrict__ c1, u32* __restrict__ c2,
                                                   u32* __restrict__ deg) {
  const u64 t = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  const u32 a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
  deg[t] = (a == b || b == c || a == c) ? 1u : 0u;
  u32 x = a, y = b, z = c;
  if (b < a && b <= c) {
    x = b, y = c, z = a;
  } else if (c < a && c < b) {
    x = c, y = a, z = b;
  }
  c0[t] = x;
  c1[t] = y;
  c2[t] = z;
}
// i = position in sorted order.  The sort is stable and started from the identity, so the first of a run of equal triples is
// the first in mesh order.  n_removed[0] degenerate, [1] duplicates among the others.
__global__ void __launch_bounds__(256) k_tri_dupflag(const u32* __restrict__ perm, const u32* __restrict__ c0, const u32* __restrict__ c1,
                                                     const u32* __restrict__ c2, const u32* __restrict__ deg, u32 nt, u32* __restrict__ keep,
                                                     u32* __restrict__ n_removed) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  bool is_deg = false, is_dup = false;
  if (i < nt) {
    const u32 t = perm[i];
    is_deg = deg[t] != 0;
    if (i > 0 && !is_deg) {
      const u32 q = perm[i - 1];
      is_dup = c0[q] == c0[t] && c1[q] == c1[t] && c2[q] == c2[t];
    }
    keep[t] = (is_deg || is_dup) ? 0u : 1u;
  }
  const u32 nd = static_cast<u32>(__popcll(__ballot(is_deg))), nu = static_cast<u32>(__popcll(__ballot(is_dup)));
  if (lane_id() == 0) {
    if (nd) atomicAdd(&n_removed[0], nd);
    if (nu) atomicAdd(&n_removed[1], nu);
  }
}
__global__ void __launch_bounds__(256) k_mark_used(const u32* __restrict__ tri, const u32* __restrict__ keep, u32 nt, u32* __restrict__ used) {
  const u64 t = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= nt || !keep[t]) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) used[tri[3 * t + k]] = 1u;  // every writer stores the same value
}
__global__ void __launch_bounds__(256) k_compact_tris(const u32* __restrict__ tri, const u32* __restrict__ keep, const u32* __restrict__ tpos,
                                                      const u32* __restrict__ vpos, u32 nt, u32* __restrict__ otri) {
  const u64 t = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= nt || !keep[t]) return;
  const u64 o = tpos[t];
#pragma unroll
  for (int k = 0; k < 3; ++k) otri[3 * o + k] = vpos[tri[3 * t + k]];
}
__global__ void __launch_bounds__(256) k_compact_verts(const float* __restrict__ pos, const float* __restrict__ nrm, const uint8_t* __restrict__ rgb,
                                                       const u32* __restrict__ used, const u32* __restrict__ vpos, u32 nv, float* __restrict__ opos,
                                                       float* __restrict__ onrm, uint8_t* __restrict__ orgb) {
  const u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= nv || !used[v]) return;
  const u64 o = vpos[v];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    opos[3 * o + k] = pos[3 * v + k];
    onrm[3 * o + k] = nrm[3 * v + k];
    orgb[3 * o + k] = rgb[3 * v + k];
  }
}

// The mesh is replaced only once every kernel has run: a failure leaves it as it was.
int clean_impl(cox_meshconn* C, uint64_t removed[3]) {
  const u32 nv = static_cast<u32>(C->n_vertices), nt = static_cast<u32>(C->n_triangles);
  if (removed) removed[0] = removed[1] = removed[2] = 0;
  if (nv == 0 && nt == 0) return COX_OK;
  u32 hm[4] = {0, 0, 0, 0};  // degenerate, duplicate, surviving triangles, surviving vertices
  DevBuf<u32> keep, tpos, used, vpos;
  if (nt) {
    DevBuf<u32> c0, c1, c2, deg, misc;
    PermSort sort;
    Scan scan;
    COX_TRY(c0.alloc(nt));
    COX_TRY(c1.alloc(nt));
    COX_TRY(c2.alloc(nt));
    COX_TRY(deg.alloc(nt));
    COX_TRY(keep.alloc(nt));
    COX_TRY(tpos.alloc(nt));
    COX_TRY(used.alloc(nv));
    COX_TRY(vpos.alloc(nv));
    COX_TRY(misc.alloc(4));
    COX_TRY(scan.init(std::max(nt, nv)));
    COX_TRY(sort.init(nt));
    COX_HIP(hipMemsetAsync(misc.p, 0, sizeof(u32) * 4, nullptr));
    COX_HIP(hipMemsetAsync(used.p, 0, sizeof(u32) * std::max<u32>(nv, 1), nullptr));
    COX_LAUNCH(k_tri_canon, nt, C->tri, nt, c0.p, c1.p, c2.p, deg.p);
    const int bits = ceil_log2(nv);  // every index is < nv
    sort.by(c2.p, bits);
    sort.by(c1.p, bits);
    sort.by(c0.p, bits);
    COX_LAUNCH(k_tri_dupflag, nt, sort.perm(), c0.p, c1.p, c2.p, deg.p, nt, keep.p, misc.p);
    COX_LAUNCH(k_mark_used, nt, C->tri, keep.p, nt, used.p);
    scan.run(keep.p, tpos.p, nt, misc.p + 2);
    scan.run(used.p, vpos.p, nv, misc.p + 3);
    COX_HIP(hipMemcpy(hm, misc.p, sizeof(hm), hipMemcpyDeviceToHost));  // the sizes of the result
  }
  const u32 nt2 = hm[2], nv2 = hm[3];
  if (nt2 == 0) {  // nothing survives (no vertex is referenced)
    COX_TRY(finish());
    C->set_vertices(nullptr, nullptr, nullptr);
    C->set_triangles(nullptr);
  } else {
    DevBuf<float> opos, onrm;
    DevBuf<uint8_t> orgb;
    DevBuf<u32> otri;
    COX_TRY(opos.alloc(3ull * nv2));
    COX_TRY(onrm.alloc(3ull * nv2));
    COX_TRY(orgb.alloc(3ull * nv2));
    COX_TRY(otri.alloc(3ull * nt2));
    COX_LAUNCH(k_compact_tris, nt, C->tri, keep.p, tpos.p, vpos.p, nt, otri.p);
    COX_LAUNCH(k_compact_verts, nv, C->pos, C->nrm, C->rgb, used.p, vpos.p, nv, opos.p, onrm.p, orgb.p);
    COX_TRY(finish());
    C->set_vertices(opos.release(), onrm.release(), orgb.release());
    C->set_triangles(otri.release());
  }
  C->n_vertices = nv2;
  C->n_triangles = nt2;
  if (removed) {
    removed[0] = hm[0];
    removed[1] = hm[1];
    removed[2] = nv - nv2;
  }
  return COX_OK;
}

// ---- Taubin smoothing --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_emit_edges(const u32* __restrict__ tri, u32 nt, u32* __restrict__ eu, u32* __restrict__ ev) {
  const u64 t = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (t >= nt) return;
  const u32 a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
  const u32 u[6] = {a, b, b, c, c, a}, v[6] = {b, a, c, b, a, c};
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    eu[6 * t + k] = u[k];
    ev[6 * t + k] = v[k];
  }
}
// sorted by (u, v): the first of each run of equal edges is a neighbour, unless it is a self-loop
__global__ void __launch_bounds__(256) k_edge_flags(const u32* __restrict__ perm, const u32* __restrict__ eu, const u32* __restrict__ ev, u32 ne,
                                                    u32* __restrict__ flag) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= ne) return;
  const u32 e = perm[i], u = eu[e], v = ev[e];
  bool first = true;
  if (i > 0) {
    const u32 q = perm[i - 1];
    first = eu[q] != u || ev[q] != v;
  }
  flag[i] = (first && u != v) ? 1u : 0u;
}
// fpos = exclusive scan of flag: neighbours before sorted position i = the CSR position.  row_begin / row_end are zero for a
// vertex without an edge.
__global__ void __launch_bounds__(256) k_csr_fill(const u32* __restrict__ perm, const u32* __restrict__ eu, const u32* __restrict__ ev,
                                                  const u32* __restrict__ flag, const u32* __restrict__ fpos, u32 ne, u32* __restrict__ row_begin,
                                                  u32* __restrict__ row_end, u32* __restrict__ col) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= ne) return;
  const u32 e = perm[i], u = eu[e], f = flag[i], at = fpos[i];
  if (f) col[at] = ev[e];
  if (i == 0 || eu[perm[i - 1]] != u) row_begin[u] = at;
  if (i + 1 == ne || eu[perm[i + 1]] != u) row_end[u] = at + f;
}
// p' = p + f * (s / float(|N|) - p), s = the neighbours' positions summed in ascending neighbour index from the first one on
__global__ void __launch_bounds__(256) k_taubin_half(const float* __restrict__ in, float* __restrict__ out, const u32* __restrict__ row_begin,
                                                     const u32* __restrict__ row_end, const u32* __restrict__ col, u32 nv, float f) {
  const u64 gi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gi >= nv) return;
  const u32 i = static_cast<u32>(gi);
  const F3 p = load3(in, i);
  const u32 b = row_begin[i], e = row_end[i];
  if (e <= b) {
    store3(out, i, p);
    return;
  }
  F3 s = load3(in, col[b]);
  for (u32 k = b + 1; k < e; ++k) s = s + load3(in, col[k]);
  const float n = static_cast<float>(e - b);
  store3(out, i, F3{p.x + f * (s.x / n - p.x), p.y + f * (s.y / n - p.y), p.z + f * (s.z / n - p.z)});
}

// ---- vertex normals ----------------------------------------------------------------------------------------------------------
// perm = the corners 0 .. 3 nt - 1 sorted (stably) by their vertex: row v = the corners of vertex v, triangles ascending
__global__ void __launch_bounds__(256) k_rows(const u32* __restrict__ perm, const u32* __restrict__ key, u32 n, u32* __restrict__ row_begin,
                                              u32* __restrict__ row_end) {
  const u64 gi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gi >= n) return;
  const u32 i = static_cast<u32>(gi), v = key[perm[i]];
  if (i == 0 || key[perm[i - 1]] != v) row_begin[v] = i;
  if (i + 1 == n || key[perm[i + 1]] != v) row_end[v] = i + 1;
}
__global__ void __launch_bounds__(256) k_vertex_normals(const float* __restrict__ pos, const u32* __restrict__ tri, const u32* __restrict__ perm,
                                                        const u32* __restrict__ row_begin, const u32* __restrict__ row_end, u32 nv, float* __restrict__ nrm) {
  const u64 gi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gi >= nv) return;
  const u32 i = static_cast<u32>(gi);
  F3 n{0.0f, 0.0f, 0.0f};
  for (u32 k = row_begin[i]; k < row_end[i]; ++k) {
    const u64 t = perm[k] / 3u;
    const F3 p0 = load3(pos, tri[3 * t]), p1 = load3(pos, tri[3 * t + 1]), p2 = load3(pos, tri[3 * t + 2]);
    n = n + cross3(p1 - p0, p2 - p0);  // unnormalised: area-weighted
  }
  store3(nrm, i, normalized3(n));
}

// ---- vertex clustering -------------------------------------------------------------------------------------------------------
// order-preserving bit pattern of a float: a < b  <=>  ordered(a) < ordered(b)
__host__ __device__ __forceinline__ u32 float_ordered(u32 bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
__host__ __device__ __forceinline__ u32 ordered_float(u32 o) { return (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o; }
// lohi[0..2] min, [3..5] max per axis as ordered patterns (initialised to all ones / zero); reduced per workgroup as k_weld_bounds does
__global__ void __launch_bounds__(256) k_bounds_f32(const float* __restrict__ pos, u32 nv, u32* __restrict__ lohi) {
  __shared__ u32 red[4][6];
  u32 lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u};
  for (u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x; v < nv; v += static_cast<u64>(gridDim.x) * blockDim.x) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const u32 o = float_ordered(__float_as_uint(pos[3 * v + k]));
      lo[k] = o < lo[k] ? o : lo[k];
      hi[k] = o > hi[k] ? o : hi[k];
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const u32 a = __shfl_xor(lo[k], off, 64), b = __shfl_xor(hi[k], off, 64);
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
    u32 r = red[0][threadIdx.x];
    for (int w = 1; w < 4; ++w) {
      const u32 q = red[w][threadIdx.x];
      r = (threadIdx.x < 3) ? (q < r ? q : r) : (q > r ? q : r);
    }
    if (threadIdx.x < 3)
      atomicMin(&lohi[threadIdx.x], r);
    else
      atomicMax(&lohi[threadIdx.x], r);
  }
}
struct CellGrid {
  float origin[3];
  float cell;
};
__host__ __device__ __forceinline__ float cell_coord(float p, float origin, float cell) { return floorf((p - origin) / cell); }
__global__ void __launch_bounds__(256) k_cells(const float* __restrict__ pos, u32 nv, CellGrid G, u32* __restrict__ cx, u32* __restrict__ cy,
                                               u32* __restrict__ cz) {
  const u64 v = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  cx[v] = static_cast<u32>(static_cast<int>(cell_coord(pos[3 * v], G.origin[0], G.cell)));
  cy[v] = static_cast<u32>(static_cast<int>(cell_coord(pos[3 * v + 1], G.origin[1], G.cell)));
  cz[v] = static_cast<u32>(static_cast<int>(cell_coord(pos[3 * v + 2], G.origin[2], G.cell)));
}
__global__ void __launch_bounds__(256) k_cell_flags(const u32* __restrict__ perm, const u32* __restrict__ cx, const u32* __restrict__ cy,
                                                    const u32* __restrict__ cz, u32 nv, u32* __restrict__ flag) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  bool first = true;
  if (i > 0) {
    const u32 v = perm[i], q = perm[i - 1];
    first = cx[q] != cx[v] || cy[q] != cy[v] || cz[q] != cz[v];
  }
  flag[i] = first ? 1u : 0u;
}
// cell id of every vertex and the range [start[c], start[c + 1]) of cell c in the sorted permutation
__global__ void __launch_bounds__(256) k_cell_ids(const u32* __restrict__ perm, const u32* __restrict__ flag, const u32* __restrict__ fpos, u32 nv,
                                                  u32* __restrict__ cid, u32* __restrict__ start) {
  const u64 gi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gi >= nv) return;
  const u32 i = static_cast<u32>(gi), c = fpos[i] + flag[i] - 1u;
  cid[perm[i]] = c;
  if (flag[i]) start[c] = i;
  if (i + 1 == nv) start[c + 1] = nv;
}
// one thread per cell, its members in ascending input index
__global__ void __launch_bounds__(256) k_cluster_avg(const float* __restrict__ pos, const float* __restrict__ nrm, const uint8_t* __restrict__ rgb,
                                                     const u32* __restrict__ perm, const u32* __restrict__ start, u32 nc, float* __restrict__ opos,
                                                     float* __restrict__ onrm, uint8_t* __restrict__ orgb) {
  const u64 gi = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (gi >= nc) return;
  const u32 c = static_cast<u32>(gi), b = start[c], e = start[c + 1];
  const u32 v0 = perm[b];
  F3 p = load3(pos, v0), n = load3(nrm, v0);
  u64 col[3] = {rgb[3ull * v0], rgb[3ull * v0 + 1], rgb[3ull * v0 + 2]};
  for (u32 k = b + 1; k < e; ++k) {
    const u32 v = perm[k];
    p = p + load3(pos, v);
    n = n + load3(nrm, v);
#pragma unroll
    for (int a = 0; a < 3; ++a) col[a] += rgb[3ull * v + a];
  }
  const u64 cnt = e - b;
  const float fc = static_cast<float>(e - b);
  store3(opos, c, F3{p.x / fc, p.y / fc, p.z / fc});
  store3(onrm, c, normalized3(n));
#pragma unroll
  for (int a = 0; a < 3; ++a) orgb[3ull * c + a] = static_cast<uint8_t>((2 * col[a] + cnt) / (2 * cnt));  // rounded mean, exact
}
__global__ void __launch_bounds__(256) k_reindex(u32* __restrict__ tri, u64 n, const u32* __restrict__ cid) {
  const u64 i = static_cast<u64>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i < n) tri[i] = cid[tri[i]];
}

}  // namespace

extern "C" {

int cox_meshconn_from_arrays(int device, const float* xyz, const float* normals, const uint8_t* rgb, const uint32_t* triangles, uint64_t n_vertices,
                             uint64_t n_triangles, cox_meshconn_t** out) {
  COX_ENTRY();
  if (!out || (n_vertices && !xyz) || (n_triangles && !triangles) || device < 0) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  if (n_vertices > 0x7FFFFFF0ull || n_triangles > 0x55555550ull) return COX_ERR_UNSUPPORTED;  // 3 nt corners are indexed with 32 bits
  for (u64 i = 0; i < 3 * n_triangles; ++i)
    if (triangles[i] >= n_vertices) return COX_ERR_INDEX_RANGE;
  COX_HIP(hipSetDevice(device));
  DevBuf<float> pos, nrm;
  DevBuf<uint8_t> col;
  DevBuf<u32> tri;
  if (n_vertices) {
    COX_TRY(pos.alloc(3 * n_vertices));
    COX_TRY(nrm.alloc(3 * n_vertices));
    COX_TRY(col.alloc(3 * n_vertices));
    COX_HIP(hipMemcpy(pos.p, xyz, sizeof(float) * 3 * n_vertices, hipMemcpyHostToDevice));
    if (normals)
      COX_HIP(hipMemcpy(nrm.p, normals, sizeof(float) * 3 * n_vertices, hipMemcpyHostToDevice));
    else
      COX_HIP(hipMemset(nrm.p, 0, sizeof(float) * 3 * n_vertices));
    if (rgb)
      COX_HIP(hipMemcpy(col.p, rgb, 3 * n_vertices, hipMemcpyHostToDevice));
    else
      COX_HIP(hipMemset(col.p, 0, 3 * n_vertices));
  }
  if (n_triangles) {
    COX_TRY(tri.alloc(3 * n_triangles));
    COX_HIP(hipMemcpy(tri.p, triangles, sizeof(u32) * 3 * n_triangles, hipMemcpyHostToDevice));
  }
  COX_TRY(finish());
  cox_meshconn* C = new (std::nothrow) cox_meshconn();
  if (!C) return COX_ERR_OUT_OF_MEMORY;
  C->device = device;
  C->n_vertices = n_vertices;
  C->n_triangles = n_triangles;
  C->pos = pos.release();
  C->nrm = nrm.release();
  C->rgb = col.release();
  C->tri = tri.release();
  *out = C;
  return COX_OK;
}

int cox_meshconn_clean(cox_meshconn_t* C, uint64_t removed[3]) {
  COX_ENTRY();
  if (!C) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  COX_HIP(hipSetDevice(C->device));
  return clean_impl(C, removed);
}

int cox_meshconn_smooth_taubin(cox_meshconn_t* C, int iterations, float lambda, float mu, double* kernel_ms) {
  COX_ENTRY();
  if (!C || iterations < 0 || !std::isfinite(lambda) || !std::isfinite(mu)) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  if (kernel_ms) *kernel_ms = 0.0;
  const u32 nv = static_cast<u32>(C->n_vertices);
  if (iterations == 0 || nv == 0 || C->n_triangles == 0) return COX_OK;  // no edge: every vertex keeps its position
  if (6 * C->n_triangles > 0xFFFFFFF0ull) return COX_ERR_UNSUPPORTED;
  COX_HIP(hipSetDevice(C->device));
  const u32 nt = static_cast<u32>(C->n_triangles), ne = 6 * nt;
  DevBuf<u32> eu, ev, flag, fpos, col, row_begin, row_end;
  DevBuf<float> other;
  PermSort sort;
  Scan scan;
  COX_TRY(eu.alloc(ne));
  COX_TRY(ev.alloc(ne));
  COX_TRY(flag.alloc(ne));
  COX_TRY(fpos.alloc(ne));
  COX_TRY(col.alloc(ne));
  COX_TRY(row_begin.alloc(nv));
  COX_TRY(row_end.alloc(nv));
  COX_TRY(other.alloc(3ull * nv));
  COX_TRY(scan.init(ne));
  COX_TRY(sort.init(ne));
  COX_HIP(hipMemsetAsync(row_begin.p, 0, sizeof(u32) * nv, nullptr));
  COX_HIP(hipMemsetAsync(row_end.p, 0, sizeof(u32) * nv, nullptr));
  COX_LAUNCH(k_emit_edges, nt, C->tri, nt, eu.p, ev.p);
  const int bits = ceil_log2(nv);
  sort.by(ev.p, bits);
  sort.by(eu.p, bits);
  COX_LAUNCH(k_edge_flags, ne, sort.perm(), eu.p, ev.p, ne, flag.p);
  scan.run(flag.p, fpos.p, ne, nullptr);
  COX_LAUNCH(k_csr_fill, ne, sort.perm(), eu.p, ev.p, flag.p, fpos.p, ne, row_begin.p, row_end.p, col.p);
  EventPair timed;
  if (timed.create() != COX_OK) return COX_ERR_NO_DEVICE;
  // 2 * iterations launches back to back: lambda into the second buffer, mu back into the mesh's own
  (void)timed.begin(nullptr);
  for (int it = 0; it < iterations; ++it) {
    COX_LAUNCH(k_taubin_half, nv, C->pos, other.p, row_begin.p, row_end.p, col.p, nv, lambda);
    COX_LAUNCH(k_taubin_half, nv, other.p, C->pos, row_begin.p, row_end.p, col.p, nv, mu);
  }
  (void)timed.end(nullptr);
  const int st = finish();
  if (st == COX_OK && kernel_ms) (void)timed.elapsed_ms(kernel_ms);
  return st;
}

int cox_meshconn_compute_normals(cox_meshconn_t* C) {
  COX_ENTRY();
  if (!C) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  const u32 nv = static_cast<u32>(C->n_vertices), nt = static_cast<u32>(C->n_triangles);
  if (nv == 0) return COX_OK;
  COX_HIP(hipSetDevice(C->device));
  if (nt == 0) {
    COX_HIP(hipMemsetAsync(C->nrm, 0, sizeof(float) * 3 * nv, nullptr));
    return finish();
  }
  const u32 nc = 3 * nt;
  DevBuf<u32> row_begin, row_end;
  PermSort sort;
  COX_TRY(row_begin.alloc(nv));
  COX_TRY(row_end.alloc(nv));
  COX_TRY(sort.init(nc));
  COX_HIP(hipMemsetAsync(row_begin.p, 0, sizeof(u32) * nv, nullptr));
  COX_HIP(hipMemsetAsync(row_end.p, 0, sizeof(u32) * nv, nullptr));
  sort.by(C->tri, ceil_log2(nv));  // corner i = 3 t + k names vertex tri[i]: emitted in triangle order, the sort is stable
  COX_LAUNCH(k_rows, nc, sort.perm(), C->tri, nc, row_begin.p, row_end.p);
  COX_LAUNCH(k_vertex_normals, nv, C->pos, C->tri, sort.perm(), row_begin.p, row_end.p, nv, C->nrm);
  return finish();
}

int cox_meshconn_simplify_clustering(cox_meshconn_t* C, float cell_size, uint64_t* n_vertices, uint64_t* n_triangles) {
  COX_ENTRY();
  if (!C || !std::isfinite(cell_size) || !(cell_size > 0.0f)) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  COX_HIP(hipSetDevice(C->device));
  const u32 nv = static_cast<u32>(C->n_vertices);
  if (nv) {
    // 1. bounds -> origin, cells per axis (the cell of the largest coordinate: the cell expression is monotone)
    DevBuf<u32> lohi;
    COX_TRY(lohi.alloc(6));
    const u32 init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
    COX_HIP(hipMemcpy(lohi.p, init, sizeof(init), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bounds_f32, dim3(std::min<u32>(grid_for(nv).x, 1024u)), dim3(256), 0, nullptr, C->pos, nv, lohi.p);
    u32 hl[6];
    COX_HIP(hipMemcpy(hl, lohi.p, sizeof(hl), hipMemcpyDeviceToHost));
    CellGrid G;
    G.cell = cell_size;
    int bits[3];
    for (int k = 0; k < 3; ++k) {
      const u32 lo_bits = ordered_float(hl[k]), hi_bits = ordered_float(hl[3 + k]);
      float lo, hi;
      std::memcpy(&lo, &lo_bits, sizeof(float));
      std::memcpy(&hi, &hi_bits, sizeof(float));
      G.origin[k] = lo - 0.5f * cell_size;
      const float top = cell_coord(hi, G.origin[k], cell_size);
      if (!(top >= 0.0f && top < 2097152.0f)) return COX_ERR_INDEX_RANGE;  // 2^21 cells or more on an axis (or no finite bound)
      bits[k] = ceil_log2(static_cast<u64>(top) + 1);
    }
    // 2. vertex indices sorted by (z, y, x) cell; one output vertex per run
    DevBuf<u32> cx, cy, cz, flag, fpos, cid, start, total;
    PermSort sort;
    Scan scan;
    COX_TRY(cx.alloc(nv));
    COX_TRY(cy.alloc(nv));
    COX_TRY(cz.alloc(nv));
    COX_TRY(flag.alloc(nv));
    COX_TRY(fpos.alloc(nv));
    COX_TRY(cid.alloc(nv));
    COX_TRY(start.alloc(static_cast<size_t>(nv) + 1));
    COX_TRY(total.alloc(1));
    COX_TRY(scan.init(nv));
    COX_TRY(sort.init(nv));
    COX_LAUNCH(k_cells, nv, C->pos, nv, G, cx.p, cy.p, cz.p);
    sort.by(cx.p, bits[0]);
    sort.by(cy.p, bits[1]);
    sort.by(cz.p, bits[2]);
    COX_LAUNCH(k_cell_flags, nv, sort.perm(), cx.p, cy.p, cz.p, nv, flag.p);
    scan.run(flag.p, fpos.p, nv, total.p);
    COX_LAUNCH(k_cell_ids, nv, sort.perm(), flag.p, fpos.p, nv, cid.p, start.p);
    u32 nc = 0;
    COX_HIP(hipMemcpy(&nc, total.p, sizeof(u32), hipMemcpyDeviceToHost));  // the size of the result
    // 3. averages, triangles re-indexed
    DevBuf<float> opos, onrm;
    DevBuf<uint8_t> orgb;
    COX_TRY(opos.alloc(3ull * nc));
    COX_TRY(onrm.alloc(3ull * nc));
    COX_TRY(orgb.alloc(3ull * nc));
    COX_LAUNCH(k_cluster_avg, nc, C->pos, C->nrm, C->rgb, sort.perm(), start.p, nc, opos.p, onrm.p, orgb.p);
    if (C->n_triangles) COX_LAUNCH(k_reindex, 3 * C->n_triangles, C->tri, 3 * C->n_triangles, cid.p);
    COX_TRY(finish());
    C->set_vertices(opos.release(), onrm.release(), orgb.release());
    C->n_vertices = nc;
  }
  // 4. no degenerate or duplicate triangle, no unreferenced vertex
  COX_TRY(clean_impl(C, nullptr));
  if (n_vertices) *n_vertices = C->n_vertices;
  if (n_triangles) *n_triangles = C->n_triangles;
  return COX_OK;
}

}  // extern "C"
