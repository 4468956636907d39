// Reading a TSDF / ESDF layer on the GPU: the one owner of the voxel address, the 2x2x2 cell of voxblox
// Interpolator<TsdfVoxel>::getVoxelsAndQVector, the 8x8 interpolation table, the trilinear value and its analytic gradient, the
// nearest voxel, and the per-lane cache of the blocks around a sample.  The arithmetic is oracle/cox_oracle.hpp's
// getVoxelsAndQVector + interpMember, expression by expression, so every caller reproduces the checker bit for bit.
//
//   voxel_ptr, locate, block_window      addresses and indices
//   cell_corner, cell_offset, interp_cell  the cell: lower corner, offset in it, then the 16 words
//   interp_table_apply, interp_q, interp_dot, interp_member, interp_value_gradient
//   point_cell                           a point's cell through the hash table (registration, alignment, tracking)
//   HtPool, BlockSet, BlockCache, SetFind  block finders (x, y, z): the hash table, and a 2x2x2 set of pool indices per lane
//   tri_sample, nearest_sample           point samples on any block finder (queries, collision, render, isosurface)
//
// Callers: cox_reg.hpp / cox_reg.hip / cox_align.hip (point_cell), cox_track.hip (point_cell, interp_value_gradient),
// cox_query.hip / cox_collide.hip / cox_render.hip (BlockSet, its finders + samples), cox_submap.hip (tri_sample on HtPool),
// cox_layer.hip (cell_corner + its own gather with colour), cox_viewgain.hip (locate, voxel_ptr).
#pragma once
#include "cox_device.hpp"
#include "cox_internal.hpp"

namespace cox {

// the read-only part of a layer a gather kernel needs (not the read-write ::LayerView of cox_frame.hpp, which the integrator and the history use)
struct LayerView {
  const u32* voxels;
  const u64* ht_keys;
  const u32* ht_vals;
  u32 ht_mask;
  float voxel_size, voxel_size_inv, block_size, block_size_inv;
};
// read on every call: a layer that grew has new buffers
inline LayerView layer_view(const cox_layer* L) {
  return LayerView{L->voxels, L->ht_keys, L->ht_vals, L->ht_cap - 1, L->voxel_size, L->voxel_size_inv, L->block_size, L->block_size_inv};
}

// pos in blocks; false when a coordinate is NaN, +-inf or beyond the packed keys
__device__ __forceinline__ bool block_scaled(const LayerView& L, const float pos[3], float sc[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) sc[k] = pos[k] * L.block_size_inv;
  return index_in_range(sc[0]) && index_in_range(sc[1]) && index_in_range(sc[2]);
}
// the same for a caller that has no use for sc (each coordinate is scaled where it is tested)
__device__ __forceinline__ bool point_in_range(const LayerView& L, const float p[3]) {
  return index_in_range(p[0] * L.block_size_inv) && index_in_range(p[1] * L.block_size_inv) && index_in_range(p[2] * L.block_size_inv);
}

// the three words of voxel (vx, vy, vz) of pool block `pool`
__device__ __forceinline__ const u32* voxel_ptr(const LayerView& L, u32 pool, int vx, int vy, int vz) {
  return L.voxels + (static_cast<size_t>(pool) * kVoxelsPerBlock + static_cast<u32>(vx + 16 * (vy + 16 * vz))) * kWordsPerVoxel;
}

// block and voxel of one coordinate: Block::getVoxelByCoordinates' containing voxel, the grid index clamped into the block
__device__ __forceinline__ void locate(const LayerView& L, float p, int* b, int* v) {
  const int bb = grid_index(p * L.block_size_inv);
  const int vv = grid_index((p - static_cast<float>(bb) * L.block_size) * L.voxel_size_inv);
  *b = bb;
  *v = vv > 15 ? 15 : (vv < 0 ? 0 : vv);
}

// block of p, and the corner / span (0 or 1 per axis) of the block set that holds the voxels g - r .. g + r around the voxel g
// containing p
__device__ __forceinline__ void block_window(const LayerView& L, const float p[3], int r, int b[3], int lo[3], int span[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    int v;
    locate(L, p[k], &b[k], &v);
    const int g = b[k] * 16 + v;
    lo[k] = (g - r) >> 4;
    span[k] = ((g + r) >> 4) - lo[k];
  }
}

static __constant__ float c_interp_table[8][8] = {{1, 0, 0, 0, 0, 0, 0, 0},   {-1, 0, 0, 0, 1, 0, 0, 0},   {-1, 0, 1, 0, 0, 0, 0, 0},
                                                  {-1, 1, 0, 0, 0, 0, 0, 0},  {1, 0, -1, 0, -1, 0, 1, 0},  {1, -1, -1, 1, 0, 0, 0, 0},
                                                  {1, -1, 0, 0, -1, 1, 0, 0}, {-1, 1, 1, -1, 1, -1, -1, 1}};

// pool index of a block (kInvalid: no key, or a key left without storage).  A block finder is a callable (x, y, z): this one
// asks the hash table, BlockCache and SetFind below answer from a resolved set where they can.
struct HtPool {
  const LayerView& L;
  __device__ __forceinline__ u32 operator()(int x, int y, int z) const {
    const u32 slot = ht_find(L.ht_keys, L.ht_mask, pack_key(x, y, z));
    return slot == kInvalid ? kInvalid : L.ht_vals[slot];
  }
};

// The lower corner of the 2x2x2 cell around pos, by comparison with the centre of the containing voxel, stepping across the
// block face where that voxel is the first of its block.  b[]: in the block of pos (grid_index(pos / block_size)), out the
// block of the corner; vi[]: the corner voxel in it.
__device__ __forceinline__ void cell_corner(const LayerView& L, const float pos[3], int b[3], int vi[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float origin = static_cast<float>(b[k]) * L.block_size;
    const float rel = pos[k] - origin;
    int v = grid_index(rel * L.voxel_size_inv);
    v = v > 15 ? 15 : (v < 0 ? 0 : v);
    const float c = origin + center_coord(v, L.voxel_size);
    if (pos[k] - c < 0.0f) {
      v--;
      if (v < 0) {
        b[k]--;
        v += 16;
      }
    }
    vi[k] = v;
  }
}
// off[]: (pos - centre of that corner) / voxel_size.  A function of its own so that a caller can take it after it has looked
// the corner's block up: three floats held across the hash probes cost the collision kernels a wave of occupancy.
__device__ __forceinline__ void cell_offset(const LayerView& L, const float pos[3], const int b[3], const int vi[3], float off[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float c0 = static_cast<float>(b[k]) * L.block_size + center_coord(vi[k], L.voxel_size);
    off[k] = (pos[k] - c0) * L.voxel_size_inv;
  }
}

// The 2x2x2 cell around pos: distances d[8] and weights w[8] in the column order (0,0,0),(0,0,1),(0,1,0),...,(1,1,1) and the
// offset (pos - centre of corner 0) / voxel_size.  b[] is the block of pos (grid_index(pos / block_size)), whose existence the
// caller has checked.  False when a block of the cell is missing or a corner voxel is invalid (weight <= 0).  find(x, y, z)
// returns a pool index or kInvalid.  The (up to 7) other blocks are resolved first, then all 16 voxel loads are issued
// independently of each other (the early-outs of a straight transcription serialise them).
template <class Find>
__device__ __forceinline__ bool interp_cell(const LayerView& L, const float pos[3], const int b_in[3], const Find& find, float d[8], float w[8],
                                            float off[3]) {
  int b[3] = {b_in[0], b_in[1], b_in[2]}, vi[3];
  cell_corner(L, pos, b, vi);
  const u32 base_pool = find(b[0], b[1], b[2]);
  if (base_pool == kInvalid) return false;
  cell_offset(L, pos, b, vi, off);
  u32 pools[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int mx = (c >> 2) & 1, my = (c >> 1) & 1, mz = c & 1;
    const bool need = (!mx || vi[0] == 15) && (!my || vi[1] == 15) && (!mz || vi[2] == 15);  // this block combination is touched
    u32 pool = base_pool;
    if (c != 0) {
      pool = kInvalid;
      if (need) pool = find(b[0] + mx, b[1] + my, b[2] + mz);
    }
    pools[c] = pool;
  }
  bool all_blocks = true;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    int v[3] = {vi[0] + ((i >> 2) & 1), vi[1] + ((i >> 1) & 1), vi[2] + (i & 1)};
    int sel = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (v[k] >= 16) {
        v[k] -= 16;
        sel |= 4 >> k;
      }
    const u32 pool = pools[sel];
    all_blocks = all_blocks && pool != kInvalid;
    const u32* vox = voxel_ptr(L, pool == kInvalid ? base_pool : pool, v[0], v[1], v[2]);
    d[i] = __uint_as_float(vox[0]);
    w[i] = __uint_as_float(vox[1]);
  }
  if (!all_blocks) return false;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (!(w[i] > 0.0f)) return false;  // Interpolator<TsdfVoxel>::isVoxelValid
  return true;
}

// M . data: the interpolation table applied to the 8 corner values, sequential float sums
__device__ __forceinline__ void interp_table_apply(const float data[8], float md[8]) {
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < 8; ++c) s += c_interp_table[r][c] * data[c];
    md[r] = s;
  }
}
// the q vector of a cell offset: (1, dx, dy, dz, dx dy, dy dz, dz dx, dx dy dz)
__device__ __forceinline__ void interp_q(const float off[3], float q[8]) {
  const float dx = off[0], dy = off[1], dz = off[2];
  q[0] = 1.0f, q[1] = dx, q[2] = dy, q[3] = dz;
  q[4] = dx * dy, q[5] = dy * dz, q[6] = dz * dx, q[7] = dx * dy * dz;
}
// q . md, a sequential float sum: the interpolated value of a cell whose table product is md
__device__ __forceinline__ float interp_dot(const float q[8], const float md[8]) {
  float v = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) v += q[i] * md[i];
  return v;
}
// Interpolator::interpMember: q . (M . data)
__device__ __forceinline__ float interp_member(const float off[3], const float data[8]) {
  float md[8], q[8];
  interp_table_apply(data, md);
  interp_q(off, q);
  return interp_dot(q, md);
}
// The trilinear value q . md and its analytic gradient (dq/dx . md, dq/dy . md, dq/dz . md) * voxel_size_inv: the residual
// and Jacobian rows of the registration cost and of the scan-to-map tracker.
__device__ __forceinline__ void interp_value_gradient(const float md[8], const float off[3], float voxel_size_inv, float* val, float g[3]) {
  const float dx = off[0], dy = off[1], dz = off[2];
  const float qx[8] = {0, 1, 0, 0, dy, 0, dz, dy * dz};
  const float qy[8] = {0, 0, 1, 0, dx, dz, 0, dz * dx};
  const float qz[8] = {0, 0, 0, 1, 0, dy, dx, dx * dy};
  float q[8];
  interp_q(off, q);
  *val = interp_dot(q, md);
  float gxf = 0.0f, gyf = 0.0f, gzf = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    gxf += qx[i] * md[i];
    gyf += qy[i] * md[i];
    gzf += qz[i] * md[i];
  }
  g[0] = gxf * voxel_size_inv;
  g[1] = gyf * voxel_size_inv;
  g[2] = gzf * voxel_size_inv;
}

// The 2x2x2 cell around pos through the hash table: md = table . corner distances and the offset off inside the cell.  False
// when pos is not finite or beyond the packed keys, the block of pos or one of the cell is missing, or a corner has weight <= 0.
__device__ __forceinline__ bool point_cell(const LayerView& L, const float pos[3], float md[8], float off[3]) {
  float sc[3];
  if (!block_scaled(L, pos, sc)) return false;
  int b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = grid_index(sc[k]);
  if (ht_find(L.ht_keys, L.ht_mask, pack_key(b[0], b[1], b[2])) == kInvalid) return false;  // block of the point must exist
  float d[8], wv[8];
  if (!interp_cell(L, pos, b, HtPool{L}, d, wv, off)) return false;
  interp_table_apply(d, md);
  return true;
}

// ---- point samples on a layer -------------------------------------------------------------------------------------------------
// Pool indices of the up to 2 x 2 x 2 blocks from lo on, resolved once; anything else is looked up in the hash table, so the
// set never changes an answer.  A query fills it once (block_cache_fill); a ray keeps it from sample to sample (move / own /
// fill).  Twelve words, and no pointer in it: the compiler keeps one per lane in LDS.
struct BlockSet {
  int lo[3];
  u32 pool[8];  // (x - lo.x) << 2 | (y - lo.y) << 1 | (z - lo.z); kInvalid when missing
  u32 have;     // bit c: pool[c] was resolved
  __device__ __forceinline__ u32 find(const LayerView& L, int x, int y, int z) const {
    const u32 dx = static_cast<u32>(x - lo[0]), dy = static_cast<u32>(y - lo[1]), dz = static_cast<u32>(z - lo[2]);
    if (dx <= 1u && dy <= 1u && dz <= 1u) {
      const u32 sel = (dx << 2) | (dy << 1) | dz;
      if ((have >> sel) & 1u) {
        u32 r = pool[0];
#pragma unroll
        for (u32 c = 1; c < 8; ++c) r = sel == c ? pool[c] : r;  // no dynamic register indexing (it would go to scratch)
        return r;
      }
    }
    return HtPool{L}(x, y, z);
  }
  // a new corner forgets the set
  __device__ __forceinline__ void move(const int nlo[3]) {
    if (nlo[0] != lo[0] || nlo[1] != lo[1] || nlo[2] != lo[2]) {
      lo[0] = nlo[0], lo[1] = nlo[1], lo[2] = nlo[2];
      have = 0u;
    }
  }
  // one block of the set (x - lo in 0..1 on every axis): looked up at most once
  __device__ __forceinline__ u32 own(const LayerView& L, int x, int y, int z) {
    const u32 sel = (static_cast<u32>(x - lo[0]) << 2) | (static_cast<u32>(y - lo[1]) << 1) | static_cast<u32>(z - lo[2]);
    if (!((have >> sel) & 1u)) {
      const u32 p = HtPool{L}(x, y, z);
#pragma unroll
      for (u32 c = 0; c < 8; ++c) pool[c] = sel == c ? p : pool[c];
      have |= 1u << sel;
    }
    return find(L, x, y, z);
  }
  // the blocks of the set within span (0 or 1 per axis) that are not resolved yet
  __device__ __forceinline__ void fill(const LayerView& L, const int span[3]) {
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int mx = (c >> 2) & 1, my = (c >> 1) & 1, mz = c & 1;
      if (mx <= span[0] && my <= span[1] && mz <= span[2] && !((have >> c) & 1u)) {
        pool[c] = HtPool{L}(lo[0] + mx, lo[1] + my, lo[2] + mz);
        have |= 1u << c;
      }
    }
  }
};
constexpr BlockSet kNoBlocks{{0, 0, 0}, {kInvalid, kInvalid, kInvalid, kInvalid, kInvalid, kInvalid, kInvalid, kInvalid}, 0u};

// The block finders on a BlockSet.  BlockCache owns its set (a query, a collision sample: filled once); SetFind looks into a
// set that its caller keeps and moves (the renderer's ray).
struct BlockCache {
  const LayerView& L;
  BlockSet s;
  __device__ __forceinline__ u32 operator()(int x, int y, int z) const { return s.find(L, x, y, z); }
};
struct SetFind {
  const LayerView& L;
  const BlockSet& s;
  __device__ __forceinline__ u32 operator()(int x, int y, int z) const { return s.find(L, x, y, z); }
};

// Resolves into a fresh bc the blocks of voxels g - R .. g + R around the voxel g that contains p (in index range): only the
// blocks that range touches, so one lookup for a point deep inside a block.  b[] gets the block of p.
template <int R>
__device__ __forceinline__ void block_cache_fill(const LayerView& L, const float p[3], BlockCache& bc, int b[3]) {
  int span[3];
  block_window(L, p, R, b, bc.s.lo, span);
  bc.s.fill(L, span);
}

// Interpolator::getInterpDistance (and getInterpWeight when want_w) at s: false when the cell is incomplete or invalid
template <class Find>
__device__ __forceinline__ bool tri_sample(const LayerView& L, const Find& find, const float s[3], float* d, float* w, bool want_w) {
  int b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = grid_index(s[k] * L.block_size_inv);
  if (find(b[0], b[1], b[2]) == kInvalid) return false;  // getBlockPtrByCoordinates(pos)
  float dd[8], ww[8], off[3];
  if (!interp_cell(L, s, b, find, dd, ww, off)) return false;
  *d = interp_member(off, dd);
  if (want_w) *w = interp_member(off, ww);
  return true;
}

// Block::getVoxelByCoordinates: the voxel of the containing block (grid index clamped into it), nullptr without the block
template <class Find>
__device__ __forceinline__ const u32* containing_voxel(const LayerView& L, const Find& find, const float s[3]) {
  int b[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) locate(L, s[k], &b[k], &v[k]);
  const u32 pool = find(b[0], b[1], b[2]);
  if (pool == kInvalid) return nullptr;
  return voxel_ptr(L, pool, v[0], v[1], v[2]);
}
// its distance and weight; valid when weight > 0
template <class Find>
__device__ __forceinline__ bool nearest_sample(const LayerView& L, const Find& find, const float s[3], float* d, float* w) {
  const u32* vox = containing_voxel(L, find, s);
  if (vox == nullptr) return false;
  *d = __uint_as_float(vox[0]);
  *w = __uint_as_float(vox[1]);
  return *w > 0.0f;
}

}  // namespace cox
