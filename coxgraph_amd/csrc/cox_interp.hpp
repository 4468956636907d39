// voxblox Interpolator<TsdfVoxel>::getVoxelsAndQVector on the GPU, shared by the registration cost (cox_reg.hip), the map
// queries (cox_query.hip) and the collision checks (cox_collide.hip).  The arithmetic is oracle/cox_oracle.hpp's getVoxelsAndQVector + interpMember, expression by
// expression, so both kernels reproduce the checker bit for bit.
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

static __constant__ float c_interp_table[8][8] = {{1, 0, 0, 0, 0, 0, 0, 0},   {-1, 0, 0, 0, 1, 0, 0, 0},   {-1, 0, 1, 0, 0, 0, 0, 0},
                                                  {-1, 1, 0, 0, 0, 0, 0, 0},  {1, 0, -1, 0, -1, 0, 1, 0},  {1, -1, -1, 1, 0, 0, 0, 0},
                                                  {1, -1, 0, 0, -1, 1, 0, 0}, {-1, 1, 1, -1, 1, -1, -1, 1}};

// pool index of a block (kInvalid: no key, or a key left without storage)
struct HtPool {
  const LayerView& L;
  __device__ __forceinline__ u32 operator()(int x, int y, int z) const {
    const u32 slot = ht_find(L.ht_keys, L.ht_mask, pack_key(x, y, z));
    return slot == kInvalid ? kInvalid : L.ht_vals[slot];
  }
};

// The 2x2x2 cell around pos: distances d[8] and weights w[8] in the column order (0,0,0),(0,0,1),(0,1,0),...,(1,1,1) and the
// offset (pos - centre of corner 0) / voxel_size.  b[] is the block of pos (grid_index(pos / block_size)), whose existence the
// caller has checked.  False when a block of the cell is missing or a corner voxel is invalid (weight <= 0).  find(x, y, z)
// returns a pool index or kInvalid.  The (up to 7) other blocks are resolved first, then all 16 voxel loads are issued
// independently of each other (the early-outs of a straight transcription serialise them).
template <class Find>
__device__ __forceinline__ bool interp_cell(const LayerView& L, const float pos[3], const int b_in[3], const Find& find, float d[8], float w[8],
                                            float off[3]) {
  int b[3] = {b_in[0], b_in[1], b_in[2]}, vi[3];
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
  const u32 base_pool = find(b[0], b[1], b[2]);
  if (base_pool == kInvalid) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float c0 = static_cast<float>(b[k]) * L.block_size + center_coord(vi[k], L.voxel_size);
    off[k] = (pos[k] - c0) * L.voxel_size_inv;
  }
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
    const u32 safe = pool == kInvalid ? base_pool : pool;
    const u32* vox = L.voxels + (static_cast<size_t>(safe) * kVoxelsPerBlock + static_cast<u32>(v[0] + 16 * (v[1] + 16 * v[2]))) * kWordsPerVoxel;
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

// Interpolator::interpMember: q . (M . data), q = (1, dx, dy, dz, dx dy, dy dz, dz dx, dx dy dz)
__device__ __forceinline__ float interp_member(const float off[3], const float data[8]) {
  float md[8];
  interp_table_apply(data, md);
  const float dx = off[0], dy = off[1], dz = off[2];
  const float q[8] = {1.0f, dx, dy, dz, dx * dy, dy * dz, dz * dx, dx * dy * dz};
  float v = 0.0f;
#pragma unroll
  for (int i = 0; i < 8; ++i) v += q[i] * md[i];
  return v;
}

// ---- point samples on a layer, shared by the map queries (cox_query.hip) and the collision checks (cox_collide.hip) ----------
// pool indices of the up to 2 x 2 x 2 blocks around a query, resolved once; anything else is looked up in the hash table
struct BlockCache {
  const LayerView& L;
  int lo[3];
  u32 pool[8];  // (x - lo.x) << 2 | (y - lo.y) << 1 | (z - lo.z); kInvalid when missing
  u32 have;     // bit c: pool[c] was resolved
  __device__ __forceinline__ u32 operator()(int x, int y, int z) const {
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
};

// Resolves into bc the blocks of voxels g - R .. g + R around the voxel g that contains p (sc = p * block_size_inv, in index
// range): only the blocks that range touches, so one lookup for a point deep inside a block.  b[] gets the block of p.
template <int R>
__device__ __forceinline__ void block_cache_fill(const LayerView& L, const float p[3], const float sc[3], BlockCache& bc, int b[3]) {
  int span[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    b[k] = grid_index(sc[k]);
    const int v = grid_index((p[k] - static_cast<float>(b[k]) * L.block_size) * L.voxel_size_inv);
    const int g = b[k] * 16 + (v > 15 ? 15 : (v < 0 ? 0 : v));
    bc.lo[k] = (g - R) >> 4;
    span[k] = ((g + R) >> 4) - bc.lo[k];
  }
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int mx = (c >> 2) & 1, my = (c >> 1) & 1, mz = c & 1;
    if (mx <= span[0] && my <= span[1] && mz <= span[2]) {
      bc.pool[c] = HtPool{L}(bc.lo[0] + mx, bc.lo[1] + my, bc.lo[2] + mz);
      bc.have |= 1u << c;
    }
  }
}

// Interpolator::getInterpDistance (and getInterpWeight when want_w) at s: false when the cell is incomplete or invalid
__device__ __forceinline__ bool tri_sample(const LayerView& L, const BlockCache& bc, const float s[3], float* d, float* w, bool want_w) {
  int b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = grid_index(s[k] * L.block_size_inv);
  if (bc(b[0], b[1], b[2]) == kInvalid) return false;  // getBlockPtrByCoordinates(pos)
  float dd[8], ww[8], off[3];
  if (!interp_cell(L, s, b, bc, dd, ww, off)) return false;
  *d = interp_member(off, dd);
  if (want_w) *w = interp_member(off, ww);
  return true;
}

// Block::getVoxelByCoordinates: the containing block, the grid index clamped into it; valid when weight > 0
__device__ __forceinline__ bool nearest_sample(const LayerView& L, const BlockCache& bc, const float s[3], float* d, float* w) {
  int b[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = grid_index(s[k] * L.block_size_inv);
  const u32 pool = bc(b[0], b[1], b[2]);
  if (pool == kInvalid) return false;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float rel = s[k] - static_cast<float>(b[k]) * L.block_size;
    const int g = grid_index(rel * L.voxel_size_inv);
    v[k] = g > 15 ? 15 : (g < 0 ? 0 : g);
  }
  const u32* vox = L.voxels + (static_cast<size_t>(pool) * kVoxelsPerBlock + static_cast<u32>(v[0] + 16 * (v[1] + 16 * v[2]))) * kWordsPerVoxel;
  *d = __uint_as_float(vox[0]);
  *w = __uint_as_float(vox[1]);
  return *w > 0.0f;
}

}  // namespace cox
