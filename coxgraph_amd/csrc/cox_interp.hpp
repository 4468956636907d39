// voxblox Interpolator<TsdfVoxel>::getVoxelsAndQVector on the GPU, shared by the registration cost (cox_reg.hip) and the map
// queries (cox_query.hip).  The arithmetic is oracle/cox_oracle.hpp's getVoxelsAndQVector + interpMember, expression by
// expression, so both kernels reproduce the checker bit for bit.
#pragma once
#include "cox_device.hpp"

namespace cox {

// the read-only part of a layer a gather kernel needs
struct LayerView {
  const u32* voxels;
  const u64* ht_keys;
  const u32* ht_vals;
  u32 ht_mask;
  float voxel_size, voxel_size_inv, block_size, block_size_inv;
};

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

}  // namespace cox
