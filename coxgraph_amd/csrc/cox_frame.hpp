// Per-frame device state shared by the kernels of every stage: counters, the layer / ray / record views, point validity and weights
// -- part of cox_integrator.hip (included there first: the kernel headers that follow use what is defined here).
#pragma once

// per-frame control words of the observed-set solve of the fast integrator (cox_fast.hpp; part of Counters, zeroed with it at frame start)
constexpr int kFastMaxRounds = 8;
struct FastCtl {
  u32 n_visits[kFastMaxRounds];   // candidate visits of round 0 (cap0 per ray) / of a later round (sum of the grown lists; 0 = the round does not run)
  u32 settled[kFastMaxRounds];    // [round]: the relaxation reached a pass that moved nothing
  u32 want_more[kFastMaxRounds];  // [round]: at that fixed point some ray is at the end of a list shorter than its walk, unstopped
  u32 passes[kFastMaxRounds];     // [round]: passes the relaxation took
  u32 ticks_work[kFastMaxRounds], ticks_wait[kFastMaxRounds];  // [round]: 100 MHz ticks workgroup 0 spent working / waiting at the barrier
  u32 grew[kFastMaxRounds];       // [round >= 1]: the round runs (k_fast_grow gave some ray its whole walk)
  u32 scan_n[kFastMaxRounds];     // [round >= 1]: rays the cap scan of the round covers (0 = the round does not run)
  u32 n_long;        // rays with a list longer than cap1 (one wave each), over all rounds
  u32 overflow;      // lists that do not fit their buffers
  u32 sequential;    // the sequential kernel produced this frame's result (k_fast_sequential)
  u32 pad[5];
  struct Bar {
    u32 arrived, pad0[15], epoch, pad1[15], moved[3], want[3], abort, pad2[9];
  } bar[kFastMaxRounds];
};
struct Counters {  // per-frame device counters, zeroed at frame start
  u32 n_valid;      // points that passed isPointValid
  u32 n_rays;       // rays cast (simple: valid points, merged: bundles)
  u32 n_ray_slots;  // ray ids in use, [0, n_ray_slots) (simple: n_points, merged: bundles)
  u32 n_records;    // sum of ray step counts
  u32 n_touched;    // blocks touched this frame
  u32 n_voxels;     // distinct voxels updated
  u32 n_updates;    // (ray, voxel) updates
  u32 n_long;       // voxels whose record run spans more than one wave
  u32 n_new_blocks;
  u32 err;
  u32 n_depth_points;
  u32 n_sorted_valid;  // valid points as seen in the sorted bundling keys (merged)
  u32 n_piece_slots;   // piece path: sum of the rays' piece bounds = slots of the piece arrays in use
  u32 n_expanded;      // piece partition: records written by k_piece_expand (what k_apply_block reads)
  u32 n_big_tiles, n_big_chunks;  // tiles whose phase 1 is split over the chip (k_big_tiles), and their chunks
  u32 n_block_tiles;              // tiles too large for k_apply_wave: k_apply_block's list
  FastCtl fast;
  // One word takes ~88 atomics/us on this chip, so counters that every wave or workgroup of a large grid adds to
  // are sharded over 64 cache lines (index = workgroup or wave id & 63) and summed by the host.
  // [s][0] valid points, [s][1] updates, [s][2] voxels, [s][3] long runs, [s][4] rays
  u32 shard[64][16];
};
enum : u32 { kShValid = 0, kShUpdates = 1, kShVoxels = 2, kShLong = 3, kShRays = 4, kShMaxBundle = 5, kShMaxRun = 6 };  // 5, 6: maxima, not sums

// the read-write view of the units that write a layer (not the read-only cox::LayerView of cox_interp.hpp, which the gather kernels use)
struct LayerView {
  u32* voxels;
  u64* ht_keys;
  u32* ht_vals;
  u32* ht_stamp;
  u32* ht_ord;
  u64* block_keys;
  u32* d_nblocks;
  u32 ht_mask;
  u32 capacity;
};

struct RayArrays {
  float *px, *py, *pz, *w;  // point_G and (merged) weight of each ray
  u32* color;               // wire-packed colour
  u32* flags;               // bit0 valid, bit1 clearing
  u64* key;                 // terminal voxel key (anti-grazing)
  u32* nsteps;              // records this ray emits
  u32* rec_off;             // exclusive scan of nsteps
  float* q;                 // merged: 8 words per ray in one 32-B line: point_G - origin (x, y, z), its length, the ray's weight, its colour, 2 unused
  u32* pbound;              // piece path: upper bound of the ray's piece count (piece_bound)
  u32* piece_off;           // exclusive scan of pbound
};

// the frame block table of the merged record walk (cox_walk.hpp, where it is explained)
struct FrameBlocks {
  u64* keys;   // [mask + 1] block key per slot; empty between frames (the binding empties the slots it reads)
  u32* ord;    // [mask + 1] ordinal of the slot's key (valid while the key is there)
  u32* slots;  // [mask + 1] the occupied slots in ordinal order: slots[0, n_touched)
  u32 mask;
};
// per-axis crossing capacity of the parallel DDA (cox_walk.hpp: wave_ray_path) and the ray flags beyond bit 0 (valid) and bit 1 (clearing)
constexpr u32 kAxisCapSmall = 128, kAxisCapLarge = 512;
constexpr u32 kRayFallback = 4u;  // ray flag: the parallel walk does not cover this ray (sequential walk on lane 0, touch and emit alike)
constexpr u32 kRayNoPath = 8u;    // ray flag: no path parked for emit (k_bundle_merge<true>: the ray's slot ends beyond the record buffers); emit walks it sequentially

// both ping-pong buffers of the record sort + where the result ended up
struct RecordView {
  const u32* key[2];
  const u32* ray[2];
  const SortInfo* info;
  const u32* d_n;
};

__device__ __forceinline__ u32 rgba_wire_order(u32 v) {  // v: little endian r | g<<8 | b<<16 | a<<24
  return ((v >> 24) & 255u) | (((v >> 16) & 255u) << 8) | (((v >> 8) & 255u) << 16) | ((v & 255u) << 24);
}
__device__ __forceinline__ u32 pack_rgba_wire(const uint8_t* rgba, u32 i) {
  if (!rgba) return 0u;
  return rgba_wire_order(reinterpret_cast<const u32*>(rgba)[i]);
}
// isPointValid.  Non-finite points (which voxblox_ros filters out before the integrator, and on which upstream's
// float -> int64 index casts are undefined) are defined as invalid here and in the oracle.
__device__ __forceinline__ bool point_valid(const FrameParams& P, F3 p, bool* clearing) {
  const float r = sqrtf(dot3(p, p));
  if (!(r <= 3.0e38f)) return false;  // NaN or inf in any coordinate
  if (r < P.min_ray) return false;
  if (r > P.max_ray) {
    if (P.allow_clear || P.freespace) {
      *clearing = true;
      return true;
    }
    return false;
  }
  *clearing = P.freespace != 0;
  return true;
}
__device__ __forceinline__ float voxel_weight(const FrameParams& P, F3 p) {
  if (P.use_const_weight) return 1.0f;
  const float dz = fabsf(p.z);
  if (dz > kEps) return 1.0f / (dz * dz);
  return 0.0f;
}
// wave-uniform values must be made visibly scalar (SGPR): hipcc's divergence analysis treats threadIdx.x >> 6 as
// per-lane, which turns every wave-cooperative loop below into a predicated / waterfall loop
__device__ __forceinline__ u32 uniform_u32(u32 v) { return static_cast<u32>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }
__device__ __forceinline__ float readlane_f32(float v, u32 lane) { return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), lane)); }
