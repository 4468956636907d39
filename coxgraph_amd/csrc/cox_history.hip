// MI355X (gfx950): observation histories behind include/coxgraph_hip_history.h -- which frames saw which part of a submap, and
// the per-triangle run-length lists of a mesh-with-history (what TsdfRecover::processMesh consumes,
// coxgraph/include/coxgraph/map_comm/tsdf_recover.h:59-99).  The rule is this project's own: DESIGN.md section 7f.
//
//   k_obs_mark      one lane per input point: validity and transform as the integrators do them, the point's 4x4x4-voxel cell; the
//                   lanes of a wave that share a cell elect a leader (ballots, as k_bundle_insert does), which probes the record's
//                   block table (allocating on a miss: ht_insert + bump pool) and ORs the frame's bit into the cell's 256-bit mask
//   k_tri_mask      one lane per triangle: OR of the masks of the cells that contain its three vertices, number of runs
//   (scan)          cox_sort.hpp's exclusive scan of the run words
//   k_tri_runs      one lane per triangle: the mask as ascending inclusive [first, last] pairs
//
// The record owns its table, pool and stream: it follows neither the layer's growth nor the integrator's frame pipeline, and
// marking is idempotent (OR), so nothing here has an order to keep.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/coxgraph_hip_history.h"
#include "cox_host.hpp"
#include "cox_sort.hpp"

using namespace cox;

#include "cox_frame.hpp"

constexpr u32 kObsCells = COX_OBS_CELLS_PER_BLOCK;
constexpr u32 kObsWords = COX_OBS_WORDS_PER_CELL;
constexpr u32 kObsBlockWords = kObsCells * kObsWords;  // 512 words = 2 KiB per block
constexpr u32 kObsNoPool = 0xFFFFFFFEu;                // table entry of a block that found the pool full
constexpr u32 kObsSpinMax = 1u << 16;
constexpr u64 kObsDefaultCapacity = 1024;
constexpr u64 kObsMaxCapacity = 1ull << 22;
enum : u32 { kCtlBlocks = 0, kCtlErr = 1, kCtlWords = 2 };

struct ObsView {
  u64* ht_keys;
  u32* ht_vals;
  u32 ht_mask;
  u32* masks;
  u64* block_keys;
  u32 capacity;
  u32* ctl;    // [kCtlBlocks] allocated blocks, [kCtlErr] sticky error bits
  u32* shard;  // [64][2] running totals: points that marked, atomic ORs issued for them
};

struct cox_obs {
  int device = 0;
  float voxel_size = 0, voxel_size_inv = 0;
  u64 capacity = 0;
  u32 ht_cap = 0;
  DevBuf<u64> ht_keys;
  DevBuf<u32> ht_vals;
  DevBuf<u32> masks;
  DevBuf<u64> block_keys;
  DevBuf<u32> ctl;
  DevBuf<u32> shard;
  PinnedBuf<u32> h_ctl;  // ctl as the last record left it (the host sees the pool fill up without a sync)
  Stream st;
  Event ev_count;            // h_ctl of the last record has landed
  Event ev_caller, ev_read;  // cox_obs_record_dev: the caller's stream so far / the cloud has been read
  bool has_record = false;
  u32 frame_id = 0;
  bool auto_grow = true;
  u64 blocks_seen = 0, blocks_delta_max = 0;
};

namespace {

// block and cell of the voxel a scaled coordinate triple falls in
__device__ __forceinline__ void cell_of(int gx, int gy, int gz, u64* key, u32* cell) {
  *key = pack_key(gx >> 4, gy >> 4, gz >> 4);
  *cell = static_cast<u32>((gx & 15) >> 2) | (static_cast<u32>((gy & 15) >> 2) << 2) | (static_cast<u32>((gz & 15) >> 2) << 4);
}

__global__ void __launch_bounds__(256) k_obs_mark(FrameParams P, ObsView O) {
  const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lane = lane_id();
  bool valid = false;
  u64 key = 0;
  u32 cell = 0;
  if (idx < P.n_points) {
    const F3 p{P.xyz[3 * idx], P.xyz[3 * idx + 1], P.xyz[3 * idx + 2]};
    bool clearing = false;
    if (point_valid(P, p, &clearing) && !clearing) {  // clearing rays carve, they have not seen a surface
      const F3 pg = transform_point(P, p);
      const float sx = pg.x * P.voxel_size_inv, sy = pg.y * P.voxel_size_inv, sz = pg.z * P.voxel_size_inv;
      if (!(index_in_range(sx) && index_in_range(sy) && index_in_range(sz))) {  // also catches NaN
        atomicOr(&O.ctl[kCtlErr], kErrRange);
      } else {
        cell_of(grid_index(sx), grid_index(sy), grid_index(sz), &key, &cell);
        valid = true;
      }
    }
  }
  // group the lanes by (block, cell) with ALU work only; the group leaders then touch memory at the same time
  bool is_leader = false;
  const u64 marking = __ballot(valid);
  u64 todo = marking;
  while (todo) {
    const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(todo))) - 1u;
    const u64 k = (static_cast<u64>(static_cast<u32>(__builtin_amdgcn_readlane(static_cast<u32>(key >> 32), leader))) << 32) |
                  static_cast<u64>(static_cast<u32>(__builtin_amdgcn_readlane(static_cast<u32>(key), leader)));
    const u32 c = static_cast<u32>(__builtin_amdgcn_readlane(cell, leader));
    const u64 peers = __ballot(valid && key == k && cell == c);
    if (lane == leader) is_leader = true;
    todo &= ~peers;
  }
  const u64 leaders = __ballot(is_leader);
  if (lane == 0 && marking) {
    u32* sh = O.shard + 2u * (blockIdx.x & 63u);
    atomicAdd(&sh[0], static_cast<u32>(__popcll(marking)));
    atomicAdd(&sh[1], static_cast<u32>(__popcll(leaders)));
  }
  u32 slot = kInvalid, pool = kInvalid;
  if (is_leader) {
    bool fresh = false;
    slot = ht_insert(O.ht_keys, O.ht_mask, key, &fresh);
    if (slot == kInvalid) {
      atomicOr(&O.ctl[kCtlErr], kErrTable);
    } else if (fresh) {
      pool = atomicAdd(&O.ctl[kCtlBlocks], 1u);
      if (pool < O.capacity) {
        O.block_keys[pool] = key;  // read by later kernels only
      } else {
        atomicSub(&O.ctl[kCtlBlocks], 1u);  // the counter settles at the capacity
        pool = kObsNoPool;                  // (the error is raised below, by everyone who meets the block)
      }
      __hip_atomic_store(&O.ht_vals[slot], pool, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // a leader that found a key another lane claimed in this launch waits for the claimer's pool index (bounded: the claimer
  // has passed the branch above, or runs in another wave)
  if (is_leader && slot != kInvalid && pool == kInvalid) {
    for (u32 spin = 0; spin < kObsSpinMax; ++spin) {
      pool = __hip_atomic_load(&O.ht_vals[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
      if (pool != kInvalid) break;
      __builtin_amdgcn_s_sleep(2);
    }
    if (pool == kInvalid) atomicOr(&O.ctl[kCtlErr], kErrRecords);
  }
  if (is_leader && pool != kInvalid) {
    if (pool >= O.capacity) {
      atomicOr(&O.ctl[kCtlErr], kErrPool);
    } else {
      u32* w = O.masks + (static_cast<size_t>(pool) * kObsCells + cell) * kObsWords + (P.frame_id >> 5);
      const u32 bit = 1u << (P.frame_id & 31u);
      // neighbouring waves mark the same cell: once the bit is visible the same-address atomics stop (a stale read costs one)
      if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);
    }
  }
}

// the table again for the first n pool blocks (after the pool has grown)
__global__ void __launch_bounds__(256) k_obs_rehash(u64* __restrict__ ht_keys, u32* __restrict__ ht_vals, u32 ht_mask, const u64* __restrict__ block_keys, u32 n,
                                                    u32* __restrict__ ctl) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bool fresh = false;
  const u32 slot = ht_insert(ht_keys, ht_mask, block_keys[i], &fresh);
  if (slot == kInvalid)
    atomicOr(&ctl[kCtlErr], kErrTable);
  else
    ht_vals[slot] = i;
}

__global__ void __launch_bounds__(256) k_obs_count_cells(const u32* __restrict__ masks, u32 n_cells, u32* __restrict__ out) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  bool any = false;
  if (i < n_cells) {
    const uint4 a = reinterpret_cast<const uint4*>(masks)[2 * static_cast<size_t>(i)], b = reinterpret_cast<const uint4*>(masks)[2 * static_cast<size_t>(i) + 1];
    any = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) != 0u;
  }
  const u64 m = __ballot(any);
  if (lane_id() == 0 && m) atomicAdd(out, static_cast<u32>(__popcll(m)));
}

// per triangle: the OR of its vertices' cells and the number of history words (two per run)
__global__ void __launch_bounds__(256) k_tri_mask(const float* __restrict__ pos, u32 n_tri, float voxel_size_inv, const u64* __restrict__ ht_keys,
                                                  const u32* __restrict__ ht_vals, u32 ht_mask, const u32* __restrict__ masks, u32 capacity,
                                                  uint4* __restrict__ tri_mask, u32* __restrict__ tri_words) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tri) return;
  u32 m[kObsWords] = {0, 0, 0, 0, 0, 0, 0, 0};
  u64 seen_key[3];
  u32 seen_cell[3];
#pragma unroll
  for (int v = 0; v < 3; ++v) {
    const float* p = pos + 9 * static_cast<size_t>(t) + 3 * v;
    const float sx = p[0] * voxel_size_inv, sy = p[1] * voxel_size_inv, sz = p[2] * voxel_size_inv;
    seen_key[v] = kEmptyKey;
    seen_cell[v] = 0;
    if (!(index_in_range(sx) && index_in_range(sy) && index_in_range(sz))) continue;
    cell_of(grid_index(sx), grid_index(sy), grid_index(sz), &seen_key[v], &seen_cell[v]);
    bool again = false;
    for (int q = 0; q < v; ++q) again = again || (seen_key[q] == seen_key[v] && seen_cell[q] == seen_cell[v]);
    if (again) continue;  // (most triangles lie in one cell)
    const u32 slot = ht_find(ht_keys, ht_mask, seen_key[v]);
    if (slot == kInvalid) continue;  // no block: nobody saw it
    const u32 pool = ht_vals[slot];
    if (pool >= capacity) continue;
    const uint4* c = reinterpret_cast<const uint4*>(masks + (static_cast<size_t>(pool) * kObsCells + seen_cell[v]) * kObsWords);
    const uint4 a = c[0], b = c[1];
    m[0] |= a.x, m[1] |= a.y, m[2] |= a.z, m[3] |= a.w, m[4] |= b.x, m[5] |= b.y, m[6] |= b.z, m[7] |= b.w;
  }
  // runs = rising edges over the 256 bits: bit set, the bit below it (the top bit of the word before, across words) clear
  u32 runs = 0, carry = 0;
#pragma unroll
  for (u32 w = 0; w < kObsWords; ++w) {
    runs += static_cast<u32>(__popc(m[w] & ~((m[w] << 1) | carry)));
    carry = m[w] >> 31;
  }
  tri_mask[2 * static_cast<size_t>(t)] = make_uint4(m[0], m[1], m[2], m[3]);
  tri_mask[2 * static_cast<size_t>(t) + 1] = make_uint4(m[4], m[5], m[6], m[7]);
  tri_words[t] = 2u * runs;
}

__global__ void __launch_bounds__(256) k_tri_runs(const uint4* __restrict__ tri_mask, const u32* __restrict__ tri_off, u32 n_tri, u32 n_words,
                                                  u32* __restrict__ history) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tri) return;
  const uint4 a = tri_mask[2 * static_cast<size_t>(t)], b = tri_mask[2 * static_cast<size_t>(t) + 1];
  const u32 m[kObsWords] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  u32 out = tri_off[t];
  u32 carry = 0;  // the bit below bit 0 of this word
#pragma unroll
  for (u32 w = 0; w < kObsWords; ++w) {
    const u32 below = (m[w] << 1) | carry;
    u32 rise = m[w] & ~below;  // first bits of runs
    u32 fall = ~m[w] & below;  // bits right after a run's last bit
    carry = m[w] >> 31;
    // a run that crossed into this word ends here before any run of this word begins, so ends and begins alternate in bit order
    while (rise | fall) {
      const u32 br = rise ? static_cast<u32>(__ffs(static_cast<int>(rise))) - 1u : 32u;
      const u32 bf = fall ? static_cast<u32>(__ffs(static_cast<int>(fall))) - 1u : 32u;
      if (bf < br) {  // end of the open run: last = the bit before
        if (out < n_words) history[out] = w * 32u + bf - 1u;
        ++out;
        fall &= fall - 1u;
      } else {
        if (out < n_words) history[out] = w * 32u + br;
        ++out;
        rise &= rise - 1u;
      }
    }
  }
  if (carry) {  // a run up to frame 255
    if (out < n_words) history[out] = 255u;
  }
}

ObsView obs_view(const cox_obs* O) {
  return ObsView{O->ht_keys, O->ht_vals, O->ht_cap - 1, O->masks, O->block_keys, static_cast<u32>(O->capacity), O->ctl, O->shard};
}

// table + pool of `capacity` blocks, empty, on the record's stream
int obs_alloc_pool(u64 capacity, DevBuf<u64>* ht_keys, DevBuf<u32>* ht_vals, DevBuf<u32>* masks, DevBuf<u64>* block_keys, u32* ht_cap, hipStream_t s) {
  *ht_cap = next_pow2(2 * capacity);
  COX_TRY(ht_keys->alloc(*ht_cap));
  COX_TRY(ht_vals->alloc(*ht_cap));
  COX_TRY(masks->alloc(capacity * kObsBlockWords));
  COX_TRY(block_keys->alloc(capacity));
  COX_HIP(hipMemsetAsync(ht_keys->p, 0xFF, sizeof(u64) * *ht_cap, s));
  COX_HIP(hipMemsetAsync(ht_vals->p, 0xFF, sizeof(u32) * *ht_cap, s));
  COX_HIP(hipMemsetAsync(masks->p, 0, sizeof(u32) * capacity * kObsBlockWords, s));  // bump-allocated blocks start out unmarked
  return COX_OK;
}

// stream idle: the pool with `capacity` blocks, the marks kept
int obs_reserve(cox_obs* O, u64 capacity) {
  // the new pool; after the swaps these hold the old one, which goes with them
  DevBuf<u64> keys, bkeys;
  DevBuf<u32> vals, masks;
  u32 ht_cap = 0;
  COX_TRY(obs_alloc_pool(capacity, &keys, &vals, &masks, &bkeys, &ht_cap, O->st));
  const u32 n = static_cast<u32>(std::min<u64>(O->h_ctl.p[kCtlBlocks], O->capacity));
  if (n) {
    COX_HIP(hipMemcpyAsync(masks, O->masks, sizeof(u32) * kObsBlockWords * n, hipMemcpyDeviceToDevice, O->st));
    COX_HIP(hipMemcpyAsync(bkeys, O->block_keys, sizeof(u64) * n, hipMemcpyDeviceToDevice, O->st));
    hipLaunchKernelGGL(k_obs_rehash, dim3((n + 255) / 256), dim3(256), 0, O->st, keys.p, vals.p, ht_cap - 1, bkeys.p, n, O->ctl.p);
  }
  COX_HIP(hipStreamSynchronize(O->st));
  O->ht_keys.swap(keys), O->ht_vals.swap(vals), O->masks.swap(masks), O->block_keys.swap(bkeys);
  O->ht_cap = ht_cap;
  O->capacity = capacity;
  return COX_OK;
}

// The pool doubles once it is half full -- or will be, at the largest rate seen between two looks (the host's view of the count is
// as old as the records still in flight).  A cloud that outruns it all the same loses marks and says so (kErrPool).
int obs_follow(cox_obs* O) {
  const u64 n_seen = O->h_ctl.p[kCtlBlocks];
  if (n_seen > O->blocks_seen) O->blocks_delta_max = std::max<u64>(O->blocks_delta_max, n_seen - O->blocks_seen);
  O->blocks_seen = n_seen;
  const u64 need = std::max<u64>(2 * n_seen, n_seen + 8 * O->blocks_delta_max);
  if (!O->auto_grow || need <= O->capacity || O->capacity >= kObsMaxCapacity) return COX_OK;
  COX_HIP(hipStreamSynchronize(O->st));
  u64 cap = O->capacity;
  while (cap < need && cap < kObsMaxCapacity) cap *= 2;
  const int st = obs_reserve(O, cap);
  if (st == COX_ERR_OUT_OF_MEMORY) {  // carry on with what there is
    O->auto_grow = false;
    return COX_OK;
  }
  return st;
}

// wait for the records, take the sticky error bits
int obs_settle(cox_obs* O, bool take_errors) {
  COX_HIP(hipSetDevice(O->device));
  COX_HIP(hipStreamSynchronize(O->st));
  u32 h[kCtlWords] = {0, 0};
  COX_HIP(hipMemcpy(h, O->ctl, sizeof(h), hipMemcpyDeviceToHost));
  O->h_ctl.p[kCtlBlocks] = h[kCtlBlocks];
  if (!take_errors || h[kCtlErr] == 0) return COX_OK;
  COX_HIP(hipMemsetAsync(O->ctl + kCtlErr, 0, sizeof(u32), O->st));
  COX_HIP(hipStreamSynchronize(O->st));
  return err_bits_to_status(h[kCtlErr]);
}

void obs_free(cox_obs* O) {
  if (!O) return;
  (void)hipSetDevice(O->device);
  if (O->st) (void)hipStreamSynchronize(O->st);
  delete O;
  (void)hipGetLastError();
}

// masks of the triangles + their history offsets in device memory; *n_words = history entries in all
struct TriHistory {
  DevBuf<uint4> mask;
  DevBuf<u32> words, off, total, sums;
};
int tri_history(const cox_meshlayer* M, cox_obs* O, TriHistory* H, u32 n_tri, u32* n_words, double* kernel_ms) {
  COX_TRY(H->mask.alloc(2 * static_cast<size_t>(n_tri)));
  COX_TRY(H->words.alloc(n_tri));
  COX_TRY(H->off.alloc(n_tri));
  COX_TRY(H->total.alloc(1));
  COX_TRY(H->sums.alloc(scan_num_blocks(n_tri) + 2));
  EventPair ev;
  if (kernel_ms && ev.create() != COX_OK) return COX_ERR_NO_DEVICE;
  if (kernel_ms) (void)ev.begin(O->st);
  hipLaunchKernelGGL(k_tri_mask, dim3((n_tri + 255) / 256), dim3(256), 0, O->st, M->pos, n_tri, O->voxel_size_inv, O->ht_keys, O->ht_vals, O->ht_cap - 1, O->masks,
                     static_cast<u32>(O->capacity), H->mask.p, H->words.p);
  const ScanWorkspace ws{H->sums.p};
  exclusive_scan_u32(H->words.p, H->off.p, nullptr, n_tri, n_tri, H->total.p, ws, O->st);
  if (kernel_ms) (void)ev.end(O->st);
  COX_HIP(hipMemcpyAsync(n_words, H->total.p, sizeof(u32), hipMemcpyDeviceToHost, O->st));
  COX_HIP(hipStreamSynchronize(O->st));
  if (kernel_ms && !ev.elapsed_ms(kernel_ms)) return COX_ERR_NO_DEVICE;
  COX_HIP(hipGetLastError());
  return COX_OK;
}
int history_args(const cox_meshlayer* M, cox_obs* O, u32* n_tri) {
  if (!M || !O) return COX_ERR_INVALID_ARG;
  COX_TRY(device_present());
  if (M->transformed || M->device != O->device || M->voxel_size != O->voxel_size || M->n_vertices % 3 != 0 || M->n_vertices / 3 > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  *n_tri = static_cast<u32>(M->n_vertices / 3);
  return obs_settle(O, false);
}

}  // namespace

bool cox_internal_obs_matches(const cox_obs* O, const cox_layer* L) { return O->device == L->device && O->voxel_size == L->voxel_size; }

int cox_internal_obs_wait(cox_obs* O) {
  COX_HIP(hipStreamSynchronize(O->st));
  return COX_OK;
}

int cox_internal_obs_record(cox_obs* O, const float T[7], const float* xyz_dev, u32 n, int freespace, float min_ray, float max_ray, int allow_clear, hipEvent_t wait_a,
                            hipEvent_t wait_b, hipEvent_t read_done, bool settle) {
  if (n && !freespace) {  // (every point of a freespace cloud is a clearing ray)
    if (settle && O->has_record) COX_HIP(hipEventSynchronize(O->ev_count));
    COX_TRY(obs_follow(O));
    FrameParams P;
    memset(&P, 0, sizeof(P));
    P.qw = T[0], P.qx = T[1], P.qy = T[2], P.qz = T[3], P.tx = T[4], P.ty = T[5], P.tz = T[6];
    P.voxel_size = O->voxel_size;
    P.voxel_size_inv = O->voxel_size_inv;
    P.min_ray = min_ray;
    P.max_ray = max_ray;
    P.allow_clear = allow_clear;
    P.n_points = n;
    P.frame_id = O->frame_id;
    P.xyz = xyz_dev;
    if (wait_a) COX_HIP(hipStreamWaitEvent(O->st, wait_a, 0));
    if (wait_b) COX_HIP(hipStreamWaitEvent(O->st, wait_b, 0));
    hipLaunchKernelGGL(k_obs_mark, dim3((n + 255) / 256), dim3(256), 0, O->st, P, obs_view(O));
    if (read_done) COX_HIP(hipEventRecord(read_done, O->st));
    COX_HIP(hipMemcpyAsync(O->h_ctl, O->ctl, sizeof(u32) * kCtlWords, hipMemcpyDeviceToHost, O->st));
    COX_HIP(hipEventRecord(O->ev_count, O->st));
    O->has_record = true;
    COX_HIP(hipGetLastError());
  } else if (read_done) {
    COX_HIP(hipEventRecord(read_done, O->st));  // nothing is read: complete as soon as what the stream holds is
  }
  return COX_OK;
}

extern "C" {

int cox_obs_create(const cox_layer_t* L, uint64_t capacity_blocks, cox_obs_t** out) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());  // (first: a machine without a GPU says so whatever it is handed)
  if (!L || !out) return COX_ERR_INVALID_ARG;
  if (capacity_blocks > kObsMaxCapacity) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(L->device));
  cox_obs* O = new (std::nothrow) cox_obs();
  if (!O) return COX_ERR_OUT_OF_MEMORY;
  O->device = L->device;
  O->voxel_size = L->voxel_size;
  O->voxel_size_inv = L->voxel_size_inv;
  O->capacity = capacity_blocks ? capacity_blocks : kObsDefaultCapacity;
  auto fail = [&](int st) {
    obs_free(O);
    return st;
  };
  bool ok = O->st.create() == COX_OK;
  for (Event* e : {&O->ev_count, &O->ev_caller, &O->ev_read}) ok = ok && e->create(false) == COX_OK;
  ok = ok && O->h_ctl.alloc(kCtlWords) == COX_OK;
  if (!ok) return fail(COX_ERR_NO_DEVICE);
  O->h_ctl.p[kCtlBlocks] = O->h_ctl.p[kCtlErr] = 0;
  if (int st = O->ctl.alloc(kCtlWords)) return fail(st);
  if (int st = O->shard.alloc(128)) return fail(st);
  if (int st = obs_alloc_pool(O->capacity, &O->ht_keys, &O->ht_vals, &O->masks, &O->block_keys, &O->ht_cap, O->st)) return fail(st);
  if (hipMemsetAsync(O->ctl, 0, sizeof(u32) * kCtlWords, O->st) != hipSuccess || hipMemsetAsync(O->shard, 0, sizeof(u32) * 128, O->st) != hipSuccess ||
      hipStreamSynchronize(O->st) != hipSuccess)
    return fail(COX_ERR_NO_DEVICE);
  (void)hipGetLastError();
  *out = O;
  return COX_OK;
}

void cox_obs_destroy(cox_obs_t* O) { obs_free(O); }

int cox_obs_clear(cox_obs_t* O) {
  COX_ENTRY();
  if (!O) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(O->device));
  COX_HIP(hipStreamSynchronize(O->st));
  COX_HIP(hipMemsetAsync(O->ht_keys, 0xFF, sizeof(u64) * O->ht_cap, O->st));
  COX_HIP(hipMemsetAsync(O->ht_vals, 0xFF, sizeof(u32) * O->ht_cap, O->st));
  COX_HIP(hipMemsetAsync(O->masks, 0, sizeof(u32) * O->capacity * kObsBlockWords, O->st));
  COX_HIP(hipMemsetAsync(O->ctl, 0, sizeof(u32) * kCtlWords, O->st));
  COX_HIP(hipMemsetAsync(O->shard, 0, sizeof(u32) * 128, O->st));
  COX_HIP(hipStreamSynchronize(O->st));
  O->h_ctl.p[kCtlBlocks] = O->h_ctl.p[kCtlErr] = 0;
  O->blocks_seen = O->blocks_delta_max = 0;
  return COX_OK;
}

int cox_obs_set_auto_grow(cox_obs_t* O, int on) {
  COX_ENTRY_NO_DRAIN();
  if (!O) return COX_ERR_INVALID_ARG;
  O->auto_grow = on != 0;
  return COX_OK;
}

int cox_obs_set_frame(cox_obs_t* O, uint32_t frame_id) {
  COX_ENTRY_NO_DRAIN();
  if (!O) return COX_ERR_INVALID_ARG;
  if (frame_id >= COX_OBS_MAX_FRAMES) return COX_ERR_INDEX_RANGE;
  O->frame_id = frame_id;  // (a by-value kernel argument of every record enqueued from now on)
  return COX_OK;
}

int cox_obs_record_dev(cox_obs_t* O, const float T_G_C[7], const float* xyz_dev, uint64_t n, int freespace, float min_ray, float max_ray, int allow_clear,
                       void* hip_stream) {
  COX_ENTRY_NO_DRAIN();
  if (!O || !T_G_C || (n && !xyz_dev) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  COX_HIP(hipSetDevice(O->device));
  hipStream_t caller = static_cast<hipStream_t>(hip_stream);
  COX_HIP(hipEventRecord(O->ev_caller, caller));
  COX_TRY(cox_internal_obs_record(O, T_G_C, xyz_dev, static_cast<u32>(n), freespace, min_ray, max_ray, allow_clear, O->ev_caller, nullptr, O->ev_read, true));
  COX_HIP(hipStreamWaitEvent(caller, O->ev_read, 0));
  return COX_OK;
}

int cox_obs_record(cox_obs_t* O, const float T_G_C[7], const float* xyz, uint64_t n, int freespace, float min_ray, float max_ray, int allow_clear) {
  COX_ENTRY_NO_DRAIN();
  if (!O || !T_G_C || (n && !xyz) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  COX_HIP(hipSetDevice(O->device));
  DevBuf<float> d;
  COX_TRY(d.alloc(3 * n));
  COX_HIP(hipMemcpyAsync(d.p, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, O->st));
  for (;;) {
    COX_TRY(cox_internal_obs_record(O, T_G_C, d.p, static_cast<u32>(n), freespace, min_ray, max_ray, allow_clear, nullptr, nullptr, nullptr, true));
    COX_HIP(hipStreamSynchronize(O->st));
    // This call waits for its cloud anyway, so it loses nothing to a full pool: double the pool and mark the cloud again (marking is
    // idempotent; the rebuilt table drops the blocks that found no room).
    if (!(O->h_ctl.p[kCtlErr] & (kErrPool | kErrTable)) || !O->auto_grow || O->capacity >= kObsMaxCapacity) break;
    const int st = obs_reserve(O, std::min<u64>(2 * O->capacity, kObsMaxCapacity));
    if (st == COX_ERR_OUT_OF_MEMORY) {
      O->auto_grow = false;
      break;
    }
    COX_TRY(st);
    const u32 keep = O->h_ctl.p[kCtlErr] & ~(kErrPool | kErrTable);
    COX_HIP(hipMemcpyAsync(O->ctl + kCtlErr, &keep, sizeof(u32), hipMemcpyHostToDevice, O->st));
    COX_HIP(hipStreamSynchronize(O->st));
  }
  return COX_OK;
}

int cox_obs_sync(cox_obs_t* O) {
  COX_ENTRY();
  if (!O) return COX_ERR_INVALID_ARG;
  return obs_settle(O, true);
}

int cox_obs_stats(cox_obs_t* O, uint64_t* n_blocks, uint64_t* n_marked_cells, uint64_t* bytes) {
  COX_ENTRY();
  if (!O) return COX_ERR_INVALID_ARG;
  COX_TRY(obs_settle(O, false));
  const u32 nb = static_cast<u32>(std::min<u64>(O->h_ctl.p[kCtlBlocks], O->capacity));
  if (n_blocks) *n_blocks = nb;
  if (bytes)
    *bytes = O->capacity * (sizeof(u32) * kObsBlockWords + sizeof(u64)) + static_cast<u64>(O->ht_cap) * (sizeof(u64) + sizeof(u32)) + sizeof(u32) * (kCtlWords + 128);
  if (n_marked_cells) {
    *n_marked_cells = 0;
    if (nb) {
      DevBuf<u32> d;
      COX_TRY(d.alloc(1));
      COX_HIP(hipMemsetAsync(d.p, 0, sizeof(u32), O->st));
      hipLaunchKernelGGL(k_obs_count_cells, dim3((nb * kObsCells + 255) / 256), dim3(256), 0, O->st, O->masks, nb * kObsCells, d.p);
      u32 h = 0;
      COX_HIP(hipMemcpyAsync(&h, d.p, sizeof(u32), hipMemcpyDeviceToHost, O->st));
      COX_HIP(hipStreamSynchronize(O->st));
      *n_marked_cells = h;
    }
  }
  return COX_OK;
}

int cox_obs_counts(cox_obs_t* O, uint64_t* n_marking_points, uint64_t* n_atomics) {
  COX_ENTRY();
  if (!O) return COX_ERR_INVALID_ARG;
  COX_TRY(obs_settle(O, false));
  u32 h[128];
  COX_HIP(hipMemcpy(h, O->shard, sizeof(h), hipMemcpyDeviceToHost));
  u64 a = 0, b = 0;
  for (int s = 0; s < 64; ++s) a += h[2 * s], b += h[2 * s + 1];
  if (n_marking_points) *n_marking_points = a;
  if (n_atomics) *n_atomics = b;
  return COX_OK;
}

int cox_obs_download(cox_obs_t* O, int32_t* block_index, uint32_t* masks, uint64_t cap_blocks, uint64_t* n_blocks) {
  COX_ENTRY();
  if (!O || !n_blocks) return COX_ERR_INVALID_ARG;
  COX_TRY(obs_settle(O, false));
  const u32 nb = static_cast<u32>(std::min<u64>(O->h_ctl.p[kCtlBlocks], O->capacity));
  *n_blocks = nb;
  if (!block_index && !masks) return COX_OK;
  if (cap_blocks < nb) return COX_ERR_BUFFER_TOO_SMALL;
  if (nb == 0) return COX_OK;
  std::vector<u64> keys(nb);
  COX_HIP(hipMemcpy(keys.data(), O->block_keys, sizeof(u64) * nb, hipMemcpyDeviceToHost));
  std::vector<u32> order(nb);
  for (u32 i = 0; i < nb; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return keys[a] < keys[b]; });  // the packed key orders (z, y, x)
  if (block_index)
    for (u32 i = 0; i < nb; ++i) {
      int x, y, z;
      unpack_key(keys[order[i]], &x, &y, &z);
      block_index[3 * i] = x, block_index[3 * i + 1] = y, block_index[3 * i + 2] = z;
    }
  if (masks) {
    std::vector<u32> pool(static_cast<size_t>(nb) * kObsBlockWords);
    COX_HIP(hipMemcpy(pool.data(), O->masks, sizeof(u32) * pool.size(), hipMemcpyDeviceToHost));
    for (u32 i = 0; i < nb; ++i) memcpy(masks + static_cast<size_t>(i) * kObsBlockWords, pool.data() + static_cast<size_t>(order[i]) * kObsBlockWords, sizeof(u32) * kObsBlockWords);
  }
  return COX_OK;
}

int cox_meshlayer_history_size(const cox_meshlayer_t* M, cox_obs_t* O, uint64_t* n_triangles, uint64_t* n_history, double* kernel_ms) {
  COX_ENTRY();
  u32 n_tri = 0;
  COX_TRY(history_args(M, O, &n_tri));
  if (n_triangles) *n_triangles = n_tri;
  if (n_history) *n_history = 0;
  if (kernel_ms) *kernel_ms = 0.0;
  if (n_tri == 0 || !n_history) return COX_OK;
  TriHistory H;
  u32 n_words = 0;
  COX_TRY(tri_history(M, O, &H, n_tri, &n_words, kernel_ms));
  *n_history = n_words;
  return COX_OK;
}

int cox_meshlayer_history(const cox_meshlayer_t* M, cox_obs_t* O, uint64_t* history_begin, uint32_t* history, uint8_t* block_has_history, uint64_t cap_triangles,
                          uint64_t cap_history, uint64_t cap_blocks) {
  COX_ENTRY();
  u32 n_tri = 0;
  COX_TRY(history_args(M, O, &n_tri));
  if (!history_begin) return COX_ERR_INVALID_ARG;
  if (cap_triangles < n_tri || (block_has_history && cap_blocks < M->n_blocks)) return COX_ERR_BUFFER_TOO_SMALL;
  history_begin[0] = 0;
  if (block_has_history) std::fill(block_has_history, block_has_history + M->n_blocks, static_cast<uint8_t>(0));
  if (n_tri == 0) return COX_OK;
  TriHistory H;
  u32 n_words = 0;
  COX_TRY(tri_history(M, O, &H, n_tri, &n_words, nullptr));
  if (cap_history < n_words || (n_words && !history)) return COX_ERR_BUFFER_TOO_SMALL;
  std::vector<u32> off(n_tri);
  COX_HIP(hipMemcpyAsync(off.data(), H.off.p, sizeof(u32) * n_tri, hipMemcpyDeviceToHost, O->st));
  if (n_words) {
    DevBuf<u32> d_hist;
    COX_TRY(d_hist.alloc(n_words));
    hipLaunchKernelGGL(k_tri_runs, dim3((n_tri + 255) / 256), dim3(256), 0, O->st, H.mask.p, H.off.p, n_tri, n_words, d_hist.p);
    COX_HIP(hipMemcpyAsync(history, d_hist.p, sizeof(u32) * n_words, hipMemcpyDeviceToHost, O->st));
    COX_HIP(hipStreamSynchronize(O->st));
  } else {
    COX_HIP(hipStreamSynchronize(O->st));
  }
  COX_HIP(hipGetLastError());
  for (u32 t = 0; t < n_tri; ++t) history_begin[t] = off[t];
  history_begin[n_tri] = n_words;
  if (block_has_history)
    for (u64 b = 0; b < M->n_blocks; ++b) {
      const u64 t0 = M->vertex_begin[b] / 3, t1 = M->vertex_begin[b + 1] / 3;
      block_has_history[b] = history_begin[t1] > history_begin[t0] ? 1 : 0;
    }
  return COX_OK;
}

}  // extern "C"
