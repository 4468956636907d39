// MI355X (gfx950): voxblox EsdfIntegrator::updateFromTsdfLayer -- an ESDF that follows a TSDF layer and, after every update,
// holds exactly the words cox_esdf_from_tsdf (cox_submap.hip) would return for the TSDF as it is now.  DESIGN.md section 7l.
//
// The ESDF layer mirrors the TSDF's pool: pool block i of the one is pool block i of the other (the TSDF's pool only ever
// grows at its end, except through cox_layer_clear and a dropped projective frame, which are detected and answered with a
// rebuild).  The state is the layer's own three words per voxel; there are no parent pointers.  One update:
//
//   mirror    new pool blocks are adopted (keys copied, hashed, linked into the 27-neighbour table)
//   classify  every block: the batch's init rule on the TSDF words, merged with the stored ESDF words; a free voxel keeps its
//             distance if it was free before with the same sign.  A block in which a word changed is dirty.
//   raise     a free voxel that is not at its init value must be supported: an observed neighbour n with |d_n| < max_distance
//             offers exactly its value.  Unsupported voxels go back to init; to convergence over the dirty blocks' surroundings.
//             What survives is an upper bound (in |d|) of the new fixed point.
//   lower     the batch's relaxation, over the blocks the two steps above changed and whatever they reach.
//
// raise and lower run one workgroup per block over an 18^3 LDS tile, like k_esdf_sweep; workgroups of inactive blocks leave at
// once, a block that changed something activates the 27 blocks around it for the next sweep, and the host reads the sweep
// counters once per kSweepsPerRead launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>

#include "../../include/coxgraph_hip_esdf.h"
#include "cox_esdf.hpp"
#include "cox_host.hpp"

using namespace cox;

namespace {

typedef unsigned long long ull;

constexpr int kSweepsPerRead = 8;
// control words on the device (u32 each; the two voxel counters are 64 bits wide)
constexpr int kCtlMismatch = 0, kCtlDirty = 1, kCtlReset = 2, kCtlChanged = 4, kCtlSwept = 6, kCtlSweepChanged = 8, kCtlSweepActive = kCtlSweepChanged + kSweepsPerRead,
              kCtlWords = kCtlSweepActive + kSweepsPerRead;
constexpr int kHostNb = kCtlWords, kHostErr = kCtlWords + 1, kHostWords = kCtlWords + 2;
constexpr size_t kBlockWords = static_cast<size_t>(kVoxelsPerBlock) * kWordsPerVoxel;

// ---- mirror --------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_esdf_keys_differ(const u64* __restrict__ a, const u64* __restrict__ b, u32 n, u32* __restrict__ flag) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && a[i] != b[i]) *flag = 1;
}
// pool blocks first .. first + n - 1 (their keys already in block_keys) enter the hash table; the block count becomes first + n
__global__ void __launch_bounds__(256) k_esdf_adopt(u64* __restrict__ ht_keys, u32* __restrict__ ht_vals, u32 ht_mask, const u64* __restrict__ block_keys, u32 first,
                                                    u32 n, u32* __restrict__ d_nblocks, u32* __restrict__ d_err) {
  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *d_nblocks = first + n;
  if (i >= n) return;
  bool fresh;
  const u32 slot = ht_insert(ht_keys, ht_mask, block_keys[first + i], &fresh);
  if (slot == kInvalid) {
    atomicOr(d_err, kErrTable);
    return;
  }
  ht_vals[slot] = first + i;
}
// the 27-neighbour rows of the new blocks, and the new blocks' entries in the rows of the blocks around them
__global__ void __launch_bounds__(256) k_esdf_link(const u64* __restrict__ ht_keys, const u32* __restrict__ ht_vals, u32 ht_mask,
                                                   const u64* __restrict__ block_keys, u32 first, u32 n, u32* __restrict__ nbr) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 27u) return;
  const u32 pool = first + t / 27u, j = t % 27u;
  int bx, by, bz;
  unpack_key(block_keys[pool], &bx, &by, &bz);
  const int x = bx + static_cast<int>(j % 3u) - 1, y = by + static_cast<int>((j / 3u) % 3u) - 1, z = bz + static_cast<int>(j / 9u) - 1;
  u32 p = kInvalid;
  if (j == 13u) {
    p = pool;
  } else if (x >= -kIdxBias && x < kIdxBias && y >= -kIdxBias && y < kIdxBias && z >= -kIdxBias && z < kIdxBias) {
    const u32 slot = ht_find(ht_keys, ht_mask, pack_key(x, y, z));
    if (slot != kInvalid) p = ht_vals[slot];
  }
  nbr[pool * 27u + j] = p;
  if (p != kInvalid && j != 13u) nbr[p * 27u + (26u - j)] = pool;  // seen from there, this block lies the opposite way
}

// ---- classify ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_esdf_classify(const u32* __restrict__ tsdf, u32* __restrict__ esdf, float min_weight, float min_distance,
                                                       float default_distance, u32* __restrict__ touched, u32* __restrict__ ctl) {
  __shared__ u32 n_changed;
  if (threadIdx.x == 0) n_changed = 0;
  __syncthreads();
  const u32 pool = blockIdx.x;
  const u32* tb = tsdf + static_cast<size_t>(pool) * kBlockWords;
  u32* eb = esdf + static_cast<size_t>(pool) * kBlockWords;
  u32 mine = 0;
  for (u32 v = threadIdx.x; v < kVoxelsPerBlock; v += 256) {
    const float d = __uint_as_float(tb[3 * v]), w = __uint_as_float(tb[3 * v + 1]);
    const u32 s0 = eb[3 * v], s1 = eb[3 * v + 1], s2 = eb[3 * v + 2];
    float ed, ew;
    u32 flags;
    esdf_init_voxel(d, w, min_weight, min_distance, default_distance, &ed, &ew, &flags);
    if (ew != 0.0f && flags == 0) {  // free now: keeps what it had if it was free before, on the same side
      const float stored = __uint_as_float(s0);
      const bool was_free = __uint_as_float(s1) > 0.0f && s2 == 0;
      if (was_free && ((stored > 0.0f) == (d > 0.0f))) ed = stored;
    }
    const u32 n0 = __float_as_uint(ed), n1 = __float_as_uint(ew);
    if (n0 != s0 || n1 != s1 || flags != s2) {
      eb[3 * v] = n0;
      eb[3 * v + 1] = n1;
      eb[3 * v + 2] = flags;
      ++mine;
    }
  }
  if (mine) atomicAdd(&n_changed, mine);
  __syncthreads();
  if (threadIdx.x == 0 && n_changed) {
    touched[pool] = 1;
    atomicAdd(&ctl[kCtlDirty], 1u);
    atomicAdd(reinterpret_cast<ull*>(&ctl[kCtlChanged]), static_cast<ull>(n_changed));
  }
}

// every block around a touched block (itself included) is active
__global__ void __launch_bounds__(256) k_esdf_activate(const u32* __restrict__ touched, const u32* __restrict__ nbr, u32 nb, u32* __restrict__ act) {
  const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nb * 27u) return;
  if (!touched[t / 27u]) return;
  const u32 p = nbr[t];
  if (p != kInvalid) act[p] = 1;
}

// ---- raise and lower -----------------------------------------------------------------------------------------------
struct SweepArgs {
  u32* voxels;
  const u32* nbr;
  u32* act_cur;
  u32* act_next;
  u32* touched;
  u32* swept;
  u32* ctl;
  float s1, s2, s3, max_distance, default_distance;
  int slot;
};

// One workgroup per block.  kRaise: unsupported free voxels go back to their init value; otherwise: the batch's relaxation
// (k_esdf_sweep of cox_submap.hip), value for value.  Both work in place on the LDS tile until nothing in it moves: a raise only
// ever takes support away and a reset voxel (at +-default, the largest |d| a free voxel can hold) supports nobody, a lowering
// only ever moves values towards zero, so stale halo values and the in-place races delay and never corrupt.
template <bool kRaise>
__global__ void __launch_bounds__(256) k_esdf_pass(SweepArgs A) {
  __shared__ float dist[kEsdfHaloCells];
  __shared__ unsigned char st[kEsdfHaloCells];  // bit 0 observed, bit 1 fixed
  __shared__ u32 nb27[27];
  __shared__ u32 on, moved, moved_any, n_voxels;
  // Which cells changed in the previous in-tile iteration, one word per (y, z) row of the tile, bit x: a voxel is looked at again
  // only if a cell of its 3 x 3 x 3 surroundings changed since it was last looked at (its value depends on nothing else), so an
  // iteration costs what the wavefront touches, not the whole block.  Two buffers: one read, one written, swapped per iteration.
  __shared__ u32 rowmask[2][kEsdfHalo * kEsdfHalo];
  const u32 pool = blockIdx.x;
  if (threadIdx.x == 0) {
    on = A.act_cur[pool];
    if (on) A.act_cur[pool] = 0;  // only this workgroup reads or clears its flag in this launch
    moved_any = 0;
    n_voxels = 0;
  }
  if (threadIdx.x < 27) nb27[threadIdx.x] = A.nbr[pool * 27u + threadIdx.x];
  __syncthreads();
  if (!on) return;
  if (threadIdx.x == 0) {
    atomicAdd(&A.ctl[kCtlSweepActive + A.slot], 1u);
    if (atomicExch(&A.swept[pool], 1u) == 0u) atomicAdd(&A.ctl[kCtlSwept], 1u);
  }
  for (u32 c = threadIdx.x; c < kEsdfHaloCells; c += 256) {
    const int hx = static_cast<int>(c % kEsdfHalo) - 1, hy = static_cast<int>((c / kEsdfHalo) % kEsdfHalo) - 1, hz = static_cast<int>(c / (kEsdfHalo * kEsdfHalo)) - 1;
    const int jx = hx < 0 ? 0 : (hx > 15 ? 2 : 1), jy = hy < 0 ? 0 : (hy > 15 ? 2 : 1), jz = hz < 0 ? 0 : (hz > 15 ? 2 : 1);
    const u32 p = nb27[jx + 3 * jy + 9 * jz];
    float d = 0.0f;
    unsigned char s = 0;
    if (p != kInvalid) {
      const u32 lin = static_cast<u32>(hx & 15) | (static_cast<u32>(hy & 15) << 4) | (static_cast<u32>(hz & 15) << 8);
      const u32* vw = A.voxels + (static_cast<size_t>(p) * kVoxelsPerBlock + lin) * kWordsPerVoxel;
      d = __hip_atomic_load(reinterpret_cast<const float*>(vw), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__uint_as_float(vw[1]) > 0.0f) s = 1 | ((vw[2] & kEsdfFixedFlag) ? 2 : 0);
    }
    dist[c] = d;
    st[c] = s;
  }
  for (int iter = 0; iter < 64; ++iter) {
    const u32* cur = rowmask[iter & 1];
    u32* nxt = rowmask[(iter & 1) ^ 1];  // read by the iteration before this one, which every thread has left
    if (threadIdx.x == 0) moved = 0;
    for (u32 r = threadIdx.x; r < kEsdfHalo * kEsdfHalo; r += 256) nxt[r] = 0;
    __syncthreads();
    bool any = false;
    for (u32 v = threadIdx.x; v < kVoxelsPerBlock; v += 256) {
      const int x = static_cast<int>(v & 15u) + 1, y = static_cast<int>((v >> 4) & 15u) + 1, z = static_cast<int>(v >> 8) + 1;
      const int row = y + kEsdfHalo * z;
      const int c = x + kEsdfHalo * row;
      if (st[c] != 1) continue;  // unobserved or fixed
      if (iter > 0) {            // the first iteration looks at everything
        u32 m = 0;
#pragma unroll
        for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
          for (int dy = -1; dy <= 1; ++dy) m |= cur[row + dy + kEsdfHalo * dz];
        if (!((m >> (x - 1)) & 7u)) continue;  // bits x - 1 .. x + 1
      }
      const float mine = dist[c];
      if (kRaise) {
        const float init = esdf_free_init(mine, A.default_distance);
        if (mine == init) continue;
        const bool supported = esdf_supported(dist, st, c, mine, A.s1, A.s2, A.s3, A.max_distance);
        if (!supported) {
          dist[c] = init;
          atomicOr(&nxt[row], 1u << x);
          any = true;
        }
      } else {
        const float now = esdf_relax_voxel(dist, st, c, mine, A.s1, A.s2, A.s3, A.max_distance);
        if (now != mine) {
          dist[c] = now;
          atomicOr(&nxt[row], 1u << x);
          any = true;
        }
      }
    }
    if (any) moved = 1;
    __syncthreads();
    const bool go = moved != 0;
    if (go && threadIdx.x == 0) moved_any = 1;
    __syncthreads();
    if (!go) break;
  }
  if (!moved_any) return;
  u32* blk = A.voxels + static_cast<size_t>(pool) * kBlockWords;
  u32 mine_n = 0;
  for (u32 v = threadIdx.x; v < kVoxelsPerBlock; v += 256) {
    const int x = static_cast<int>(v & 15u) + 1, y = static_cast<int>((v >> 4) & 15u) + 1, z = static_cast<int>(v >> 8) + 1;
    const int c = x + kEsdfHalo * (y + kEsdfHalo * z);
    if (st[c] != 1) continue;
    const u32 now = __float_as_uint(dist[c]);
    if (blk[3 * v] != now) {  // nobody else writes this block
      __hip_atomic_store(reinterpret_cast<float*>(&blk[3 * v]), dist[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ++mine_n;
    }
  }
  if (mine_n) atomicAdd(&n_voxels, mine_n);
  // the tile may have stopped at the iteration cap, so the block itself stays active as well
  if (threadIdx.x < 27 && nb27[threadIdx.x] != kInvalid) A.act_next[nb27[threadIdx.x]] = 1;
  __syncthreads();
  if (threadIdx.x == 0) {
    A.touched[pool] = 1;
    atomicAdd(&A.ctl[kCtlSweepChanged + A.slot], 1u);
    atomicAdd(reinterpret_cast<ull*>(&A.ctl[kRaise ? kCtlReset : kCtlChanged]), static_cast<ull>(n_voxels));
  }
}

}  // namespace

struct cox_esdf {
  cox_layer* tsdf = nullptr;
  cox_layer* E = nullptr;
  int device = 0;      // the TSDF's; kept here so that destroying the handle never reads the TSDF
  cox_esdf_config cfg{};
  Stream stream;
  bool valid = false;  // E mirrors the first nb pool blocks of the TSDF and is the fixed point of what the last update saw
  u32 nb = 0;          // blocks mirrored
  u32 hi = 0;          // pool blocks of E that may hold anything but zeros
  u32 frame_id = 0;    // the TSDF's frame counter at the last update (cox_layer_clear takes it back to zero)
  u64 cap = 0;         // blocks the arrays below are sized for (E's capacity)
  DevBuf<u32> d_nbr;  // [cap][27]
  DevBuf<u32> d_act[2];
  DevBuf<u32> d_touched;  // classify or raise changed the block in this update
  DevBuf<u32> d_swept;
  DevBuf<u32> d_ctl;     // kCtlWords
  PinnedBuf<u32> h_ctl;  // kHostWords
};

namespace {

int grow_arrays(cox_esdf* H) {
  const u64 cap = H->E->capacity;
  if (cap <= H->cap && H->d_nbr) return COX_OK;
  // the new set; after the swaps these hold the old one, which goes with them
  DevBuf<u32> nbr, a0, a1, touched, swept;
  bool ok = nbr.alloc(27 * cap) == COX_OK && a0.alloc(cap) == COX_OK && a1.alloc(cap) == COX_OK && touched.alloc(cap) == COX_OK && swept.alloc(cap) == COX_OK;
  if (ok && H->d_nbr && H->nb) ok = cox_hip_status(hipMemcpy(nbr, H->d_nbr, sizeof(u32) * 27 * H->nb, hipMemcpyDeviceToDevice)) == COX_OK;
  if (!ok) return COX_ERR_OUT_OF_MEMORY;
  H->d_nbr.swap(nbr), H->d_act[0].swap(a0), H->d_act[1].swap(a1), H->d_touched.swap(touched), H->d_swept.swap(swept);
  H->cap = cap;
  return COX_OK;
}

// control words -> host; everything enqueued on the stream so far has run when this returns
int read_ctl(cox_esdf* H) {
  COX_HIP(hipMemcpyAsync(H->h_ctl, H->d_ctl, sizeof(u32) * kCtlWords, hipMemcpyDeviceToHost, H->stream));
  COX_HIP(hipStreamSynchronize(H->stream));
  return COX_OK;
}

// raise or lower to convergence, from the blocks around the touched ones
template <bool kRaise>
int run_phase(cox_esdf* H, u32 nb, uint64_t* n_sweeps) {
  cox_layer* E = H->E;
  hipStream_t s = H->stream;
  COX_HIP(hipMemsetAsync(H->d_act[0], 0, sizeof(u32) * H->cap, s));
  COX_HIP(hipMemsetAsync(H->d_act[1], 0, sizeof(u32) * H->cap, s));
  hipLaunchKernelGGL(k_esdf_activate, dim3((27u * nb + 255) / 256), dim3(256), 0, s, H->d_touched, H->d_nbr, nb, H->d_act[0]);
  const float vs = E->voxel_size;
  SweepArgs A{E->voxels, H->d_nbr, nullptr, nullptr, H->d_touched, H->d_swept, H->d_ctl, 1.0f * vs, std::sqrt(2.0f) * vs, std::sqrt(3.0f) * vs,
              H->cfg.max_distance_m, H->cfg.default_distance_m, 0};
  // as the batch: a sweep moves the wavefront at least one block further
  const int max_sweeps = 8 + 4 * static_cast<int>(std::ceil(H->cfg.max_distance_m / E->block_size)) + 4096;
  int parity = 0;
  for (int done = 0; done < max_sweeps; done += kSweepsPerRead) {
    COX_HIP(hipMemsetAsync(H->d_ctl + kCtlSweepChanged, 0, sizeof(u32) * 2 * kSweepsPerRead, s));
    for (int k = 0; k < kSweepsPerRead; ++k) {
      A.act_cur = H->d_act[parity], A.act_next = H->d_act[parity ^ 1], A.slot = k;
      hipLaunchKernelGGL(k_esdf_pass<kRaise>, dim3(nb), dim3(256), 0, s, A);
      parity ^= 1;
    }
    COX_HIP(hipGetLastError());
    COX_TRY(read_ctl(H));
    for (int k = 0; k < kSweepsPerRead; ++k) {
      if (H->h_ctl.p[kCtlSweepActive + k]) *n_sweeps += 1;
      if (H->h_ctl.p[kCtlSweepChanged + k] == 0) return COX_OK;  // nothing moved: nothing is active after it
    }
  }
  return COX_ERR_INTERNAL;
}

int update_impl(cox_esdf* H, cox_esdf_update_stats* st) {
  cox_layer* T = H->tsdf;
  cox_layer* E = H->E;
  COX_HIP(hipSetDevice(T->device));
  // a projective integrator may still owe the layer a frame it has to redo (cox_layer_order_writer does the same for a writer)
  if (T->settle_writer && T->settle_ctx == T->last_writer) T->settle_writer(T->settle_ctx);
  hipStream_t s = H->stream;
  cox_layer_wait_writes(T, s);  // frames still in flight on the TSDF
  // 1. mirror the blocks
  COX_HIP(hipMemsetAsync(H->d_ctl, 0, sizeof(u32) * kCtlWords, s));
  const bool was_valid = H->valid;
  H->valid = false;  // until this update has come through
  if (was_valid && H->nb)  // H->nb <= the TSDF's capacity, which never shrinks
    hipLaunchKernelGGL(k_esdf_keys_differ, dim3((H->nb + 255) / 256), dim3(256), 0, s, T->block_keys, E->block_keys, H->nb, H->d_ctl + kCtlMismatch);
  COX_HIP(hipMemcpyAsync(H->h_ctl + kHostNb, T->d_nblocks, sizeof(u32), hipMemcpyDeviceToHost, s));
  COX_HIP(hipMemcpyAsync(H->h_ctl + kHostErr, T->d_err, sizeof(u32), hipMemcpyDeviceToHost, s));
  COX_TRY(read_ctl(H));
  if (H->h_ctl.p[kHostErr]) return err_bits_to_status(H->h_ctl.p[kHostErr]);  // as cox_esdf_from_tsdf: no ESDF of a layer in error
  const u32 nb = static_cast<u32>(std::min<u64>(H->h_ctl.p[kHostNb], T->capacity));
  const bool rebuild = !was_valid || nb < H->nb || H->h_ctl.p[kCtlMismatch] != 0 || T->frame_id < H->frame_id;
  H->frame_id = T->frame_id;
  if (rebuild) {
    COX_HIP(hipMemsetAsync(E->ht_keys, 0xFF, sizeof(u64) * E->ht_cap, s));
    COX_HIP(hipMemsetAsync(E->ht_vals, 0xFF, sizeof(u32) * E->ht_cap, s));
    if (H->hi) COX_HIP(hipMemsetAsync(E->voxels, 0, sizeof(u32) * kBlockWords * H->hi, s));
    COX_HIP(hipMemsetAsync(E->d_nblocks, 0, sizeof(u32), s));
    COX_HIP(hipStreamSynchronize(s));
    *E->h_nblocks = 0;
    H->nb = 0;
    H->hi = 0;
  }
  if (nb > E->capacity) {  // the pool follows the TSDF's: doubled, like the TSDF's own
    const u64 want = std::min<u64>(std::max<u64>(2 * E->capacity, nb), std::max<u64>(T->capacity, nb));
    COX_TRY(cox_internal_layer_reserve(E, want));  // device-wide sync; keeps blocks, keys and count
  }
  COX_TRY(grow_arrays(H));
  COX_HIP(hipMemsetAsync(H->d_touched, 0, sizeof(u32) * H->cap, s));
  COX_HIP(hipMemsetAsync(H->d_swept, 0, sizeof(u32) * H->cap, s));
  const u32 n_new = nb - H->nb;
  if (n_new) {
    H->hi = std::max(H->hi, nb);
    COX_HIP(hipMemcpyAsync(E->block_keys + H->nb, T->block_keys + H->nb, sizeof(u64) * n_new, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_esdf_adopt, dim3((n_new + 255) / 256), dim3(256), 0, s, E->ht_keys, E->ht_vals, E->ht_cap - 1, E->block_keys, H->nb, n_new,
                       E->d_nblocks, E->d_err);
    hipLaunchKernelGGL(k_esdf_link, dim3((27u * n_new + 255) / 256), dim3(256), 0, s, E->ht_keys, E->ht_vals, E->ht_cap - 1, E->block_keys, H->nb, n_new,
                       H->d_nbr);
    *E->h_nblocks = nb;
    H->nb = nb;
  }
  st->n_blocks = nb;
  st->n_new_blocks = n_new;
  st->rebuilt = rebuild ? 1u : 0u;
  if (nb == 0) {
    COX_HIP(hipStreamSynchronize(s));
    H->valid = true;
    return COX_OK;
  }
  // 2. classify every block by content
  hipLaunchKernelGGL(k_esdf_classify, dim3(nb), dim3(256), 0, s, T->voxels, E->voxels, H->cfg.min_weight, H->cfg.min_distance_m, H->cfg.default_distance_m,
                     H->d_touched, H->d_ctl);
  COX_HIP(hipGetLastError());
  COX_TRY(read_ctl(H));
  st->n_dirty_blocks = H->h_ctl.p[kCtlDirty];
  if (st->n_dirty_blocks) {
    // 3. raise (an ESDF that started empty holds init values only: nothing to raise), then 4. lower
    if (!rebuild) COX_TRY(run_phase<true>(H, nb, &st->n_raise_sweeps));
    COX_TRY(run_phase<false>(H, nb, &st->n_lower_sweeps));
  }
  ull v64[2];
  memcpy(v64, H->h_ctl + kCtlReset, sizeof(v64));  // reset, changed
  st->n_reset_voxels = v64[0];
  st->n_changed_voxels = v64[1];
  st->n_swept_blocks = H->h_ctl.p[kCtlSwept];
  u32 err = 0;
  COX_HIP(hipMemcpyAsync(H->h_ctl + kHostErr, E->d_err, sizeof(u32), hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  err = H->h_ctl.p[kHostErr];
  if (err) return err_bits_to_status(err);
  H->valid = true;
  return COX_OK;
}

}  // namespace

extern "C" {

int cox_esdf_create(cox_layer_t* tsdf, const cox_esdf_config* cfg_in, cox_esdf_t** out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!tsdf || !out) return COX_ERR_INVALID_ARG;
  cox_esdf_config cfg;
  if (cfg_in)
    cfg = *cfg_in;
  else
    cox_esdf_config_default(&cfg);
  if (!(cfg.max_distance_m > 0.0f) || !(cfg.min_distance_m > 0.0f) || !(cfg.default_distance_m > 0.0f)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(tsdf->device));
  cox_esdf* H = new (std::nothrow) cox_esdf();
  if (!H) return COX_ERR_OUT_OF_MEMORY;
  H->tsdf = tsdf;
  H->device = tsdf->device;
  H->cfg = cfg;
  int st = cox_layer_create(tsdf->voxel_size, kVps, tsdf->device, 64, &H->E);
  if (st == COX_OK) st = grow_arrays(H);
  if (st == COX_OK) {
    if (H->stream.create() != COX_OK || H->d_ctl.alloc(kCtlWords) != COX_OK || H->h_ctl.alloc(kHostWords) != COX_OK) st = COX_ERR_NO_DEVICE;
  }
  if (st != COX_OK) {
    cox_esdf_destroy(H);
    return st;
  }
  memset(H->h_ctl, 0, sizeof(u32) * kHostWords);
  *out = H;
  return COX_OK;
}

void cox_esdf_destroy(cox_esdf_t* H) {
  if (!H) return;
  (void)hipSetDevice(H->device);
  if (H->stream) (void)hipStreamSynchronize(H->stream);
  if (H->E) cox_layer_destroy(H->E);
  delete H;
}

int cox_esdf_update(cox_esdf_t* H, cox_esdf_update_stats* stats) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  const auto t0 = std::chrono::steady_clock::now();
  cox_esdf_update_stats st{};
  const int rc = update_impl(H, &st);
  st.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (stats) *stats = st;
  return rc;
}

int cox_esdf_layer(cox_esdf_t* H, cox_layer_t** layer) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !layer) return COX_ERR_INVALID_ARG;
  *layer = H->E;
  return COX_OK;
}

int cox_esdf_invalidate(cox_esdf_t* H) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  H->valid = false;
  return COX_OK;
}

}  // extern "C"
