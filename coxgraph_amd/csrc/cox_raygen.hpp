// Ray generation (stages H, P, M): one ray per point (simple), or points bundled by terminal voxel and merged by the sequential
// weighted mean (merged: frame hash, sort keys + bundle boundaries, merge) -- part of cox_integrator.hip (included there, in this
// order: the kernels use what is defined above them in that file).
#pragma once

// ---- simple: one ray per point, ray id = mixed-order sequence number --------------------------
__global__ void __launch_bounds__(256) k_rays_simple(const FrameParams* __restrict__ Pp, RayArrays R,
                                                     Counters* cnt) {
  const FrameParams P = *Pp;
  const u32 seq = blockIdx.x * blockDim.x + threadIdx.x;
  if (seq == 0) cnt->n_ray_slots = P.n_points;
  if (seq >= P.n_points) return;
  const u32 idx = mixed_index(seq, P.n_points);
  const F3 p{P.xyz[3 * idx], P.xyz[3 * idx + 1], P.xyz[3 * idx + 2]};
  bool clearing = false;
  const bool valid = point_valid(P, p, &clearing);
  u32 nsteps = 0, flags = 0;
  if (valid) {
    const F3 pg = transform_point(P, p);
    Dda d;
    dda_setup(d, P, pg, clearing);
    if (d.range_error) atomicOr(&cnt->err, kErrRange);
    nsteps = d.nsteps;
    flags = 1u | (clearing ? 2u : 0u);
    R.px[seq] = pg.x;
    R.py[seq] = pg.y;
    R.pz[seq] = pg.z;
    R.w[seq] = voxel_weight(P, p);
    R.color[seq] = pack_rgba_wire(P.rgba, idx);
  }
  R.flags[seq] = flags;
  R.nsteps[seq] = nsteps;
  const u64 m = __ballot(valid);
  if (lane_id() == 0 && m) {
    u32* sh = cnt->shard[(seq >> 6) & 63u];
    atomicAdd(&sh[kShValid], static_cast<u32>(__popcll(m)));
    atomicAdd(&sh[kShRays], static_cast<u32>(__popcll(m)));
  }
}

// ---- merged: bundle points by terminal voxel ---------------------------------------------------
// thread = point (so neighbouring lanes are neighbouring pixels and mostly share a terminal voxel): the lanes of a
// wave that hold the same key elect one leader, which inserts the key in the per-frame hash once and records the
// smallest sequence number of the group as a candidate for the bundle's first visit.
// First kernel of a frame: with by_value the frame's parameter block arrives as a kernel argument and workgroup 0
// stores it for the kernels that follow (saves the 4 us H2D blit per frame); captured stage graphs keep the copy.
// n_dev (by_value only): the frame's point count is still on the device (depth front end): every workgroup takes it from there.
__device__ __forceinline__ u32 pow2_above(u32 n) {  // power of two > n (FrameParams::np2)
  u32 p = 1;
  while (p <= n && p < 0x80000000u) p <<= 1;
  return p;
}
__global__ void __launch_bounds__(256) k_bundle_insert(FrameParams* __restrict__ Pp, FrameParams Pv, int by_value, const u32* __restrict__ n_dev, u64* __restrict__ fh_keys,
                                                       u32* __restrict__ fh_first, u32 fh_mask, u32* __restrict__ pslot, Counters* cnt) {
  // (the count is taken into a scalar of its own: writing it into the by-value parameter struct sends the whole struct through
  // scratch memory -- 42 MB of writes and 11 us per launch, seen in the PMC pass)
  const FrameParams P = by_value ? Pv : *Pp;
  const u32 n_points = (by_value && n_dev) ? min(*n_dev, P.n_points) : P.n_points;
  if (by_value && blockIdx.x == 0 && threadIdx.x == 0) {
    *Pp = Pv;
    if (n_dev) {
      Pp->n_points = n_points;
      Pp->np2 = pow2_above(n_points);
    }
  }
  const u32 idx = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 lane = lane_id();
  bool valid = false;
  u64 key = 0;
  u32 seq = kInvalid;
  if (idx < n_points) {
    seq = mixed_sequence(idx, n_points);
    const F3 p{P.xyz[3 * idx], P.xyz[3 * idx + 1], P.xyz[3 * idx + 2]};
    bool clearing = false;
    valid = point_valid(P, p, &clearing);
    if (valid) {
      const F3 pg = transform_point(P, p);
      const float sx = pg.x * P.voxel_size_inv, sy = pg.y * P.voxel_size_inv, sz = pg.z * P.voxel_size_inv;
      if (!(index_in_range(sx) && index_in_range(sy) && index_in_range(sz))) {  // also catches NaN
        atomicOr(&cnt->err, kErrRange);
        valid = false;
      } else {
        key = pack_key(grid_index(sx), grid_index(sy), grid_index(sz)) | (clearing ? (1ull << 63) : 0ull);
      }
    }
  }
  // group the lanes by key (ALU only), then let all group leaders touch memory at the same time
  u32 my_leader = lane, group_min = kInvalid;
  bool is_leader = false;
  u64 todo = __ballot(valid);
  while (todo) {
    const u32 leader = static_cast<u32>(__ffsll(static_cast<long long>(todo))) - 1u;
    const u64 k = (static_cast<u64>(static_cast<u32>(__builtin_amdgcn_readlane(static_cast<u32>(key >> 32), leader))) << 32) |
                  static_cast<u64>(static_cast<u32>(__builtin_amdgcn_readlane(static_cast<u32>(key), leader)));
    const bool mine = valid && key == k;
    const u64 peers = __ballot(mine);
    u32 mn = mine ? seq : kInvalid;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mn = min(mn, static_cast<u32>(__shfl_xor(static_cast<int>(mn), off, 64)));
    if (mine) my_leader = leader;
    if (lane == leader) {
      is_leader = true;
      group_min = mn;
    }
    todo &= ~peers;
  }
  u32 sl = kInvalid;
  if (is_leader) {
    bool fresh;
    sl = ht_insert(fh_keys, fh_mask, key, &fresh);
    if (sl == kInvalid)
      atomicOr(&cnt->err, kErrTable);
    else if (__hip_atomic_load(&fh_first[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > group_min)
      atomicMin(&fh_first[sl], group_min);  // a stale (larger) value read above only costs this atomic
  }
  const u32 got = static_cast<u32>(__shfl(static_cast<int>(sl), static_cast<int>(my_leader), 64));
  const u32 slot = valid ? got : kInvalid;
  if (idx < n_points) pslot[idx] = slot;  // kInvalid for points that are not integrated; indexed by point (coalesced)
  const u64 m = __ballot(valid && slot != kInvalid);
  if (lane == 0 && m) atomicAdd(&cnt->shard[(idx >> 6) & 63u][kShValid], static_cast<u32>(__popcll(m)));
}
// the same for the frames whose parameter block is uploaded by a copy (simple, fast, captured stage graphs): one thread patches it
__global__ void k_params_count(FrameParams* __restrict__ Pp, const u32* __restrict__ n_dev) {
  const u32 n = min(*n_dev, Pp->n_points);
  Pp->n_points = n;
  Pp->np2 = pow2_above(n);
}
// sort key of a point = (clearing ? np2 : 0) + first sequence number of its bundle; value = seq.  Also publishes the
// key width of the bundling sort.
//
// Everything the frame needs to know about bundle boundaries is known HERE, before the sort.  A point is the HEAD of its bundle
// when it is the bundle's first visit: fh_first[slot] == seq, i.e. (key & (np2 - 1)) == value -- a property of the pair, which
// the sort carries along.  The sort is stable and a bundle's points share one key, so the head is also the bundle's first element
// in sorted order.  The bundle's ordinal is the number of heads with a smaller key = heads of the non-clearing class first, then
// the clearing ones, each class in sequence order: a prefix count over head flags in SEQUENCE order, which needs nothing from the
// sorted array.  So one workgroup per tile of kHeadTile consecutive sequence numbers writes
//   hrank[seq]            for a head: its exclusive rank among the heads of its class inside the tile
//   tile_heads[tile][4]   heads of the non-clearing class, heads of the clearing class, valid points, (unused)
// and the scatter kernel of the sort's last pass turns them into bstart[] (BundleBounds below) at the moment it places the head.
// The tile is also the radix sort's tile (while rs_tile_shift == 0, which the host checks): with `counts` given, the workgroup
// leaves counts[tile][digit] and the digit totals of the sort's pass 0 exactly as k_rs_hist<11> would, and that launch is skipped.
constexpr u32 kHeadTile = kRsTile;
constexpr u32 kHeadTileShift = 11;
static_assert((1u << kHeadTileShift) == kHeadTile, "kHeadTile");
constexpr u32 kKeysThreads = 1024;  // 2 rounds of dependent gathers (pslot -> fh_first, fh_keys) per thread: with 256 threads the 8 rounds were 13 us
constexpr u32 kKeysWaves = kKeysThreads / 64;
constexpr u32 kHeadRounds = kHeadTile / kKeysThreads;
__global__ void __launch_bounds__(kKeysThreads) k_bundle_keys(const FrameParams* __restrict__ Pp, const u64* __restrict__ fh_keys, const u32* __restrict__ fh_first,
                                                     const u32* __restrict__ pslot, u32* __restrict__ skey, u32* __restrict__ sval, u32* __restrict__ hrank,
                                                     u32* __restrict__ tile_heads, SortInfo* sort_info, u32* __restrict__ counts /* or nullptr */,
                                                     u32* __restrict__ totals) {
  __shared__ u32 h[1u << 11];
  __shared__ u32 wcnt[kHeadRounds][kKeysWaves];  // per (round, wave): heads of either class and valid points, 8 bits each
  const u32 n = Pp->n_points, np2 = Pp->np2;
  u32 nbits = 1;  // clearing bit + log2(np2); kInvalid's low bits exceed every valid key
  while ((1u << (nbits - 1)) < np2) ++nbits;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    sort_info->nbits = nbits;
    sort_info->parity = 0;
    sort_info->base = 0;
  }
  const u32 tile = blockIdx.x;
  if (tile * kHeadTile >= n) return;
  int shift;
  u32 dbits;
  (void)rs_pass_digits<11>(nbits, 0, &shift, &dbits);  // pass 0: shift 0
  const u32 kDigits = 1u << dbits;
  if (counts) {
    for (u32 d = threadIdx.x; d < kDigits; d += kKeysThreads) h[d] = 0;
    __syncthreads();
  }
  const u32 lane = lane_id(), wave = threadIdx.x >> 6;
  const u64 lower = (1ull << lane) - 1ull;
  u32 rank_in_wave[kHeadRounds];
  u32 head_mask = 0, clr_mask = 0;
#pragma unroll
  for (u32 q = 0; q < kHeadRounds; ++q) {  // sequence order inside the tile = (round, wave, lane)
    const u32 seq = tile * kHeadTile + q * kKeysThreads + threadIdx.x;
    u32 slot = kInvalid;
    if (seq < n) slot = pslot[mixed_index(seq, n)];  // the bundling sort starts from visiting order: gather on the read side
    u32 k = kInvalid;
    bool head = false, clr = false;
    if (slot != kInvalid) {
      const u32 first = fh_first[slot];
      clr = (fh_keys[slot] >> 63) != 0;
      k = first + (clr ? np2 : 0u);
      head = first == seq;
    }
    if (seq < n) {
      skey[seq] = k;
      sval[seq] = seq;
      if (counts) atomicAdd(&h[(k >> shift) & (kDigits - 1)], 1u);
    }
    const u64 b0 = __ballot(head && !clr), b1 = __ballot(head && clr), bv = __ballot(slot != kInvalid);
    rank_in_wave[q] = static_cast<u32>(__popcll((clr ? b1 : b0) & lower));
    head_mask |= (head ? 1u : 0u) << q;
    clr_mask |= (clr ? 1u : 0u) << q;
    if (lane == 0) wcnt[q][wave] = static_cast<u32>(__popcll(b0)) | (static_cast<u32>(__popcll(b1)) << 8) | (static_cast<u32>(__popcll(bv)) << 16);
  }
  __syncthreads();
  u32 run0 = 0, run1 = 0, runv = 0;
#pragma unroll
  for (u32 q = 0; q < kHeadRounds; ++q) {
#pragma unroll
    for (u32 w = 0; w < kKeysWaves; ++w) {
      if (w == wave && ((head_mask >> q) & 1u)) hrank[tile * kHeadTile + q * kKeysThreads + threadIdx.x] = (((clr_mask >> q) & 1u) ? run1 : run0) + rank_in_wave[q];
      const u32 c = wcnt[q][w];
      run0 += c & 255u;
      run1 += (c >> 8) & 255u;
      runv += c >> 16;
    }
  }
  if (threadIdx.x == 0) {
    tile_heads[4 * tile + 0] = run0;
    tile_heads[4 * tile + 1] = run1;
    tile_heads[4 * tile + 2] = runv;
  }
  if (counts) {
    for (u32 d = threadIdx.x; d < kDigits; d += kKeysThreads) {
      const u32 c = h[d];
      counts[static_cast<size_t>(tile) * kDigits + d] = c;  // the layout of k_rs_hist
      if (c) atomicAdd(&totals[d], c);
    }
  }
}
// the two ping-pong buffers of the bundling sort + where its result ended up
struct BundleView {
  const u32* key[2];
  const u32* val[2];
  const SortInfo* info;
};
// Hook of the bundling sort's scatter kernel (cox_sort.hpp: RsNoHook), active in the sort's last pass: the position at which a head
// is placed is the start of its bundle, and its ordinal = (heads of the classes before its own) + (heads of its class in the tiles
// before its own) + (its rank inside the tile).  Every workgroup adds the tile counts up itself (a frame has ~150 tiles; no ticket,
// no flag between workgroups); workgroup 0 publishes the totals -- also for an empty frame.  The prefixes of the first kHeadLdsTiles
// tiles (4 M points) sit in LDS; a head of a later tile adds the remaining counts up from memory.
// The frame hash is sized for "every point its own bundle" (6 MB) but a frame fills a few thousand slots: instead of a memset per
// frame, the slots the frame used are put back to empty once its keys have been read -- here, once per bundle, by its head (round 3
// did it per point behind the sort, round 2 had a launch of its own for it right behind k_bundle_keys).
constexpr u32 kHeadLdsTiles = 2048;
struct BundleBounds {
  static constexpr bool kActive = true;
  static constexpr u32 kLdsWords = 2 * kHeadLdsTiles + 8;
  const FrameParams* Pp;
  const u32* tile_heads;
  const u32* hrank;
  const u32* pslot;
  u32* bstart;
  Counters* cnt;
  u64* fh_keys;  // self clean-up of the frame hash; nullptr: the frame does not clean up after itself (anti-grazing)
  u32* fh_first;
  u32 fh_mask;
  __device__ __forceinline__ void begin(u32 n, u32* lds) const {
    u32* scratch = lds + 2 * kHeadLdsTiles;
    const u32 n_tiles = (n + kHeadTile - 1) / kHeadTile;
    u32 carry = 0;
    for (u32 cls = 0; cls < 2; ++cls) {  // the clearing class goes on where the non-clearing one ends
      for (u32 b = 0; b < n_tiles; b += 256) {
        const u32 t = b + threadIdx.x;
        const u32 v = (t < n_tiles) ? tile_heads[4 * t + cls] : 0u;
        u32 tot;
        const u32 ex = block_exclusive_scan<4>(v, &tot, scratch);
        if (t < n_tiles && t < kHeadLdsTiles) lds[cls * kHeadLdsTiles + t] = carry + ex;
        carry += tot;
      }
    }
    if (blockIdx.x == 0) {
      u32 v = 0;
      for (u32 t = threadIdx.x; t < n_tiles; t += 256) v += tile_heads[4 * t + 2];
      u32 n_valid;
      (void)block_exclusive_scan<4>(v, &n_valid, scratch);
      if (threadIdx.x == 0) {
        cnt->n_rays = carry;  // number of bundles
        cnt->n_ray_slots = carry;
        cnt->n_sorted_valid = n_valid;  // invalid keys sort last
      }
    }
    if (threadIdx.x == 0) {
      scratch[4] = n;
      scratch[5] = Pp->np2;
    }
    __syncthreads();
  }
  struct Fetched {
    u32 ord, slot;
  };
  __device__ __forceinline__ bool wants(u32 key, u32 val, const u32* lds) const {  // a bundle head
    const u32 np2 = lds[2 * kHeadLdsTiles + 5];
    return key != kInvalid && (key & (np2 - 1u)) == val;
  }
  __device__ __forceinline__ Fetched fetch(u32 key, u32 val, const u32* lds) const {
    const u32 n = lds[2 * kHeadLdsTiles + 4], np2 = lds[2 * kHeadLdsTiles + 5];
    const u32 cls = key >= np2 ? 1u : 0u;
    const u32 tile = val >> kHeadTileShift;
    u32 ord;
    if (tile < kHeadLdsTiles) {
      ord = lds[cls * kHeadLdsTiles + tile];
    } else {
      ord = lds[cls * kHeadLdsTiles + kHeadLdsTiles - 1];
      for (u32 t = kHeadLdsTiles - 1; t < tile; ++t) ord += tile_heads[4 * t + cls];
    }
    ord += hrank[val];
    return Fetched{ord < n ? ord : kInvalid, fh_keys ? pslot[mixed_index(val, n)] : kInvalid};
  }
  __device__ __forceinline__ void commit(const Fetched& f, u32 pos) const {
    if (f.ord != kInvalid) bstart[f.ord] = pos;
    if (f.slot <= fh_mask) {  // (kInvalid: an invalid point, or a frame that does not clean up)
      fh_keys[f.slot] = kEmptyKey;
      fh_first[f.slot] = 0xFFFFFFFFu;
    }
  }
};

// two waves per bundle: the sequential weighted mean of its points in visiting order, bit-exact with the
// single-threaded reference loop
//     merged = (merged * W + p * w) / (W + w);  colour = blend(colour, W, c, w);  W += w
// Each component is a recurrence  val <- f_k(val)  whose operands do not depend on the running value:
//     x, y, z (wave 0):     val <- (val * W_k + p * w) / (W_k + w)                   one IEEE divide per step
//     a, b, g, r (wave 1):  val <- round(val * (W_k/(W_k+w)) + c * (w/(W_k+w)))      multiply-add-round per step
// 64 points at a time are gathered in parallel and their operands are computed lane-parallel into an LDS table
// [point][component]; lanes 0-3 then carry one component each through the dependent chain with one (prefetched)
// LDS read per step and no branches.  The chain length is the bundle size, so the two chains of a big bundle run
// side by side on different SIMDs instead of back to back.  Skipped points (w < eps, or anything after the first
// point of a clearing bundle) are the identity step: (M, A, D) = (1, 0, 1).
typedef float MergeOp __attribute__((ext_vector_type(4)));  // (M, A, D, 1/D)

// Piece path (k_touch_pieces): a PIECE is a maximal run of consecutive steps of one ray inside one tile (block, z slab:
// 16 x 16 x 1 voxels) -- the voxel coordinates of a walk are monotone, so a ray meets a tile in one run of at most 31
// steps.  Pieces are written at fixed slots (exclusive scan of this bound over the rays), which keeps them in ray order
// without a sort key for it.  The wave walk starts a piece at every round of 64 steps, at every z step and at every
// change of the x / y block; its per-axis step counts are at most n_axis + 1 (wave_ray_path generates n_axis + 2 crossing
// times and rejects a walk that uses the last one).  Rays that are known here to take the sequential walk get the
// trivial bound (one piece per step); the + 4 covers a ray whose walk is only found to need the fallback later (and the
// sequential walk makes no round pieces) -- if even that is exceeded the frame is dropped and reported, never wrong.
__device__ __forceinline__ u32 piece_bound(const Dda& d, u32 axis_cap) {
  const u32 ns = d.nsteps;
  if (ns == 0) return 0;
  const u32 gen = ns + 1;
  const u32 g0 = min(d.n_axis[0] + 2, gen), g1 = min(d.n_axis[1] + 2, gen), g2 = min(d.n_axis[2] + 2, gen);
  if (d.sgn[0] == 0 || d.sgn[1] == 0 || d.sgn[2] == 0 || g0 > axis_cap || g1 > axis_cap || g2 > axis_cap || ns > 3 * axis_cap) return ns;
  const u32 b = (ns + 63) / 64 + (d.n_axis[2] + 1) + ((d.n_axis[0] + 1) / 16 + 1) + ((d.n_axis[1] + 1) / 16 + 1) + 4;
  return min(b, ns);
}

// the walk of one ray on its wave (cox_walk.hpp, which follows this file): what k_touch_wave does per ray
template <u32 kAxisCap>
__device__ void wave_touch_ray(const FrameParams& P, const RayArrays& R, const FrameBlocks& B, u32 r, u32 ns, u32 flags, Dda d, u64 own_key, float* tl, u32* path,
                               u32 lane, u32* __restrict__ park, Counters* cnt, const u64* __restrict__ fh_keys, u32 fh_mask);

// The walk placed in the merge (IntegratorPlan::touch_in_merge; small axis cap only): what the xyz wave of a bundle needs to do
// k_touch_wave<kAxisCapSmall>'s work for the ray it has just written.  The path of ray m is parked in a slot of its own,
// path[m * path_stride, + nsteps): no offset, so no scan in front of the walk.
struct MergeWalk {
  FrameBlocks blocks;
  u32* path;        // the spare record-sort buffer, rec_cap words
  u32 path_stride;  // IntegratorPlan::steps_max: no ray of the configuration has more steps
  u32 rec_cap;
  const u64* fh_keys;  // the bundle hash (anti-grazing)
  u32 fh_mask;
};

// kWalk = false is the kernel as it was (its code is unchanged by the template: pieces, the walk in stage T or in a launch of its own)
template <bool kWalk>
__global__ void __launch_bounds__(256) k_bundle_merge(const FrameParams* __restrict__ Pp, BundleView V, const u32* __restrict__ bstart, RayArrays R, Counters* cnt,
                                                      u32 piece_axis_cap, MergeWalk walk) {
  const FrameParams P = *Pp;
  const u32 np2 = P.np2;
  const float* __restrict__ xyz = P.xyz;
  const uint8_t* __restrict__ rgba = P.rgba;
  typedef const float __attribute__((address_space(1))) * GlobalF32;
  typedef const u32 __attribute__((address_space(1))) * GlobalU32;
  const GlobalF32 gxyz = (GlobalF32)xyz;  // (device memory: see the gather below)
  const GlobalU32 grgba = (GlobalU32)rgba;
  const u32 spar = uniform_u32(V.info->parity & 1u);
  const u32* __restrict__ skey = V.key[spar];
  const u32* __restrict__ sval = V.val[spar];
  __shared__ MergeOp ops[4][64][4];
  const u32 n_bundles = uniform_u32(cnt->n_rays);
  const u32 n_valid = uniform_u32(cnt->n_sorted_valid);
  const u32 tid = blockIdx.x * blockDim.x + threadIdx.x;
  const u32 nthreads = gridDim.x * blockDim.x;
  const u32 lane = lane_id();
  const u32 role = lane & 3u;
  MergeOp(*tbl)[4] = ops[threadIdx.x >> 6];
  for (u32 task = uniform_u32(tid >> 6); task < 2 * n_bundles; task += nthreads >> 6) {
    const u32 m = task >> 1;
    const bool colour_wave = (task & 1u) != 0;
    // The loads of a task in as few dependent levels as they have: both bundle starts together (the last bundle reads its own start
    // twice instead of branching around the second load), then the class of the bundle and the points of the first two chunks.
    const u32 begin = uniform_u32(bstart[m]);
    const u32 next_start = uniform_u32(bstart[min(m + 1u, n_bundles - 1u)]);
    const u32 end = (m + 1 < n_bundles) ? next_start : n_valid;
    if (colour_wave && rgba == nullptr) {  // no colours: Color() stays (0,0,0,0)
      if (lane == 0) {
        R.color[m] = 0u;
        reinterpret_cast<u32*>(R.q)[static_cast<size_t>(m) * 8u + 5u] = 0u;
      }
      continue;
    }
    // Software pipeline of the chunk loop: while the chain of chunk k runs, the points of chunk k + 1 (gathered through sv_b, which
    // arrived during chunk k - 1) and the sorted values of chunk k + 2 are in flight, so neither dependent level of the gather sits
    // between two chains.  All of it is set here, per task: nothing is carried from one task of the grid-stride loop into the next.
    // A load is issued only for i < end (never sval at or beyond end); a clearing bundle that is done drops what is in flight.
    // The gather only loads (the colour's bytes are put in wire order where it is used: an operation on the loaded value here would
    // wait for it in front of the chain), and it loads through global pointers: a pointer read from FrameParams is a generic one to
    // the compiler, and a flat load in flight makes every LDS wait of the chain a wait for that load as well.
    auto gather = [&](bool has, u32 sv, float& x, float& y, float& z, u32& c) {
      x = 0.0f;
      y = 0.0f;
      z = 0.0f;
      c = 0u;
      if (has) {
        const u32 idx = mixed_index(sv, P.n_points);
        x = gxyz[3 * idx];
        y = gxyz[3 * idx + 1];
        z = gxyz[3 * idx + 2];
        if (colour_wave) c = grgba[idx];
      }
    };
    const u32 key0 = skey[begin];
    const u32 sv_a = (begin + lane < end) ? sval[begin + lane] : 0u;
    u32 sv_b = (begin + 64u + lane < end) ? sval[begin + 64u + lane] : 0u;  // sorted values one chunk ahead of the points in flight
    float npx, npy, npz;                                                    // the next chunk's points
    u32 ncol;
    gather(begin + lane < end, sv_a, npx, npy, npz, ncol);
    const bool clearing = uniform_u32(key0) >= np2;
    if (!colour_wave && lane == 0) atomicMax(&cnt->shard[m & 63u][kShMaxBundle], end - begin);
    float val = 0.0f;  // this lane's component of the running mean / colour channel
    float W = 0.0f;    // uniform
    u64 key = 0;
    bool done = false;
    for (u32 base = begin; base < end && !done; base += 64) {
      const u32 i = base + lane;
      const u32 cnt_in = min(64u, end - base);
      const float px = npx, py = npy, pz = npz;
      const u32 col = rgba_wire_order(ncol);
      const float w = (i < end) ? voxel_weight(P, F3{px, py, pz}) : 0.0f;
      // ahead of the chain: the next chunk's points and the sorted values of the chunk behind it
      gather(i + 64u < end, sv_b, npx, npy, npz, ncol);
      sv_b = (i + 128u < end) ? sval[i + 128u] : 0u;
      if (base == begin && !colour_wave) {
        const F3 pg = transform_point(P, F3{readlane_f32(px, 0), readlane_f32(py, 0), readlane_f32(pz, 0)});
        key = pack_key(grid_index(pg.x * P.voxel_size_inv), grid_index(pg.y * P.voxel_size_inv), grid_index(pg.z * P.voxel_size_inv));
      }
      // which points take part
      bool used = (lane < cnt_in) && !(w < kEps);
      if (clearing) {  // only the first point of a clearing bundle is used
        const u64 um = __ballot(used);
        used = used && (lane == static_cast<u32>(__ffsll(static_cast<long long>(um))) - 1u);
        if (um) done = true;
      }
      // W before each point of the chunk (skipped points leave W unchanged)
      float Wpre;
      const u64 in_mask = (cnt_in == 64) ? ~0ull : ((1ull << cnt_in) - 1ull);
      if (!clearing && (__ballot(w == 1.0f) & in_mask) == in_mask && W == truncf(W) && W < 8388608.0f) {
        Wpre = W + static_cast<float>(lane);  // integers: every partial sum is exact
      } else {
        float run = W;
        Wpre = W;
        const u64 used_mask = __ballot(used);
        for (u32 k = 0; k < cnt_in; ++k) {
          if (lane == k) Wpre = run;
          const float wk = readlane_f32(w, k);
          if ((used_mask >> k) & 1ull) run += wk;
        }
      }
      const float den = Wpre + w;
      const float Wnext = used ? den : Wpre;
      const bool d_ok = !used || (den >= 9.094947e-13f && den <= 1.0995116e12f);  // divisor range of the fast division
      // operand table of this chunk; rows beyond the chunk are the identity so the chain can run in groups of 4
      {
        MergeOp* row = tbl[lane];
        const MergeOp ident{1.0f, 0.0f, 1.0f, 1.0f};
        if (!used) {
#pragma unroll
          for (u32 c = 0; c < 4; ++c) row[c] = ident;
        } else if (!colour_wave) {
          const float r0 = __builtin_amdgcn_rcpf(den);
          const float r = __builtin_fmaf(__builtin_fmaf(-den, r0, 1.0f), r0, r0);  // one Newton step: < 1 ulp from 1/den
          row[0] = MergeOp{Wpre, px * w, den, r};
          row[1] = MergeOp{Wpre, py * w, den, r};
          row[2] = MergeOp{Wpre, pz * w, den, r};
          row[3] = ident;
        } else {
          const float fa = Wpre / den, fb = w / den;  // colour blend factors of this point
#pragma unroll
          for (u32 c = 0; c < 4; ++c) row[c] = MergeOp{fa, static_cast<float>(static_cast<int>((col >> (8u * c)) & 255u)) * fb, 1.0f, 0.0f};
        }
      }
      wave_lds_handover();
      // the dependent chain
      MergeOp nxt = tbl[0][role];
      if (!colour_wave) {
        // IEEE division with everything that depends only on the divisor hoisted off the chain: r = refined 1/D sits in
        // the table; q0 = N r, then two residual corrections -- the same Newton sequence the compiler emits for '/',
        // minus its range scaling.  A correctly rounded quotient is unique, so the bits equal the oracle's '/' whenever
        // no intermediate can leave the normal range; |N| and |D| are tracked off the critical path and the chunk is
        // redone with plain '/' if they ever left [2^-40, 2^40] (or N was 0, where the sign of zero would differ).
        const float val_in = val;
        float n_lo = 1.0f, n_hi = 1.0f;
        // groups of 4 steps with the next group's operands already in flight: the LDS latency (~100 cycles) would
        // otherwise bound every step of the chain
        // Two register sets in turn (eight steps per round): the operands of one group of four are read from LDS while the other
        // group's steps run, with scheduling barriers so that the reads are issued where they are written -- left alone, the compiler
        // moves each group's first read to the top of its own steps and waits for it there (~100 cycles per four steps on the chain).
        // Rows beyond the chunk are the identity, so a trailing group of four is harmless.
        MergeOp a0 = tbl[0][role], a1 = tbl[1][role], a2 = tbl[2][role], a3 = tbl[3][role];
        // (Going on with q1 and checking off the chain that the second correction would not have changed it does not pay: one step
        // in a hundred needs that correction, so nearly every chunk of 3 x 64 steps had to be redone.)
#define COX_MERGE_STEP(op)                                  \
  {                                                         \
    const float N = val * (op).x + (op).y;                  \
    n_lo = fminf(n_lo, fabsf(N));                           \
    n_hi = fmaxf(n_hi, fabsf(N));                           \
    const float q0 = N * (op).w;                            \
    const float e0 = __builtin_fmaf(-(op).z, q0, N);        \
    const float q1 = __builtin_fmaf(e0, (op).w, q0);        \
    const float e1 = __builtin_fmaf(-(op).z, q1, N);        \
    val = __builtin_fmaf(e1, (op).w, q1);                   \
  }
        for (u32 k = 0; k < cnt_in; k += 8) {
          const u32 kb = (k + 4) & 63u;
          const MergeOp b0 = tbl[kb][role], b1 = tbl[kb + 1][role], b2 = tbl[kb + 2][role], b3 = tbl[kb + 3][role];
          __builtin_amdgcn_sched_barrier(0);
          COX_MERGE_STEP(a0)
          COX_MERGE_STEP(a1)
          COX_MERGE_STEP(a2)
          COX_MERGE_STEP(a3)
          __builtin_amdgcn_sched_barrier(0);
          const u32 ka = (k + 8) & 63u;
          a0 = tbl[ka][role];
          a1 = tbl[ka + 1][role];
          a2 = tbl[ka + 2][role];
          a3 = tbl[ka + 3][role];
          __builtin_amdgcn_sched_barrier(0);
          COX_MERGE_STEP(b0)
          COX_MERGE_STEP(b1)
          COX_MERGE_STEP(b2)
          COX_MERGE_STEP(b3)
          __builtin_amdgcn_sched_barrier(0);
        }
#undef COX_MERGE_STEP
        const bool bad = (lane < 3) && !(n_lo >= 9.094947e-13f && n_hi <= 1.0995116e12f);  // NaN fails too
        if (__ballot(bad || !d_ok)) {
          val = val_in;
          nxt = tbl[0][role];
          for (u32 k = 0; k < cnt_in; ++k) {
            const MergeOp op = nxt;
            nxt = tbl[(k + 1) & 63u][role];
            val = (val * op.x + op.y) / op.z;
          }
        }
      } else {
        // (the same two register sets in turn; the identity rows leave an integer as it is)
        // roundf(x) for x >= 0 (a blend of non-negative values with non-negative factors): trunc(x), plus one where the -- exactly
        // computed -- fraction reaches a half; two dependent operations fewer than the sign-preserving general form.
#define COX_COLOUR_STEP(op)                                 \
  {                                                         \
    const float x = val * (op).x + (op).y;                  \
    const float t = truncf(x);                              \
    val = (x - t >= 0.5f) ? t + 1.0f : t;                   \
  }
        MergeOp a0 = tbl[0][role], a1 = tbl[1][role], a2 = tbl[2][role], a3 = tbl[3][role];
        for (u32 k = 0; k < cnt_in; k += 8) {
          const u32 kb = (k + 4) & 63u;
          const MergeOp b0 = tbl[kb][role], b1 = tbl[kb + 1][role], b2 = tbl[kb + 2][role], b3 = tbl[kb + 3][role];
          __builtin_amdgcn_sched_barrier(0);
          COX_COLOUR_STEP(a0)
          COX_COLOUR_STEP(a1)
          COX_COLOUR_STEP(a2)
          COX_COLOUR_STEP(a3)
          __builtin_amdgcn_sched_barrier(0);
          const u32 ka = (k + 8) & 63u;
          a0 = tbl[ka][role];
          a1 = tbl[ka + 1][role];
          a2 = tbl[ka + 2][role];
          a3 = tbl[ka + 3][role];
          __builtin_amdgcn_sched_barrier(0);
          COX_COLOUR_STEP(b0)
          COX_COLOUR_STEP(b1)
          COX_COLOUR_STEP(b2)
          COX_COLOUR_STEP(b3)
          __builtin_amdgcn_sched_barrier(0);
        }
#undef COX_COLOUR_STEP
      }
      wave_lds_handover();
      W = readlane_f32(Wnext, cnt_in - 1);
    }
    if (colour_wave) {
      u32 mcolor = 0;
#pragma unroll
      for (u32 c = 0; c < 4; ++c) mcolor |= (static_cast<u32>(static_cast<int>(readlane_f32(val, c))) & 255u) << (8u * c);
      if (lane == 0) {
        R.color[m] = mcolor;
        reinterpret_cast<u32*>(R.q)[static_cast<size_t>(m) * 8u + 5u] = mcolor;  // (the ray's line: the wave apply takes the colour from there)
      }
    } else {
      const float mx = readlane_f32(val, 0), my = readlane_f32(val, 1), mz = readlane_f32(val, 2);
      auto write_ray = [&](const F3& pg, const Dda& d, u32 flags) {  // one lane
        if (d.range_error) atomicOr(&cnt->err, kErrRange);
        R.px[m] = pg.x;
        R.py[m] = pg.y;
        R.pz[m] = pg.z;
        R.w[m] = W;
        R.flags[m] = flags;
        R.key[m] = key;
        R.nsteps[m] = d.nsteps;
        if (piece_axis_cap) R.pbound[m] = piece_bound(d, piece_axis_cap);
        {
          // what compute_sdf derives from the ray alone, with its own operations, once per ray instead of once per step
          const F3 dv = pg - F3{P.tx, P.ty, P.tz};
          typedef float F4 __attribute__((ext_vector_type(4)));
          F4* q = reinterpret_cast<F4*>(R.q + static_cast<size_t>(m) * 8u);
          q[0] = F4{dv.x, dv.y, dv.z, sqrtf(dot3(dv, dv))};
          R.q[static_cast<size_t>(m) * 8u + 4u] = W;  // (word 5 is the colour, written by the bundle's colour wave)
        }
      };
      if constexpr (kWalk) {
        // The ray is wave-uniform: every lane sets it up, lane 0 writes it, and the wave walks it here, in the shadow of the frame's
        // longer bundles.  The walk's scratch (crossing times and path: 3 KB) is the wave's own operand table (4 KB), free since the
        // last chunk's hand-over.
        static_assert(6 * kAxisCapSmall * sizeof(u32) <= sizeof(ops[0]), "the walk's scratch fits the wave's operand table");
        const F3 pg = transform_point(P, F3{mx, my, mz});
        Dda d;
        dda_setup(d, P, pg, clearing);
        const u32 ns = d.nsteps;
        // (a slot that would end beyond the record buffers: COX_RECORD_CAP only -- emit then walks the ray itself)
        const bool fits = ns <= walk.path_stride && (static_cast<u64>(m) + 1ull) * walk.path_stride <= static_cast<u64>(walk.rec_cap);
        const u32 flags = 1u | (clearing ? 2u : 0u) | (fits ? 0u : kRayNoPath);
        if (lane == 0) write_ray(pg, d, flags);
        if (ns != 0) {
          float* tl = reinterpret_cast<float*>(tbl);
          wave_touch_ray<kAxisCapSmall>(P, R, walk.blocks, m, ns, flags, d, key, tl, reinterpret_cast<u32*>(tl + 3 * kAxisCapSmall), lane,
                                        fits ? walk.path + m * walk.path_stride : nullptr, cnt, walk.fh_keys, walk.fh_mask);
          wave_lds_handover();  // (the sequential fallback leaves without one) the next task fills the operand table
        }
      } else if (lane == 0) {
        const F3 pg = transform_point(P, F3{mx, my, mz});
        Dda d;
        dda_setup(d, P, pg, clearing);
        write_ray(pg, d, 1u | (clearing ? 2u : 0u));
      }
    }
  }
}
