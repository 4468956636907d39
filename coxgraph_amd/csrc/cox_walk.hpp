// The record walk (stage T): touch (allocate blocks, give every block touched this frame a dense ordinal) and emit ((voxel id, ray)
// records, ray-major), lane per ray and wave per ray (parallel DDA) -- part of cox_integrator.hip (included there, in this order:
// the kernels use what is defined above them in that file).  The wave walk of `merged` takes its ordinals from a table of the
// frame's own and leaves the layer to k_bind_blocks (FrameBlocks, below), so it may run ahead of the layer update.
#pragma once

// ---- touch: allocate blocks, give every block touched this frame a dense ordinal ---------------
// anti-grazing (merged only): skip voxels that are the terminal voxel of another (non-clearing) bundle
__device__ __forceinline__ bool grazing_skip(const FrameParams& P, const u64* fh_keys, u32 fh_mask, bool clearing, u64 own_key, int x, int y, int z) {
  if (!P.anti_grazing) return false;
  const u64 k = pack_key(x, y, z);
  if (!clearing && k == own_key) return false;
  return ht_find(fh_keys, fh_mask, k) != kInvalid;
}

__global__ void __launch_bounds__(256) k_touch(const FrameParams* __restrict__ Pp, RayArrays R, LayerView L, u32* __restrict__ touched_slots, Counters* cnt, u32* layer_err,
                                               const u64* __restrict__ fh_keys, u32 fh_mask) {
  const FrameParams P = *Pp;
  const u32 n_slots = cnt->n_ray_slots;
  for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n_slots; r += gridDim.x * blockDim.x) {
    const u32 ns = R.nsteps[r];
    if (ns == 0) continue;
    const bool clearing = (R.flags[r] & 2u) != 0;
    const F3 pg{R.px[r], R.py[r], R.pz[r]};
    const u64 own_key = P.anti_grazing ? R.key[r] : 0ull;
    Dda d;
    dda_setup(d, P, pg, clearing);
    u64 last_bkey = kEmptyKey;
    for (u32 s = 0; s < ns; ++s) {
      const int x = d.c[0], y = d.c[1], z = d.c[2];
      dda_step(d);
      if (grazing_skip(P, fh_keys, fh_mask, clearing, own_key, x, y, z)) continue;
      const u64 bkey = pack_key(x >> 4, y >> 4, z >> 4);
      if (bkey == last_bkey) continue;
      last_bkey = bkey;
      bool fresh;
      const u32 slot = ht_insert(L.ht_keys, L.ht_mask, bkey, &fresh);
      if (slot == kInvalid) {
        atomicOr(layer_err, kErrTable);
        continue;
      }
      if (fresh) {
        const u32 pool = atomicAdd(L.d_nblocks, 1u);
        if (pool < L.capacity) {
          L.ht_vals[slot] = pool;  // read by later kernels only
          L.block_keys[pool] = bkey;
          atomicAdd(&cnt->n_new_blocks, 1u);
        } else {
          atomicSub(L.d_nblocks, 1u);     // the counter settles at the capacity
          atomicOr(layer_err, kErrPool);  // ht_vals[slot] stays kInvalid: updates to this block are dropped, and every later
                                          // frame that meets the key reports the error again (emit kernels)
        }
      }
      if (__hip_atomic_load(&L.ht_stamp[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != P.frame_id &&
          atomicExch(&L.ht_stamp[slot], P.frame_id) != P.frame_id) {
        const u32 ord = atomicAdd(&cnt->n_touched, 1u);
        touched_slots[ord] = slot;
        L.ht_ord[slot] = ord;
      }
    }
  }
}

// every emit kernel starts by publishing, per block touched this frame, what the update kernels need of it
__device__ __forceinline__ void fill_ord_info(const LayerView& L, const u32* __restrict__ touched_slots, int4* __restrict__ ord_info, u32 n_touched) {
  for (u32 ord = blockIdx.x * blockDim.x + threadIdx.x; ord < n_touched; ord += gridDim.x * blockDim.x) {
    const u32 slot = touched_slots[ord];
    int bx, by, bz;
    unpack_key(L.ht_keys[slot], &bx, &by, &bz);
    ord_info[ord] = make_int4(bx * 16, by * 16, bz * 16, static_cast<int>(L.ht_vals[slot]));
  }
}

// ---- emit: (voxel id, ray id) records, ray-major ------------------------------------------------
// voxel id = ordinal of the block within this frame << 12 | linear voxel index.  Also publishes the key
// width the record sort needs.
__global__ void __launch_bounds__(256) k_emit(const FrameParams* __restrict__ Pp, RayArrays R, LayerView L, u32* __restrict__ rec_key, u32* __restrict__ rec_ray, u32 rec_cap,
                                              Counters* cnt, SortInfo* sort_info, const u64* __restrict__ fh_keys, u32 fh_mask, const u32* __restrict__ touched_slots,
                                              int4* __restrict__ ord_info, int by_block) {
  const FrameParams P = *Pp;
  const u32 n_slots = cnt->n_ray_slots;
  fill_ord_info(L, touched_slots, ord_info, cnt->n_touched);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // ordinals are < n_touched; kInvalid's low bits (all ones) must sort after every valid id
    u32 bits = 12;
    while ((1ull << (bits - 12)) < static_cast<u64>(cnt->n_touched) + 1ull) ++bits;
    const bool overflow = cnt->n_records > rec_cap;
    // block apply (by_block & 255 = its tile shift): a stable partition by tile is all the global order it needs; bit 8 of
    // by_block: one pass on the low 12 bits of the tile id (buckets) is enough
    const u32 shift = static_cast<u32>(by_block) & 255u;
    sort_info->nbits = overflow ? 0u : ((by_block & 256) ? min(bits - shift, 12u) : bits - shift);  // 0 bits: every sort pass exits at once
    sort_info->parity = 0;
    sort_info->base = shift;
    if (overflow) atomicOr(&cnt->err, kErrRecords);
  }
  if (cnt->n_records > rec_cap) return;  // frame dropped as a whole (reported at sync); never a partial update
  for (u32 r = blockIdx.x * blockDim.x + threadIdx.x; r < n_slots; r += gridDim.x * blockDim.x) {
    const u32 ns = R.nsteps[r];
    if (ns == 0) continue;
    const u32 off = R.rec_off[r];
    const bool clearing = (R.flags[r] & 2u) != 0;
    const F3 pg{R.px[r], R.py[r], R.pz[r]};
    const u64 own_key = P.anti_grazing ? R.key[r] : 0ull;
    Dda d;
    dda_setup(d, P, pg, clearing);
    u64 last_bkey = kEmptyKey;
    u32 last_ord = kInvalid;
    for (u32 s = 0; s < ns; ++s) {
      const int x = d.c[0], y = d.c[1], z = d.c[2];
      dda_step(d);
      u32 vid = kInvalid;
      if (!grazing_skip(P, fh_keys, fh_mask, clearing, own_key, x, y, z)) {
        const u64 bkey = pack_key(x >> 4, y >> 4, z >> 4);
        if (bkey != last_bkey) {
          last_bkey = bkey;
          const u32 slot = ht_find(L.ht_keys, L.ht_mask, bkey);
          last_ord = (slot != kInvalid && L.ht_vals[slot] != kInvalid) ? L.ht_ord[slot] : kInvalid;
          if (last_ord == kInvalid) atomicOr(&cnt->err, kErrPool);  // block without storage: this update is lost
        }
        if (last_ord != kInvalid) vid = (last_ord << 12) | static_cast<u32>((x & 15) | ((y & 15) << 4) | ((z & 15) << 8));
      }
      rec_key[off + s] = vid;
      rec_ray[off + s] = r;
    }
  }
}

// ---- wave-per-ray traversal (few, long rays: the merged integrator's bundles) -----------------------------
// A DDA is a dependent chain, so lane-per-ray leaves the chip empty when a frame has only a few thousand rays.
// Here one wave walks one ray in parallel and reproduces the sequential argmin walk bit for bit:
//   - per axis, the plane-crossing times are the reference's own repeated float additions
//     T_k(j+1) = fl(T_k(j) + t_step_k) (three short chains, one lane each, into LDS);
//   - "pick the smallest t, first axis wins ties" is a 3-way stable merge of those sorted sequences, so the
//     position of crossing (k, j) in the walk is j + #{crossings of the other axes that precede it}, found by
//     binary search; the same counts are the voxel's offset from the start voxel;
//   - rays the argument does not cover (a zero ray component gives -inf / NaN times, very long rays, or a walk
//     that would need more crossings of one axis than were generated) fall back to the sequential walk on lane 0.
// per-axis crossing capacity of the parallel DDA: two instantiations, the small one (12 KB of LDS per workgroup instead
// of 48 KB, so every ray of a frame is resident at once) whenever no ray of the configuration can cross more planes
// (kAxisCapSmall, kAxisCapLarge and the ray flags kRayFallback, kRayNoPath: cox_frame.hpp -- the bundle merge uses them too)

__device__ __forceinline__ u32 pack_path(u32 jx, u32 jy, u32 jz) { return jx | (jy << 10) | (jz << 20); }
// entries of the sorted array a[0, n) that precede t: a[i] < t, or a[i] <= t when inclusive
__device__ __forceinline__ u32 count_before(const float* a, u32 n, float t, bool inclusive) {
  u32 lo = 0, hi = n;
  while (lo < hi) {
    const u32 mid = (lo + hi) >> 1;
    const float v = a[mid];
    const bool before = inclusive ? (v <= t) : (v < t);
    if (before)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
// The same count, found from an estimate: the sequence is a[i] = fl(a[i-1] + step), i.e. a[0] + i * step up to rounding, so
// (t - a[0]) / step lands within an entry or two of the partition point; the table decides (a sorted array has ONE partition
// point of "before", whichever way it is approached), and anything odd (infinite steps, an estimate that is far off) goes
// to the binary search.  Two or three LDS reads instead of nine dependent ones: the ranking was 2/3 of the wave walk.
__device__ __forceinline__ u32 count_before_guided(const float* a, u32 n, float t, bool inclusive, float a0, float inv_step) {
  if (n == 0) return 0;
  const float est = (t - a0) * inv_step;
  if (!(est > -4.0f && est < 1.0e6f)) return count_before(a, n, t, inclusive);  // NaN / inf / far outside
  u32 c = min(n, static_cast<u32>(max(0.0f, est)) + 1u);  // candidate count
#pragma unroll 1
  for (int guard = 0; guard < 6; ++guard) {
    if (c < n) {
      const float v = a[c];
      if (inclusive ? (v <= t) : (v < t)) {
        ++c;
        continue;
      }
    }
    if (c > 0) {
      const float v = a[c - 1];
      if (!(inclusive ? (v <= t) : (v < t))) {
        --c;
        continue;
      }
    }
    return c;
  }
  return count_before(a, n, t, inclusive);
}
// sequential argmin step that also reports the chosen axis
__device__ __forceinline__ int dda_step_axis(Dda& d) {
  int k = 0;
  float best = d.t_next[0];
  if (d.t_next[1] < best) {
    best = d.t_next[1];
    k = 1;
  }
  if (d.t_next[2] < best) k = 2;
  d.c[0] += (k == 0) ? d.sgn[0] : 0;
  d.c[1] += (k == 1) ? d.sgn[1] : 0;
  d.c[2] += (k == 2) ? d.sgn[2] : 0;
  d.t_next[0] = (k == 0) ? d.t_next[0] + d.t_step[0] : d.t_next[0];
  d.t_next[1] = (k == 1) ? d.t_next[1] + d.t_step[1] : d.t_next[1];
  d.t_next[2] = (k == 2) ? d.t_next[2] + d.t_step[2] : d.t_next[2];
  return k;
}
// Fills path[0, ns) (LDS, this wave's) with the packed per-axis crossing counts of every step.  Returns false
// when the ray needs the sequential fallback (nothing usable was written).
// `limit`: only the first min(ns, limit) steps are wanted (the fast integrator's capped candidate lists).  Each axis then
// needs its first limit + 1 crossings only: a crossing whose rank is below the limit is preceded by fewer than `limit`
// crossings of any other axis, so the truncated sequences still count them exactly; everything else is discarded.
template <u32 kAxisCap>
__device__ __forceinline__ bool wave_ray_path(const Dda& d0, u32 ns, float* tl /*[3][kAxisCap]*/, u32* path, u32 lane, u32 limit = 0xFFFFFFFFu) {
  if (d0.sgn[0] == 0 || d0.sgn[1] == 0 || d0.sgn[2] == 0) return false;
  const u32 want = min(ns, limit);
  const u32 gen = (want < 0xFFFFFFFEu) ? want + 1u : want;
  const u32 f0 = d0.n_axis[0] + 2, f1 = d0.n_axis[1] + 2, f2 = d0.n_axis[2] + 2;  // whole sequences (two entries past the last crossing)
  const u32 g0 = min(f0, gen), g1 = min(f1, gen), g2 = min(f2, gen);              // generated
  if (g0 > kAxisCap || g1 > kAxisCap || g2 > kAxisCap || want > 3 * kAxisCap) return false;
  const u32 L = want - 1;
  if (lane < 3) {
    // the per-axis values are picked with selects on opaque copies: left alone, the compiler turns "lane == 0 ? a[0] :
    // lane == 1 ? a[1] : a[2]" into a[lane] and moves the whole Dda into scratch memory (72 B per lane written per ray)
    float tn0 = d0.t_next[0], tn1 = d0.t_next[1], tn2 = d0.t_next[2], ts0 = d0.t_step[0], ts1 = d0.t_step[1], ts2 = d0.t_step[2];
    asm volatile("" : "+v"(tn0), "+v"(tn1), "+v"(tn2), "+v"(ts0), "+v"(ts1), "+v"(ts2));
    float T = (lane == 0) ? tn0 : (lane == 1) ? tn1 : tn2;
    const float st = (lane == 0) ? ts0 : (lane == 1) ? ts1 : ts2;
    const u32 g = (lane == 0) ? g0 : (lane == 1) ? g1 : g2;
    float* row = tl + lane * kAxisCap;
    for (u32 j = 0; j < g; ++j) {
      row[j] = T;
      T += st;
    }
  }
  wave_lds_handover();
  const u32 E = g0 + g1 + g2;
  const float inv_step[3] = {1.0f / d0.t_step[0], 1.0f / d0.t_step[1], 1.0f / d0.t_step[2]};  // (estimates only: the tables decide)
  bool bad = false;
  for (u32 eb = 0; eb < E; eb += 64) {
    const u32 e = eb + lane;
    if (e < E) {
      const u32 k = (e < g0) ? 0u : (e < g0 + g1) ? 1u : 2u;
      const u32 j = (k == 0) ? e : (k == 1) ? e - g0 : e - g0 - g1;
      const float t = tl[k * kAxisCap + j];
      if (isnan(t)) bad = true;
      // crossings that precede (k, j): own axis j, lower axes on <=, higher axes on <
      const u32 c0 = (k == 0) ? j : count_before_guided(tl, g0, t, true, d0.t_next[0], inv_step[0]);
      const u32 c1 = (k == 1) ? j : count_before_guided(tl + kAxisCap, g1, t, k > 1, d0.t_next[1], inv_step[1]);
      const u32 c2 = (k == 2) ? j : count_before_guided(tl + 2 * kAxisCap, g2, t, false, d0.t_next[2], inv_step[2]);
      const u32 rank = c0 + c1 + c2;
      if (rank < L) {
        path[rank + 1] = pack_path(c0 + (k == 0 ? 1u : 0u), c1 + (k == 1 ? 1u : 0u), c2 + (k == 2 ? 1u : 0u));
        const u32 f = (k == 0) ? f0 : (k == 1) ? f1 : f2;
        if (j == f - 1) bad = true;  // the walk would go on to a crossing past the ones the ray has
      }
    }
  }
  if (lane == 0) path[0] = 0;
  wave_lds_handover();
  return __ballot(bad) == 0ull;
}

// returns the block's hash slot (kInvalid: table full)
__device__ __forceinline__ u32 touch_block(const FrameParams& P, const LayerView& L, u64 bkey, u32* touched_slots, Counters* cnt, u32* layer_err) {
  bool fresh;
  const u32 slot = ht_insert(L.ht_keys, L.ht_mask, bkey, &fresh);
  if (slot == kInvalid) {
    atomicOr(layer_err, kErrTable);
    return kInvalid;
  }
  if (fresh) {
    const u32 pool = atomicAdd(L.d_nblocks, 1u);
    if (pool < L.capacity) {
      L.ht_vals[slot] = pool;  // read by later kernels only
      L.block_keys[pool] = bkey;
      atomicAdd(&cnt->n_new_blocks, 1u);
    } else {
      atomicSub(L.d_nblocks, 1u);     // the counter settles at the capacity
      atomicOr(layer_err, kErrPool);  // ht_vals[slot] stays kInvalid: updates to this block are dropped, and every later
                                      // frame that meets the key reports the error again (emit kernels)
    }
  }
  if (__hip_atomic_load(&L.ht_stamp[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != P.frame_id &&
      atomicExch(&L.ht_stamp[slot], P.frame_id) != P.frame_id) {
    const u32 ord = atomicAdd(&cnt->n_touched, 1u);
    touched_slots[ord] = slot;
    L.ht_ord[slot] = ord;
  }
  return slot;
}

// ---- the frame block table (merged record walk) ---------------------------------------------------------------------------------
// The ordinal of a block is a dense number per distinct block key of THIS frame, so the walk takes it from a table of the frame's
// own (one per record set: open addressing on the packed block key, sized with the layer's table, so a frame that fits the layer's
// fits the frame's) and touches no layer word.  The layer comes in with the binding (k_bind_blocks), one thread per touched block:
// the only step of a frame that has to follow the previous frame's update.
// (struct FrameBlocks: cox_frame.hpp, with the other views)
// the first inserter of a key hands out its ordinal (the walk; emit runs in a later launch and only looks up)
__device__ __forceinline__ void touch_frame_block(const FrameBlocks& B, u64 bkey, Counters* cnt) {
  bool fresh;
  const u32 slot = ht_insert(B.keys, B.mask, bkey, &fresh);
  if (slot == kInvalid) {  // more distinct blocks than the layer's table has slots: the layer could not take them either
    atomicOr(&cnt->err, kErrTable);
    return;
  }
  if (fresh) {
    const u32 ord = atomicAdd(&cnt->n_touched, 1u);
    B.ord[slot] = ord;
    B.slots[ord] = slot;
  }
}
__device__ __forceinline__ u32 frame_block_ord(const FrameBlocks& B, u64 bkey) {
  const u32 slot = ht_find(B.keys, B.mask, bkey);
  return slot != kInvalid ? B.ord[slot] : kInvalid;
}
// Binding: block ordinal -> layer.  Inserts the key into the layer's table, gives a new block its storage exactly as touch_block
// does, publishes what the update kernels need of the block (ord_info) and empties the frame table's slot.  Every key is bound by
// one thread (the frame table holds it once), so the (slot, pool) pair of a fresh key has one writer; keys of earlier frames
// were bound by earlier launches.
__device__ __forceinline__ void bind_touched_blocks(const LayerView& L, const FrameBlocks& B, int4* __restrict__ ord_info, Counters* cnt, u32* layer_err) {
  const u32 n_touched = cnt->n_touched;
  for (u32 ord = blockIdx.x * blockDim.x + threadIdx.x; ord < n_touched; ord += gridDim.x * blockDim.x) {
    const u32 fslot = B.slots[ord];
    const u64 bkey = B.keys[fslot];
    B.keys[fslot] = kEmptyKey;
    u32 pool = kInvalid;
    bool fresh;
    const u32 slot = ht_insert(L.ht_keys, L.ht_mask, bkey, &fresh);
    if (slot == kInvalid) {
      atomicOr(layer_err, kErrTable);
    } else if (fresh) {
      pool = atomicAdd(L.d_nblocks, 1u);
      if (pool < L.capacity) {
        L.ht_vals[slot] = pool;
        L.block_keys[pool] = bkey;
        atomicAdd(&cnt->n_new_blocks, 1u);
      } else {
        atomicSub(L.d_nblocks, 1u);     // the counter settles at the capacity
        atomicOr(layer_err, kErrPool);  // ht_vals[slot] stays kInvalid: every later frame that meets the key reports the error again
        pool = kInvalid;
      }
    } else {
      pool = L.ht_vals[slot];
    }
    if (pool == kInvalid) atomicOr(&cnt->err, kErrPool);  // block without storage: its updates are lost (the apply kernels skip it)
    int bx, by, bz;
    unpack_key(bkey, &bx, &by, &bz);
    ord_info[ord] = make_int4(bx * 16, by * 16, bz * 16, static_cast<int>(pool));
  }
}
// a launch of its own where no k_block_starts follows (full record sort); the tile apply binds at the head of k_block_starts_bind
__global__ void __launch_bounds__(256) k_bind_blocks(LayerView L, FrameBlocks B, int4* __restrict__ ord_info, Counters* cnt, u32* layer_err) {
  bind_touched_blocks(L, B, ord_info, cnt, layer_err);
}

// The wave walk of ONE ray, for every kernel that touches from it (k_touch_wave; k_bundle_merge<true>, on the wave that has just
// produced the ray): the parallel path into `tl` / `path` (LDS, this wave's: 3 * kAxisCap words each), the ray's flags, its path
// parked at `park` (nullptr: not parked) for k_emit_wave, and its blocks into the frame block table.  Every argument is wave-uniform
// and `d` is the ray's dda_setup; `flags` comes in without kRayFallback.
template <u32 kAxisCap>
__device__ void wave_touch_ray(const FrameParams& P, const RayArrays& R, const FrameBlocks& B, u32 r, u32 ns, u32 flags, Dda d, u64 own_key, float* tl, u32* path,
                               u32 lane, u32* __restrict__ park, Counters* cnt, const u64* __restrict__ fh_keys, u32 fh_mask) {
  const bool clearing = (flags & 2u) != 0;
  const bool par = wave_ray_path<kAxisCap>(d, ns, tl, path, lane);
  if (lane == 0) R.flags[r] = par ? flags : (flags | kRayFallback);
  if (par) {
    u64 carry = kEmptyKey;
    for (u32 base = 0; base < ns; base += 64) {
      const u32 s = base + lane;
      const bool act = s < ns;
      u64 bkey = kEmptyKey;
      bool skip = false;
      if (act) {
        const u32 p = path[s];
        if (park) park[s] = p;  // emit reads the walk instead of redoing it
        const int x = d.c[0] + static_cast<int>(p & 1023u) * d.sgn[0];
        const int y = d.c[1] + static_cast<int>((p >> 10) & 1023u) * d.sgn[1];
        const int z = d.c[2] + static_cast<int>(p >> 20) * d.sgn[2];
        skip = grazing_skip(P, fh_keys, fh_mask, clearing, own_key, x, y, z);
        bkey = pack_key(x >> 4, y >> 4, z >> 4);
      }
      // a voxel touches its block unless the previous voxel THAT WAS NOT SKIPPED lies in the same block (a block whose
      // first voxel on the ray is skipped by anti-grazing must still be allocated by the next one; found by the fuzzer)
      const u64 kept = __ballot(act && !skip);
      const u64 kept_below = kept & ((1ull << lane) - 1ull);
      const int src = kept_below ? (63 - __clzll(static_cast<long long>(kept_below))) : 0;
      const u64 prev_kept = __shfl(bkey, src, 64);
      const u64 prev = kept_below ? prev_kept : carry;
      if (act && !skip && bkey != prev) touch_frame_block(B, bkey, cnt);
      if (kept) carry = __shfl(bkey, 63 - __clzll(static_cast<long long>(kept)), 64);
    }
    wave_lds_handover();  // the next user of this wave's LDS scratch
  } else if (lane == 0) {
    // sequential fallback
    u64 last_bkey = kEmptyKey;
    for (u32 s = 0; s < ns; ++s) {
      const int x = d.c[0], y = d.c[1], z = d.c[2];
      dda_step(d);
      if (grazing_skip(P, fh_keys, fh_mask, clearing, own_key, x, y, z)) continue;
      const u64 bkey = pack_key(x >> 4, y >> 4, z >> 4);
      if (bkey == last_bkey) continue;
      last_bkey = bkey;
      touch_frame_block(B, bkey, cnt);
    }
  }
}

template <u32 kAxisCap>
__global__ void __launch_bounds__(256) k_touch_wave(const FrameParams* __restrict__ Pp, RayArrays R, FrameBlocks B, u32* __restrict__ path_out, u32 rec_cap, Counters* cnt,
                                                    const u64* __restrict__ fh_keys, u32 fh_mask) {
  const FrameParams P = *Pp;
  __shared__ float lds_t[4][3 * kAxisCap];
  __shared__ u32 lds_path[4][3 * kAxisCap];
  const u32 n_slots = uniform_u32(cnt->n_ray_slots);
  const bool overflow = uniform_u32(cnt->n_records) > rec_cap;
  const u32 lane = lane_id();
  const u32 wave = threadIdx.x >> 6;
  float* tl = lds_t[wave];
  u32* path = lds_path[wave];
  const u32 waves_total = (gridDim.x * blockDim.x) >> 6;
  for (u32 r = uniform_u32((blockIdx.x * blockDim.x + threadIdx.x) >> 6); r < n_slots; r += waves_total) {
    const u32 ns = uniform_u32(R.nsteps[r]);
    if (ns == 0) continue;
    const u32 flags = uniform_u32(R.flags[r]) & ~(kRayFallback | kRayNoPath);
    const F3 pg{readlane_f32(R.px[r], 0), readlane_f32(R.py[r], 0), readlane_f32(R.pz[r], 0)};
    const u64 own_key = P.anti_grazing ? R.key[r] : 0ull;
    const u32 off = uniform_u32(R.rec_off[r]);
    Dda d;
    dda_setup(d, P, pg, (flags & 2u) != 0);
    wave_touch_ray<kAxisCap>(P, R, B, r, ns, flags, d, own_key, tl, path, lane, overflow ? nullptr : path_out + off, cnt, fh_keys, fh_mask);
  }
}

// path_stride: where the walk parked ray r's path -- 0: at its record offset, path_in[rec_off[r] + s] (k_touch_wave); otherwise in a
// slot of that many words of the ray's own, path_in[r * path_stride + s] (k_bundle_merge<true>, which runs ahead of the offsets' scan)
__global__ void __launch_bounds__(256) k_emit_wave(const FrameParams* __restrict__ Pp, RayArrays R, FrameBlocks B, const u32* __restrict__ path_in, u32* __restrict__ rec_key,
                                                   u32* __restrict__ rec_ray, u32 rec_cap, Counters* cnt, SortInfo* sort_info,
                                                   const u64* __restrict__ fh_keys, u32 fh_mask, int by_block, u32 path_stride) {
  const FrameParams P = *Pp;
  const u32 n_slots = uniform_u32(cnt->n_ray_slots);
  const bool overflow = uniform_u32(cnt->n_records) > rec_cap;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // ordinals are < n_touched; kInvalid's low bits (all ones) must sort after every valid id
    u32 bits = 12;
    while ((1ull << (bits - 12)) < static_cast<u64>(cnt->n_touched) + 1ull) ++bits;
    const u32 shift = static_cast<u32>(by_block) & 255u;
    sort_info->nbits = overflow ? 0u : ((by_block & 256) ? min(bits - shift, 12u) : bits - shift);  // 0 bits: every sort pass exits at once
    sort_info->parity = 0;
    sort_info->base = shift;
    if (overflow) atomicOr(&cnt->err, kErrRecords);
  }
  if (overflow) return;  // frame dropped as a whole (reported at sync); never a partial update
  const u32 lane = lane_id();
  const u32 waves_total = (gridDim.x * blockDim.x) >> 6;
  for (u32 r = uniform_u32((blockIdx.x * blockDim.x + threadIdx.x) >> 6); r < n_slots; r += waves_total) {
    const u32 ns = uniform_u32(R.nsteps[r]);
    if (ns == 0) continue;
    const u32 flags = uniform_u32(R.flags[r]);
    const bool clearing = (flags & 2u) != 0;
    const u32 off = uniform_u32(R.rec_off[r]);
    const F3 pg{readlane_f32(R.px[r], 0), readlane_f32(R.py[r], 0), readlane_f32(R.pz[r], 0)};
    const u64 own_key = P.anti_grazing ? R.key[r] : 0ull;
    Dda d;
    dda_setup(d, P, pg, clearing);
    if (!(flags & (kRayFallback | kRayNoPath))) {
      const u32 pbase = path_stride ? r * path_stride : off;
      u64 carry_key = kEmptyKey;
      u32 carry_ord = kInvalid;
      for (u32 base = 0; base < ns; base += 64) {
        const u32 s = base + lane;
        const bool act = s < ns;
        u64 bkey = kEmptyKey;
        bool skip = false;
        u32 lin = 0;
        if (act) {
          const u32 p = path_in[pbase + s];
          const int x = d.c[0] + static_cast<int>(p & 1023u) * d.sgn[0];
          const int y = d.c[1] + static_cast<int>((p >> 10) & 1023u) * d.sgn[1];
          const int z = d.c[2] + static_cast<int>(p >> 20) * d.sgn[2];
          skip = grazing_skip(P, fh_keys, fh_mask, clearing, own_key, x, y, z);
          bkey = pack_key(x >> 4, y >> 4, z >> 4);
          lin = static_cast<u32>((x & 15) | ((y & 15) << 4) | ((z & 15) << 8));
        }
        u64 prev = __shfl_up(bkey, 1, 64);
        if (lane == 0) prev = carry_key;
        const bool is_head = act && bkey != prev;
        u32 ord = kInvalid;
        if (is_head) {
          ord = frame_block_ord(B, bkey);  // (a block the binding leaves without storage keeps its ordinal: the apply kernels skip it)
        }
        // every lane takes the ordinal of the nearest head at or below it, or the carry of the previous round
        const u64 heads = __ballot(is_head);
        const u64 below = heads & ((lane == 63) ? ~0ull : ((2ull << lane) - 1ull));
        const int src = below ? (63 - __clzll(static_cast<long long>(below))) : 0;
        const u32 head_ord = static_cast<u32>(__shfl(static_cast<int>(ord), src, 64));
        const u32 my_ord = below ? head_ord : carry_ord;
        if (act) {
          rec_key[off + s] = (skip || my_ord == kInvalid) ? kInvalid : ((my_ord << 12) | lin);
          rec_ray[off + s] = r;
        }
        carry_key = __shfl(bkey, 63, 64);
        carry_ord = static_cast<u32>(__shfl(static_cast<int>(my_ord), 63, 64));
      }
    } else if (lane == 0) {
      u64 last_bkey = kEmptyKey;
      u32 last_ord = kInvalid;
      for (u32 s = 0; s < ns; ++s) {
        const int x = d.c[0], y = d.c[1], z = d.c[2];
        dda_step(d);
        u32 vid = kInvalid;
        if (!grazing_skip(P, fh_keys, fh_mask, clearing, own_key, x, y, z)) {
          const u64 bkey = pack_key(x >> 4, y >> 4, z >> 4);
          if (bkey != last_bkey) {
            last_bkey = bkey;
            last_ord = frame_block_ord(B, bkey);
          }
          if (last_ord != kInvalid) vid = (last_ord << 12) | static_cast<u32>((x & 15) | ((y & 15) << 4) | ((z & 15) << 8));
        }
        rec_key[off + s] = vid;
        rec_ray[off + s] = r;
      }
    }
  }
}
