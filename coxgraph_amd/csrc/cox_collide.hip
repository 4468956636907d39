// MI355X (gfx950): collision checks of planner paths against an ESDF (or TSDF) layer, behind include/coxgraph_hip_collide.h.
//
// What active_3d_planning's RRTStar and RecheckCollision ask of the map, as coxgraph configures them
// (coxgraph_sim/config/reconstruction_planner.yaml): is this sample traversable, how far is this segment free, which nodes of
// the tree survive the new map.
//
//   sample_state              rule S, one device function: the blocks around the sample are resolved once (BlockCache of
//                             cox_interp.hpp) and serve the nearest voxel ("observed") and the trilinear cell (the distance)
//   k_collide_points          one lane per point
//   k_collide_segments<G>     G lanes (64: a wave, 32: half of one) share a segment and take consecutive samples in rounds; a
//                             ballot after each round finds the first blocked sample, the group stops at the first round that
//                             has one.  Neighbouring lanes read neighbouring voxels.
//   k_collide_trajectories<G> the same loop over given points (CSR)
//   k_prune_small             pointer jumping over (ancestor, ok) words in LDS, one workgroup, trees of <= kPruneSmall nodes
//   k_prune_init/round/finish the same with one launch per round on two global buffers
//
// Rules and arithmetic: DESIGN.md section 7k.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "../../include/coxgraph_hip_collide.h"
#include "cox_host.hpp"
#include "cox_interp.hpp"

using namespace cox;

static_assert(sizeof(cox_collide_record) == 32, "cox_collide_record is 32 bytes");

namespace {

typedef unsigned long long ull;

constexpr int kThreads = 256;
constexpr u32 kPruneSmall = 4096;  // nodes a single workgroup prunes in LDS (2 x 16 KiB)
constexpr int kPruneThreads = 1024;
constexpr u64 kMaxTree = 1ull << 30;
constexpr u32 kDefaultMaxSamples = 4096, kMaxMaxSamples = 1u << 24;

struct CollideParams {
  float radius, clearing_radius, centre[3];
  float ds, max_ext, crop_margin, crop_min_length;
  u32 max_samples;
  int optimistic, crop;
};

__device__ __forceinline__ float dot_self(float x, float y, float z) { return (x * x + y * y) + z * z; }

// rule S: COX_C_* of the sample p; *dist holds the trilinear distance when COX_C_DISTANCE is set
__device__ __forceinline__ u32 sample_state(const LayerView& L, const CollideParams& P, const float p[3], float* dist) {
  if (!point_in_range(L, p)) return COX_C_INVALID;  // NaN, +-inf, beyond the keys
  // the trilinear cell reaches g - 1 .. g + 1, one more voxel on each side for rounding at block faces; the nearest voxel is g
  BlockCache bc{L, kNoBlocks};
  int b[3];
  block_cache_fill<2>(L, p, bc, b);
  float d = 0.0f, w = 0.0f;
  if (nearest_sample(L, bc, p, &d, &w)) {  // EsdfMap::isObserved
    float dv = 0.0f, wv = 0.0f;
    if (!tri_sample(L, bc, p, &dv, &wv, false)) return COX_C_OBSERVED;  // getDistanceAtPosition fails: not traversable
    *dist = dv;
    return COX_C_OBSERVED | COX_C_DISTANCE | (dv > P.radius ? COX_C_TRAVERSABLE : 0u);
  }
  if (P.clearing_radius > 0.0f) {
    const float r = sqrtf(dot_self(p[0] - P.centre[0], p[1] - P.centre[1], p[2] - P.centre[2]));
    return r < P.clearing_radius ? (COX_C_CLEARED | COX_C_TRAVERSABLE) : 0u;
  }
  return P.optimistic ? COX_C_TRAVERSABLE : 0u;
}

__global__ void __launch_bounds__(kThreads) k_collide_points(LayerView L, CollideParams P, const float* __restrict__ xyz, u64 n,
                                                             uint8_t* __restrict__ state, float* __restrict__ distance, ull* __restrict__ stats) {
  const u64 i = static_cast<u64>(blockIdx.x) * kThreads + threadIdx.x;
  const bool live = i < n;
  if (live) {
    const float p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    float d = 0.0f;
    const u32 st = sample_state(L, P, p, &d);
    if (state) state[i] = static_cast<uint8_t>(st);
    if (distance && (st & COX_C_DISTANCE)) distance[i] = d;
  }
  const ull mask = __ballot(live);
  if (lane_id() == 0 && mask) atomicAdd(&stats[0], static_cast<ull>(__popcll(mask)));
}

// The scan G lanes share: samples 0 .. count - 1 (pos(i, p) gives sample i) in rounds of G, stopping at the first round with a
// blocked sample.  Every lane of the wave calls it (count = 0 for a group without work); the loop runs until every group of the
// wave is done, so the ballots are taken in uniform control flow.  Returns the smallest blocked index, or count; *evaluated is
// the number of samples this group looked at.
template <int G, class Pos>
__device__ __forceinline__ u32 first_blocked_scan(const LayerView& L, const CollideParams& P, u32 count, const Pos& pos, u32* evaluated) {
  const u32 lane = lane_id();
  const u32 sub = lane & (G - 1);
  const int shift = G == 64 ? 0 : static_cast<int>(lane & 32u);
  const ull group_mask = G == 64 ? ~0ull : 0xFFFFFFFFull;
  u32 first = count, base = 0, seen = 0;
  bool done = count == 0;
  while (__ballot(!done) != 0ull) {
    const u32 i = base + sub;
    bool blocked = false;
    if (!done && i < count) {
      float p[3], d;
      pos(i, p);
      blocked = (sample_state(L, P, p, &d) & COX_C_TRAVERSABLE) == 0u;
    }
    const ull hits = (__ballot(blocked) >> shift) & group_mask;
    if (!done) {
      const u32 left = count - base;
      seen += left < static_cast<u32>(G) ? left : static_cast<u32>(G);
      if (hits) {
        first = base + static_cast<u32>(__builtin_ctzll(hits));
        done = true;
      } else if (left <= static_cast<u32>(G)) {
        done = true;
      }
      base += G;
    }
  }
  *evaluated = seen;
  return first;
}

// per workgroup: the groups' counts are summed in LDS, one pair of global atomics per workgroup
__device__ __forceinline__ void add_stats(u32 evaluated, u32 skipped, bool leader, ull* stats) {
  __shared__ u32 s_counts[2];
  if (threadIdx.x == 0) s_counts[0] = s_counts[1] = 0u;
  __syncthreads();
  if (leader && evaluated) atomicAdd(&s_counts[0], evaluated);
  if (leader && skipped) atomicAdd(&s_counts[1], skipped);
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_counts[0]) atomicAdd(&stats[0], static_cast<ull>(s_counts[0]));
    if (s_counts[1]) atomicAdd(&stats[1], static_cast<ull>(s_counts[1]));
  }
}

__device__ __forceinline__ bool finite3(const float v[3]) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

struct SegmentPos {
  float a[3], dir[3], nf;
  __device__ __forceinline__ void operator()(u32 i, float p[3]) const {
    const float t = static_cast<float>(i) / nf;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = a[k] + t * dir[k];
  }
};

// rule L; every lane of a group computes the segment's scalars redundantly (they are the same in all of them)
template <int G>
__global__ void __launch_bounds__(kThreads) k_collide_segments(LayerView L, CollideParams P, const float* __restrict__ a_in, const float* __restrict__ b_in,
                                                               u64 n, cox_collide_record* __restrict__ out, ull* __restrict__ stats) {
  const u64 seg = static_cast<u64>(blockIdx.x) * (kThreads / G) + threadIdx.x / G;
  const bool live = seg < n;
  const bool leader = live && (threadIdx.x & (G - 1)) == 0;
  SegmentPos sp{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 1.0f};
  float len = 0.0f;
  u32 flags = 0, ns = 0, count = 0;
  if (live) {
    float b[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      sp.a[k] = a_in[3 * seg + k];
      b[k] = b_in[3 * seg + k];
      sp.dir[k] = b[k] - sp.a[k];
    }
    len = sqrtf(dot_self(sp.dir[0], sp.dir[1], sp.dir[2]));
    if (!(finite3(sp.a) && finite3(b) && isfinite(len))) {
      flags = COX_SEG_INVALID;
    } else {
      if (P.max_ext > 0.0f && len > P.max_ext) {
        const float s = P.max_ext / len;
#pragma unroll
        for (int k = 0; k < 3; ++k) sp.dir[k] = sp.dir[k] * s;
        len = sqrtf(dot_self(sp.dir[0], sp.dir[1], sp.dir[2]));
        flags |= COX_SEG_CLAMPED;
      }
      const float nfl = ceilf(len / P.ds);
      ns = nfl >= 4294967296.0f ? 0xFFFFFFFFu : static_cast<u32>(nfl);
      if (ns < 1u) ns = 1u;
      if (ns > P.max_samples) {
        flags |= COX_SEG_TOO_LONG;
      } else {
        sp.nf = static_cast<float>(ns);
        count = ns + 1u;
      }
    }
  }
  u32 evaluated = 0;
  const u32 fb = first_blocked_scan<G>(L, P, count, sp, &evaluated);
  if (leader) {
    cox_collide_record r;
    r.n_samples = ns;
    r.first_blocked = fb;
    r.flags = flags;
    r.pad = 0u;
    const float nan = __uint_as_float(0x7FC00000u);
    r.free_length = nan;
    r.goal[0] = r.goal[1] = r.goal[2] = nan;
    if (count) {
      const bool feasible = fb == count;
      if (feasible) r.flags |= COX_SEG_FEASIBLE;
      if (P.crop) {
        const bool long_enough = !(len < P.crop_min_length);  // the planner's early return
        if (feasible) {
          r.free_length = len;
          if (long_enough) {
#pragma unroll
            for (int k = 0; k < 3; ++k) r.goal[k] = sp.a[k] + sp.dir[k];
            r.flags |= COX_SEG_GOAL;
          }
        } else {
          const float fl = len * (static_cast<float>(static_cast<int>(fb) - 1) / sp.nf) - P.crop_margin;
          r.free_length = fl;
          if (long_enough && fl > P.crop_min_length) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const float u = sp.dir[k] / len;
              r.goal[k] = sp.a[k] + u * fl;
            }
            r.flags |= COX_SEG_GOAL;
          }
        }
      }
    }
    out[seg] = r;
  }
  add_stats(evaluated, count - evaluated, leader, stats);
}

struct TrajectoryPos {
  const float* xyz;
  __device__ __forceinline__ void operator()(u32 i, float p[3]) const {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = xyz[3 * static_cast<u64>(i) + k];
  }
};

// rule T
template <int G>
__global__ void __launch_bounds__(kThreads) k_collide_trajectories(LayerView L, CollideParams P, const u64* __restrict__ offsets, u64 n_traj,
                                                                   const float* __restrict__ xyz, u64 n_points, cox_collide_record* __restrict__ out,
                                                                   ull* __restrict__ stats) {
  const u64 t = static_cast<u64>(blockIdx.x) * (kThreads / G) + threadIdx.x / G;
  const bool live = t < n_traj;
  const bool leader = live && (threadIdx.x & (G - 1)) == 0;
  u32 count = 0;
  TrajectoryPos tp{xyz};
  if (live) {
    u64 end = offsets[t + 1], begin = offsets[t];
    if (end > n_points) end = n_points;
    if (begin > end) begin = end;
    const u64 m = end - begin;
    count = m > 0x7FFFFFFFull ? 0x7FFFFFFFu : static_cast<u32>(m);  // base + lane stays below 2^32
    tp.xyz = xyz + 3 * begin;
  }
  u32 evaluated = 0;
  const u32 fb = first_blocked_scan<G>(L, P, count, tp, &evaluated);
  if (leader) {
    cox_collide_record r;
    r.n_samples = count;
    r.first_blocked = fb;
    r.flags = fb == count ? COX_SEG_FEASIBLE : 0u;
    r.pad = 0u;
    const float nan = __uint_as_float(0x7FC00000u);
    r.free_length = nan;
    r.goal[0] = r.goal[1] = r.goal[2] = nan;
    out[t] = r;
  }
  add_stats(evaluated, count - evaluated, leader, stats);
}

// ---- rule R: pointer jumping -----------------------------------------------------------------------------------------------
// One word per node: bit 0 = every segment from the node up to (not including) its ancestor is feasible; bits 1.. = ancestor + 2,
// where 0 stands for "the walk failed" (a parent index out of range) and 1 for "a root was reached".  A round replaces the
// ancestor by the ancestor's ancestor; after ceil(log2 n) rounds every node of a proper forest has reached a root, and a node that
// still has an ancestor then is on or under a cycle.
constexpr u32 kWalkFailed = 0u, kRootReached = 1u;

__device__ __forceinline__ u32 prune_word(int parent, u32 n, bool feasible) {
  u32 anc;
  if (parent == -1)
    anc = kRootReached;
  else if (parent < 0 || static_cast<u32>(parent) >= n)
    anc = kWalkFailed;
  else
    anc = static_cast<u32>(parent) + 2u;
  return (anc << 1) | (feasible ? 1u : 0u);
}
__device__ __forceinline__ u32 prune_jump(u32 w, u32 wa) { return (wa & ~1u) | (w & wa & 1u); }  // wa: the word of w's ancestor
__device__ __forceinline__ uint8_t prune_keep(u32 w) {
  const u32 anc = w >> 1;
  if (anc != kRootReached) return COX_TREE_INVALID;
  return (w & 1u) ? COX_TREE_KEEP : 0u;
}

__global__ void __launch_bounds__(kPruneThreads) k_prune_small(const int* __restrict__ parent, const uint8_t* __restrict__ feasible, u64 stride, u32 n,
                                                               int rounds, uint8_t* __restrict__ keep) {
  __shared__ u32 buf[2][kPruneSmall];
  for (u32 i = threadIdx.x; i < n; i += kPruneThreads) buf[0][i] = prune_word(parent[i], n, (feasible[i * stride] & 1u) != 0u);
  __syncthreads();
  int cur = 0;
  for (int r = 0; r < rounds; ++r) {
    for (u32 i = threadIdx.x; i < n; i += kPruneThreads) {
      const u32 w = buf[cur][i];
      const u32 anc = w >> 1;
      buf[cur ^ 1][i] = anc >= 2u ? prune_jump(w, buf[cur][anc - 2u]) : w;
    }
    __syncthreads();
    cur ^= 1;
  }
  for (u32 i = threadIdx.x; i < n; i += kPruneThreads) keep[i] = prune_keep(buf[cur][i]);
}

__global__ void __launch_bounds__(kThreads) k_prune_init(const int* __restrict__ parent, const uint8_t* __restrict__ feasible, u64 stride, u32 n,
                                                         u32* __restrict__ words) {
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) words[i] = prune_word(parent[i], n, (feasible[i * stride] & 1u) != 0u);
}
__global__ void __launch_bounds__(kThreads) k_prune_round(const u32* __restrict__ in, u32* __restrict__ out, u32 n) {
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const u32 w = in[i];
  const u32 anc = w >> 1;
  out[i] = anc >= 2u ? prune_jump(w, in[anc - 2u]) : w;
}
__global__ void __launch_bounds__(kThreads) k_prune_finish(const u32* __restrict__ words, u32 n, uint8_t* __restrict__ keep) {
  const u32 i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) keep[i] = prune_keep(words[i]);
}

bool config_ok(const cox_collide_config& c) {
  const float s[] = {c.collision_radius, c.clearing_radius, c.sample_spacing, c.max_extension_range, c.crop_margin, c.crop_min_length};
  if (!finite_all(s, 6) || !finite_all(c.clearing_centre, 3)) return false;
  if (c.clearing_radius < 0.0f || c.sample_spacing < 0.0f || c.crop_margin < 0.0f || c.crop_min_length < 0.0f) return false;
  return c.max_samples <= kMaxMaxSamples;
}

}  // namespace

struct cox_collide {
  cox_layer* layer = nullptr;
  cox_collide_config cfg;
  CollideParams P;
  int group = 32;
  bool profiling = false, timing_pending = false;
  Stream stream;
  EventPair ev;
  DevBuf<ull> d_stats;  // evaluated, skipped
  u64 n_launches = 0;
  double kernel_ms = 0.0;
  DevBuf<u32> d_words;      // pointer-jumping buffers, 2 x n
  DevBuf<uint8_t> d_stage;  // staging of the host entry points
};

namespace {

// a profiled call: events around its kernels on s; the time is collected by the next host entry point or cox_collide_stats
void settle_timing(cox_collide* H) {
  if (!H->timing_pending) return;
  H->timing_pending = false;
  double ms = 0.0;
  if (hipEventSynchronize(H->ev.b) != hipSuccess)
    (void)hipGetLastError();
  else if (H->ev.elapsed_ms(&ms))
    H->kernel_ms += ms;
}
struct Timed {
  cox_collide* H;
  hipStream_t s;
  Timed(cox_collide* h, hipStream_t st) : H(h), s(st) {
    if (H->profiling) {
      settle_timing(H);
      (void)H->ev.begin(s);
    }
  }
  ~Timed() {
    if (H->profiling) {
      (void)H->ev.end(s);
      H->timing_pending = true;
    }
  }
};

u32 blocks_for(u64 items, u64 per_block) { return static_cast<u32>((items + per_block - 1) / per_block); }

int enqueue_points(cox_collide* H, const float* xyz, u64 n, uint8_t* state, float* distance, hipStream_t s) {
  hipLaunchKernelGGL(k_collide_points, dim3(blocks_for(n, kThreads)), dim3(kThreads), 0, s, layer_view(H->layer), H->P, xyz, n, state, distance,
                     H->d_stats.p);
  H->n_launches++;
  COX_HIP(hipGetLastError());
  return COX_OK;
}

int enqueue_segments(cox_collide* H, const float* a, const float* b, u64 n, cox_collide_record* out, hipStream_t s) {
  const LayerView V = layer_view(H->layer);  // read on every call: a layer that grew has new buffers
  if (H->group == 64)
    hipLaunchKernelGGL((k_collide_segments<64>), dim3(blocks_for(n, kThreads / 64)), dim3(kThreads), 0, s, V, H->P, a, b, n, out, H->d_stats.p);
  else
    hipLaunchKernelGGL((k_collide_segments<32>), dim3(blocks_for(n, kThreads / 32)), dim3(kThreads), 0, s, V, H->P, a, b, n, out, H->d_stats.p);
  H->n_launches++;
  COX_HIP(hipGetLastError());
  return COX_OK;
}

int enqueue_trajectories(cox_collide* H, const u64* offsets, u64 n_traj, const float* xyz, u64 n_points, cox_collide_record* out, hipStream_t s) {
  const LayerView V = layer_view(H->layer);
  if (H->group == 64)
    hipLaunchKernelGGL((k_collide_trajectories<64>), dim3(blocks_for(n_traj, kThreads / 64)), dim3(kThreads), 0, s, V, H->P, offsets, n_traj, xyz,
                       n_points, out, H->d_stats.p);
  else
    hipLaunchKernelGGL((k_collide_trajectories<32>), dim3(blocks_for(n_traj, kThreads / 32)), dim3(kThreads), 0, s, V, H->P, offsets, n_traj, xyz,
                       n_points, out, H->d_stats.p);
  H->n_launches++;
  COX_HIP(hipGetLastError());
  return COX_OK;
}

int enqueue_prune(cox_collide* H, const int32_t* parent, const uint8_t* feasible, u64 stride, u64 n64, uint8_t* keep, hipStream_t s) {
  const u32 n = static_cast<u32>(n64);
  const int rounds = ceil_log2(n64) + 1;
  if (n <= kPruneSmall) {
    hipLaunchKernelGGL(k_prune_small, dim3(1), dim3(kPruneThreads), 0, s, parent, feasible, stride, n, rounds, keep);
    H->n_launches++;
  } else {
    COX_TRY(H->d_words.grow(2 * n64));
    u32* w0 = H->d_words.p;
    u32* w1 = H->d_words.p + n64;
    const dim3 grid(blocks_for(n64, kThreads));
    hipLaunchKernelGGL(k_prune_init, grid, dim3(kThreads), 0, s, parent, feasible, stride, n, w0);
    for (int r = 0; r < rounds; ++r) {
      hipLaunchKernelGGL(k_prune_round, grid, dim3(kThreads), 0, s, w0, w1, n);
      u32* t = w0;
      w0 = w1;
      w1 = t;
    }
    hipLaunchKernelGGL(k_prune_finish, grid, dim3(kThreads), 0, s, w0, n, keep);
    H->n_launches += static_cast<u64>(rounds) + 2;
  }
  COX_HIP(hipGetLastError());
  return COX_OK;
}

int check_batch(u64 n, u64 per_block) { return n > 0x7FFFFFFFull * per_block ? COX_ERR_INVALID_ARG : COX_OK; }  // grid size

// the common head of every entry point that launches
int begin_call(cox_collide* H, hipStream_t s) {
  COX_HIP(hipSetDevice(H->layer->device));
  cox_layer_wait_writes(H->layer, s);  // frames still in flight on the layer
  return COX_OK;
}

int collide_resources(cox_collide* H) {
  COX_TRY(H->stream.create());
  COX_TRY(H->ev.create());
  COX_TRY(H->d_stats.alloc(2));
  return cox_hip_status(hipMemset(H->d_stats.p, 0, 2 * sizeof(ull)));
}

}  // namespace

extern "C" {

void cox_collide_config_default(cox_collide_config* cfg) {
  if (!cfg) return;
  cfg->collision_radius = 2.0f;
  cfg->collision_optimistic = 0;
  cfg->clearing_radius = 0.0f;
  for (int k = 0; k < 3; ++k) cfg->clearing_centre[k] = 0.0f;
  cfg->sample_spacing = 0.05f;
  cfg->max_samples = kDefaultMaxSamples;
  cfg->max_extension_range = 1.5f;
  cfg->crop = 1;
  cfg->crop_margin = 0.3f;
  cfg->crop_min_length = 0.5f;
}

int cox_collide_create(cox_layer_t* layer, const cox_collide_config* cfg, cox_collide_t** out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!layer || !out) return COX_ERR_INVALID_ARG;
  cox_collide_config c;
  if (cfg)
    c = *cfg;
  else
    cox_collide_config_default(&c);
  if (!config_ok(c)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(layer->device));
  cox_collide* H = new (std::nothrow) cox_collide();
  if (!H) return COX_ERR_OUT_OF_MEMORY;
  H->layer = layer;
  H->cfg = c;
  CollideParams& P = H->P;
  P.radius = c.collision_radius, P.clearing_radius = c.clearing_radius;
  for (int k = 0; k < 3; ++k) P.centre[k] = c.clearing_centre[k];
  P.ds = c.sample_spacing == 0.0f ? layer->voxel_size : c.sample_spacing;
  P.max_ext = c.max_extension_range, P.crop_margin = c.crop_margin, P.crop_min_length = c.crop_min_length;
  P.max_samples = c.max_samples ? c.max_samples : kDefaultMaxSamples;
  P.optimistic = c.collision_optimistic != 0, P.crop = c.crop != 0;
  if (collide_resources(H) != COX_OK) {
    cox_collide_destroy(H);
    return COX_ERR_NO_DEVICE;
  }
  *out = H;
  return COX_OK;
}

void cox_collide_destroy(cox_collide_t* H) {
  if (!H) return;
  (void)hipSetDevice(H->layer->device);
  if (H->stream) (void)hipStreamSynchronize(H->stream);
  delete H;
}

int cox_collide_set_clearing_centre(cox_collide_t* H, const float centre[3]) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || !centre || !finite_all(centre, 3)) return COX_ERR_INVALID_ARG;
  for (int k = 0; k < 3; ++k) H->P.centre[k] = H->cfg.clearing_centre[k] = centre[k];
  return COX_OK;
}

int cox_collide_set_group_size(cox_collide_t* H, int lanes) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H || (lanes != 32 && lanes != 64)) return COX_ERR_INVALID_ARG;
  H->group = lanes;
  return COX_OK;
}

int cox_collide_set_profiling(cox_collide_t* H, int on) {
  COX_ENTRY_NO_DRAIN();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (!on) settle_timing(H);
  H->profiling = on != 0;
  return COX_OK;
}

int cox_collide_stats(cox_collide_t* H, cox_collide_stats_t* out, int reset) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H || !out) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(H->layer->device));
  settle_timing(H);
  ull c[2] = {0, 0};
  COX_HIP(hipMemcpy(c, H->d_stats.p, sizeof(c), hipMemcpyDeviceToHost));
  out->n_samples_evaluated = c[0];
  out->n_samples_skipped = c[1];
  out->n_launches = H->n_launches;
  out->kernel_ms = H->kernel_ms;
  if (reset) {
    COX_HIP(hipMemset(H->d_stats.p, 0, sizeof(c)));
    H->n_launches = 0;
    H->kernel_ms = 0.0;
  }
  return COX_OK;
}

int cox_collide_points(cox_collide_t* H, const float* xyz, uint64_t n, uint8_t* state, float* distance) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  if (!xyz) return COX_ERR_INVALID_ARG;
  COX_TRY(check_batch(n, kThreads));
  hipStream_t s = H->stream;
  COX_TRY(begin_call(H, s));
  // staging: xyz | distance | state
  const u64 b_xyz = 12 * n, b_d = distance ? 4 * n : 0, b_s = state ? n : 0;
  COX_TRY(H->d_stage.grow(b_xyz + b_d + b_s));
  float* d_xyz = reinterpret_cast<float*>(H->d_stage.p);
  float* d_d = distance ? reinterpret_cast<float*>(H->d_stage.p + b_xyz) : nullptr;
  uint8_t* d_s = state ? H->d_stage.p + b_xyz + b_d : nullptr;
  COX_HIP(hipMemcpyAsync(d_xyz, xyz, b_xyz, hipMemcpyHostToDevice, s));
  if (d_d) COX_HIP(hipMemsetAsync(d_d, 0xFF, b_d, s));  // NaN where nothing is written
  {
    Timed t(H, s);
    COX_TRY(enqueue_points(H, d_xyz, n, d_s, d_d, s));
  }
  if (distance) COX_HIP(hipMemcpyAsync(distance, d_d, b_d, hipMemcpyDeviceToHost, s));
  if (state) COX_HIP(hipMemcpyAsync(state, d_s, b_s, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  return COX_OK;
}

int cox_collide_points_dev(cox_collide_t* H, const float* xyz_dev, uint64_t n, uint8_t* state_dev, float* distance_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  if (!xyz_dev) return COX_ERR_INVALID_ARG;
  COX_TRY(check_batch(n, kThreads));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  COX_TRY(begin_call(H, s));
  Timed t(H, s);
  return enqueue_points(H, xyz_dev, n, state_dev, distance_dev, s);
}

int cox_collide_segments(cox_collide_t* H, const float* a, const float* b, uint64_t n, cox_collide_record* out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  if (!a || !b || !out) return COX_ERR_INVALID_ARG;
  COX_TRY(check_batch(n, kThreads / 64));
  hipStream_t s = H->stream;
  COX_TRY(begin_call(H, s));
  // staging: records | a | b
  const u64 b_rec = sizeof(cox_collide_record) * n, b_pts = 12 * n;
  COX_TRY(H->d_stage.grow(b_rec + 2 * b_pts));
  cox_collide_record* d_rec = reinterpret_cast<cox_collide_record*>(H->d_stage.p);
  float* d_a = reinterpret_cast<float*>(H->d_stage.p + b_rec);
  float* d_b = reinterpret_cast<float*>(H->d_stage.p + b_rec + b_pts);
  COX_HIP(hipMemcpyAsync(d_a, a, b_pts, hipMemcpyHostToDevice, s));
  COX_HIP(hipMemcpyAsync(d_b, b, b_pts, hipMemcpyHostToDevice, s));
  {
    Timed t(H, s);
    COX_TRY(enqueue_segments(H, d_a, d_b, n, d_rec, s));
  }
  COX_HIP(hipMemcpyAsync(out, d_rec, b_rec, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  return COX_OK;
}

int cox_collide_segments_dev(cox_collide_t* H, const float* a_dev, const float* b_dev, uint64_t n, cox_collide_record* out_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  if (!a_dev || !b_dev || !out_dev || (reinterpret_cast<uintptr_t>(out_dev) & 3u)) return COX_ERR_INVALID_ARG;
  COX_TRY(check_batch(n, kThreads / 64));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  COX_TRY(begin_call(H, s));
  Timed t(H, s);
  return enqueue_segments(H, a_dev, b_dev, n, out_dev, s);
}

}  // extern "C"

namespace {

int check_csr(const uint64_t* offsets, u64 n_traj, u64 n_points) {
  if (offsets[0] > n_points) return COX_ERR_INVALID_ARG;
  for (u64 t = 0; t < n_traj; ++t) {
    if (offsets[t + 1] < offsets[t] || offsets[t + 1] > n_points) return COX_ERR_INVALID_ARG;
    if (offsets[t + 1] - offsets[t] > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  }
  return COX_OK;
}

// host form of trajectories and tree: parent / keep NULL -> trajectories only
int host_trajectories(cox_collide* H, const uint64_t* offsets, const int32_t* parent, u64 n, const float* xyz, u64 n_points, cox_collide_record* out,
                      uint8_t* keep) {
  COX_TRY(check_csr(offsets, n, n_points));
  hipStream_t s = H->stream;
  COX_TRY(begin_call(H, s));
  // staging: records | offsets | xyz | parent | keep
  const u64 b_rec = sizeof(cox_collide_record) * n, b_off = 8 * (n + 1), b_xyz = 12 * n_points, b_par = parent ? 4 * n : 0, b_keep = keep ? n : 0;
  COX_TRY(H->d_stage.grow(b_rec + b_off + b_xyz + b_par + b_keep));
  uint8_t* base = H->d_stage.p;
  cox_collide_record* d_rec = reinterpret_cast<cox_collide_record*>(base);
  u64* d_off = reinterpret_cast<u64*>(base + b_rec);
  float* d_xyz = reinterpret_cast<float*>(base + b_rec + b_off);
  int32_t* d_par = reinterpret_cast<int32_t*>(base + b_rec + b_off + b_xyz);
  uint8_t* d_keep = base + b_rec + b_off + b_xyz + b_par;
  COX_HIP(hipMemcpyAsync(d_off, offsets, b_off, hipMemcpyHostToDevice, s));
  if (b_xyz) COX_HIP(hipMemcpyAsync(d_xyz, xyz, b_xyz, hipMemcpyHostToDevice, s));
  if (parent) COX_HIP(hipMemcpyAsync(d_par, parent, b_par, hipMemcpyHostToDevice, s));
  {
    Timed t(H, s);
    COX_TRY(enqueue_trajectories(H, d_off, n, d_xyz, n_points, d_rec, s));
    if (parent) COX_TRY(enqueue_prune(H, d_par, reinterpret_cast<const uint8_t*>(&d_rec->flags), sizeof(cox_collide_record), n, d_keep, s));
  }
  if (out) COX_HIP(hipMemcpyAsync(out, d_rec, b_rec, hipMemcpyDeviceToHost, s));
  if (keep) COX_HIP(hipMemcpyAsync(keep, d_keep, b_keep, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  return COX_OK;
}

}  // namespace

extern "C" {

int cox_collide_trajectories(cox_collide_t* H, const uint64_t* offsets, uint64_t n_traj, const float* xyz, uint64_t n_points, cox_collide_record* out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n_traj == 0) return COX_OK;
  if (!offsets || !out || (n_points > 0 && !xyz)) return COX_ERR_INVALID_ARG;
  COX_TRY(check_batch(n_traj, kThreads / 64));
  return host_trajectories(H, offsets, nullptr, n_traj, xyz, n_points, out, nullptr);
}

int cox_collide_trajectories_dev(cox_collide_t* H, const uint64_t* offsets_dev, uint64_t n_traj, const float* xyz_dev, uint64_t n_points,
                                 cox_collide_record* out_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n_traj == 0) return COX_OK;
  if (!offsets_dev || !out_dev || (n_points > 0 && !xyz_dev) || (reinterpret_cast<uintptr_t>(out_dev) & 3u)) return COX_ERR_INVALID_ARG;
  COX_TRY(check_batch(n_traj, kThreads / 64));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  COX_TRY(begin_call(H, s));
  Timed t(H, s);
  return enqueue_trajectories(H, offsets_dev, n_traj, xyz_dev, n_points, out_dev, s);
}

int cox_collide_prune_dev(cox_collide_t* H, const int32_t* parent_dev, const uint8_t* feasible_dev, uint64_t feasible_stride, uint64_t n,
                          uint8_t* keep_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  if (!parent_dev || !feasible_dev || !keep_dev || feasible_stride == 0 || n > kMaxTree) return COX_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  COX_HIP(hipSetDevice(H->layer->device));
  Timed t(H, s);
  return enqueue_prune(H, parent_dev, feasible_dev, feasible_stride, n, keep_dev, s);
}

int cox_collide_tree(cox_collide_t* H, const uint64_t* offsets, const int32_t* parent, uint64_t n_nodes, const float* xyz, uint64_t n_points,
                     cox_collide_record* out, uint8_t* keep) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n_nodes == 0) return COX_OK;
  if (!offsets || !parent || !keep || (n_points > 0 && !xyz) || n_nodes > kMaxTree) return COX_ERR_INVALID_ARG;
  return host_trajectories(H, offsets, parent, n_nodes, xyz, n_points, out, keep);
}

int cox_collide_tree_dev(cox_collide_t* H, const uint64_t* offsets_dev, const int32_t* parent_dev, uint64_t n_nodes, const float* xyz_dev,
                         uint64_t n_points, cox_collide_record* out_dev, uint8_t* keep_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!H) return COX_ERR_INVALID_ARG;
  if (n_nodes == 0) return COX_OK;
  if (!offsets_dev || !parent_dev || !out_dev || !keep_dev || (n_points > 0 && !xyz_dev) || n_nodes > kMaxTree ||
      (reinterpret_cast<uintptr_t>(out_dev) & 3u))
    return COX_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  COX_TRY(begin_call(H, s));
  Timed t(H, s);
  COX_TRY(enqueue_trajectories(H, offsets_dev, n_nodes, xyz_dev, n_points, out_dev, s));
  return enqueue_prune(H, parent_dev, reinterpret_cast<const uint8_t*>(&out_dev->flags), sizeof(cox_collide_record), n_nodes, keep_dev, s);
}

}  // extern "C"
