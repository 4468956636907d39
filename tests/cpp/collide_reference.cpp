// Test-side reference of the GPU collision checks (coxgraph_amd/csrc/cox_collide.hip), loaded by tests/collide_ref.py through
// ctypes.  Rules S, L, T and R of DESIGN.md section 7k, one expression at a time, single-threaded, no early exit.
//
// The trilinear branch is the CPU checker's own getVoxelsAndQVector + interpMember (oracle/cox_oracle.hpp) on an oracle Layer
// rebuilt from wire arrays; "observed" is Block::getVoxelByCoordinates as tests/cpp/map_reference.cpp restates it.  Rule R is a
// plain walk to the root with a visited set.
// Build: g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -fno-fast-math (as oracle/Makefile).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../oracle/cox_oracle.hpp"

using namespace coxo;

namespace {

enum : uint32_t { kTraversable = 1, kObserved = 2, kDistance = 4, kCleared = 8, kInvalid = 16 };
enum : uint32_t { kFeasible = 1, kGoal = 2, kClamped = 4, kTooLong = 8, kSegInvalid = 16 };
enum : uint8_t { kKeep = 1, kTreeInvalid = 2 };

struct Config {  // cox_collide_config
  float collision_radius;
  int32_t collision_optimistic;
  float clearing_radius;
  float clearing_centre[3];
  float sample_spacing;
  uint32_t max_samples;
  float max_extension_range;
  int32_t crop;
  float crop_margin;
  float crop_min_length;
};

struct Record {  // cox_collide_record
  uint32_t n_samples, first_blocked, flags;
  float free_length, goal[3];
  uint32_t pad;
};
static_assert(sizeof(Record) == 32, "record size");

float dotSelf(float x, float y, float z) { return (x * x + y * y) + z * z; }
bool inRange(float s) { return s > -1048575.0f && s < 1048575.0f; }

// EsdfMap::isObserved: the voxel containing pos (Block::getVoxelByCoordinates) has weight > 0
bool isObserved(const Layer& L, V3 pos) {
  const Block* blk = L.getBlockPtr(blockIndexFromPoint(pos, L.block_size_inv));
  if (!blk) return false;
  const GIdx gi = gridIndexFromPoint(pos - blk->origin, L.voxel_size_inv);
  int vi[3] = {static_cast<int>(gi.x), static_cast<int>(gi.y), static_cast<int>(gi.z)};
  for (int k = 0; k < 3; ++k) vi[k] = std::max(std::min(vi[k], L.vps - 1), 0);
  return blk->voxels[linearIndex(vi[0], vi[1], vi[2], L.vps)].weight > 0.0f;
}

// EsdfMap::getDistanceAtPosition(pos, interpolate = true)
bool getDistance(const Layer& L, V3 pos, float* d) {
  const Interp it = getVoxelsAndQVector(L, pos);
  if (!it.ok) return false;
  const float dx = it.off[0], dy = it.off[1], dz = it.off[2];
  const float q[8] = {1.0f, dx, dy, dz, dx * dy, dy * dz, dz * dx, dx * dy * dz};
  *d = interpMember(q, it.d);
  return true;
}

// rule S
uint32_t sampleState(const Layer& L, const Config& c, V3 p, float* dist) {
  if (!(inRange(p.x * L.block_size_inv) && inRange(p.y * L.block_size_inv) && inRange(p.z * L.block_size_inv))) return kInvalid;
  if (isObserved(L, p)) {
    float d;
    if (!getDistance(L, p, &d)) return kObserved;
    if (dist) *dist = d;
    return kObserved | kDistance | (d > c.collision_radius ? kTraversable : 0u);
  }
  if (c.clearing_radius > 0.0f) {
    const float r = std::sqrt(dotSelf(p.x - c.clearing_centre[0], p.y - c.clearing_centre[1], p.z - c.clearing_centre[2]));
    return r < c.clearing_radius ? (kCleared | kTraversable) : 0u;
  }
  return c.collision_optimistic ? kTraversable : 0u;
}

bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

void blankRecord(Record* r) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  std::memset(r, 0, sizeof(Record));
  r->free_length = nan;
  r->goal[0] = r->goal[1] = r->goal[2] = nan;
}

// rule L.  margin (may be null): the smallest |distance - collision_radius| over the samples looked at
Record segment(const Layer& L, const Config& c, const float* a, const float* b, float* margin, uint64_t* n_looked) {
  Record r;
  blankRecord(&r);
  float dir[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  float len = std::sqrt(dotSelf(dir[0], dir[1], dir[2]));
  if (!(finite3(a) && finite3(b) && std::isfinite(len))) {
    r.flags = kSegInvalid;
    return r;
  }
  if (c.max_extension_range > 0.0f && len > c.max_extension_range) {
    const float s = c.max_extension_range / len;
    for (int k = 0; k < 3; ++k) dir[k] = dir[k] * s;
    len = std::sqrt(dotSelf(dir[0], dir[1], dir[2]));
    r.flags |= kClamped;
  }
  const float ds = c.sample_spacing == 0.0f ? L.voxel_size : c.sample_spacing;
  const float nfl = std::ceil(len / ds);
  uint32_t n = nfl >= 4294967296.0f ? 0xFFFFFFFFu : static_cast<uint32_t>(nfl);
  if (n < 1u) n = 1u;
  r.n_samples = n;
  const uint32_t max_samples = c.max_samples ? c.max_samples : 4096u;
  if (n > max_samples) {
    r.flags |= kTooLong;
    return r;
  }
  uint32_t first = n + 1u;
  for (uint32_t i = 0; i <= n; ++i) {
    const float t = static_cast<float>(i) / static_cast<float>(n);
    const V3 p{a[0] + t * dir[0], a[1] + t * dir[1], a[2] + t * dir[2]};
    float d = 0.0f;
    const uint32_t st = sampleState(L, c, p, &d);
    if (n_looked) ++*n_looked;
    if (margin && (st & kDistance)) *margin = std::min(*margin, std::fabs(d - c.collision_radius));
    if (!(st & kTraversable) && first == n + 1u) first = i;
  }
  r.first_blocked = first;
  const bool feasible = first == n + 1u;
  if (feasible) r.flags |= kFeasible;
  if (c.crop) {
    const bool long_enough = !(len < c.crop_min_length);
    if (feasible) {
      r.free_length = len;
      if (long_enough) {
        for (int k = 0; k < 3; ++k) r.goal[k] = a[k] + dir[k];
        r.flags |= kGoal;
      }
    } else {
      const float free_length = len * (static_cast<float>(static_cast<int>(first) - 1) / static_cast<float>(n)) - c.crop_margin;
      r.free_length = free_length;
      if (long_enough && free_length > c.crop_min_length) {
        for (int k = 0; k < 3; ++k) {
          const float u = dir[k] / len;
          r.goal[k] = a[k] + u * free_length;
        }
        r.flags |= kGoal;
      }
    }
  }
  return r;
}

// rule T
Record trajectory(const Layer& L, const Config& c, const float* xyz, uint64_t m) {
  Record r;
  blankRecord(&r);
  r.n_samples = static_cast<uint32_t>(m);
  uint32_t first = static_cast<uint32_t>(m);
  for (uint64_t i = 0; i < m; ++i) {
    const uint32_t st = sampleState(L, c, V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}, nullptr);
    if (!(st & kTraversable)) {
      first = static_cast<uint32_t>(i);
      break;
    }
  }
  r.first_blocked = first;
  if (first == m) r.flags = kFeasible;
  return r;
}

}  // namespace

extern "C" {

// the layer given as wire arrays (block_idx 3 int32 per block, words 4096 * 3 uint32 per block)
void* collide_ref_build(float voxel_size, uint64_t n_blocks, const int32_t* block_idx, const uint32_t* words) {
  Layer* L = new Layer(voxel_size, 16);
  for (uint64_t i = 0; i < n_blocks; ++i) {
    Block* b = L->allocateBlock(BIdx{block_idx[3 * i], block_idx[3 * i + 1], block_idx[3 * i + 2]});
    for (int v = 0; v < 4096; ++v) wordsToVoxel(words + (i * 4096 + v) * 3, &b->voxels[v]);
  }
  return L;
}

void collide_ref_free(void* h) { delete static_cast<Layer*>(h); }

// state[n], distance[n] (left untouched without the distance flag)
void collide_ref_points(const void* h, const Config* c, const float* xyz, uint64_t n, uint8_t* state, float* distance) {
  const Layer& L = *static_cast<const Layer*>(h);
  for (uint64_t i = 0; i < n; ++i) {
    float d = 0.0f;
    const uint32_t st = sampleState(L, *c, V3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}, &d);
    state[i] = static_cast<uint8_t>(st);
    if ((st & kDistance) && distance) distance[i] = d;
  }
}

// out[n]; *min_margin: the smallest |distance - collision_radius| over every sample of the batch; *n_samples: samples looked at.
// Returns the seconds spent.
double collide_ref_segments(const void* h, const Config* c, const float* a, const float* b, uint64_t n, Record* out, float* min_margin,
                            uint64_t* n_samples) {
  const Layer& L = *static_cast<const Layer*>(h);
  float margin = std::numeric_limits<float>::infinity();
  uint64_t looked = 0;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t i = 0; i < n; ++i) out[i] = segment(L, *c, a + 3 * i, b + 3 * i, &margin, &looked);
  const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (min_margin) *min_margin = margin;
  if (n_samples) *n_samples = looked;
  return sec;
}

void collide_ref_trajectories(const void* h, const Config* c, const uint64_t* offsets, uint64_t n_traj, const float* xyz, Record* out) {
  const Layer& L = *static_cast<const Layer*>(h);
  for (uint64_t t = 0; t < n_traj; ++t) out[t] = trajectory(L, *c, xyz + 3 * offsets[t], offsets[t + 1] - offsets[t]);
}

// rule R: every node walks to its root; visited marks the nodes of the current walk
void collide_ref_prune(const int32_t* parent, const uint8_t* feasible, uint64_t stride, uint64_t n, uint8_t* keep) {
  std::vector<uint64_t> visited(n, ~0ull);
  for (uint64_t i = 0; i < n; ++i) {
    bool ok = true, valid = true;
    int64_t j = static_cast<int64_t>(i);
    while (true) {
      if (visited[j] == i) {  // a cycle
        valid = false;
        break;
      }
      visited[j] = i;
      ok = ok && (feasible[static_cast<uint64_t>(j) * stride] & 1u);
      const int32_t p = parent[j];
      if (p == -1) break;
      if (p < 0 || static_cast<uint64_t>(p) >= n) {
        valid = false;
        break;
      }
      j = p;
    }
    keep[i] = !valid ? kTreeInvalid : (ok ? kKeep : 0);
  }
}

}  // extern "C"
