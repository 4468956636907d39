// Test-side reference of the view-gain evaluator (coxgraph_amd/csrc/cox_viewgain.hip), loaded by tests/viewgain_ref.py through ctypes.
//
// Written from the rules of DESIGN.md section 7j, not from the kernel: single-threaded, ray by ray, one std::unordered_set of
// voxel indices per view, every look-up through the oracle Layer's block map (oracle/cox_oracle.hpp), rebuilt from the engine's
// downloaded wire arrays.  No bitmap, no block cache, no box of the view.
// Build: g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -fno-fast-math (as oracle/Makefile).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <unordered_set>
#include <vector>

#include "../../oracle/cox_oracle.hpp"

using namespace coxo;

namespace {

struct Config {  // cox_viewgain_config
  int32_t w, h;
  float K[4];
  float min_range, ray_length, ray_step, min_weight, surface_distance;
  float frontier_voxel_weight, new_voxel_weight, min_impact_factor, ray_angle_x, ray_angle_y;
  int32_t accurate_frontiers, surface_frontiers, use_box;
  float box_min[3], box_max[3];
  uint64_t workspace_bytes;
};

struct Record {
  double gain, surface_gain;
  uint64_t surface_gain_q32;
  uint32_t n_visible, n_free, n_occupied, n_surface_counted, n_unknown, n_frontier;
  uint32_t n_borderline;  // occupied visible voxels whose impact is within 1e-5 (relative) of min_impact_factor
  uint32_t pad;
  uint64_t n_samples;
};

enum : uint8_t { kFree = 0, kOccupied = 1, kUnknown = 2, kFrontier = 3 };
enum State { sFree, sOccupied, sUnknown };

struct Visible {
  GIdx g;
  uint8_t cls;
  float value;
};

bool inRange(float s) { return s > -1048575.0f && s < 1048575.0f; }

int floorDiv16(int64_t g) { return static_cast<int>(g >> 4); }

// rule 3 for the voxel with global index g
State stateOf(const Layer& L, const Config& c, GIdx g, float* weight) {
  const Block* blk = L.getBlockPtr(BIdx{floorDiv16(g.x), floorDiv16(g.y), floorDiv16(g.z)});
  if (!blk) return sUnknown;
  const TsdfVoxel& v = blk->voxels[linearIndex(static_cast<int>(g.x & 15), static_cast<int>(g.y & 15), static_cast<int>(g.z & 15), 16)];
  *weight = v.weight;
  if (!(v.weight > c.min_weight)) return sUnknown;
  return v.distance <= c.surface_distance ? sOccupied : sFree;
}

float centre(const Layer& L, int64_t g) {
  const int b = floorDiv16(g);
  const int v = static_cast<int>(g & 15);
  return static_cast<float>(b) * L.block_size + (static_cast<float>(v) + 0.5f) * L.voxel_size;
}

bool isFrontier(const Layer& L, const Config& c, GIdx g) {
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int axes = (dx != 0) + (dy != 0) + (dz != 0);
        if (axes == 0 || (!c.accurate_frontiers && axes != 1)) continue;
        float w;
        const State s = stateOf(L, c, GIdx{g.x + dx, g.y + dy, g.z + dz}, &w);
        if (c.surface_frontiers ? s == sOccupied : s != sUnknown) return true;
      }
  return false;
}

// one view: the record, and (when list != nullptr) the visible set in insertion order
void evaluateView(const Layer& L, const Config& c, const float T[7], Record* out, std::vector<Visible>* list) {
  const Transform Tf{T[0], T[1], T[2], T[3], V3{T[4], T[5], T[6]}};
  const float o[3] = {T[4], T[5], T[6]};
  const float step = c.ray_step == 0.0f ? L.voxel_size : c.ray_step;
  const float angle_xy = c.ray_angle_x * c.ray_angle_y;
  Record R{};
  std::unordered_set<GIdx, LongIndexHash> seen;
  for (int v = 0; v < c.h; ++v)
    for (int u = 0; u < c.w; ++u) {
      // rule 1
      const float x = (static_cast<float>(u) - c.K[2]) / c.K[0];
      const float y = (static_cast<float>(v) - c.K[3]) / c.K[1];
      const float n = std::sqrt(x * x + y * y + 1.0f);
      const V3 dg = rotate(Tf, V3{x / n, y / n, 1.0f / n});
      const float dir[3] = {dg.x, dg.y, dg.z};
      // rule 2
      for (uint32_t k = 0;; ++k) {
        const float d = static_cast<float>(k) * step;
        if (!(d < c.ray_length)) break;
        if (d < c.min_range) continue;
        float p[3];
        for (int a = 0; a < 3; ++a) p[a] = o[a] + d * dir[a];
        if (!(inRange(p[0] * L.block_size_inv) && inRange(p[1] * L.block_size_inv) && inRange(p[2] * L.block_size_inv))) break;
        ++R.n_samples;
        int64_t g[3];
        for (int a = 0; a < 3; ++a) {
          const int b = static_cast<int>(std::floor(p[a] * L.block_size_inv + kEps));
          int vi = static_cast<int>(std::floor((p[a] - static_cast<float>(b) * L.block_size) * L.voxel_size_inv + kEps));
          vi = vi > 15 ? 15 : (vi < 0 ? 0 : vi);
          g[a] = 16 * static_cast<int64_t>(b) + vi;
        }
        const GIdx gi{g[0], g[1], g[2]};
        float weight = 0.0f;
        const State s = stateOf(L, c, gi, &weight);
        // rule 4
        bool in_box = true;
        if (c.use_box)
          for (int a = 0; a < 3; ++a) {
            const float cc = centre(L, g[a]);
            if (cc < c.box_min[a] || cc > c.box_max[a]) in_box = false;
          }
        if (in_box && seen.insert(gi).second) {
          // rule 5
          ++R.n_visible;
          uint8_t cls = kFree;
          float value = 0.0f;
          if (s == sOccupied) {
            cls = kOccupied;
            ++R.n_occupied;
            const float dx = centre(L, g[0]) - o[0], dy = centre(L, g[1]) - o[1], dz = centre(L, g[2]) - o[2];
            const float z = std::sqrt(dx * dx + dy * dy + dz * dz);
            const float a = 2.0f * std::atan2(L.voxel_size, 2.0f * z);
            const float nw = a * a / angle_xy / (z * z);
            const float imp = nw / (nw + weight);
            if (imp > c.min_impact_factor) {
              ++R.n_surface_counted;
              R.surface_gain_q32 += static_cast<uint64_t>(static_cast<double>(imp) * 4294967296.0);
              value = imp;
            }
            if (std::fabs(static_cast<double>(imp) - static_cast<double>(c.min_impact_factor)) <= 1e-5 * static_cast<double>(c.min_impact_factor))
              ++R.n_borderline;
          } else if (s == sUnknown) {
            ++R.n_unknown;
            if (c.frontier_voxel_weight > 0.0f && isFrontier(L, c, gi)) {
              cls = kFrontier;
              ++R.n_frontier;
              value = c.frontier_voxel_weight;
            } else {
              cls = kUnknown;
              value = c.new_voxel_weight;
            }
          } else {
            ++R.n_free;
          }
          if (list) list->push_back(Visible{gi, cls, value});
        }
        if (s == sOccupied) break;
      }
    }
  R.surface_gain = static_cast<double>(R.surface_gain_q32) / 4294967296.0;
  R.gain = R.surface_gain + static_cast<double>(c.frontier_voxel_weight) * static_cast<double>(R.n_frontier) +
           static_cast<double>(c.new_voxel_weight) * static_cast<double>(R.n_unknown - R.n_frontier);
  *out = R;
}

}  // namespace

extern "C" {

// the layer given as wire arrays (block_idx 3 int32 per block, words 4096 * 3 uint32 per block)
void* viewgain_ref_build(float voxel_size, uint64_t n_blocks, const int32_t* block_idx, const uint32_t* words) {
  Layer* L = new Layer(voxel_size, 16);
  for (uint64_t i = 0; i < n_blocks; ++i) {
    Block* b = L->allocateBlock(BIdx{block_idx[3 * i], block_idx[3 * i + 1], block_idx[3 * i + 2]});
    for (int v = 0; v < 4096; ++v) wordsToVoxel(words + (i * 4096 + v) * 3, &b->voxels[v]);
  }
  return L;
}

void viewgain_ref_free(void* h) { delete static_cast<Layer*>(h); }

// returns the seconds taken
double viewgain_ref_evaluate(const void* h, const Config* cfg, const float* poses, uint64_t n_views, Record* out) {
  const Layer& L = *static_cast<const Layer*>(h);
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t i = 0; i < n_views; ++i) evaluateView(L, *cfg, poses + 7 * i, out + i, nullptr);
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the visible set of one view in ascending (z, y, x) order; returns its size, writes at most cap entries
uint64_t viewgain_ref_visible(const void* h, const Config* cfg, const float pose[7], uint64_t cap, int32_t* xyz, uint8_t* cls, float* value) {
  const Layer& L = *static_cast<const Layer*>(h);
  Record R;
  std::vector<Visible> list;
  evaluateView(L, *cfg, pose, &R, &list);
  std::sort(list.begin(), list.end(), [](const Visible& a, const Visible& b) {
    if (a.g.z != b.g.z) return a.g.z < b.g.z;
    if (a.g.y != b.g.y) return a.g.y < b.g.y;
    return a.g.x < b.g.x;
  });
  for (uint64_t i = 0; i < list.size() && i < cap; ++i) {
    xyz[3 * i] = static_cast<int32_t>(list[i].g.x), xyz[3 * i + 1] = static_cast<int32_t>(list[i].g.y), xyz[3 * i + 2] = static_cast<int32_t>(list[i].g.z);
    cls[i] = list[i].cls;
    value[i] = list[i].value;
  }
  return list.size();
}

}  // extern "C"
