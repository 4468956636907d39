// Test-side reference of the GPU map queries (coxgraph_amd/csrc/cox_query.hip), loaded by tests/map_ref.py through ctypes.
//
// The trilinear branch is the CPU checker's own getVoxelsAndQVector + interpMember (oracle/cox_oracle.hpp), run on an oracle
// Layer rebuilt from the engine's downloaded wire arrays.  What the checker does not have -- the nearest lookup
// (Block::getVoxelByCoordinates), Interpolator::getGradient's central differences and getAdaptiveDistanceAndGradient's
// fallback -- is restated here, single-threaded, in the float order DESIGN.md section 7e writes down.
// Build: g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -fno-fast-math (as oracle/Makefile).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <tuple>
#include <vector>

#include "../../oracle/cox_oracle.hpp"

using namespace coxo;

namespace {

enum { kNearest = 0, kInterpolate = 1, kAdaptive = 2 };
enum : uint8_t { kValue = 1, kTrilinear = 2, kGradient = 4 };

// Interpolator::getInterpDistance / getInterpWeight
bool triSample(const Layer& L, V3 pos, float* d, float* w) {
  const Interp it = getVoxelsAndQVector(L, pos);
  if (!it.ok) return false;
  const float dx = it.off[0], dy = it.off[1], dz = it.off[2];
  const float q[8] = {1.0f, dx, dy, dz, dx * dy, dy * dz, dz * dx, dx * dy * dz};
  *d = interpMember(q, it.d);
  *w = interpMember(q, it.w);
  return true;
}

// Interpolator::getNearestDistance: Block::getVoxelByCoordinates, valid when weight > 0
bool nearestSample(const Layer& L, V3 pos, float* d, float* w) {
  const Block* blk = L.getBlockPtr(blockIndexFromPoint(pos, L.block_size_inv));
  if (!blk) return false;
  const GIdx gi = gridIndexFromPoint(pos - blk->origin, L.voxel_size_inv);
  int vi[3] = {static_cast<int>(gi.x), static_cast<int>(gi.y), static_cast<int>(gi.z)};
  for (int k = 0; k < 3; ++k) vi[k] = std::max(std::min(vi[k], L.vps - 1), 0);
  const TsdfVoxel& v = blk->voxels[linearIndex(vi[0], vi[1], vi[2], L.vps)];
  *d = v.distance;
  *w = v.weight;
  return v.weight > 0.0f;
}

bool sample(const Layer& L, V3 pos, bool tri, float* d, float* w) { return tri ? triSample(L, pos, d, w) : nearestSample(L, pos, d, w); }

// Interpolator::getGradient(pos, &grad, interpolate)
bool getGradient(const Layer& L, V3 pos, bool tri, float g[3]) {
  if (!L.getBlockPtr(blockIndexFromPoint(pos, L.block_size_inv))) return false;
  float grad[3] = {0.0f, 0.0f, 0.0f};
  for (int i = 0; i < 3; ++i) {
    for (int sign = -1; sign <= 1; sign += 2) {
      float o[3] = {0.0f, 0.0f, 0.0f};
      o[i] = static_cast<float>(sign) * L.voxel_size;
      float od, ow;
      if (!sample(L, pos + V3{o[0], o[1], o[2]}, tri, &od, &ow)) return false;
      grad[i] += od * static_cast<float>(sign);
    }
  }
  const float two_h = 2.0f * L.voxel_size;
  for (int i = 0; i < 3; ++i) g[i] = grad[i] / two_h;
  return true;
}

bool inRange(float s) { return s > -1048575.0f && s < 1048575.0f; }

}  // namespace

extern "C" {

// the layer given as wire arrays (block_idx 3 int32 per block, words 4096 * 3 uint32 per block)
void* map_ref_build(float voxel_size, uint64_t n_blocks, const int32_t* block_idx, const uint32_t* words) {
  Layer* L = new Layer(voxel_size, 16);
  for (uint64_t i = 0; i < n_blocks; ++i) {
    Block* b = L->allocateBlock(BIdx{block_idx[3 * i], block_idx[3 * i + 1], block_idx[3 * i + 2]});
    for (int v = 0; v < 4096; ++v) wordsToVoxel(words + (i * 4096 + v) * 3, &b->voxels[v]);
  }
  return L;
}

void map_ref_free(void* h) { delete static_cast<Layer*>(h); }

// cox_layer_query's semantics; outputs are left untouched where a status bit is clear.  Returns the seconds spent.
double map_ref_query(const void* h, const float* xyz, uint64_t n, int mode, int want_gradient, float* distance, float* weight, float* gradient,
                     uint8_t* status) {
  const Layer& L = *static_cast<const Layer*>(h);
  const auto t0 = std::chrono::steady_clock::now();
  for (uint64_t i = 0; i < n; ++i) {
    const V3 p{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    uint8_t st = 0;
    float d = 0.0f, w = 0.0f, g[3] = {0.0f, 0.0f, 0.0f};
    if (inRange(p.x * L.block_size_inv) && inRange(p.y * L.block_size_inv) && inRange(p.z * L.block_size_inv)) {
      if (mode != kNearest) {
        const bool vd = triSample(L, p, &d, &w);
        const bool vg = want_gradient && getGradient(L, p, true, g);
        if (mode == kInterpolate)
          st = (vd ? kValue | kTrilinear : 0) | (vg ? kGradient : 0);
        else if (vd && (vg || !want_gradient))
          st = kValue | kTrilinear | (want_gradient ? kGradient : 0);
      }
      if (mode == kNearest || (mode == kAdaptive && st == 0)) {
        const bool vd = nearestSample(L, p, &d, &w);
        const bool vg = want_gradient && getGradient(L, p, false, g);
        st = (vd ? kValue : 0) | (vg ? kGradient : 0);
      }
    }
    if (status) status[i] = st;
    if (st & kValue) {
      if (distance) distance[i] = d;
      if (weight) weight[i] = w;
    }
    if ((st & kGradient) && gradient)
      for (int k = 0; k < 3; ++k) gradient[3 * i + k] = g[k];
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// createFreePointcloudFromEsdfLayer(esdf, min_distance): observed voxels (weight > 0) with distance >= min_distance, blocks in
// (z, y, x) order, voxels in linear index order; centre = origin + centerCoord.  NULL outputs: the count only.
uint64_t map_ref_free_points(const void* h, float min_distance, float* xyz, float* intensity) {
  const Layer& L = *static_cast<const Layer*>(h);
  std::vector<BIdx> order;
  for (const auto& kv : L.blocks) order.push_back(kv.first);
  std::sort(order.begin(), order.end(), [](const BIdx& a, const BIdx& b) { return std::tie(a.z, a.y, a.x) < std::tie(b.z, b.y, b.x); });
  uint64_t n = 0;
  for (const BIdx& bi : order) {
    const Block* b = L.getBlockPtr(bi);
    for (int v = 0; v < L.vps * L.vps * L.vps; ++v) {
      const TsdfVoxel& vox = b->voxels[v];
      if (!(vox.weight > 0.0f) || !(vox.distance >= min_distance)) continue;
      if (xyz) {
        const int x = v % L.vps, y = (v / L.vps) % L.vps, z = v / (L.vps * L.vps);
        xyz[3 * n] = b->origin.x + centerCoord(x, L.voxel_size);
        xyz[3 * n + 1] = b->origin.y + centerCoord(y, L.voxel_size);
        xyz[3 * n + 2] = b->origin.z + centerCoord(z, L.voxel_size);
      }
      if (intensity) intensity[n] = vox.distance;
      ++n;
    }
  }
  return n;
}

}  // extern "C"
