// Test-side reference of the GPU renderer (coxgraph_amd/csrc/cox_render.hip), loaded by tests/render_ref.py through ctypes.
//
// The trilinear sample is the CPU checker's own getVoxelsAndQVector + interpMember (oracle/cox_oracle.hpp), run on an oracle
// Layer rebuilt from the engine's downloaded wire arrays.  The march itself -- pixel to ray, the empty-block skip, the adaptive
// sample, the step rule, the hit interpolation, the normal and the colour -- is restated here, single-threaded, in the float
// order DESIGN.md section 7g writes down.  No block cache: every lookup goes to the layer's map.
// Build: g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -fno-fast-math (as oracle/Makefile).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include "../../oracle/cox_oracle.hpp"

using namespace coxo;

namespace {

enum : uint8_t { kHit = 1, kNormal = 2, kColor = 4, kBudget = 8 };

struct Config {
  float min_depth, max_depth, step_scale, min_step_voxels;
  uint32_t max_samples;
};
struct Stats {
  uint64_t n_hits, n_samples, n_block_skips, n_budget;
  double seconds;
};

// Interpolator::getInterpDistance
bool triSample(const Layer& L, V3 pos, float* d) {
  const Interp it = getVoxelsAndQVector(L, pos);
  if (!it.ok) return false;
  const float dx = it.off[0], dy = it.off[1], dz = it.off[2];
  const float q[8] = {1.0f, dx, dy, dz, dx * dy, dy * dz, dz * dx, dx * dy * dz};
  *d = interpMember(q, it.d);
  return true;
}

// Block::getVoxelByCoordinates
const TsdfVoxel* containingVoxel(const Layer& L, V3 pos) {
  const Block* blk = L.getBlockPtr(blockIndexFromPoint(pos, L.block_size_inv));
  if (!blk) return nullptr;
  const GIdx gi = gridIndexFromPoint(pos - blk->origin, L.voxel_size_inv);
  int vi[3] = {static_cast<int>(gi.x), static_cast<int>(gi.y), static_cast<int>(gi.z)};
  for (int k = 0; k < 3; ++k) vi[k] = std::max(std::min(vi[k], L.vps - 1), 0);
  return &blk->voxels[linearIndex(vi[0], vi[1], vi[2], L.vps)];
}

// Interpolator::getGradient(pos, &grad, interpolate = true); the caller has checked the block of pos
bool triGradient(const Layer& L, V3 pos, float g[3]) {
  float grad[3] = {0.0f, 0.0f, 0.0f};
  for (int i = 0; i < 3; ++i) {
    for (int sign = -1; sign <= 1; sign += 2) {
      float o[3] = {0.0f, 0.0f, 0.0f};
      o[i] = static_cast<float>(sign) * L.voxel_size;
      float od;
      if (!triSample(L, pos + V3{o[0], o[1], o[2]}, &od)) return false;
      grad[i] += od * static_cast<float>(sign);
    }
  }
  const float two_h = 2.0f * L.voxel_size;
  for (int i = 0; i < 3; ++i) g[i] = grad[i] / two_h;
  return true;
}

bool inRange(float s) { return s > -1048575.0f && s < 1048575.0f; }
bool pointInRange(const Layer& L, V3 p) { return inRange(p.x * L.block_size_inv) && inRange(p.y * L.block_size_inv) && inRange(p.z * L.block_size_inv); }

}  // namespace

extern "C" {

// the layer given as wire arrays (block_idx 3 int32 per block, words 4096 * 3 uint32 per block)
void* render_ref_build(float voxel_size, uint64_t n_blocks, const int32_t* block_idx, const uint32_t* words) {
  Layer* L = new Layer(voxel_size, 16);
  for (uint64_t i = 0; i < n_blocks; ++i) {
    Block* b = L->allocateBlock(BIdx{block_idx[3 * i], block_idx[3 * i + 1], block_idx[3 * i + 2]});
    for (int v = 0; v < 4096; ++v) wordsToVoxel(words + (i * 4096 + v) * 3, &b->voxels[v]);
  }
  return L;
}

void render_ref_free(void* h) { delete static_cast<Layer*>(h); }

// cox_layer_render's semantics: every pixel of every output given is written.  samples (may be NULL) gets the sample count of
// every ray.
void render_ref_render(const void* h, const float T[7], int w, int hgt, const float K[4], const Config* cfg, float* depth, float* normal, uint8_t* rgba,
                       uint8_t* status, uint32_t* samples, Stats* stats) {
  const Layer& L = *static_cast<const Layer*>(h);
  const auto t0 = std::chrono::steady_clock::now();
  const Transform Tf{T[0], T[1], T[2], T[3], V3{T[4], T[5], T[6]}};
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float min_step = cfg->min_step_voxels * L.voxel_size, half_voxel = 0.5f * L.voxel_size;
  Stats S{0, 0, 0, 0, 0.0};
  for (int v = 0; v < hgt; ++v) {
    for (int u = 0; u < w; ++u) {
      const float xn = (static_cast<float>(u) - cx) / fx;
      const float yn = (static_cast<float>(v) - cy) / fy;
      const V3 dc{xn, yn, 1.0f};
      const V3 dg = rotate(Tf, dc);
      const float len = std::sqrt(dot(dc, dc));
      const float o[3] = {Tf.t.x, Tf.t.y, Tf.t.z}, dir[3] = {dg.x, dg.y, dg.z};
      uint8_t st = 0;
      uint32_t n_samples = 0;
      float t_hit = nan, nrm[3] = {nan, nan, nan};
      uint8_t col[4] = {0, 0, 0, 0};
      float t = cfg->min_depth, t_prev = 0.0f, d_prev = 0.0f;
      bool have_prev = false;
      while (t <= cfg->max_depth) {
        if (n_samples >= cfg->max_samples) {
          st = kBudget;
          break;
        }
        ++n_samples;
        const V3 p{o[0] + t * dir[0], o[1] + t * dir[1], o[2] + t * dir[2]};
        if (!pointInRange(L, p)) break;
        const BIdx bi = blockIndexFromPoint(p, L.block_size_inv);
        if (!L.getBlockPtr(bi)) {
          have_prev = false;
          ++S.n_block_skips;
          const int b[3] = {bi.x, bi.y, bi.z};
          float t_exit = std::numeric_limits<float>::infinity();
          for (int k = 0; k < 3; ++k) {
            if (dir[k] != 0.0f) {
              const float face = static_cast<float>(dir[k] > 0.0f ? b[k] + 1 : b[k]) * L.block_size;
              t_exit = std::min(t_exit, (face - o[k]) / dir[k]);
            }
          }
          const float t_new = t_exit + half_voxel / len;
          t = t_new > t ? t_new : t + L.voxel_size / len;
          continue;
        }
        float d = 0.0f;
        bool ok = triSample(L, p, &d);
        if (!ok) {
          const TsdfVoxel* vox = containingVoxel(L, p);
          if (vox) {
            d = vox->distance;
            ok = vox->weight > 0.0f;
          }
        }
        if (!ok) {
          have_prev = false;
          t = t + L.voxel_size / len;
          continue;
        }
        if (have_prev && d_prev > 0.0f && d <= 0.0f) {
          t_hit = t_prev + ((t - t_prev) * d_prev) / (d_prev - d);
          st = kHit;
          break;
        }
        t_prev = t;
        d_prev = d;
        have_prev = true;
        t = t + std::max(std::fabs(d) * cfg->step_scale, min_step) / len;
      }
      if (st & kHit) {
        const V3 p{o[0] + t_hit * dir[0], o[1] + t_hit * dir[1], o[2] + t_hit * dir[2]};
        if (pointInRange(L, p)) {
          const TsdfVoxel* vox = containingVoxel(L, p);
          if (vox) {
            if (vox->weight > 0.0f) {
              col[0] = vox->color.r, col[1] = vox->color.g, col[2] = vox->color.b, col[3] = vox->color.a;
              st |= kColor;
            }
            float g[3];
            if (triGradient(L, p, g)) {
              const V3 n = normalized(V3{g[0], g[1], g[2]});
              nrm[0] = n.x, nrm[1] = n.y, nrm[2] = n.z;
              st |= kNormal;
            }
          }
        }
      }
      const size_t i = static_cast<size_t>(v) * static_cast<size_t>(w) + static_cast<size_t>(u);
      if (depth) depth[i] = t_hit;
      if (normal)
        for (int k = 0; k < 3; ++k) normal[3 * i + k] = nrm[k];
      if (rgba) std::memcpy(rgba + 4 * i, col, 4);
      if (status) status[i] = st;
      if (samples) samples[i] = n_samples;
      S.n_samples += n_samples;
      S.n_hits += (st & kHit) ? 1 : 0;
      S.n_budget += (st & kBudget) ? 1 : 0;
    }
  }
  S.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (stats) *stats = S;
}

}  // extern "C"
