// DepthImageIntegrator of coxgraph_amd/host/coxgraph_hip_map.hpp: one frame of a fronto-parallel wall
//   -> the voxels on the optical axis hold the distance to the wall, nothing behind the truncation band is observed
//   -> renderView of the fused layer sees the wall again, and integrateView takes that image into a second layer
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_map.hpp"

using namespace coxgraph_hip;

int main() {
  if (cox_device_count() == 0) {
    try {
      TsdfLayer layer(0.10f);
    } catch (const std::runtime_error& e) {
      std::printf("no GPU: %s\n", e.what());
      return 77;
    }
    return 1;
  }
  const float voxel = 0.10f, z0 = 2.0f, trunc = 0.3f;
  const int w = 48, h = 36;
  const float K[4] = {39.0f, 39.0f, 23.5f, 17.5f};
  TsdfLayer layer(voxel);
  DepthImageIntegrator::Config cfg = DepthImageIntegrator::defaultConfig();
  cfg.truncation_distance = trunc, cfg.min_depth_m = 0.3f, cfg.max_depth_m = 3.0f, cfg.use_const_weight = 1, cfg.use_weight_dropoff = 0;
  DepthImageIntegrator integ(cfg, &layer);
  Transformation T;  // camera axes = world axes, on a line of voxel centres
  T.t[0] = 0.05f, T.t[1] = 0.05f, T.t[2] = 0.0f;
  std::vector<float> depth(static_cast<size_t>(w) * h, z0);
  std::vector<Color> colors(depth.size(), Color{200, 100, 50, 255});
  integ.integrateDepthImage(T, depth, colors, w, h, K);
  integ.sync();
  const cox_depthfuse_stats st = integ.lastStats();
  if (st.n_valid_pixels != depth.size() || st.n_touched_blocks == 0 || st.n_new_blocks != st.n_touched_blocks || st.n_updated_voxels < 1000) return 10;
  if (layer.getNumberOfAllocatedBlocks() != st.n_new_blocks) return 11;
  // the axis voxels: centre (0.05, 0.05, z) holds clamp(z0 - z)
  LayerQuery q(layer.handle());
  int n_axis = 0;
  for (int k = 3; k < 23; ++k) {
    const float z = (static_cast<float>(k) + 0.5f) * voxel;
    float d = 0.0f, wgt = 0.0f;
    const Point p{{0.05f, 0.05f, z}};
    if (!q.getDistanceAtPosition(p, false, &d) || !q.getWeightAtPosition(p, false, &wgt)) return 20;
    const float want = std::fmax(-trunc, std::fmin(trunc, z0 - z));
    if (std::fabs(d - want) > 1e-4f || std::fabs(wgt - 1.0f) > 1e-4f) {
      std::printf("axis voxel z=%g: d=%g (want %g) w=%g\n", z, d, want, wgt);
      return 21;
    }
    ++n_axis;
  }
  if (q.isObserved(Point{{0.05f, 0.05f, 2.55f}})) return 22;  // behind the truncation band
  // a second frame: weights count the frames
  integ.integrateDepthImage(T, depth, std::vector<Color>(), w, h, K);
  float w2 = 0.0f;
  if (!q.getWeightAtPosition(Point{{0.05f, 0.05f, 1.05f}}, false, &w2) || std::fabs(w2 - 2.0f) > 1e-4f) return 23;
  if (integ.lastStats().n_new_blocks != 0 || integ.lastStats().n_coloured_voxels != 0) return 24;
  // render -> fuse
  RenderedView view;
  renderView(layer.handle(), T, w, h, K, &view);
  size_t n_hit = 0;
  for (size_t i = 0; i < view.depth.size(); ++i)
    if (view.status[i] & COX_R_HIT) {
      if (std::fabs(view.depth[i] - z0) > 0.05f) return 30;
      ++n_hit;
    }
  if (n_hit < view.depth.size() / 2) return 31;
  TsdfLayer second(voxel);
  DepthImageIntegrator integ2(cfg, &second);
  integ2.integrateView(T, view, K);
  integ2.sync();
  if (integ2.lastStats().n_valid_pixels != n_hit || second.getNumberOfAllocatedBlocks() == 0) return 32;
  std::printf("depthfuse smoke ok: %zu blocks, %llu voxels, %d axis voxels, %zu rendered hits, %zu blocks in the second layer\n",
              layer.getNumberOfAllocatedBlocks(), static_cast<unsigned long long>(st.n_updated_voxels), n_axis, n_hit, second.getNumberOfAllocatedBlocks());
  return 0;
}
