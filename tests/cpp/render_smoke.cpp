// renderView of coxgraph_amd/host/coxgraph_hip_map.hpp on a GPU-fused layer: a room corner (walls x = 3, y = 2.5, floor z = -1.2)
// fused from five frames and rendered back from the middle one must give that frame's own depths.
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_map.hpp"

using namespace coxgraph_hip;

static const int kW = 128, kH = 96;
static const float kK[4] = {100.0f, 100.0f, 63.5f, 47.5f};

// analytic z-depth image of the corner from a camera at the origin turned by yaw about z, and the pose
static void renderFrame(double yaw, std::vector<float>* depth, Transformation* T_G_C) {
  depth->assign(static_cast<size_t>(kW) * kH, std::nanf(""));
  const double c = std::cos(yaw), s = std::sin(yaw);
  // optical frame: z forward, x right, y down; R_G_C = Rz(yaw) * [[0,0,1],[-1,0,0],[0,-1,0]]
  const double R[9] = {s, 0.0, c, -c, 0.0, s, 0.0, -1.0, 0.0};
  for (int v = 0; v < kH; ++v)
    for (int u = 0; u < kW; ++u) {
      const double dc[3] = {(u - 63.5) / 100.0, (v - 47.5) / 100.0, 1.0};
      const double d[3] = {R[0] * dc[0] + R[1] * dc[1] + R[2] * dc[2], R[3] * dc[0] + R[4] * dc[1] + R[5] * dc[2], R[6] * dc[0] + R[7] * dc[1] + R[8] * dc[2]};
      double t = 1e30;
      if (d[0] > 1e-9) t = std::min(t, 3.0 / d[0]);
      if (d[1] > 1e-9) t = std::min(t, 2.5 / d[1]);
      if (d[2] < -1e-9) t = std::min(t, -1.2 / d[2]);
      if (t < 20.0) (*depth)[static_cast<size_t>(v) * kW + u] = static_cast<float>(t);
    }
  const double hw = std::cos(0.5 * yaw), hz = std::sin(0.5 * yaw);
  const double o[4] = {0.5, -0.5, 0.5, -0.5};
  T_G_C->q[0] = static_cast<float>(hw * o[0] - hz * o[3]);
  T_G_C->q[1] = static_cast<float>(hw * o[1] - hz * o[2]);
  T_G_C->q[2] = static_cast<float>(hw * o[2] + hz * o[1]);
  T_G_C->q[3] = static_cast<float>(hw * o[3] + hz * o[0]);
  T_G_C->t[0] = T_G_C->t[1] = T_G_C->t[2] = 0.0f;
}

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
  const float voxel = 0.10f;
  TsdfLayer layer(voxel);
  TsdfIntegratorConfig cfg;
  cfg.default_truncation_distance = 0.3f, cfg.use_const_weight = 1, cfg.max_ray_length_m = 10.0f, cfg.min_ray_length_m = 0.2f;
  auto integ = TsdfIntegrator::create("merged", cfg, &layer);
  std::vector<float> depth, mid_depth;
  Transformation T, mid_T;
  for (int f = 0; f < 5; ++f) {
    renderFrame(0.1 * f, &depth, &T);
    if (f == 2) mid_depth = depth, mid_T = T;
    Pointcloud pts;
    Colors cols;
    for (int v = 0; v < kH; ++v)
      for (int u = 0; u < kW; ++u) {
        const float d = depth[static_cast<size_t>(v) * kW + u];
        if (!std::isfinite(d)) continue;
        pts.push_back({{d * ((static_cast<float>(u) - kK[2]) / kK[0]), d * ((static_cast<float>(v) - kK[3]) / kK[1]), d}});
        cols.push_back(Color{static_cast<uint8_t>(u), static_cast<uint8_t>(v), 128, 255});
      }
    integ->integratePointCloud(T, pts, cols, false);
  }
  RenderedView view;
  renderView(layer.handle(), mid_T, kW, kH, kK, &view);
  if (view.width != kW || view.depth.size() != static_cast<size_t>(kW) * kH) return 10;
  size_t want = 0, hit = 0, close = 0, with_normal = 0, with_color = 0;
  for (size_t i = 0; i < view.depth.size(); ++i) {
    const bool h = (view.status[i] & COX_R_HIT) != 0;
    if (h != std::isfinite(view.depth[i])) return 11;  // NaN exactly where nothing was hit
    if (!std::isfinite(mid_depth[i])) continue;
    ++want;
    if (!h) continue;
    ++hit;
    if (std::fabs(view.depth[i] - mid_depth[i]) < voxel) ++close;
    if (view.status[i] & COX_R_NORMAL) {
      ++with_normal;
      const Point& n = view.normal[i];
      if (std::fabs(std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) - 1.0f) > 1e-4f) return 12;
    }
    if (view.status[i] & COX_R_COLOR) {
      ++with_color;
      if (view.color[i].a != 255 || view.color[i].b != 128) return 13;  // every fused point had b = 128, a = 255
    }
  }
  std::printf("render smoke: %zu pixels wanted, %zu hit, %zu within a voxel, %zu normals, %zu colours; %llu samples, %.3f ms\n", want, hit, close, with_normal,
              with_color, static_cast<unsigned long long>(view.stats.n_samples), view.stats.kernel_ms);
  if (view.stats.n_hits < hit || view.stats.n_budget != 0) return 14;
  if (hit < want * 9 / 10 || close < hit * 9 / 10 || with_normal < hit / 2 || with_color < hit * 9 / 10) return 15;
  // a custom configuration goes through: one sample per ray can only run out of budget
  cox_render_config rc;
  cox_render_config_default(&rc);
  rc.max_samples = 1;
  renderView(layer.handle(), mid_T, kW, kH, kK, &view, &rc);
  if (view.stats.n_hits != 0 || view.stats.n_budget == 0) return 16;
  std::printf("render smoke ok\n");
  return 0;
}
