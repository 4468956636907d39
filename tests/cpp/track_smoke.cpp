// ScanToMapRegisterer of coxgraph_amd/host/coxgraph_hip_track.hpp on a GPU-fused layer: a room corner (walls x = 3, y = 2.5, floor
// z = -1.2) fused from five frames; the middle frame's scan, handed in with a pose prior that is off, must be pulled back: lower
// cost, the same end point from two priors, and a scan that misses the map must be reported lost with the prior untouched.
// (Nothing is asserted about the distance to the true pose: on a fused layer the minimiser sits a fraction of a voxel from it.)
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_track.hpp"

using namespace coxgraph_hip;

static const int kW = 128, kH = 96;
static const float kK[4] = {100.0f, 100.0f, 63.5f, 47.5f};

// the points of the corner seen from a camera at the origin turned by yaw about z, and the pose
static void makeFrame(double yaw, Pointcloud* pts, Colors* cols, Transformation* T_G_C) {
  pts->clear();
  cols->clear();
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
      if (t >= 20.0) continue;
      const float z = static_cast<float>(t);
      pts->push_back({{z * ((static_cast<float>(u) - kK[2]) / kK[0]), z * ((static_cast<float>(v) - kK[3]) / kK[1]), z}});
      cols->push_back(Color{static_cast<uint8_t>(u), static_cast<uint8_t>(v), 128, 255});
    }
  const double hw = std::cos(0.5 * yaw), hz = std::sin(0.5 * yaw);
  const double o[4] = {0.5, -0.5, 0.5, -0.5};
  T_G_C->q[0] = static_cast<float>(hw * o[0] - hz * o[3]);
  T_G_C->q[1] = static_cast<float>(hw * o[1] - hz * o[2]);
  T_G_C->q[2] = static_cast<float>(hw * o[2] + hz * o[1]);
  T_G_C->q[3] = static_cast<float>(hw * o[3] + hz * o[0]);
  T_G_C->t[0] = T_G_C->t[1] = T_G_C->t[2] = 0.0f;
}

static double dist(const Transformation& a, const Transformation& b) {
  double s = 0.0;
  for (int k = 0; k < 3; ++k) s += (a.t[k] - b.t[k]) * static_cast<double>(a.t[k] - b.t[k]);
  return std::sqrt(s);
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
  Pointcloud pts, scan;
  Colors cols;
  Transformation T, truth;
  for (int f = 0; f < 5; ++f) {
    makeFrame(0.1 * f, &pts, &cols, &T);
    if (f == 2) scan = pts, truth = T;
    integ->integratePointCloud(T, pts, cols, false);
  }
  ScanToMapRegisterer::Config tc;
  tc.dof = 6;
  tc.stride = 4;
  if (tc.max_iterations != 15 || tc.min_points != 32) return 10;  // the defaults came through
  ScanToMapRegisterer reg(layer.handle(), tc);
  Transformation ends[2];
  for (int k = 0; k < 2; ++k) {
    Transformation prior = truth, refined;
    prior.t[0] += k ? -0.06f : 0.05f;
    prior.t[1] += k ? 0.04f : -0.03f;
    prior.t[2] += 0.04f;
    cox_track_result r;
    const bool ok = reg.refineSensorPose(scan, prior, &refined, &r);
    std::printf("track smoke: prior %d -> %s after %u iterations, %llu of %llu points used, cost %.4f -> %.4f, moved %.4f m, %.4f m from the fused frame's pose, %.3f ms\n",
                k, ScanToMapRegisterer::statusString(r.status), r.iterations, static_cast<unsigned long long>(r.last_n_used),
                static_cast<unsigned long long>(r.last_n_considered), r.first_cost, r.last_cost, dist(refined, prior), dist(refined, truth), r.kernel_ms);
    if (!ok || r.status != COX_TRACK_CONVERGED) return 11;
    if (r.iterations < 2 || r.iterations > tc.max_iterations) return 12;
    if (!(r.last_cost < r.first_cost)) return 13;
    if (r.last_n_considered != (scan.size() + 3) / 4 || r.last_n_used < r.last_n_considered / 2) return 14;
    double nn = 0.0;
    for (int q = 0; q < 4; ++q) nn += r.T_G_C[q] * r.T_G_C[q];
    if (std::fabs(nn - 1.0) > 1e-12) return 15;
    for (int q = 0; q < 3; ++q)
      if (static_cast<float>(r.T_G_C[4 + q]) != refined.t[q]) return 16;
    ends[k] = refined;
  }
  if (dist(ends[0], ends[1]) > 1e-3) return 17;  // one minimiser
  // a scan that misses the map
  Transformation far = truth, out;
  far.t[0] = 60.0f;
  cox_track_result r;
  if (reg.refineSensorPose(scan, far, &out, &r)) return 18;
  if (r.status != COX_TRACK_LOST || r.iterations != 1 || r.last_n_used != 0 || out.t[0] != 60.0f || out.q[0] != far.q[0]) return 19;
  // no points at all
  if (reg.refineSensorPose(Pointcloud(), truth, &out, &r) || r.status != COX_TRACK_LOST || r.last_n_considered != 0) return 20;
  // a configuration the engine refuses
  ScanToMapRegisterer::Config bad;
  bad.dof = 5;
  try {
    ScanToMapRegisterer nope(layer.handle(), bad);
    return 21;
  } catch (const std::runtime_error&) {
  }
  std::printf("track smoke ok\n");
  return 0;
}
