// VoxelWeightEvaluator of coxgraph_amd/host/coxgraph_hip_planning.hpp on a map server's combined map:
//   two GPU-fused submaps -> MapServer::updatePastTsdf -> a yaw sweep of 12 candidate views at one position, scored in one call;
//   every record must equal the same view scored alone, the views towards the fused corner must see its surface, the views away
//   from it nothing but unknown space, and the visible set of a view must have the size its record reports.
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_map.hpp"
#include "../../coxgraph_amd/host/coxgraph_hip_planning.hpp"

using namespace coxgraph_hip;

// a room corner (walls x = 3, y = 2.5, floor z = -1.2) seen by a camera at the origin turned by yaw about z
static void renderFrame(double yaw, Pointcloud* pts, Colors* cols, Transformation* T_G_C) {
  pts->clear();
  cols->clear();
  const double c = std::cos(yaw), s = std::sin(yaw);
  // optical frame: z forward, x right, y down; R_G_C = Rz(yaw) * [[0,0,1],[-1,0,0],[0,-1,0]]
  const double R[9] = {s, 0.0, c, -c, 0.0, s, 0.0, -1.0, 0.0};
  for (int v = 0; v < 96; ++v)
    for (int u = 0; u < 128; ++u) {
      const double dc[3] = {(u - 63.5) / 100.0, (v - 47.5) / 100.0, 1.0};
      const double d[3] = {R[0] * dc[0] + R[1] * dc[1] + R[2] * dc[2], R[3] * dc[0] + R[4] * dc[1] + R[5] * dc[2], R[6] * dc[0] + R[7] * dc[1] + R[8] * dc[2]};
      double t = 1e30;
      if (d[0] > 1e-9) t = std::min(t, 3.0 / d[0]);
      if (d[1] > 1e-9) t = std::min(t, 2.5 / d[1]);
      if (d[2] < -1e-9) t = std::min(t, -1.2 / d[2]);
      if (t > 20.0) continue;
      pts->push_back({{static_cast<float>(t * dc[0]), static_cast<float>(t * dc[1]), static_cast<float>(t * dc[2])}});
      cols->push_back(Color{static_cast<uint8_t>(u), static_cast<uint8_t>(v), 128, 255});
    }
  *T_G_C = VoxelWeightEvaluator::yawSweep(Point{{0.0f, 0.0f, 0.0f}}, 1, yaw)[0];
}

static bool same(const cox_view_gain& a, const cox_view_gain& b) {
  return a.gain == b.gain && a.surface_gain == b.surface_gain && a.surface_gain_q32 == b.surface_gain_q32 && a.n_visible == b.n_visible &&
         a.n_free == b.n_free && a.n_occupied == b.n_occupied && a.n_surface_counted == b.n_surface_counted && a.n_unknown == b.n_unknown &&
         a.n_frontier == b.n_frontier;
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
  VoxgraphSubmap::Config sm_cfg;
  sm_cfg.tsdf_voxel_size = voxel;
  sm_cfg.capacity_blocks = 2048;
  TsdfIntegratorConfig cfg;
  cfg.default_truncation_distance = 0.3f, cfg.use_const_weight = 1, cfg.max_ray_length_m = 10.0f, cfg.min_ray_length_m = 0.2f;
  SubmapCollection collection(sm_cfg, 1);
  const double ranges[2][2] = {{-0.3, 0.2}, {0.3, 0.8}};
  for (int k = 0; k < 2; ++k) {
    Transformation T_M_S;
    T_M_S.t[0] = 0.03f * static_cast<float>(k);
    VoxgraphSubmap::Ptr sm(new VoxgraphSubmap(T_M_S, static_cast<SubmapID>(k), sm_cfg));
    auto integ = TsdfIntegrator::create("merged", cfg, sm->getTsdfMapPtr()->getTsdfLayerPtr());
    for (int f = 0; f < 5; ++f) {
      Pointcloud pts;
      Colors cols;
      Transformation T;
      renderFrame(ranges[k][0] + (ranges[k][1] - ranges[k][0]) * f / 4.0, &pts, &cols, &T);
      integ->integratePointCloud(T, pts, cols, false);
    }
    collection.addSubmap(sm, 0, static_cast<SubmapID>(k));
  }
  MapServer server(sm_cfg);
  server.updatePastTsdf(collection);
  if (server.getTsdfLayer().getNumberOfAllocatedBlocks() < 8) return 10;

  const RayCasterSensor sensor;
  if (sensor.rays_x != 35 || sensor.rays_y != 96 || sensor.K[0] != 64.0f || sensor.K[2] != 17.0f || sensor.K[3] != 48.0f || sensor.ray_length != 5.0f) return 11;
  VoxelWeightEvaluator evaluator(server.getTsdfLayerPtr()->handle(), sensor);
  if (evaluator.config().frontier_voxel_weight != 1.0f || evaluator.config().min_impact_factor != 0.01f) return 12;
  const std::vector<Transformation> sweep = VoxelWeightEvaluator::yawSweep(Point{{0.0f, 0.0f, 0.0f}}, 12);
  if (sweep.size() != 12) return 13;
  cox_viewgain_stats stats;
  const std::vector<cox_view_gain> gains = evaluator.computeGains(sweep, &stats);
  if (gains.size() != 12 || stats.n_chunks != 1 || stats.n_samples == 0) return 14;
  for (int k = 0; k < 12; ++k) {
    const cox_view_gain alone = evaluator.computeGains(std::vector<Transformation>(1, sweep[k]))[0];
    std::printf("yaw %3d deg: gain %9.3f  visible %6u  free %6u  occupied %5u (%5u counted)  unknown %6u  frontier %5u\n", 30 * k, gains[k].gain,
                gains[k].n_visible, gains[k].n_free, gains[k].n_occupied, gains[k].n_surface_counted, gains[k].n_unknown, gains[k].n_frontier);
    if (!same(alone, gains[k])) return 20 + k;
    if (gains[k].n_visible != gains[k].n_free + gains[k].n_occupied + gains[k].n_unknown) return 40;
    if (gains[k].gain != gains[k].surface_gain + static_cast<double>(gains[k].n_frontier)) return 41;
  }
  // yaw 0 and 30 deg look into the fused corner, yaw 180 deg at nothing that was ever observed beyond the camera's own surroundings
  if (gains[0].n_occupied == 0 || gains[1].n_occupied == 0 || gains[0].n_free == 0) return 50;
  if (gains[6].n_occupied != 0 || gains[6].n_unknown == 0) return 51;
  int best = 0;
  for (int k = 1; k < 12; ++k)
    if (gains[k].gain > gains[best].gain) best = k;
  if (gains[best].n_occupied == 0) return 52;  // the best view looks at the corner
  // the visible set of a view has the size its record reports
  float T0[7];
  sweep[0].pack(T0);
  uint64_t n_set = 0;
  if (cox_viewgain_visible(evaluator.handle(), T0, 0, nullptr, nullptr, nullptr, &n_set) != COX_OK || n_set != gains[0].n_visible) return 60;
  std::vector<uint8_t> classes(n_set);
  if (cox_viewgain_visible(evaluator.handle(), T0, n_set, nullptr, classes.data(), nullptr, &n_set) != COX_OK) return 61;
  uint32_t n_occ = 0;
  for (uint8_t c : classes) n_occ += c == COX_VG_OCCUPIED;
  if (n_occ != gains[0].n_occupied) return 62;
  // no views: nothing to do; a configuration the engine refuses
  if (!evaluator.computeGains(std::vector<Transformation>()).empty()) return 70;
  VoxelWeightEvaluator::Config bad;
  bad.ray_angle_x = -1.0f;
  try {
    VoxelWeightEvaluator nope(server.getTsdfLayerPtr()->handle(), sensor, bad);
    return 71;
  } catch (const std::runtime_error&) {
  }
  std::printf("viewgain smoke ok: best yaw %d deg, %llu samples in %.3f ms\n", 30 * best, static_cast<unsigned long long>(stats.n_samples), stats.kernel_ms);
  return 0;
}
