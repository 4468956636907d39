// The incremental ESDF through coxgraph_amd/host/coxgraph_hip_map.hpp: frames are fused into a TSDF layer, EsdfIntegrator::
// updateFromTsdfLayer() runs between them (frames still in flight), and after every update the ESDF layer is compared word for
// word with cox_esdf_from_tsdf on the same TSDF.  Exit code 0 = all good; 77 = no GPU.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_map.hpp"

using namespace coxgraph_hip;

// a room corner (walls x = 3, y = 2.5, floor z = -1.2) seen by a camera at the origin turned by yaw about z
static void renderFrame(double yaw, Pointcloud* pts, Colors* cols, Transformation* T_G_C) {
  pts->clear();
  cols->clear();
  const double c = std::cos(yaw), s = std::sin(yaw);
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
  const double hw = std::cos(0.5 * yaw), hz = std::sin(0.5 * yaw);
  const double o[4] = {0.5, -0.5, 0.5, -0.5};
  T_G_C->q[0] = static_cast<float>(hw * o[0] - hz * o[3]);
  T_G_C->q[1] = static_cast<float>(hw * o[1] - hz * o[2]);
  T_G_C->q[2] = static_cast<float>(hw * o[2] + hz * o[1]);
  T_G_C->q[3] = static_cast<float>(hw * o[3] + hz * o[0]);
  T_G_C->t[0] = T_G_C->t[1] = T_G_C->t[2] = 0.0f;
}

// 0: the same words; otherwise a code
static int compareWithBatch(cox_layer_t* tsdf, const cox_esdf_config& cfg, cox_layer_t* inc, uint64_t* n_blocks) {
  cox_layer_t* batch = nullptr;
  if (cox_esdf_from_tsdf(tsdf, &cfg, &batch) != COX_OK) return 1;
  LayerHandle keep(batch);
  uint64_t na = 0, nb = 0;
  if (cox_layer_download(inc, nullptr, nullptr, 0, &na) != COX_OK || cox_layer_download(batch, nullptr, nullptr, 0, &nb) != COX_OK) return 2;
  if (na != nb) return 3;
  std::vector<int32_t> ia(3 * na), ib(3 * nb);
  std::vector<uint32_t> wa(na * 12288), wb(nb * 12288);
  if (na && (cox_layer_download(inc, ia.data(), wa.data(), na, &na) != COX_OK || cox_layer_download(batch, ib.data(), wb.data(), nb, &nb) != COX_OK)) return 4;
  if (ia != ib) return 5;
  if (wa != wb) return 6;
  *n_blocks = na;
  return 0;
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
  TsdfLayer layer(voxel, 16, 0, 64);  // a small pool: it grows while the ESDF follows
  TsdfIntegratorConfig cfg;
  cfg.default_truncation_distance = 0.3f, cfg.use_const_weight = 1, cfg.max_ray_length_m = 10.0f, cfg.min_ray_length_m = 0.2f;
  auto integ = TsdfIntegrator::create("merged", cfg, &layer);
  EsdfIntegrator::Config ecfg;
  cox_esdf_config_default(&ecfg);
  ecfg.max_distance_m = 2.0f, ecfg.default_distance_m = 2.0f, ecfg.min_distance_m = 1.5f * voxel;
  EsdfIntegrator esdf(ecfg, &layer);
  uint64_t nb = 0, swept_max = 0;
  cox_esdf_update_stats st = esdf.updateFromTsdfLayer();  // an empty layer
  if (st.n_blocks != 0 || compareWithBatch(layer.handle(), ecfg, esdf.getEsdfLayer(), &nb) != 0) return 10;
  for (int f = 0; f < 9; ++f) {
    Pointcloud pts;
    Colors cols;
    Transformation T;
    renderFrame(-0.5 + 0.12 * f, &pts, &cols, &T);
    integ->integratePointCloud(T, pts, cols, false);
    if (f % 2) continue;  // an update after every second frame, the frame still in flight
    st = esdf.updateFromTsdfLayer();
    const int rc = compareWithBatch(layer.handle(), ecfg, esdf.getEsdfLayer(), &nb);
    std::printf("frame %d: %llu blocks (%llu new, %llu dirty, %llu swept), raise %llu lower %llu sweeps, rebuilt %u, compare %d\n", f,
                static_cast<unsigned long long>(st.n_blocks), static_cast<unsigned long long>(st.n_new_blocks),
                static_cast<unsigned long long>(st.n_dirty_blocks), static_cast<unsigned long long>(st.n_swept_blocks),
                static_cast<unsigned long long>(st.n_raise_sweeps), static_cast<unsigned long long>(st.n_lower_sweeps), st.rebuilt, rc);
    if (rc != 0) return 20 + rc;
    if (st.n_blocks != nb || (f > 0 && st.rebuilt)) return 30;
    swept_max = std::max<uint64_t>(swept_max, st.n_swept_blocks);
  }
  if (nb < 8 || swept_max == 0) return 31;
  st = esdf.updateFromTsdfLayer();  // nothing changed
  if (st.n_dirty_blocks != 0 || st.n_raise_sweeps != 0 || st.n_lower_sweeps != 0 || st.n_swept_blocks != 0) return 40;
  st = esdf.updateFromTsdfLayerBatch();
  if (!st.rebuilt || compareWithBatch(layer.handle(), ecfg, esdf.getEsdfLayer(), &nb) != 0) return 41;
  // the borrowed layer answers EsdfMap queries
  float d = 0.0f;
  if (!esdf.getEsdfMap().getDistanceAtPosition(Point{{1.0f, 0.5f, 0.0f}}, false, &d) || !(d > 0.0f)) return 50;
  std::printf("esdf smoke ok: %llu blocks, distance at (1, 0.5, 0) = %.3f\n", static_cast<unsigned long long>(nb), d);
  return 0;
}
