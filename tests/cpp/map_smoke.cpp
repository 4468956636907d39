// The map server's flow through coxgraph_amd/host/coxgraph_hip_map.hpp (coxgraph/src/client/map_server.cpp:61-147):
//   three GPU-fused submaps -> MapServer::updatePastTsdf (must equal the same cox_layer_merge calls made by hand, bit for bit)
//   -> ESDF -> traversable cloud -> EsdfMap-style batch queries on the combined map
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_map.hpp"

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
  const double hw = std::cos(0.5 * yaw), hz = std::sin(0.5 * yaw);
  const double o[4] = {0.5, -0.5, 0.5, -0.5};
  T_G_C->q[0] = static_cast<float>(hw * o[0] - hz * o[3]);
  T_G_C->q[1] = static_cast<float>(hw * o[1] - hz * o[2]);
  T_G_C->q[2] = static_cast<float>(hw * o[2] + hz * o[1]);
  T_G_C->q[3] = static_cast<float>(hw * o[3] + hz * o[0]);
  T_G_C->t[0] = T_G_C->t[1] = T_G_C->t[2] = 0.0f;
}

static bool sameDownload(cox_layer_t* a, cox_layer_t* b) {
  uint64_t na = 0, nb = 0;
  if (cox_layer_download(a, nullptr, nullptr, 0, &na) != COX_OK || cox_layer_download(b, nullptr, nullptr, 0, &nb) != COX_OK || na != nb) return false;
  std::vector<int32_t> ia(3 * na), ib(3 * nb);
  std::vector<uint32_t> wa(na * 12288), wb(nb * 12288);
  if (na && (cox_layer_download(a, ia.data(), wa.data(), na, &na) != COX_OK || cox_layer_download(b, ib.data(), wb.data(), nb, &nb) != COX_OK)) return false;
  return ia == ib && wa == wb;
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
  const double ranges[3][2] = {{-0.5, 0.0}, {-0.2, 0.3}, {0.1, 0.6}};
  for (int k = 0; k < 3; ++k) {
    Transformation T_M_S;
    T_M_S.t[0] = 0.03f * static_cast<float>(k);  // each submap sits 3 cm further along x, turned by a small yaw
    const float half = 0.01f * static_cast<float>(k);
    T_M_S.q[0] = std::cos(half);
    T_M_S.q[3] = std::sin(half);
    VoxgraphSubmap::Ptr sm(new VoxgraphSubmap(T_M_S, static_cast<SubmapID>(2 - k), sm_cfg));  // ids added in descending order
    auto integ = TsdfIntegrator::create("merged", cfg, sm->getTsdfMapPtr()->getTsdfLayerPtr());
    for (int f = 0; f < 5; ++f) {
      Pointcloud pts;
      Colors cols;
      Transformation T;
      renderFrame(ranges[k][0] + (ranges[k][1] - ranges[k][0]) * f / 4.0, &pts, &cols, &T);
      integ->integratePointCloud(T, pts, cols, false);
    }
    collection.addSubmap(sm, 0, static_cast<SubmapID>(2 - k));
  }
  // ---- updatePastTsdf == the merges by hand, ascending id ----
  MapServer server(sm_cfg);
  server.updatePastTsdf(collection);
  TsdfLayer by_hand(voxel);
  for (SubmapID id = 0; id < 3; ++id) {
    const VoxgraphSubmap::ConstPtr sm = collection.getSubmapConstPtr(id);
    float T[7];
    sm->getPose().pack(T);
    if (cox_layer_merge(sm->getTsdfMap().getTsdfLayer().handle(), T, by_hand.handle()) != COX_OK) return 10;
  }
  if (server.getTsdfLayer().getNumberOfAllocatedBlocks() < 8) {
    std::printf("combined layer: %zu blocks\n", server.getTsdfLayer().getNumberOfAllocatedBlocks());
    return 11;
  }
  if (!sameDownload(server.getTsdfLayer().handle(), by_hand.handle())) return 12;
  server.updatePastTsdf(collection);  // clears first: the same layer again
  if (!sameDownload(server.getTsdfLayer().handle(), by_hand.handle())) return 13;
  // ---- ESDF, traversable cloud ----
  Pointcloud free_pts;
  std::vector<float> free_d;
  if (server.getConfig().traversability_radius != 1.0f) return 20;
  server.getTraversable(&free_pts, &free_d);
  Pointcloud near_pts;
  std::vector<float> near_d;
  server.getTraversable(0.0f, &near_pts, &near_d);
  if (near_pts.size() <= free_pts.size() || near_pts.size() != near_d.size()) return 21;
  for (float d : free_d)
    if (!(d >= 1.0f)) return 22;
  // ---- batch queries on the combined ESDF: the free points are observed and their nearest distance is their intensity ----
  LayerQuery esdf = server.getEsdfMap();
  std::vector<float> dist;
  std::vector<int> observed;
  esdf.batchGetDistanceAtPosition(near_pts, &dist, &observed, false);
  for (size_t i = 0; i < near_pts.size(); ++i)
    if (!observed[i] || dist[i] != near_d[i]) return 30;
  esdf.batchGetDistanceAtPosition(near_pts, &dist, &observed, true);
  size_t n_interp = 0;
  for (int o : observed) n_interp += o;
  if (n_interp < near_pts.size() / 2) return 31;
  Pointcloud grads;
  esdf.batchGetDistanceAndGradientAtPosition(near_pts, &dist, &grads, &observed);
  size_t n_grad = 0;
  for (int o : observed) n_grad += o;
  if (n_grad < near_pts.size() / 2) return 32;
  float d1 = 0.0f;
  Point g1;
  if (!esdf.isObserved(near_pts[0]) || !esdf.getDistanceAtPosition(near_pts[0], false, &d1) || d1 != near_d[0]) return 33;
  esdf.getDistanceAndGradientAtPosition(near_pts[0], &d1, &g1);
  if (esdf.isObserved(Point{{1000.0f, 1000.0f, 1000.0f}})) return 34;
  std::printf("map smoke ok: %zu blocks, %zu free points (%zu at >= 1 m), %zu interpolated, %zu with gradient\n",
              server.getTsdfLayer().getNumberOfAllocatedBlocks(), near_pts.size(), free_pts.size(), n_interp, n_grad);
  return 0;
}
