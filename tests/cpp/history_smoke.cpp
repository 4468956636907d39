// The client's mesh-with-history flow through coxgraph_amd/host/coxgraph_hip_mesh.hpp and its consumer:
//   stamped clouds -> TsdfIntegrator with an ObservationHistory -> generateSubmapMesh -> generateSubmapMeshMsg(history)
//   -> TsdfRecover::processMesh into a fresh layer                                  (tsdf_client.launch:19,46; tsdf_recover.h:59-99)
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>

#include "../../coxgraph_amd/host/coxgraph_hip_mesh.hpp"

using namespace coxgraph_hip;

// a room corner (walls x = 3, y = 2.5, floor z = -1.2) seen by a camera at the origin turned by yaw about z
static void renderFrame(double yaw, Pointcloud* pts, Colors* cols, Transformation* T_G_C) {
  pts->clear();
  cols->clear();
  const double c = std::cos(yaw), s = std::sin(yaw);
  const double R[9] = {s, 0.0, c, -c, 0.0, s, 0.0, -1.0, 0.0};  // Rz(yaw) * optical-to-body
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

int main() {
  if (cox_device_count() == 0) {
    cox_obs_t* h = nullptr;
    if (cox_obs_create(nullptr, 0, &h) != COX_ERR_NO_DEVICE) return 1;
    try {
      TsdfLayer layer(0.10f);
    } catch (const std::runtime_error& e) {
      std::printf("no GPU: %s\n", e.what());
      return 77;
    }
    return 1;
  }
  const float voxel = 0.10f;
  const int n_frames = 9;
  VoxgraphSubmap::Config sm_cfg;
  sm_cfg.tsdf_voxel_size = voxel;
  sm_cfg.capacity_blocks = 2048;
  TsdfIntegratorConfig cfg;
  cfg.default_truncation_distance = 0.3f, cfg.use_const_weight = 1, cfg.max_ray_length_m = 10.0f, cfg.min_ray_length_m = 0.2f;
  VoxgraphSubmap::Ptr sm(new VoxgraphSubmap(Transformation(), 0, sm_cfg));
  TsdfLayer* layer = sm->getTsdfMapPtr()->getTsdfLayerPtr();
  auto integ = TsdfIntegrator::create("merged", cfg, layer);
  ObservationHistory::Ptr history(new ObservationHistory(*layer));
  integ->setObservationHistory(history);
  MeshMsg msg;
  const uint32_t sec0 = 1600000000u, nsec0 = 900000000u;  // (the stamps cross a second boundary)
  for (int f = 0; f < n_frames; ++f) {
    Pointcloud pts;
    Colors cols;
    StampedTransformation pose;
    renderFrame(-0.5 + f / 8.0, &pts, &cols, &pose.T_G_C);
    const uint64_t ns = nsec0 + 50000000ull * static_cast<uint64_t>(f);
    pose.sec = sec0 + static_cast<uint32_t>(ns / 1000000000ull), pose.nsec = static_cast<uint32_t>(ns % 1000000000ull);
    integ->setFrameStamp(pose.sec, pose.nsec);
    integ->integratePointCloud(pose.T_G_C, pts, cols, false);
    msg.trajectory.push_back(pose);
  }
  history->sync();
  if (history->getNumberOfAllocatedBlocks() == 0) return 10;
  // ids beyond the consumer's uint8_t key are refused, not wrapped; the id in use stays
  if (cox_obs_set_frame(history->handle(), 255) != COX_OK || cox_obs_set_frame(history->handle(), 256) != COX_ERR_INDEX_RANGE) return 11;
  // the depth-image entry points do not record: refused while a history is attached
  {
    const float T[7] = {1, 0, 0, 0, 0, 0, 0}, K[4] = {100, 100, 2, 2}, depth[16] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1};
    if (cox_integrate_depth_async(integ->handle(), T, depth, nullptr, 4, 4, K) != COX_ERR_UNSUPPORTED) return 12;
  }
  // ---- the client: mesh + message with histories ----
  SubmapVisuals visuals;
  MeshLayer::Ptr mesh;
  visuals.generateSubmapMesh(sm, &mesh);
  if (!mesh || mesh->getNumberOfVertices() < 3000) return 20;
  visuals.generateSubmapMeshMsg(mesh, *history, &msg);
  size_t n_tri = 0, n_seen = 0, n_pairs = 0;
  for (const MeshBlockMsg& b : msg.mesh_blocks) {
    n_tri += b.x.size() / 3;
    for (const std::vector<uint32_t>& h : b.history) {
      if (h.size() % 2) return 21;
      for (size_t k = 0; k < h.size(); k += 2) {
        if (h[k] > h[k + 1] || h[k + 1] >= static_cast<uint32_t>(n_frames) || (k && h[k] <= h[k - 1] + 1)) return 22;  // ascending, apart, within the stream
        n_pairs += h[k + 1] - h[k] + 1;
      }
      n_seen += h.empty() ? 0 : 1;
    }
  }
  // most triangles were seen by somebody, and the camera turned: not every frame saw every triangle
  if (n_seen < n_tri / 2 || n_pairs >= n_tri * static_cast<size_t>(n_frames)) return 23;
  // ---- the server: recover mode rebuilds a TSDF from it ----
  TsdfLayer recovered(voxel, 16, 0, 2048);
  auto recover_integ = TsdfIntegrator::create("merged", cfg, &recovered);
  MeshConverter conv;
  std::vector<PointXYZRGB> cloud;
  processMesh(&conv, recover_integ.get(), &recovered, msg, nullptr, &cloud);
  recover_integ->sync();
  if (recovered.getNumberOfAllocatedBlocks() == 0 || cloud.size() < 3 * n_seen) return 30;
  // a mesh that has left its layer's frame has no histories
  const float T_move[7] = {1, 0, 0, 0, 0.5f, 0, 0};
  uint64_t nt = 0, nh = 0;
  if (cox_meshlayer_transform(mesh->handle(), T_move) != COX_OK) return 40;
  if (cox_meshlayer_history_size(mesh->handle(), history->handle(), &nt, &nh, nullptr) != COX_ERR_INVALID_ARG) return 41;
  integ->setObservationHistory(nullptr);
  std::printf("history smoke ok: %zu triangles, %zu with a history, %zu (triangle, frame) pairs of %zu, recovered %zu blocks from %zu points\n", n_tri, n_seen,
              n_pairs, n_tri * static_cast<size_t>(n_frames), recovered.getNumberOfAllocatedBlocks(), cloud.size());
  return 0;
}
