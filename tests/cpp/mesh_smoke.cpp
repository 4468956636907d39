// The client's and the server's mesh flows through coxgraph_amd/host/coxgraph_hip_mesh.hpp:
//   VoxgraphSubmap -> SubmapVisuals::generateSubmapMesh -> generateSubmapMeshMsg -> PLY   (map_server.cpp:119-150)
//   two submaps with poses -> getFinalGlobalMesh                                            (server_visualizer.cpp:20-142)
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).  argv[1]: directory
// for the PLY files (tests/test_gpu_mesh.py reads them back).
#include <cmath>
#include <cstdio>
#include <string>

#include "../../coxgraph_amd/host/coxgraph_hip_mesh.hpp"

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

int main(int argc, char** argv) {
  if (cox_device_count() == 0) {
    try {
      TsdfLayer layer(0.10f);
    } catch (const std::runtime_error& e) {
      std::printf("no GPU: %s\n", e.what());
      return 77;
    }
    return 1;
  }
  const std::string dir = argc > 1 ? argv[1] : ".";
  const float voxel = 0.10f;
  VoxgraphSubmap::Config sm_cfg;
  sm_cfg.tsdf_voxel_size = voxel;
  sm_cfg.capacity_blocks = 2048;
  TsdfIntegratorConfig cfg;
  cfg.default_truncation_distance = 0.3f, cfg.use_const_weight = 1, cfg.max_ray_length_m = 10.0f, cfg.min_ray_length_m = 0.2f;
  SubmapCollection collection(sm_cfg, 1);
  const double ranges[2][2] = {{-0.5, 0.1}, {-0.1, 0.5}};
  for (int k = 0; k < 2; ++k) {
    Transformation T_M_S;
    T_M_S.t[0] = 0.05f * static_cast<float>(k);  // the second submap sits 5 cm further along x
    VoxgraphSubmap::Ptr sm(new VoxgraphSubmap(T_M_S, static_cast<SubmapID>(k), sm_cfg));
    auto integ = TsdfIntegrator::create("merged", cfg, sm->getTsdfMapPtr()->getTsdfLayerPtr());
    for (int f = 0; f < 7; ++f) {
      Pointcloud pts;
      Colors cols;
      Transformation T;
      renderFrame(ranges[k][0] + (ranges[k][1] - ranges[k][0]) * f / 6.0, &pts, &cols, &T);
      integ->integratePointCloud(T, pts, cols, false);
    }
    collection.addSubmap(sm, 0, static_cast<SubmapID>(k));
  }
  // ---- the client: mesh + message of submap 0 ----
  SubmapVisuals visuals;
  MeshLayer::Ptr mesh;
  visuals.generateSubmapMesh(collection.getSubmapConstPtr(0), &mesh);
  if (!mesh || mesh->getNumberOfVertices() < 3000 || mesh->getNumberOfVertices() % 3) return 10;
  MeshMsg msg;
  visuals.generateSubmapMeshMsg(mesh, &msg);
  if (msg.mesh_blocks.size() != mesh->getNumberOfAllocatedMeshes() || !(msg.block_edge_length == 16 * voxel)) return 11;
  size_t n_msg = 0;
  for (const MeshBlockMsg& b : msg.mesh_blocks) {
    if (b.x.empty() || b.x.size() % 3 || b.r.size() != b.x.size()) return 12;
    // decoded with recover mode's formula, every vertex lies in or at the edge of its block (walls x = 3, y = 2.5, floor z = -1.2)
    for (size_t v = 0; v < b.x.size(); ++v) {
      const float p[3] = {(static_cast<float>(b.x[v]) * (2.0f / 65535) + static_cast<float>(b.index[0])) * msg.block_edge_length,
                          (static_cast<float>(b.y[v]) * (2.0f / 65535) + static_cast<float>(b.index[1])) * msg.block_edge_length,
                          (static_cast<float>(b.z[v]) * (2.0f / 65535) + static_cast<float>(b.index[2])) * msg.block_edge_length};
      const float d = std::min(std::fabs(p[0] - 3.0f), std::min(std::fabs(p[1] - 2.5f), std::fabs(p[2] + 1.2f)));
      if (d > 2.0f * voxel) return 13;
    }
    n_msg += b.x.size();
  }
  if (n_msg != mesh->getNumberOfVertices()) return 14;
  // ---- the server: global mesh of both submaps at their poses, PLY ----
  ConnectedMesh global;
  getFinalGlobalMesh(collection, 1.0f, 0.5f * voxel, &global, dir + "/global_mesh.ply");
  if (global.size() < 1000 || global.indices.size() % 3) return 20;
  for (uint32_t i : global.indices)
    if (i >= global.size()) return 21;
  ConnectedMesh single;
  std::vector<const MeshLayer*> parts{mesh.get()};
  createConnectedMesh(parts, {collection.getSubmapConstPtr(0)->getPose()}, 0.5f * voxel, &single);
  if (!outputMeshAsPly(dir + "/submap0_mesh.ply", single)) return 22;
  if (single.indices.size() != mesh->getNumberOfVertices() || single.size() >= global.size()) return 23;
  std::printf("mesh smoke ok: submap 0 %zu blocks %zu vertices (%zu welded), global %zu vertices %zu triangles\n", mesh->getNumberOfAllocatedMeshes(),
              mesh->getNumberOfVertices(), single.size(), global.size(), global.indices.size() / 3);
  return 0;
}
