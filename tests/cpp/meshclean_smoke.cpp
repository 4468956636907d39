// The server's global mesh with its clean-up through coxgraph_amd/host/coxgraph_hip_mesh.hpp:
//   two submaps with poses -> getFinalGlobalMesh(collection, min_weight, GlobalMeshCleanup, &mesh, ply)   (server_visualizer.cpp:67-86)
// once with the chain run once over all submaps (the default) and once after every submap (the reference's loop).
// Exit code 0 = all good; 77 = no GPU.  argv[1]: directory for the PLY files (tests/test_gpu_meshclean.py reads them back).
#include <array>
#include <cmath>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_mesh.hpp"

using namespace coxgraph_hip;

// a room corner (walls x = 3, y = 2.5, floor z = -1.2) seen by a camera at the origin turned by yaw about z
static void renderFrame(double yaw, Pointcloud* pts, Colors* cols, Transformation* T_G_C) {
  pts->clear();
  cols->clear();
  const double c = std::cos(yaw), s = std::sin(yaw);
  const double R[9] = {s, 0.0, c, -c, 0.0, s, 0.0, -1.0, 0.0};  // optical frame: z forward, x right, y down
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

// no degenerate or duplicate triangle, no unreferenced vertex, every index in range
static int checkClean(const ConnectedMesh& m) {
  std::set<std::array<uint32_t, 3>> seen;
  std::vector<char> used(m.size(), 0);
  for (size_t t = 0; t < m.indices.size(); t += 3) {
    std::array<uint32_t, 3> c{{m.indices[t], m.indices[t + 1], m.indices[t + 2]}};
    for (uint32_t i : c) {
      if (i >= m.size()) return 1;
      used[i] = 1;
    }
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return 2;
    while (c[0] > c[1] || c[0] > c[2]) c = {{c[1], c[2], c[0]}};
    if (!seen.insert(c).second) return 3;
  }
  for (char u : used)
    if (!u) return 4;
  return 0;
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
    T_M_S.t[0] = 0.05f * static_cast<float>(k);
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
  ConnectedMesh raw, cleaned, again, looped;
  getFinalGlobalMesh(collection, 1.0f, 0.06f, &raw);
  GlobalMeshCleanup cleanup;
  cleanup.taubin_iterations = 10;
  getFinalGlobalMesh(collection, 1.0f, cleanup, &cleaned, dir + "/global_mesh_clean.ply");
  getFinalGlobalMesh(collection, 1.0f, cleanup, &again);
  if (cleaned.size() < 100 || cleaned.indices.size() % 3 || cleaned.indices.empty()) return 20;
  if (const int st = checkClean(cleaned)) return 20 + st;
  if (cleaned.size() > raw.size() || cleaned.indices.size() >= raw.indices.size()) return 25;
  if (cleaned.vertices != again.vertices || cleaned.normals != again.normals || cleaned.colors != again.colors || cleaned.indices != again.indices) return 26;
  // the surface is still the room's: every vertex within two voxels of a wall or the floor; normals are unit or zero
  for (size_t v = 0; v < cleaned.size(); ++v) {
    const float* p = &cleaned.vertices[3 * v];
    const float* n = &cleaned.normals[3 * v];
    const float d = std::min(std::fabs(p[0] - 3.0f), std::min(std::fabs(p[1] - 2.5f), std::fabs(p[2] + 1.2f)));
    if (d > 2.0f * voxel) return 27;
    const float nn = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(std::fabs(nn - 1.0f) < 1e-4f || nn == 0.0f)) return 28;
  }
  cleanup.cleanup_every_submap = true;
  getFinalGlobalMesh(collection, 1.0f, cleanup, &looped, dir + "/global_mesh_loop.ply");
  if (looped.size() < 100 || looped.indices.empty()) return 30;
  if (const int st = checkClean(looped)) return 30 + st;
  std::printf("meshclean smoke ok: raw %zu vertices %zu triangles, cleaned %zu / %zu, per-submap loop %zu / %zu\n", raw.size(), raw.indices.size() / 3,
              cleaned.size(), cleaned.indices.size() / 3, looped.size(), looped.indices.size() / 3);
  return 0;
}
