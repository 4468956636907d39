// Submap meshes in C++ (header-only, C++14): what coxgraph reaches through
//   SubmapVisuals::generateSubmapMesh + generateSubmapMeshMsg   coxgraph/src/client/map_server.cpp:119-150 (the client's mesh of
//                                                               every submap; with publish_mesh_with_trajectory set, the
//                                                               voxblox_msgs/Mesh that recover mode consumes)
//   ServerVisualizer::getFinalGlobalMesh                        coxgraph/src/server/visualizer/server_visualizer.cpp:20-142 (every
//                                                               submap meshed, moved by its optimised T_M_S, welded, written as PLY)
// on top of include/coxgraph_hip_mesh.h: the meshes stay on the submap's GPU until they are downloaded or welded.  The Open3D
// steps of the reference's global mesh (merge / dedupe / Taubin smooth / vertex clustering) run on the GPU too: GlobalMeshCleanup.
#pragma once
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "../../include/coxgraph_hip_history.h"
#include "../../include/coxgraph_hip_mesh.h"
#include "coxgraph_hip_submap.hpp"

namespace coxgraph_hip {

// voxblox::MeshLayer on the GPU
class MeshLayer {
 public:
  typedef std::shared_ptr<MeshLayer> Ptr;
  explicit MeshLayer(cox_meshlayer_t* h) : h_(h) {}
  ~MeshLayer() { cox_meshlayer_destroy(h_); }
  MeshLayer(const MeshLayer&) = delete;
  MeshLayer& operator=(const MeshLayer&) = delete;
  cox_meshlayer_t* handle() const { return h_; }
  size_t getNumberOfAllocatedMeshes() const {
    uint64_t nb = 0;
    check(cox_meshlayer_size(h_, &nb, nullptr, nullptr), "MeshLayer");
    return nb;
  }
  size_t getNumberOfVertices() const {
    uint64_t nv = 0;
    check(cox_meshlayer_size(h_, nullptr, &nv, nullptr), "MeshLayer");
    return nv;
  }

 private:
  cox_meshlayer_t* h_;
};

// The message is recover mode's MeshMsg (coxgraph_hip_adapters.hpp): generateVoxbloxMeshMsg fills block_edge_length and the
// blocks' index / x y z / r g b; fillMeshHistories adds the histories of an ObservationHistory; the trajectory stays the caller's.
enum class ColorMode { kColor = COX_MESH_COLOR, kNormals = COX_MESH_NORMALS, kGray = COX_MESH_GRAY, kLambert = COX_MESH_LAMBERT, kLambertColor = COX_MESH_LAMBERT_COLOR };

// voxblox::Mesh after createConnectedMesh: welded vertices, triangles as index triples
struct ConnectedMesh {
  std::vector<float> vertices, normals;  // 3 per vertex
  std::vector<uint8_t> colors;           // r g b per vertex
  std::vector<uint32_t> indices;         // 3 per triangle
  size_t size() const { return vertices.size() / 3; }
};

// generateVoxbloxMeshMsg(mesh_layer, color_mode, &msg)
inline void generateVoxbloxMeshMsg(const MeshLayer& mesh_layer, ColorMode color_mode, MeshMsg* msg) {
  uint64_t nb = 0, nv = 0;
  float edge = 0.0f;
  check(cox_meshlayer_size(mesh_layer.handle(), &nb, &nv, &edge), "generateVoxbloxMeshMsg");
  std::vector<int32_t> idx(3 * nb);
  std::vector<uint64_t> begin(nb + 1);
  check(cox_meshlayer_download(mesh_layer.handle(), idx.data(), begin.data(), nullptr, nullptr, nullptr, nb, 0), "generateVoxbloxMeshMsg");
  std::vector<uint16_t> x(nv), y(nv), z(nv);
  std::vector<uint8_t> r(nv), g(nv), b(nv);
  if (nv) check(cox_meshlayer_msg(mesh_layer.handle(), static_cast<int>(color_mode), x.data(), y.data(), z.data(), r.data(), g.data(), b.data(), nv),
                "generateVoxbloxMeshMsg");
  msg->block_edge_length = edge;
  msg->mesh_blocks.resize(nb);
  for (uint64_t k = 0; k < nb; ++k) {
    MeshBlockMsg& m = msg->mesh_blocks[k];
    for (int a = 0; a < 3; ++a) m.index[a] = idx[3 * k + a];
    const uint64_t s = begin[k], e = begin[k + 1];
    m.x.assign(x.begin() + s, x.begin() + e);
    m.y.assign(y.begin() + s, y.begin() + e);
    m.z.assign(z.begin() + s, z.begin() + e);
    m.r.assign(r.begin() + s, r.begin() + e);
    m.g.assign(g.begin() + s, g.begin() + e);
    m.b.assign(b.begin() + s, b.begin() + e);
  }
}

// the per-triangle observation histories of mesh_layer (still in its layer's frame) into a message generateVoxbloxMeshMsg has
// filled from it; a block none of whose triangles was seen keeps an empty history (recover mode skips it)
inline void fillMeshHistories(const MeshLayer& mesh_layer, const ObservationHistory& history, MeshMsg* msg) {
  uint64_t nt = 0, nh = 0;
  check(cox_meshlayer_history_size(mesh_layer.handle(), history.handle(), &nt, &nh, nullptr), "fillMeshHistories");
  const size_t nb = msg->mesh_blocks.size();
  std::vector<uint64_t> begin(nt + 1);
  std::vector<uint32_t> runs(nh);
  std::vector<uint8_t> has(nb);
  check(cox_meshlayer_history(mesh_layer.handle(), history.handle(), begin.data(), runs.data(), has.data(), nt, nh, nb), "fillMeshHistories");
  uint64_t t = 0;
  for (size_t k = 0; k < nb; ++k) {
    MeshBlockMsg& m = msg->mesh_blocks[k];
    const size_t n = m.x.size() / 3;
    m.history.clear();
    if (has[k]) {
      m.history.resize(n);
      for (size_t i = 0; i < n; ++i) m.history[i].assign(runs.begin() + begin[t + i], runs.begin() + begin[t + i + 1]);
    }
    t += n;
  }
  if (t != nt) throw std::runtime_error("fillMeshHistories: the message is not this mesh layer's");
}

// createConnectedMesh over several mesh layers, each moved by its pose first
inline void createConnectedMesh(const std::vector<const MeshLayer*>& parts, const std::vector<Transformation>& poses, float proximity_threshold,
                                ConnectedMesh* out) {
  if (parts.size() != poses.size()) throw std::runtime_error("createConnectedMesh: one pose per part");
  std::vector<const cox_meshlayer_t*> h;
  std::vector<float> T(7 * parts.size());
  for (size_t i = 0; i < parts.size(); ++i) {
    h.push_back(parts[i]->handle());
    poses[i].pack(&T[7 * i]);
  }
  cox_meshconn_t* c = nullptr;
  uint64_t nv = 0, nt = 0;
  check(cox_meshlayer_connected(h.data(), T.data(), h.size(), proximity_threshold, &c, &nv, &nt), "createConnectedMesh");
  out->vertices.resize(3 * nv);
  out->normals.resize(3 * nv);
  out->colors.resize(3 * nv);
  out->indices.resize(3 * nt);
  const int st = cox_meshconn_download(c, out->vertices.data(), out->normals.data(), out->colors.data(), out->indices.data(), nv, nt);
  cox_meshconn_destroy(c);
  check(st, "createConnectedMesh");
}

// voxblox outputMeshAsPly: binary little-endian, the layout coxgraph_amd/mesh_io.py reads
inline bool outputMeshAsPly(const std::string& path, const ConnectedMesh& mesh) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const size_t nv = mesh.size(), nt = mesh.indices.size() / 3;
  std::fprintf(f,
               "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
               "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
               "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
               nv, nt);
  bool ok = true;
  for (size_t v = 0; v < nv && ok; ++v) {
    ok = std::fwrite(&mesh.vertices[3 * v], sizeof(float), 3, f) == 3 && std::fwrite(&mesh.normals[3 * v], sizeof(float), 3, f) == 3 &&
         std::fwrite(&mesh.colors[3 * v], 1, 3, f) == 3;
  }
  for (size_t t = 0; t < nt && ok; ++t) {
    const unsigned char three = 3;
    const int32_t i[3] = {static_cast<int32_t>(mesh.indices[3 * t]), static_cast<int32_t>(mesh.indices[3 * t + 1]), static_cast<int32_t>(mesh.indices[3 * t + 2])};
    ok = std::fwrite(&three, 1, 1, f) == 1 && std::fwrite(i, sizeof(int32_t), 3, f) == 3;
  }
  return std::fclose(f) == 0 && ok;
}

// coxgraph::SubmapVisuals (the part map_server.cpp and server_visualizer.cpp call)
class SubmapVisuals {
 public:
  struct Config {
    float mesh_min_weight = 2.0f;  // coxgraph_client.yaml:52-54 (the server's visualizer uses 1.0, server.yaml:19-22)
    ColorMode color_mode = ColorMode::kLambertColor;
  };
  SubmapVisuals() {}
  explicit SubmapVisuals(const Config& config) : config_(config) {}

  // the submap's TSDF in its own frame -> a mesh layer on the submap's GPU
  void generateSubmapMesh(const VoxgraphSubmap::ConstPtr& submap_ptr, MeshLayer::Ptr* mesh_layer_ptr) const {
    if (!submap_ptr || !mesh_layer_ptr) throw std::runtime_error("generateSubmapMesh: null argument");
    cox_meshlayer_t* h = nullptr;
    check(cox_meshlayer_from_layer(submap_ptr->getTsdfMap().getTsdfLayer().handle(), config_.mesh_min_weight, &h, nullptr, nullptr), "generateSubmapMesh");
    mesh_layer_ptr->reset(new MeshLayer(h));
  }
  void generateSubmapMeshMsg(const MeshLayer::Ptr& mesh_layer_ptr, MeshMsg* mesh_msg) const {
    generateSubmapMeshMsg(mesh_layer_ptr, config_.color_mode, mesh_msg);
  }
  void generateSubmapMeshMsg(const MeshLayer::Ptr& mesh_layer_ptr, ColorMode color_mode, MeshMsg* mesh_msg) const {
    if (!mesh_layer_ptr || !mesh_msg) throw std::runtime_error("generateSubmapMeshMsg: null argument");
    generateVoxbloxMeshMsg(*mesh_layer_ptr, color_mode, mesh_msg);
  }
  // publish_mesh_with_history (tsdf_client.launch:19,46): the message with the histories recorded while the submap was fused
  void generateSubmapMeshMsg(const MeshLayer::Ptr& mesh_layer_ptr, const ObservationHistory& history, MeshMsg* mesh_msg) const {
    generateSubmapMeshMsg(mesh_layer_ptr, config_.color_mode, mesh_msg);
    fillMeshHistories(*mesh_layer_ptr, history, mesh_msg);
  }

 private:
  Config config_;
};

// ServerVisualizer::getFinalGlobalMesh without Open3D: every submap of the collection meshed, moved by its (optimised) pose, welded
// at proximity_threshold and, when path is not empty, written as PLY.  Submaps in id order.
inline void getFinalGlobalMesh(const SubmapCollection& collection, float mesh_min_weight, float proximity_threshold, ConnectedMesh* combined_mesh,
                               const std::string& ply_path = std::string()) {
  SubmapVisuals::Config cfg;
  cfg.mesh_min_weight = mesh_min_weight;
  const SubmapVisuals visuals(cfg);
  std::vector<MeshLayer::Ptr> meshes;
  std::vector<const MeshLayer*> parts;
  std::vector<Transformation> poses;
  for (SubmapID id : collection.getIDs()) {
    const VoxgraphSubmap::ConstPtr sm = collection.getSubmapConstPtr(id);
    meshes.emplace_back();
    visuals.generateSubmapMesh(sm, &meshes.back());
    parts.push_back(meshes.back().get());
    poses.push_back(sm->getPose());
  }
  createConnectedMesh(parts, poses, proximity_threshold, combined_mesh);
  if (!ply_path.empty() && !outputMeshAsPly(ply_path, *combined_mesh)) throw std::runtime_error("getFinalGlobalMesh: cannot write " + ply_path);
}

// The Open3D chain of ServerVisualizer::getFinalGlobalMesh (server_visualizer.cpp:67-86) with the reference's constants:
// MergeCloseVertices(0.06), RemoveDuplicatedVertices / Triangles, FilterSmoothTaubin(100), SimplifyVertexClustering(0.05).
struct GlobalMeshCleanup {
  float proximity_threshold = 0.06f;
  int taubin_iterations = 100;
  float lambda = 0.5f;
  float mu = -0.53f;
  float cluster_size = 0.05f;
  bool recompute_normals = true;      // smoothing and clustering leave the normals stale
  bool cleanup_every_submap = false;  // true: the reference's loop, the chain after every appended submap
};

namespace detail {
struct MeshConnHandle {  // owns a cox_meshconn_t
  cox_meshconn_t* h = nullptr;
  MeshConnHandle() {}
  ~MeshConnHandle() { cox_meshconn_destroy(h); }
  MeshConnHandle(const MeshConnHandle&) = delete;
  MeshConnHandle& operator=(const MeshConnHandle&) = delete;
};
inline void downloadConnectedMesh(const cox_meshconn_t* c, ConnectedMesh* out) {
  uint64_t nv = 0, nt = 0;
  check(cox_meshconn_size(c, &nv, &nt), "downloadConnectedMesh");
  out->vertices.assign(3 * nv, 0.0f);
  out->normals.assign(3 * nv, 0.0f);
  out->colors.assign(3 * nv, 0);
  out->indices.assign(3 * nt, 0);
  check(cox_meshconn_download(c, out->vertices.data(), out->normals.data(), out->colors.data(), out->indices.data(), nv, nt), "downloadConnectedMesh");
}
// clean -> smooth -> cluster -> normals, in place on the device
inline void cleanupConnectedMesh(cox_meshconn_t* c, const GlobalMeshCleanup& cleanup) {
  check(cox_meshconn_clean(c, nullptr), "cleanupConnectedMesh: clean");
  check(cox_meshconn_smooth_taubin(c, cleanup.taubin_iterations, cleanup.lambda, cleanup.mu, nullptr), "cleanupConnectedMesh: smooth");
  check(cox_meshconn_simplify_clustering(c, cleanup.cluster_size, nullptr, nullptr), "cleanupConnectedMesh: cluster");
  if (cleanup.recompute_normals) check(cox_meshconn_compute_normals(c), "cleanupConnectedMesh: normals");
}
}  // namespace detail

// ServerVisualizer::getFinalGlobalMesh with its clean-up: every submap meshed, moved by its pose and welded at
// cleanup.proximity_threshold; the combined mesh stays on the device through clean, smooth, cluster and normals and is downloaded
// once.  The reference runs the chain again after every submap it appends, so early submaps are smoothed once per later submap;
// the default here runs it once over all submaps (cleanup_every_submap = false).  With cleanup_every_submap the loop is the
// reference's: the cleaned mesh so far and the next submap's welded mesh are concatenated (through the host: one round trip per
// submap), then the chain runs on the result.
inline void getFinalGlobalMesh(const SubmapCollection& collection, float mesh_min_weight, const GlobalMeshCleanup& cleanup, ConnectedMesh* combined_mesh,
                               const std::string& ply_path = std::string()) {
  SubmapVisuals::Config cfg;
  cfg.mesh_min_weight = mesh_min_weight;
  const SubmapVisuals visuals(cfg);
  std::vector<MeshLayer::Ptr> meshes;
  std::vector<const cox_meshlayer_t*> parts;
  std::vector<float> T;
  for (SubmapID id : collection.getIDs()) {
    const VoxgraphSubmap::ConstPtr sm = collection.getSubmapConstPtr(id);
    meshes.emplace_back();
    visuals.generateSubmapMesh(sm, &meshes.back());
    parts.push_back(meshes.back()->handle());
    T.resize(T.size() + 7);
    sm->getPose().pack(&T[T.size() - 7]);
  }
  if (!cleanup.cleanup_every_submap) {
    detail::MeshConnHandle c;
    check(cox_meshlayer_connected(parts.data(), T.data(), parts.size(), cleanup.proximity_threshold, &c.h, nullptr, nullptr), "getFinalGlobalMesh");
    detail::cleanupConnectedMesh(c.h, cleanup);
    detail::downloadConnectedMesh(c.h, combined_mesh);
  } else {
    *combined_mesh = ConnectedMesh();
    for (size_t k = 0; k < parts.size(); ++k) {
      ConnectedMesh next;
      {
        detail::MeshConnHandle part;
        check(cox_meshlayer_connected(&parts[k], &T[7 * k], 1, cleanup.proximity_threshold, &part.h, nullptr, nullptr), "getFinalGlobalMesh");
        detail::downloadConnectedMesh(part.h, &next);
      }
      const uint32_t base = static_cast<uint32_t>(combined_mesh->size());
      combined_mesh->vertices.insert(combined_mesh->vertices.end(), next.vertices.begin(), next.vertices.end());
      combined_mesh->normals.insert(combined_mesh->normals.end(), next.normals.begin(), next.normals.end());
      combined_mesh->colors.insert(combined_mesh->colors.end(), next.colors.begin(), next.colors.end());
      for (uint32_t i : next.indices) combined_mesh->indices.push_back(base + i);
      detail::MeshConnHandle c;
      check(cox_meshconn_from_arrays(collection.getConfig().device, combined_mesh->vertices.data(), combined_mesh->normals.data(), combined_mesh->colors.data(),
                                     combined_mesh->indices.data(), combined_mesh->size(), combined_mesh->indices.size() / 3, &c.h),
            "getFinalGlobalMesh");
      detail::cleanupConnectedMesh(c.h, cleanup);
      detail::downloadConnectedMesh(c.h, combined_mesh);
    }
  }
  if (!ply_path.empty() && !outputMeshAsPly(ply_path, *combined_mesh)) throw std::runtime_error("getFinalGlobalMesh: cannot write " + ply_path);
}

}  // namespace coxgraph_hip
