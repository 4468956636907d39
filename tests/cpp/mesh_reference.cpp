// Test-side reference of the GPU mesher (coxgraph_amd/csrc/cox_mesher.hip), loaded by tests/test_gpu_mesh.py through ctypes.
//
// Vertex positions and the block / cube order come from the CPU checker's own marching cubes (oracle/cox_oracle_submap.hpp:
// blocksInZyxOrder + mcBlock), run on an oracle Layer rebuilt from the engine's downloaded wire arrays.  What the checker does
// not have -- face normals, vertex colours (MeshIntegrator::updateMeshColor), the wire encoding and the colour modes of
// voxblox's mesh_vis.h -- is restated here, single-threaded, in the float order DESIGN.md section 7d writes down.
// Build: g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -fno-fast-math (as oracle/Makefile).
#include <chrono>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../oracle/cox_oracle.hpp"
#include "../../oracle/cox_oracle_submap.hpp"

using namespace coxo;

namespace {

struct RefMesh {
  std::vector<int32_t> block_index;
  std::vector<uint64_t> vertex_begin{0};
  std::vector<float> xyz, nrm;
  std::vector<uint8_t> rgb;
  uint64_t n_missing = 0;
  double mesh_seconds = 0.0;
};

// updateMeshColor: containing voxel, or the block found by coordinates and the voxel clamped into it; valid when weight > min_weight
Color vertexColor(const Layer& L, const Block* b, V3 v, float min_weight, uint64_t* n_missing) {
  const GIdx gi = gridIndexFromPoint(v - b->origin, L.voxel_size_inv);
  const TsdfVoxel* vox = nullptr;
  if (gi.x >= 0 && gi.x < L.vps && gi.y >= 0 && gi.y < L.vps && gi.z >= 0 && gi.z < L.vps) {
    vox = &b->voxels[linearIndex(static_cast<int>(gi.x), static_cast<int>(gi.y), static_cast<int>(gi.z), L.vps)];
  } else {
    const Block* nb = L.getBlockPtr(blockIndexFromPoint(v, L.block_size_inv));
    if (!nb) {
      ++*n_missing;
      return Color();
    }
    const GIdx g = gridIndexFromPoint(v - nb->origin, L.voxel_size_inv);
    int l[3] = {static_cast<int>(g.x), static_cast<int>(g.y), static_cast<int>(g.z)};
    for (int k = 0; k < 3; ++k) l[k] = std::max(std::min(l[k], L.vps - 1), 0);
    vox = &nb->voxels[linearIndex(l[0], l[1], l[2], L.vps)];
  }
  return vox->weight > min_weight ? vox->color : Color();
}

uint8_t unitToByte(float u) {
  const float c = std::min(u, 1.0f) * 255.0f;
  return static_cast<uint8_t>(c > 0.0f ? static_cast<int>(c) : 0);
}
uint16_t encodeCoord(float p, float block_edge, int index) {
  const float q = (p / block_edge - static_cast<float>(index)) / (2.0f / 65535.0f);
  if (!(q > 0.0f)) return 0;
  if (q >= 65535.0f) return 65535;
  return static_cast<uint16_t>(q);
}

}  // namespace

extern "C" {

// mesh of the layer given as wire arrays (block_idx 3 int32 per block, words 4096 * 3 uint32 per block)
void* mesh_ref_build(float voxel_size, uint64_t n_blocks, const int32_t* block_idx, const uint32_t* words, float min_weight) {
  Layer L(voxel_size, 16);
  for (uint64_t i = 0; i < n_blocks; ++i) {
    Block* b = L.allocateBlock(BIdx{block_idx[3 * i], block_idx[3 * i + 1], block_idx[3 * i + 2]});
    for (int v = 0; v < 4096; ++v) wordsToVoxel(words + (i * 4096 + v) * 3, &b->voxels[v]);
  }
  RefMesh* M = new RefMesh();
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<V3> verts;
  for (const Block* b : blocksInZyxOrder(L)) {
    verts.clear();
    mcBlock(L, b, min_weight, &verts);
    if (verts.empty()) continue;
    M->block_index.insert(M->block_index.end(), {b->index.x, b->index.y, b->index.z});
    for (size_t t = 0; t + 2 < verts.size(); t += 3) {
      const V3 n = normalized(cross(verts[t + 1] - verts[t], verts[t + 2] - verts[t]));  // points to the positive side
      for (int j = 0; j < 3; ++j) {
        const V3 v = verts[t + j];
        const Color c = vertexColor(L, b, v, min_weight, &M->n_missing);
        M->xyz.insert(M->xyz.end(), {v.x, v.y, v.z});
        M->nrm.insert(M->nrm.end(), {n.x, n.y, n.z});
        M->rgb.insert(M->rgb.end(), {c.r, c.g, c.b});
      }
    }
    M->vertex_begin.push_back(M->vertex_begin.back() + verts.size());
  }
  M->mesh_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return M;
}

void mesh_ref_free(void* h) { delete static_cast<RefMesh*>(h); }

void mesh_ref_size(const void* h, uint64_t* n_blocks, uint64_t* n_vertices, uint64_t* n_missing, double* mesh_seconds) {
  const RefMesh* M = static_cast<const RefMesh*>(h);
  *n_blocks = M->block_index.size() / 3;
  *n_vertices = M->xyz.size() / 3;
  *n_missing = M->n_missing;
  *mesh_seconds = M->mesh_seconds;
}

void mesh_ref_get(const void* h, int32_t* block_index, uint64_t* vertex_begin, float* xyz, float* nrm, uint8_t* rgb) {
  const RefMesh* M = static_cast<const RefMesh*>(h);
  std::memcpy(block_index, M->block_index.data(), M->block_index.size() * sizeof(int32_t));
  std::memcpy(vertex_begin, M->vertex_begin.data(), M->vertex_begin.size() * sizeof(uint64_t));
  std::memcpy(xyz, M->xyz.data(), M->xyz.size() * sizeof(float));
  std::memcpy(nrm, M->nrm.data(), M->nrm.size() * sizeof(float));
  std::memcpy(rgb, M->rgb.data(), M->rgb.size());
}

// generateVoxbloxMeshMsg of the reference mesh; mode as cox_mesh_color_mode
void mesh_ref_msg(const void* h, float block_edge, int mode, uint16_t* x, uint16_t* y, uint16_t* z, uint8_t* r, uint8_t* g, uint8_t* b) {
  const RefMesh* M = static_cast<const RefMesh*>(h);
  const V3 l1 = normalized(V3{0.8f, -0.2f, 0.7f}), l2 = normalized(V3{-0.5f, 0.2f, 0.2f});
  const size_t nb = M->block_index.size() / 3;
  for (size_t k = 0; k < nb; ++k)
    for (uint64_t v = M->vertex_begin[k]; v < M->vertex_begin[k + 1]; ++v) {
      x[v] = encodeCoord(M->xyz[3 * v], block_edge, M->block_index[3 * k]);
      y[v] = encodeCoord(M->xyz[3 * v + 1], block_edge, M->block_index[3 * k + 1]);
      z[v] = encodeCoord(M->xyz[3 * v + 2], block_edge, M->block_index[3 * k + 2]);
      const V3 n{M->nrm[3 * v], M->nrm[3 * v + 1], M->nrm[3 * v + 2]};
      uint8_t c[3] = {M->rgb[3 * v], M->rgb[3 * v + 1], M->rgb[3 * v + 2]};
      if (mode == 1) {  // normals
        const float f[3] = {n.x, n.y, n.z};
        for (int i = 0; i < 3; ++i) c[i] = unitToByte(f[i] * 0.5f + 0.5f);
      } else if (mode == 2) {  // gray
        c[0] = c[1] = c[2] = unitToByte(0.5f);
      } else if (mode == 3 || mode == 4) {  // lambert, lambert_color
        const float d1 = std::max(dot(n, l1), 0.0f), d2 = std::max(dot(n, l2), 0.0f);
        for (int i = 0; i < 3; ++i) {
          const float base = (mode == 3) ? 0.5f : static_cast<float>(c[i]) / 255.0f;
          c[i] = unitToByte((d1 * base + d2 * base) + 0.2f);
        }
      }
      r[v] = c[0];
      g[v] = c[1];
      b[v] = c[2];
    }
}

}  // extern "C"
