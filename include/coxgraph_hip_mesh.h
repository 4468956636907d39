/* Triangle meshes of TSDF layers on the GPU: voxblox's MeshLayer, createConnectedMesh and generateVoxbloxMeshMsg behind a C ABI.
 *
 * What coxgraph's client publishes for every submap (SubmapVisuals::generateSubmapMesh + generateSubmapMeshMsg,
 * coxgraph/src/client/map_server.cpp:119-150) and what the server writes as its final global mesh (every submap meshed, moved by
 * its optimised T_M_S, concatenated; coxgraph/src/server/visualizer/server_visualizer.cpp:20-142).  Kept apart from
 * coxgraph_hip.h on purpose: these entry points have no counterpart in the CPU checker of the test suite.
 *
 * Conventions are those of coxgraph_hip.h (COX_OK or a negative cox_status; NULL handles/outputs -> COX_ERR_INVALID_ARG; no
 * usable GPU -> COX_ERR_NO_DEVICE).  Every call is synchronous.  Rules and arithmetic: DESIGN.md section 7d. */
#ifndef COXGRAPH_HIP_MESH_H_
#define COXGRAPH_HIP_MESH_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* voxblox::MeshLayer: one mesh per block that has at least one triangle, blocks in (z, y, x) order of their index.  Vertices
 * are not shared: triangle t is vertices 3t, 3t+1, 3t+2 of its block, emitted in voxblox's (col + 2, col + 1, col) order; every
 * vertex carries its triangle's face normal and the colour of the TSDF voxel that contains it. */
typedef struct cox_meshlayer cox_meshlayer_t;
/* createConnectedMesh: vertices welded on a proximity grid, triangles as index triples */
typedef struct cox_meshconn cox_meshconn_t;

/* voxblox ColorMode for the wire message (mesh_vis.h) */
typedef enum cox_mesh_color_mode {
  COX_MESH_COLOR = 0,         /* the vertex colour */
  COX_MESH_NORMALS = 1,       /* (n * 0.5 + 0.5) * 255 */
  COX_MESH_GRAY = 2,          /* 0.5 * 255 */
  COX_MESH_LAMBERT = 3,       /* two lights + ambient over gray 0.5 */
  COX_MESH_LAMBERT_COLOR = 4  /* two lights + ambient over the vertex colour */
} cox_mesh_color_mode;

/* MeshIntegrator::generateMesh(only_mesh_updated_blocks = false, clear_updated_flag = false) over the whole layer.  A corner
 * is valid when its weight > min_weight.  Orders behind every frame enqueued on the layer so far.  n_blocks / n_triangles
 * may be NULL.  An empty layer gives an empty mesh. */
int cox_meshlayer_from_layer(cox_layer_t* layer, float min_weight, cox_meshlayer_t** out, uint64_t* n_blocks, uint64_t* n_triangles);
void cox_meshlayer_destroy(cox_meshlayer_t* mesh);
/* sizes; any output may be NULL.  block_edge_length = voxel size * 16 (MeshLayer::block_size) */
int cox_meshlayer_size(const cox_meshlayer_t* mesh, uint64_t* n_blocks, uint64_t* n_vertices, float* block_edge_length);
/* vertices whose colour voxel lay in no allocated block (default colour given; voxblox would dereference a null block) and
 * the HIP-event time of the two mesh kernels (count, write) of the call that built the mesh, in ms */
int cox_meshlayer_stats(const cox_meshlayer_t* mesh, uint64_t* n_color_missing, double kernel_ms[2]);
/* host copies: block_index 3 int32 per block, vertex_begin n_blocks + 1 offsets, xyz / normals 3 floats per vertex, rgb 3 bytes
 * per vertex.  Any output may be NULL (not copied); COX_ERR_BUFFER_TOO_SMALL when a capacity is below the size. */
int cox_meshlayer_download(const cox_meshlayer_t* mesh, int32_t* block_index, uint64_t* vertex_begin, float* xyz, float* normals, uint8_t* rgb,
                           uint64_t cap_blocks, uint64_t cap_vertices);
/* device pointers to the per-vertex arrays (valid until the mesh is destroyed) */
int cox_meshlayer_data_dev(const cox_meshlayer_t* mesh, const float** xyz_dev, const float** normals_dev, const uint8_t** rgb_dev, uint64_t* n_vertices);
/* in place: positions p -> T p, normals n -> R n (T = qw qx qy qz tx ty tz, Eigen's _transformVector order).  Block indices
 * and vertex ranges are kept: a moved mesh is for the global mesh, not for cox_meshlayer_msg. */
int cox_meshlayer_transform(cox_meshlayer_t* mesh, const float T[7]);
/* generateVoxbloxMeshMsg: x/y/z = uint16((p / block_edge - index) / (2 / 65535)), r/g/b from color_mode, in the layout cox_mesh_msg
 * points to (vertex_begin and block_index of cox_meshlayer_download).  Host buffers of cap_vertices entries. */
int cox_meshlayer_msg(const cox_meshlayer_t* mesh, int color_mode, uint16_t* x, uint16_t* y, uint16_t* z, uint8_t* r, uint8_t* g, uint8_t* b,
                      uint64_t cap_vertices);

/* One connected mesh of several meshes (all on one GPU), each moved by its own T (7 floats per part; T_per_part NULL = no move)
 * before welding: a vertex whose cell round(p / proximity_threshold) already holds an earlier vertex
 * (earlier part, then earlier vertex) becomes that vertex.  The surviving vertices keep mesh order and their normal / colour; one
 * triangle per input triangle, degenerate ones included.  n_parts = 0 gives an empty mesh on the current device.
 * COX_ERR_INDEX_RANGE when the vertices span more than 2^21 cells on an axis. */
int cox_meshlayer_connected(const cox_meshlayer_t* const* parts, const float* T_per_part, uint64_t n_parts, float proximity_threshold, cox_meshconn_t** out,
                            uint64_t* n_vertices, uint64_t* n_triangles);
void cox_meshconn_destroy(cox_meshconn_t* mesh);
int cox_meshconn_size(const cox_meshconn_t* mesh, uint64_t* n_vertices, uint64_t* n_triangles);
/* xyz / normals 3 floats, rgb 3 bytes per vertex, triangles 3 uint32 per triangle; any output may be NULL */
int cox_meshconn_download(const cox_meshconn_t* mesh, float* xyz, float* normals, uint8_t* rgb, uint32_t* triangles, uint64_t cap_vertices,
                          uint64_t cap_triangles);

/* ---- clean-up of a connected mesh, in place (what the reference's server leaves to Open3D; rules: DESIGN.md section 7h) ----
 * Every result is deterministic: the same call on the same mesh gives the same bits.  "Mesh order" = vertex / triangle index order. */

/* A connected mesh from host arrays (xyz 3 floats, normals 3 floats or NULL = zero, rgb 3 bytes or NULL = zero per vertex; 3 uint32
 * per triangle).  COX_ERR_INDEX_RANGE when a triangle names a vertex >= n_vertices.  Empty input gives an empty mesh. */
int cox_meshconn_from_arrays(int device, const float* xyz, const float* normals_or_null, const uint8_t* rgb_or_null, const uint32_t* triangles,
                             uint64_t n_vertices, uint64_t n_triangles, cox_meshconn_t** out);
/* RemoveDegenerateTriangles + RemoveDuplicatedTriangles + RemoveUnreferencedVertices: (a) a triangle with two equal indices is
 * dropped; (b) of the triangles with the same canonical form (the rotation with the smallest index first: orientation counts) the
 * first in mesh order stays, with its own rotation; (c) vertices no surviving triangle names are dropped, the others keep mesh
 * order, position, normal and colour; triangles are re-indexed.  removed (may be NULL) = the counts of (a), (b), (c). */
int cox_meshconn_clean(cox_meshconn_t* mesh, uint64_t removed[3]);
/* FilterSmoothTaubin (Open3D's defaults: lambda 0.5, mu -0.53): per iteration a lambda half-step, then a mu half-step.  A half-step
 * with factor f moves every vertex at once: p' = p + f * (s / float(|N|) - p), s = the float32 sum of the positions of N = the
 * vertices that share a triangle edge with it, in ascending index; a vertex without neighbour stays.  Normals and colours are not
 * touched (cox_meshconn_compute_normals refreshes the normals).  kernel_ms (may be NULL): HIP-event time of the 2 * iterations
 * launches.  COX_ERR_INVALID_ARG for iterations < 0 or a factor that is not finite. */
int cox_meshconn_smooth_taubin(cox_meshconn_t* mesh, int iterations, float lambda, float mu, double* kernel_ms);
/* SimplifyVertexClustering with average contraction: per axis origin = min(p) - 0.5f * cell_size and
 * cell = int(floorf((p - origin) / cell_size)) in float32; one vertex per occupied cell, in ascending (z, y, x) cell order;
 * position = float32 sum of the members in ascending index / float(count), colour = rounded integer mean, normal = normalized
 * sum; triangles re-indexed, then cleaned as cox_meshconn_clean does.  COX_ERR_INVALID_ARG unless cell_size is finite and > 0;
 * COX_ERR_INDEX_RANGE when an axis spans 2^21 cells or more.  n_vertices / n_triangles (may be NULL): the new sizes. */
int cox_meshconn_simplify_clustering(cox_meshconn_t* mesh, float cell_size, uint64_t* n_vertices, uint64_t* n_triangles);
/* ComputeVertexNormals: normalized sum, over the triangles of a vertex in ascending index, of cross(p1 - p0, p2 - p0) (area
 * weighted); (0, 0, 0) for a vertex without triangle. */
int cox_meshconn_compute_normals(cox_meshconn_t* mesh);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_MESH_H_ */
