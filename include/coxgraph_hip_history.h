/* Observation histories: which frames saw which part of a submap, recorded while the frames are fused, and the per-triangle
 * run-length lists a mesh-with-history carries (voxblox_msgs/Mesh with ObsHistory, as recover mode consumes it:
 * coxgraph/include/coxgraph/map_comm/tsdf_recover.h:59-99, mesh_converter.h:87-199).
 *
 * The fork of voxblox that records histories on the client is not part of the reference tree, so the rule is this project's own
 * (DESIGN.md section 7f): a frame marks the 4x4x4-voxel cell every one of its surface points lands in; a triangle's history is the
 * union of the cells that contain its three vertices.  Kept apart from coxgraph_hip.h on purpose: these entry points have no
 * counterpart in the CPU checker of the test suite.
 *
 * Conventions are those of coxgraph_hip.h (COX_OK or a negative cox_status; NULL handles/outputs -> COX_ERR_INVALID_ARG; no
 * usable GPU -> COX_ERR_NO_DEVICE). */
#ifndef COXGRAPH_HIP_HISTORY_H_
#define COXGRAPH_HIP_HISTORY_H_
#include "coxgraph_hip.h"
#include "coxgraph_hip_mesh.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COX_OBS_MAX_FRAMES 256 /* frame ids 0..255: the consumer's key is a uint8_t (mesh_converter.h:194-199) */
#define COX_OBS_CELLS_PER_BLOCK 64
#define COX_OBS_WORDS_PER_CELL 8

/* the record of one submap: per allocated 16^3 block 64 cells of 4x4x4 voxels (cell = (x >> 2) + 4 * (y >> 2) + 16 * (z >> 2) of the
 * voxel's local index), per cell a 256-bit mask, bit f (word f >> 5, bit f & 31) set when frame f marked the cell */
typedef struct cox_obs cox_obs_t;

/* geometry (device, voxel size) from `geometry`; the record has a block table and pool of its own and does not follow that
 * layer afterwards.  capacity_blocks = 0 picks a default; the pool doubles as it fills (cox_obs_set_auto_grow) */
int cox_obs_create(const cox_layer_t* geometry, uint64_t capacity_blocks, cox_obs_t** out);
/* an integrator it is attached to must be detached (or destroyed) first */
void cox_obs_destroy(cox_obs_t* obs);
/* forget everything (the submap was cut: next to cox_layer_clear).  The frame id is kept. */
int cox_obs_clear(cox_obs_t* obs);
int cox_obs_set_auto_grow(cox_obs_t* obs, int on);
/* the id under which clouds are recorded until it is changed.  frame_id > 255 -> COX_ERR_INDEX_RANGE (not wrapped), the id stays */
int cox_obs_set_frame(cox_obs_t* obs, uint32_t frame_id);
/* Record one cloud (points in the sensor frame, device memory): a point marks the cell of grid_index(T_G_C p / voxel_size) when it
 * passes isPointValid with min_ray / max_ray and is not a clearing ray (beyond max_ray, or any point of a freespace cloud;
 * allow_clear only decides whether such a point is a clearing ray or dropped: neither marks).  Enqueued on the record's own
 * stream behind what hip_stream (the stream that produced xyz_dev; NULL = the null stream) holds so far; hip_stream then waits
 * until the cloud has been read.  Not waited for: cox_obs_sync reports a pool that ran out. */
int cox_obs_record_dev(cox_obs_t* obs, const float T_G_C[7], const float* xyz_dev, uint64_t n, int freespace, float min_ray, float max_ray, int allow_clear,
                       void* hip_stream);
/* the same from host memory; returns when the cloud is recorded.  With auto-grow on it loses nothing to a full pool: the pool is
 * doubled and the cloud marked again (marking is idempotent). */
int cox_obs_record(cox_obs_t* obs, const float T_G_C[7], const float* xyz, uint64_t n, int freespace, float min_ray, float max_ray, int allow_clear);
/* wait for every record enqueued so far; COX_ERR_POOL_EXHAUSTED when marks were lost because the pool was full (auto-grow off, or
 * a cloud outran it), COX_ERR_INDEX_RANGE for points beyond the index range.  Reported once. */
int cox_obs_sync(cox_obs_t* obs);
/* allocated blocks, cells with at least one mark, device bytes held; any output may be NULL.  Waits like cox_obs_sync. */
int cox_obs_stats(cox_obs_t* obs, uint64_t* n_blocks, uint64_t* n_marked_cells, uint64_t* bytes);
/* running totals since creation / clear: points that marked, and atomic-OR candidates left after the lanes of a wave that share a
 * cell merged (one per distinct cell per wave) */
int cox_obs_counts(cox_obs_t* obs, uint64_t* n_marking_points, uint64_t* n_atomics);
/* blocks in packed-key (z, y, x) order like cox_layer_download: block_index 3 int32 per block, masks 64 * 8 uint32 per block.
 * NULL buffers: only *n_blocks.  COX_ERR_BUFFER_TOO_SMALL when cap_blocks is below the count. */
int cox_obs_download(cox_obs_t* obs, int32_t* block_index, uint32_t* masks, uint64_t cap_blocks, uint64_t* n_blocks);

/* While a record is attached, every cox_integrate_points, _ex (deintegrate = 0), _dev and _async call of the integrator (all four
 * methods) also records its cloud under the record's current frame id, from the device copy the integrator holds, on the
 * record's stream.  Deintegration does not unmark.  The depth-image entry points return COX_ERR_UNSUPPORTED while attached.
 * obs = NULL detaches.  The record must share the layer's device and voxel size (COX_ERR_INVALID_ARG). */
int cox_integrator_attach_history(cox_integrator_t* integ, cox_obs_t* obs);

/* Histories of a mesh that is still in its layer's frame (after cox_meshlayer_transform: COX_ERR_INVALID_ARG): per triangle the OR of the
 * masks of the cells containing its three vertices (a missing block counts as all zero), as ascending inclusive [first, last]
 * runs, adjacent frames in one run.  Sizes first: n_history counts uint32 entries (two per run). */
int cox_meshlayer_history_size(const cox_meshlayer_t* mesh, cox_obs_t* obs, uint64_t* n_triangles, uint64_t* n_history, double* kernel_ms);
/* ... in the layout cox_mesh_msg consumes: history_begin[n_triangles + 1], history[n_history], block_has_history[n_blocks] (1 iff some
 * triangle of the block has a run; blocks as in cox_meshlayer_download) */
int cox_meshlayer_history(const cox_meshlayer_t* mesh, cox_obs_t* obs, uint64_t* history_begin, uint32_t* history, uint8_t* block_has_history,
                          uint64_t cap_triangles, uint64_t cap_history, uint64_t cap_blocks);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_HISTORY_H_ */
