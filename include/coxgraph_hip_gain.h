/* Scoring candidate views for exploration on the GPU: a batch of sensor poses in, one gain record per pose out -- the voxels a
 * ray-casting sensor model would see from each pose, each counted once per view, and what seeing them is worth
 * (coxgraph_amd/csrc/cox_viewgain.hip).  The consumer is the exploration planner coxgraph's multi-robot experiments feed the
 * combined map into (coxgraph_sim/launch/utils/reconstruction_planner.launch, coxgraph_sim/config/reconstruction_planner.yaml).
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_render.h: these entry points have no counterpart in the CPU checker
 * of the test suite.  Conventions are those of coxgraph_hip_map.h (COX_OK or a negative cox_status; no usable GPU ->
 * COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG).  Every call orders behind every frame enqueued on the layer
 * before it.  One call at a time per handle.  Rules and arithmetic: DESIGN.md section 7j. */
#ifndef COXGRAPH_HIP_GAIN_H_
#define COXGRAPH_HIP_GAIN_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_viewgain cox_viewgain_t;

typedef struct cox_viewgain_config {
  int32_t w, h;                 /* ray grid (already down-sampled by the caller) */
  float K[4];                   /* fx, fy, cx, cy of that grid */
  float min_range, ray_length;  /* samples with min_range <= d < ray_length */
  float ray_step;               /* 0: the layer's voxel size */
  float min_weight;             /* observed: weight > min_weight */
  float surface_distance;       /* occupied: observed and distance <= surface_distance */
  float frontier_voxel_weight;  /* worth of an unknown voxel next to the known map; <= 0: no voxel is classed a frontier */
  float new_voxel_weight;       /* worth of every other unknown voxel */
  float min_impact_factor;      /* an occupied voxel counts when its impact is above this */
  float ray_angle_x, ray_angle_y; /* angle between neighbouring rays of the full-resolution sensor (rad) */
  int32_t accurate_frontiers;   /* 0: 6 face neighbours, 1: all 26 */
  int32_t surface_frontiers;    /* 1: a neighbour must be occupied, 0: observed is enough */
  int32_t use_box;              /* target bounding volume on voxel centres: centres outside are not in the visible set */
  float box_min[3], box_max[3];
  uint64_t workspace_bytes;     /* cap of the de-duplication workspace; 0: 256 MiB */
} cox_viewgain_config;

typedef struct cox_view_gain { /* one per view */
  double gain;                 /* surface_gain + frontier_voxel_weight * n_frontier + new_voxel_weight * (n_unknown - n_frontier) */
  double surface_gain;         /* sum of the counted occupied voxels' impacts = surface_gain_q32 / 2^32 */
  uint64_t surface_gain_q32;   /* sum of (uint64_t)((double)impact * 2^32) */
  uint32_t n_visible;          /* distinct voxels the rays sampled (inside the box, when one is used) */
  uint32_t n_free, n_occupied; /* of those: observed and not occupied; occupied */
  uint32_t n_surface_counted;  /* occupied voxels whose impact is above min_impact_factor */
  uint32_t n_unknown;          /* unobserved voxels, frontiers included */
  uint32_t n_frontier;
} cox_view_gain;

typedef struct cox_viewgain_stats {
  uint64_t n_samples; /* voxel look-ups of all rays of all views (samples in [min_range, ray_length) that were in index range) */
  uint64_t n_chunks;  /* launches of the march kernel the batch was cut into */
  double kernel_ms;   /* device time from the first kernel of the call to the last */
} cox_viewgain_stats;

/* class of a visible voxel (cox_viewgain_visible) */
#define COX_VG_FREE 0u
#define COX_VG_OCCUPIED 1u
#define COX_VG_UNKNOWN 2u
#define COX_VG_FRONTIER 3u

/* From coxgraph_sim/config/reconstruction_planner.yaml (lines 71-91): frontier_voxel_weight 1, new_voxel_weight 0,
 * min_impact_factor 0.01, ray_angle_x 0.002454, ray_angle_y 0.002681, accurate_frontiers 1, surface_frontiers 1, ray_length 5,
 * and the grid 35 x 96 with K = {64, 64, 17, 48}: the yaml's 172 x 480 camera (focal length 320) under its down-sampling factor
 * of 5, rounded up, principal point at the centre.
 * This engine's choice: min_range 0, ray_step 0 (the layer's voxel size), min_weight 0 (the map queries' rule for "observed"),
 * surface_distance 0, use_box 0, workspace_bytes 0 (256 MiB). */
void cox_viewgain_config_default(cox_viewgain_config* cfg);

/* An evaluator against `layer` (which must outlive it; the layer may be written and may grow between calls).  It owns the ray
 * table of the grid and the de-duplication workspace.  cfg NULL: the defaults.
 * COX_ERR_INVALID_ARG: a NULL layer or out; w or h <= 0 (or w * h > 0x7FFFFFFF); fx or fy == 0; a non-finite K, range, step,
 * weight, factor, angle, distance or box; ray_length <= min_range; min_range < 0; ray_step < 0; ray_angle_x * ray_angle_y <= 0;
 * a box with min > max; more than 2^20 steps in a ray (ray_length / step). */
int cox_viewgain_create(cox_layer_t* layer, const cox_viewgain_config* cfg, cox_viewgain_t** out);
void cox_viewgain_destroy(cox_viewgain_t* h);

/* Bytes of workspace one view takes: a bitmap over the cube of voxels within ray_length (plus slack) of the view's origin at the
 * layer's voxel size.  A batch is cut into chunks of workspace_bytes / this many views. */
uint64_t cox_viewgain_view_bytes(const cox_viewgain_t* h);

/* n_views poses T_G_C = {qw, qx, qy, qz, tx, ty, tz} (unit quaternions) -> out[n_views].  Host buffers; synchronous.  stats may
 * be NULL.  A view's record does not depend on the batch it is in or on how the batch is cut into chunks.
 * n_views = 0: COX_OK, nothing written.  COX_ERR_INVALID_ARG: a NULL handle, poses or out; a non-finite pose.
 * COX_ERR_OUT_OF_MEMORY: one view's workspace need exceeds workspace_bytes (also when a quaternion far from unit length
 * stretches a view's rays beyond its share of the workspace). */
int cox_viewgain_evaluate(cox_viewgain_t* h, const float* T_G_C, uint64_t n_views, cox_view_gain* out, cox_viewgain_stats* stats);
/* the same with device buffers on the layer's GPU (out_dev 8-byte aligned), enqueued on hip_stream (NULL: the null stream) behind
 * every frame enqueued on the layer so far; returns without waiting.  Poses cannot be checked here: a view whose origin is not
 * finite or outside the index range is empty, and a view whose rays a non-unit quaternion stretches beyond its share of the
 * workspace gets gain = surface_gain = NaN and zero counts.  The layer may not be grown (cox_layer_reserve, an integrator's next
 * frame) while the call is in flight. */
int cox_viewgain_evaluate_dev(cox_viewgain_t* h, const float* poses_dev, uint64_t n_views, cox_view_gain* out_dev, void* hip_stream);

/* The visible set of one view, for inspection and visualisation: voxel_xyz[3 * i ..] the global voxel index, cls[i] the class
 * above, value[i] what the voxel adds to the gain (an occupied voxel's impact, 0 when it does not count), in ascending (z, y, x)
 * order of the global index.  *n the size of the set.  cap = 0 with NULL buffers queries *n; COX_ERR_BUFFER_TOO_SMALL when
 * cap < *n.  Any of the three buffers may be NULL. */
int cox_viewgain_visible(cox_viewgain_t* h, const float T_G_C[7], uint64_t cap, int32_t* voxel_xyz, uint8_t* cls, float* value, uint64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_GAIN_H_ */
