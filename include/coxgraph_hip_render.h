/* Rendering a layer from a pose on the GPU: depth, normal and colour images of the zero crossing of a TSDF (or of an ESDF kept
 * in TSDF wire layout), one ray per pixel, marched through the layer (coxgraph_amd/csrc/cox_render.hip).
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_map.h: these entry points have no counterpart in the CPU checker
 * of the test suite.  Conventions are those of coxgraph_hip_map.h (COX_OK or a negative cox_status; no usable GPU ->
 * COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG).  Every call orders behind every frame enqueued on the layer
 * before it.  The rendered depth image has the layout cox_integrate_depth_dev consumes: w * h floats, row-major, z-depth in
 * metres, NaN where the ray found no surface.  Rules and arithmetic: DESIGN.md section 7g. */
#ifndef COXGRAPH_HIP_RENDER_H_
#define COXGRAPH_HIP_RENDER_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_render_config {
  float min_depth;       /* z-depth the march starts at (m) */
  float max_depth;       /* ... and ends at */
  float step_scale;      /* a sample at distance d is followed by a step of |d| * step_scale ... */
  float min_step_voxels; /* ... but of at least this many voxels */
  uint32_t max_samples;  /* samples (block probes included) a ray may take; a ray that runs out gets COX_R_BUDGET */
} cox_render_config;

typedef struct cox_render_stats {
  uint64_t n_hits;        /* pixels with COX_R_HIT */
  uint64_t n_samples;     /* samples taken by all rays, block probes included */
  uint64_t n_block_skips; /* of those, probes that met an unallocated block and jumped to its far side */
  uint64_t n_budget;      /* pixels with COX_R_BUDGET */
  double kernel_ms;       /* device time of the kernel */
} cox_render_stats;

/* status bits per pixel */
#define COX_R_HIT 1u    /* a positive-to-non-positive crossing was found: depth written */
#define COX_R_NORMAL 2u /* normal written (all six gradient samples succeeded) */
#define COX_R_COLOR 4u  /* the voxel containing the hit point is observed: its colour written */
#define COX_R_BUDGET 8u /* max_samples reached before a hit, a miss or max_depth */

/* step_scale 0.75, min_step_voxels 0.25, min_depth 0.1, max_depth 10, max_samples 4096 */
void cox_render_config_default(cox_render_config* cfg);

/* One ray per pixel (u, v) of a w x h pinhole image with K = {fx, fy, cx, cy} at pose T_G_C = {qw, qx, qy, qz, tx, ty, tz}.
 * depth[w * h] the z-depth of the hit, normal[3 * w * h] the unit gradient of the distance there (world frame, pointing into
 * free space), rgba[4 * w * h] the colour {r, g, b, a} of the voxel containing the hit point, status[w * h] the bits above.
 * Any output may be NULL.  Where a bit is clear the matching output holds NaN (depth, normal) or 0 (rgba).  cfg NULL: the
 * defaults.  Host buffers; synchronous.  stats may be NULL.
 * COX_ERR_INVALID_ARG: a NULL layer, pose or K; w or h <= 0 or w * h > 0x7FFFFFFF; a non-finite pose or K; fx or fy == 0;
 * max_depth <= min_depth, min_depth < 0 or step_scale <= 0 (NaN fields included). */
int cox_layer_render(cox_layer_t* layer, const float T_G_C[7], int w, int h, const float K[4], const cox_render_config* cfg, float* depth,
                     float* normal, uint8_t* rgba, uint8_t* status, cox_render_stats* stats);
/* the same with device buffers on the layer's GPU, enqueued on hip_stream (NULL: the null stream) behind every frame enqueued
 * on the layer so far; returns without waiting.  Every pixel of every buffer given is written, misses included.  rgba_dev must be
 * 4-byte aligned (COX_ERR_INVALID_ARG otherwise).  The layer may not be grown (cox_layer_reserve, an integrator's next frame) while the render is in flight. */
int cox_layer_render_dev(cox_layer_t* layer, const float T_G_C[7], int w, int h, const float K[4], const cox_render_config* cfg, float* depth_dev,
                         float* normal_dev, uint8_t* rgba_dev, uint8_t* status_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_RENDER_H_ */
