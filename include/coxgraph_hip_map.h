/* Reading maps back on the GPU: voxblox's Interpolator / EsdfMap / TsdfMap point queries and createFreePointcloudFromEsdfLayer
 * behind a C ABI.
 *
 * What coxgraph's MapServer hands to its consumers (updatePastTsdf -> publishEsdf -> publishTraversable,
 * coxgraph/src/client/map_server.cpp:61-147) and what a planner asks of the published maps through voxblox's EsdfMap / TsdfMap
 * (getDistanceAtPosition, getDistanceAndGradientAtPosition, isObserved, getWeightAtPosition and their batch forms).  Kept
 * apart from coxgraph_hip.h on purpose: these entry points have no counterpart in the CPU checker of the test suite.
 *
 * Conventions are those of coxgraph_hip.h (COX_OK or a negative cox_status; no usable GPU -> COX_ERR_NO_DEVICE, checked
 * first; a NULL layer -> COX_ERR_INVALID_ARG).  Every call orders behind every frame enqueued on the layer before it.  One
 * kernel serves TSDF and ESDF layers: the ESDF is kept in TSDF wire layout with weight 1 for observed voxels, so "weight > 0"
 * is both Interpolator<TsdfVoxel>::isVoxelValid and EsdfVoxel::observed.  Rules and arithmetic: DESIGN.md section 7e. */
#ifndef COXGRAPH_HIP_MAP_H_
#define COXGRAPH_HIP_MAP_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which branch of voxblox's Interpolator answers a query */
typedef enum cox_query_mode {
  COX_QUERY_NEAREST = 0,     /* getDistance(pos, interpolate = false): Block::getVoxelByCoordinates */
  COX_QUERY_INTERPOLATE = 1, /* getDistance(pos, interpolate = true): trilinear over the 8 surrounding voxels */
  COX_QUERY_ADAPTIVE = 2     /* getAdaptiveDistanceAndGradient: trilinear when distance (and gradient) succeed, else nearest */
} cox_query_mode;

/* status bits per query */
#define COX_Q_VALUE 1u     /* distance / weight written */
#define COX_Q_TRILINEAR 2u /* ... from the trilinear branch (else nearest) */
#define COX_Q_GRADIENT 4u  /* gradient written (central differences, h = voxel size, same branch as the distance) */

/* n points (3 floats each, the layer's frame) -> distance[n], weight[n], gradient[3n], status[n].  Any output may be NULL; the
 * gradient is computed only when want_gradient != 0.  Host buffers; synchronous.  Where a status bit is clear the matching
 * outputs hold NaN.  Points that are NaN, infinite or outside the block-index range get status 0. */
int cox_layer_query(cox_layer_t* layer, const float* xyz, uint64_t n, int mode, int want_gradient, float* distance, float* weight, float* gradient,
                    uint8_t* status);
/* the same with device buffers on the layer's GPU, enqueued on hip_stream (NULL: the null stream) behind every frame enqueued
 * on the layer so far; returns without waiting.  Where a status bit is clear the matching outputs are left untouched.  The
 * layer may not be grown (cox_layer_reserve, an integrator's next frame) while the query is in flight. */
int cox_layer_query_dev(cox_layer_t* layer, const float* xyz_dev, uint64_t n, int mode, int want_gradient, float* distance_dev, float* weight_dev,
                        float* gradient_dev, uint8_t* status_dev, void* hip_stream);

/* createFreePointcloudFromEsdfLayer(esdf, min_distance, &cloud): every observed voxel (weight > 0) with distance >= min_distance,
 * as its centre (block_index * block_size + (v + 0.5) * voxel_size, in float) and intensity = distance.  Blocks in the order of
 * cox_layer_download ((z, y, x) of the block index), voxels in linear index order inside a block.  xyz gets 3 floats per point,
 * intensity 1; either may be NULL.  Both NULL: *n only.  COX_ERR_BUFFER_TOO_SMALL when cap < *n. */
int cox_layer_free_points(cox_layer_t* esdf, float min_distance, float* xyz, float* intensity, uint64_t cap, uint64_t* n);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_MAP_H_ */
