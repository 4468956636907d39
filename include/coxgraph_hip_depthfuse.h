/* Fusing depth and colour images of a pinhole camera into a TSDF layer on the GPU (coxgraph_amd/csrc/cox_depthfuse.hip): the
 * voxel-projective integrator.  Every voxel of the blocks the camera's frustum can reach is projected into the depth image, reads
 * its depth there and is updated with the ray casters' voxel arithmetic, so a layer written by this integrator and by `merged`
 * means the same thing.  The image layout is the renderer's and the tracker's (w * h floats, row-major, z-depth in metres, NaN where
 * there is nothing, K = {fx, fy, cx, cy}, pixel centres at integer coordinates): render -> track -> fuse stays on the device.
 * The rule of one frame (steps 1-9), what a frame keeps of the layer's invariants, kernels and measurements: DESIGN.md section 7m.
 * The layer after a frame is a function of the layer before it and the inputs, bit for bit.
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_esdf.h: these entry points have no counterpart in the CPU checker
 * of the test suite.  Conventions are those of coxgraph_hip_map.h (COX_OK or a negative cox_status; no usable GPU ->
 * COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG).  One call at a time per handle. */
#ifndef COXGRAPH_HIP_DEPTHFUSE_H_
#define COXGRAPH_HIP_DEPTHFUSE_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_depthfuse cox_depthfuse_t;

/* A frame visits the blocks of an axis-aligned box around the frustum ("candidates").  A frame whose box holds more blocks than
 * this is refused with COX_ERR_INVALID_ARG before anything is enqueued: every grid and scratch buffer of a frame is sized by the
 * candidate count.  2^21 blocks: a 1280 x 720 image with max_depth_m = 10 at 1 cm voxels needs at most 104^3 = 1.12 million in any
 * orientation (a bound: the frustum's diameter, the far plane's diagonal, is 16.02 m, which spans at most 102 blocks of 0.16 m,
 * plus two for the widening; measured: the largest box of the 40 orientations tests/test_depthfuse_abi_cpu.py tries has 0.69
 * million), and the count is one chunk of the scan of block sums. */
#define COX_DEPTHFUSE_MAX_CANDIDATES (1u << 21)

typedef struct cox_depthfuse_config {
  float truncation_distance;
  float max_weight;
  float min_depth_m;             /* limits on the VOXEL's z in the camera frame, not on the surface */
  float max_depth_m;
  int32_t voxel_carving_enabled;
  int32_t use_const_weight;      /* 1: weight 1 per observation; 0: 1 / D^2 */
  int32_t use_weight_dropoff;
  int32_t interpolation_scheme;  /* 0 nearest, 1 minimum of the cell, 2 bilinear, 3 adaptive (bilinear, the near side across a gap) */
  float adaptive_gap_m;
  uint32_t reserved;             /* 0 */
} cox_depthfuse_config;

typedef struct cox_depthfuse_stats {
  uint64_t n_valid_pixels;       /* finite and > 0 */
  uint64_t n_candidate_blocks;   /* blocks of the box around the frustum */
  uint64_t n_touched_blocks;     /* blocks in which a voxel was written */
  uint64_t n_new_blocks;         /* ... that were allocated by this frame */
  uint64_t n_updated_voxels;
  uint64_t n_coloured_voxels;
  double kernel_ms;              /* HIP-event time of the frame's two halves (selection and scans; update) */
} cox_depthfuse_stats;

/* truncation 0.1 m, max_weight 1e4, depth 0.1 .. 5 m, carving, 1 / D^2 weights with drop-off, scheme 3, gap 0.5 m */
void cox_depthfuse_config_default(cox_depthfuse_config* cfg);

/* An integrator bound to `layer` (which must outlive the handle); a writer of the layer like any cox_integrator_t, in call order
 * with them.  cfg NULL: the defaults.  COX_ERR_INVALID_ARG: a truncation that is not > 0, or not > voxel_size with drop-off on; a
 * max_weight that is not > 0; depth limits or a gap that are not finite and > 0; a scheme outside 0..3. */
int cox_depthfuse_create(cox_layer_t* layer, const cox_depthfuse_config* cfg, cox_depthfuse_t** out);
/* waits for the handle's stream first */
void cox_depthfuse_destroy(cox_depthfuse_t* h);

/* One frame from host arrays: T_G_C = {qw, qx, qy, qz, x, y, z} (unit quaternion), depth[w * height], rgba[4 * w * height] or
 * NULL (the colour words are then left alone), K = {fx, fy, cx, cy}.  Returned by the call itself, with the layer unchanged and
 * nothing enqueued: COX_ERR_INVALID_ARG (a size < 1 or > 2^15, fx or fy not finite and > 0, cx, cy or T not finite, more than
 * COX_DEPTHFUSE_MAX_CANDIDATES candidate blocks), COX_ERR_INDEX_RANGE (the box leaves +-2^20 block indices),
 * COX_ERR_POOL_EXHAUSTED (the frame's new blocks do not fit and auto-grow is off, or growing failed).  The call waits once, for
 * the selection (it needs the number of blocks to allocate); the update is enqueued and not waited for. */
int cox_depthfuse_integrate(cox_depthfuse_t* h, const float T_G_C[7], const float* depth, const uint8_t* rgba_or_null, int w, int height,
                            const float K[4]);
/* The same with device arrays on the layer's GPU.  The frame orders behind what producer_stream (a hipStream_t; NULL: the null
 * stream) holds at the call, and producer_stream then waits until the frame has read the images, so the buffers may be reused or
 * freed in stream order on it. */
int cox_depthfuse_integrate_dev(cox_depthfuse_t* h, const float T_G_C[7], const float* depth_dev, const uint8_t* rgba_dev_or_null, int w, int height,
                                const float K[4], void* producer_stream);
/* waits for every frame of this handle; returns the layer's sticky device error, if any */
int cox_depthfuse_sync(cox_depthfuse_t* h);
/* of the last frame (waits for it); all zero after a frame that was refused */
int cox_depthfuse_last_stats(cox_depthfuse_t* h, cox_depthfuse_stats* out);
/* The layer's block indices in POOL order (new blocks of a frame go to the end of the pool in ascending (z, y, x)): waits for
 * the layer's writers; *n_blocks is the count, COX_ERR_BUFFER_TOO_SMALL when cap_blocks is less (block_idx_xyz may then be NULL). */
int cox_depthfuse_pool_order(cox_depthfuse_t* h, int32_t* block_idx_xyz, uint64_t cap_blocks, uint64_t* n_blocks);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_DEPTHFUSE_H_ */
