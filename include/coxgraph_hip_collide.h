/* Checking planner paths against a map on the GPU: batches of points, straight segments, stored trajectories and whole trees in,
 * one record per item out of one call (coxgraph_amd/csrc/cox_collide.hip).  The consumer is the exploration planner coxgraph's
 * multi-robot experiments feed the combined map into (coxgraph_sim/config/reconstruction_planner.yaml: system_constraints,
 * trajectory_generator RRTStar, generator_updater RecheckCollision); coxgraph_hip_gain.h is the other half of what it asks.
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_map.h: these entry points have no counterpart in the CPU checker
 * of the test suite.  Conventions are those of coxgraph_hip_map.h (COX_OK or a negative cox_status; no usable GPU ->
 * COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG).  Every call orders behind every frame enqueued on the layer
 * before it.  One call at a time per handle.  The layer is normally an ESDF in TSDF wire layout; a TSDF layer is accepted too
 * (the rules read distance and weight only).  Rules and arithmetic: DESIGN.md section 7k. */
#ifndef COXGRAPH_HIP_COLLIDE_H_
#define COXGRAPH_HIP_COLLIDE_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_collide cox_collide_t;

typedef struct cox_collide_config {
  float collision_radius;       /* traversable: observed, trilinear distance produced and distance > collision_radius */
  int32_t collision_optimistic; /* what an unobserved sample outside the clearing sphere is */
  float clearing_radius;        /* > 0: unobserved samples closer than this to clearing_centre are traversable */
  float clearing_centre[3];     /* the robot's position (cox_collide_set_clearing_centre) */
  float sample_spacing;         /* metres between samples of a segment; 0: the layer's voxel size */
  uint32_t max_samples;         /* a segment of more sampling intervals than this is COX_SEG_TOO_LONG; 0: 4096 */
  float max_extension_range;    /* > 0: longer segments are shortened to this length first */
  int32_t crop;                 /* produce goals: the far end of a feasible segment, a cropped one of a blocked segment */
  float crop_margin;            /* metres taken off the free length of a blocked segment */
  float crop_min_length;        /* a goal needs a free length above this (and a segment at least this long) */
} cox_collide_config;

/* state of a sample (cox_collide_points) */
#define COX_C_TRAVERSABLE 1u
#define COX_C_OBSERVED 2u  /* the voxel containing the sample has weight > 0 (EsdfMap::isObserved) */
#define COX_C_DISTANCE 4u  /* the trilinear distance was produced */
#define COX_C_CLEARED 8u   /* unobserved, inside the clearing sphere */
#define COX_C_INVALID 16u  /* NaN, infinite or outside the block-index range */

/* flags of a record */
#define COX_SEG_FEASIBLE 1u /* no sample is blocked */
#define COX_SEG_GOAL 2u     /* goal[] holds a goal */
#define COX_SEG_CLAMPED 4u  /* shortened to max_extension_range */
#define COX_SEG_TOO_LONG 8u /* more than max_samples intervals: not feasible, nothing sampled, n_samples saturates at 2^32 - 1 */
#define COX_SEG_INVALID 16u /* an end point (or the difference of the two) is not finite: not feasible, n_samples = 0 */

/* keep[] of a tree */
#define COX_TREE_KEEP 1u
#define COX_TREE_INVALID 2u /* the walk from the node towards a root meets a parent index out of range or a cycle (keep is clear) */

typedef struct cox_collide_record { /* one per segment or trajectory, 32 bytes */
  uint32_t n_samples;     /* segment: sampling intervals n (samples 0 .. n); trajectory: its points */
  uint32_t first_blocked; /* smallest index of a sample that is not traversable; none: n + 1 (segment), the length (trajectory) */
  uint32_t flags;         /* COX_SEG_* */
  float free_length;      /* segment with crop on: its length when feasible, else the cropped free length; NaN otherwise */
  float goal[3];          /* NaN without COX_SEG_GOAL */
  uint32_t pad;
} cox_collide_record;

typedef struct cox_collide_stats {
  uint64_t n_samples_evaluated; /* samples whose state was computed */
  uint64_t n_samples_skipped;   /* samples of blocked items the early exit never looked at */
  uint64_t n_launches;          /* kernels enqueued */
  double kernel_ms;             /* device time of the calls' kernels while profiling was on (HIP events) */
} cox_collide_stats_t;

/* From coxgraph_sim/config/reconstruction_planner.yaml: collision_radius 2.0, collision_optimistic false, clearing_radius 0,
 * crop_segments true with crop_margin 0.3 and crop_min_length 0.5, max_extension_range 1.5, sample_spacing = v_max /
 * sampling_rate = 1 / 20 = 0.05.  This engine's: clearing_centre 0, max_samples 4096. */
void cox_collide_config_default(cox_collide_config* cfg);

/* A checker against `layer` (which must outlive it; the layer may be written and may grow between calls).  cfg NULL: the defaults.
 * COX_ERR_INVALID_ARG: a NULL layer or out; a non-finite field; clearing_radius, sample_spacing, crop_margin or crop_min_length
 * < 0; max_samples > 2^24. */
int cox_collide_create(cox_layer_t* layer, const cox_collide_config* cfg, cox_collide_t** out);
void cox_collide_destroy(cox_collide_t* h);
/* the robot moves between calls; applies to calls made after it */
int cox_collide_set_clearing_centre(cox_collide_t* h, const float centre[3]);
/* lanes that share one segment or trajectory: 64 (a wave) or 32 (two items per wave).  Records do not depend on it. */
int cox_collide_set_group_size(cox_collide_t* h, int lanes);
int cox_collide_set_profiling(cox_collide_t* h, int on);
/* counters since creation or the last reset, of the calls that have finished on the device (waits for a profiled call) */
int cox_collide_stats(cox_collide_t* h, cox_collide_stats_t* out, int reset);

/* n points (3 floats each, the layer's frame) -> state[n] of COX_C_*, distance[n] (either may be NULL).  Host buffers;
 * synchronous; distance is NaN without COX_C_DISTANCE. */
int cox_collide_points(cox_collide_t* h, const float* xyz, uint64_t n, uint8_t* state, float* distance);
/* the same with device buffers on the layer's GPU, enqueued on hip_stream (NULL: the null stream) behind every frame enqueued on
 * the layer so far; returns without waiting.  distance is left untouched without COX_C_DISTANCE.  The layer may not be grown
 * (cox_layer_reserve, an integrator's next frame) while a _dev call is in flight. */
int cox_collide_points_dev(cox_collide_t* h, const float* xyz_dev, uint64_t n, uint8_t* state_dev, float* distance_dev, void* hip_stream);

/* n straight segments a[3n] -> b[3n] -> out[n].  A record does not depend on the batch it is in. */
int cox_collide_segments(cox_collide_t* h, const float* a, const float* b, uint64_t n, cox_collide_record* out);
int cox_collide_segments_dev(cox_collide_t* h, const float* a_dev, const float* b_dev, uint64_t n, cox_collide_record* out_dev, void* hip_stream);

/* n_traj stored trajectories in CSR form: trajectory t is the points offsets[t] .. offsets[t + 1] - 1 of xyz (n_points points,
 * 3 floats each); every given point is judged, nothing is resampled.  An empty trajectory is feasible.
 * Host form: COX_ERR_INVALID_ARG when offsets decrease, exceed n_points or a trajectory has 2^31 points or more.  Device
 * form: offsets are clamped into [0, n_points] (a decreasing pair is an empty trajectory) and a trajectory to its first 2^31 - 1 points. */
int cox_collide_trajectories(cox_collide_t* h, const uint64_t* offsets, uint64_t n_traj, const float* xyz, uint64_t n_points, cox_collide_record* out);
int cox_collide_trajectories_dev(cox_collide_t* h, const uint64_t* offsets_dev, uint64_t n_traj, const float* xyz_dev, uint64_t n_points,
                                 cox_collide_record* out_dev, void* hip_stream);

/* RecheckCollision's rule on a tree: keep[i] = (feasible[i * feasible_stride] & 1) && keep[parent[i]], parent[i] = -1 for a root,
 * nodes in any order; keep[i] is COX_TREE_KEEP, 0 or COX_TREE_INVALID.  feasible_stride in bytes (1: a byte array; 32 with
 * feasible pointing at the flags of a record array).  n <= 2^30. */
int cox_collide_prune_dev(cox_collide_t* h, const int32_t* parent_dev, const uint8_t* feasible_dev, uint64_t feasible_stride, uint64_t n,
                          uint8_t* keep_dev, void* hip_stream);

/* trajectories + prune in one call: node i of the tree owns trajectory i.  out may be NULL in the host form. */
int cox_collide_tree(cox_collide_t* h, const uint64_t* offsets, const int32_t* parent, uint64_t n_nodes, const float* xyz, uint64_t n_points,
                     cox_collide_record* out, uint8_t* keep);
int cox_collide_tree_dev(cox_collide_t* h, const uint64_t* offsets_dev, const int32_t* parent_dev, uint64_t n_nodes, const float* xyz_dev,
                         uint64_t n_points, cox_collide_record* out_dev, uint8_t* keep_dev, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_COLLIDE_H_ */
