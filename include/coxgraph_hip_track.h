/* Scan-to-map registration on the GPU: refine a sensor pose T_G_C against a TSDF layer by Gauss-Newton on the point-to-implicit-
 * surface cost sum_p w_p d(T p)^2, d the layer's trilinear distance (coxgraph_amd/csrc/cox_track.hip).
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_map.h: these entry points have no counterpart in the CPU checker
 * of the test suite.  Conventions are those of coxgraph_hip_map.h (COX_OK or a negative cox_status; no usable GPU ->
 * COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG).  Every call orders behind every frame enqueued on the layer before
 * it and returns when its result is on the host.  Device inputs (xyz_dev, depth_dev) must be complete when the call is made: the
 * work runs on the tracker's own stream.  The rule, iteration by iteration, and its arithmetic: DESIGN.md section 7i.
 *
 * The linear solve of an iteration, (H + damping diag(H)) delta = -b with n = dof unknowns, is a dense lower Cholesky in float64
 * in exactly this order (no fused multiply-adds):
 *   A[i][j] = H[i][j] (i != j), A[i][i] = H[i][i] + damping * H[i][i]
 *   for j = 0 .. n-1:
 *     s = A[j][j]; for k = 0 .. j-1: s = s - L[j][k] * L[j][k]
 *     if not (s > 0) or s is not finite: COX_TRACK_DEGENERATE
 *     L[j][j] = sqrt(s)
 *     for i = j+1 .. n-1: s = A[i][j]; for k = 0 .. j-1: s = s - L[i][k] * L[j][k]; L[i][j] = s / L[j][j]
 *   for i = 0 .. n-1:  s = -b[i]; for k = 0 .. i-1: s = s - L[i][k] * y[k];       y[i] = s / L[i][i]
 *   for i = n-1 .. 0:  s = y[i];  for k = i+1 .. n-1: s = s - L[k][i] * delta[k]; delta[i] = s / L[i][i] */
#ifndef COXGRAPH_HIP_TRACK_H_
#define COXGRAPH_HIP_TRACK_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_track cox_track_t;

typedef struct cox_track_config {
  int32_t dof;                  /* 4: x, y, z, yaw (about the world z axis);  6: x, y, z and a rotation vector */
  uint32_t max_iterations;      /* Gauss-Newton iterations of a refine call at the most */
  uint32_t stride;              /* every stride-th point (pixel) of the scan is considered; >= 1 */
  uint32_t min_points;          /* fewer used points than this: COX_TRACK_LOST */
  float max_abs_distance;       /* > 0: points with |d| above it are not used */
  float reserved;               /* (0) */
  double huber_delta;           /* > 0: weight huber_delta / |d| where |d| > huber_delta */
  double damping;               /* Levenberg damping of the diagonal, relative: H + damping diag(H) */
  double translation_tolerance; /* converged when the step is no longer than this (m) ... */
  double rotation_tolerance;    /* ... and turns by no more than this (rad) */
  double min_inlier_ratio;      /* fewer used points than this share of the considered ones: COX_TRACK_LOST */
} cox_track_config;

typedef enum cox_track_status {
  COX_TRACK_CONVERGED = 0,      /* the last step was within both tolerances (and was taken) */
  COX_TRACK_MAX_ITERATIONS = 1, /* max_iterations steps taken, the last one above a tolerance */
  COX_TRACK_LOST = 2,           /* too few points of the scan met the map: the pose at that iteration's start stands */
  COX_TRACK_DEGENERATE = 3      /* a pivot of the Cholesky factorisation was <= 0 or not finite: the pose stands */
} cox_track_status;

typedef struct cox_track_result {
  int32_t status;      /* cox_track_status */
  uint32_t iterations; /* evaluations of the normal equations (the one that stopped the loop included) */
  uint64_t first_n_used, first_n_considered; /* of the first iteration */
  uint64_t last_n_used, last_n_considered;   /* of the last one */
  double first_cost, last_cost;              /* sum w d^2 at the pose the first / the last iteration started from */
  double last_step_translation;              /* |delta_t| (m) and |omega| (rad) of the last step taken; 0 when none was */
  double last_step_rotation;
  double T_G_C[7];  /* the refined pose in float64: qw, qx, qy, qz (unit), tx, ty, tz */
  double kernel_ms; /* device time from the first launch of the call to the last */
} cox_track_result;

/* status bits per point of cox_track_evaluate_dev */
#define COX_TRACK_CONSIDERED 1u /* index a multiple of stride, coordinates finite: p_G written */
#define COX_TRACK_USED 2u       /* ... and the point met the map: d and g written */

/* Candidates (points whose index is a multiple of stride) one pass of the grid covers: 256 workgroups of 256 lanes.  A scan with more
 * of them is walked in several passes by the same workgroups. */
#define COX_TRACK_GRID_PASS 65536u

/* dof 4, max_iterations 15, stride 1, max_abs_distance 0, huber_delta 0, damping 1e-6, translation_tolerance 1e-4,
 * rotation_tolerance 1e-4, min_points 32, min_inlier_ratio 0.3 */
void cox_track_config_default(cox_track_config* cfg);

/* A tracker against `layer` (which must outlive it; the layer may grow and be written between calls).  cfg NULL: the defaults.
 * COX_ERR_INVALID_ARG: dof not 4 or 6, stride 0, a negative or NaN tolerance, damping, huber_delta, max_abs_distance or
 * min_inlier_ratio. */
int cox_track_create(const cox_layer_t* layer, const cox_track_config* cfg, cox_track_t** out);
void cox_track_destroy(cox_track_t* track);

/* The per-point values of one iteration at pose T_G_C = {qw, qx, qy, qz, tx, ty, tz}: pG_d_g[7 * i ..] = p_G (3), d, g (3) of scan
 * point i, status[i] the bits above.  p_G is NaN where COX_TRACK_CONSIDERED is clear, d and g where COX_TRACK_USED is.  Device
 * buffers; either output may be NULL. */
int cox_track_evaluate_dev(cox_track_t* track, const float T_G_C[7], const float* xyz_dev, uint64_t n, float* pG_d_g_dev, uint8_t* status_dev);

/* One evaluation of the normal equations at T_G_C, no update: H row-major with row stride 6 (the leading dof x dof part; the rest 0),
 * b likewise, cost = sum w d^2, counts = {n_used, n_considered}.  Any output may be NULL. */
int cox_track_normal_eq_dev(cox_track_t* track, const float T_G_C[7], const float* xyz_dev, uint64_t n, double H[36], double b[6], double* cost,
                            uint64_t counts[2]);

/* Refine T_prior against the layer with the n sensor-frame points xyz (3 floats each).  T_refined (may be NULL) is result->T_G_C
 * rounded to float; result may be NULL.  The prior is used as given (its quaternion must have a finite, non-zero norm).  n = 0 and
 * scans that miss the map return COX_OK with status COX_TRACK_LOST and the prior as the pose. */
int cox_track_refine_dev(cox_track_t* track, const float T_prior[7], const float* xyz_dev, uint64_t n, float T_refined[7], cox_track_result* result);
/* the same with host points */
int cox_track_refine(cox_track_t* track, const float T_prior[7], const float* xyz, uint64_t n, float T_refined[7], cox_track_result* result);
/* the same with a depth image on the device in the layout of cox_integrate_depth_dev and of cox_layer_render_dev's depth output
 * (w * h floats, row-major, z-depth in metres), K = {fx, fy, cx, cy}.  Pixel i = v * w + u is the scan point
 * d * ((u - cx) / fx, (v - cy) / fy, 1) in float; pixels that are not finite or <= 0 are not considered; stride runs over i. */
int cox_track_refine_depth_dev(cox_track_t* track, const float T_prior[7], const float* depth_dev, int w, int h, const float K[4], float T_refined[7],
                               cox_track_result* result);
/* one evaluation of the normal equations on a depth image (cox_track_normal_eq_dev's outputs) */
int cox_track_normal_eq_depth_dev(cox_track_t* track, const float T_G_C[7], const float* depth_dev, int w, int h, const float K[4], double H[36],
                                  double b[6], double* cost, uint64_t counts[2]);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_TRACK_H_ */
