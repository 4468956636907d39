/* Aligning two submaps without a prior: thousands of candidate 4-DoF poses of one (reference points, reading layer) pair scored
 * in one launch, and a deterministic coarse-to-fine search on top of the scores that ends inside the basin of the registration
 * cost (coxgraph_amd/csrc/cox_align.hip).  It produces the T_A_B that coxgraph::server::PoseGraphInterface's
 * addLoopClosureMeasurement / addForceRegistrationConstraint need when no visual loop closure (a MapFusion message) exists.
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_map.h: these entry points have no counterpart in the CPU checker
 * of the test suite.  COX_OK or a negative cox_status.  cox_align_config_default, cox_align_grid and cox_align_select are host
 * computations and need no GPU; every other entry point checks for a usable GPU first (COX_ERR_NO_DEVICE), then its arguments
 * (COX_ERR_INVALID_ARG).  Every sweep orders behind every frame enqueued on the reading layer before it.  One call at a time
 * per handle.  Poses are doubles x, y, z, yaw as cox_reg_* take them.  Rule and arithmetic: DESIGN.md section 7o. */
#ifndef COXGRAPH_HIP_ALIGN_H_
#define COXGRAPH_HIP_ALIGN_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_align cox_align_t;

#define COX_ALIGN_Q 1024u                  /* score quanta of a perfect inlier */
#define COX_ALIGN_MAX_CANDIDATES (1u << 20) /* per sweep */
#define COX_ALIGN_MAX_KEEP 64u
#define COX_ALIGN_MAX_LEVELS 16u           /* refinement levels of a search */
#define COX_ALIGN_MAX_GRID (1ull << 24)    /* poses of one grid */

typedef struct cox_align_config {
  float inlier_distance;         /* the tau a caller passes to cox_align_sweep by default: finite, > 0 */
  uint32_t pad;
  double no_correspondence_cost; /* as cox_reg_config */
} cox_align_config;

typedef struct cox_align_score { /* one per candidate, 24 bytes */
  uint64_t score;    /* sum over the points of (inlier ? max(0, Q - floor(e * Q / tau)) : 0), e = |d - interpolated distance| */
  uint32_t n_corr;   /* points with a correspondence */
  uint32_t n_inlier; /* ... whose e <= tau */
  double cost;       /* 0.5 * scale^2 * sum r^2: the cost cox_reg_normal_eq returns at that pose pair, in another summation order */
} cox_align_score;

typedef struct cox_align_search_config {
  double center[4];      /* of the level-0 grid */
  double half_extent[4]; /* >= 0 */
  double step[4];        /* level-0 grid step per axis, >= 0; 0 freezes the axis at every level */
  float inlier_distance; /* tau of level 0: finite, > 0 */
  float tau_min;         /* tau is halved per level and never goes below this: finite, > 0 */
  uint32_t levels;       /* refinement levels after level 0, <= COX_ALIGN_MAX_LEVELS */
  uint32_t keep;         /* K: candidates kept per level, 1 .. COX_ALIGN_MAX_KEEP */
  uint32_t min_corr;     /* a candidate with fewer correspondences is never kept */
  uint32_t pad;
} cox_align_search_config;

typedef struct cox_align_level { /* what one level of a search did (for tests and diagnosis) */
  uint64_t n_candidates;
  double step[4];
  float inlier_distance;
  uint32_t n_kept;
  uint32_t kept_index[COX_ALIGN_MAX_KEEP]; /* into the level's candidate list, in selection order */
  double kept_pose[4 * COX_ALIGN_MAX_KEEP];
  cox_align_score kept_score[COX_ALIGN_MAX_KEEP];
} cox_align_level;

/* inlier_distance 0.4 (twice voxgraph's default registration truncation at 0.2 m voxels), no_correspondence_cost 0 */
void cox_align_config_default(cox_align_config* cfg);

/* A scorer for `reference` against `reading` (a TSDF or an ESDF layer in wire layout on the same GPU; both must outlive the
 * handle; the layer may be written and may grow between calls).  cfg NULL: the defaults. */
int cox_align_create(const cox_regpoints_t* reference, const cox_layer_t* reading, const cox_align_config* cfg, cox_align_t** out);
void cox_align_destroy(cox_align_t* h);
/* The m points of a sweep: sample_idx[m] into the reference set, repeats allowed (a copy is kept on the GPU); NULL: all points in
 * order again.  COX_ERR_INVALID_ARG: an index >= the size of the set, m >= 2^31. */
int cox_align_set_samples(cox_align_t* h, const uint32_t* sample_idx, uint64_t m);

/* scores_out[c] for the candidate reference poses poses_ref[4 c .. 4 c + 3], c < n_candidates, against the one reading pose.
 * inlier_distance is the tau of this sweep.  A record depends on its own pose only: not on the batch, its place in it or the run.  A
 * non-finite pose gives the record of a pose at which no point has a correspondence.  n_candidates 0: COX_OK, nothing written.
 * COX_ERR_INVALID_ARG: a NULL pointer, inlier_distance <= 0 or not finite, n_candidates > COX_ALIGN_MAX_CANDIDATES. */
int cox_align_sweep(cox_align_t* h, const double pose_read[4], const double* poses_ref, uint64_t n_candidates, float inlier_distance,
                    cox_align_score* scores_out);

/* The grid around center: per axis k, m_k = step[k] > 0 ? llround(half_extent[k] / step[k]) : 0 and the values center[k] +
 * step[k] * j, j = -m_k .. m_k; poses in C order, x slowest and yaw fastest (yaw is not wrapped).  *n_poses is the count; poses_out
 * (4 doubles each, may be NULL to ask for the count) is filled when cap >= count, else COX_ERR_BUFFER_TOO_SMALL.
 * COX_ERR_INVALID_ARG: a NULL pointer, a non-finite or negative entry, more than COX_ALIGN_MAX_GRID poses.  No GPU needed. */
int cox_align_grid(const double center[4], const double half_extent[4], const double step[4], double* poses_out, uint64_t cap, uint64_t* n_poses);

/* The first `keep` of the candidates with n_corr >= min_corr, by score descending and then index ascending: idx_out[keep],
 * *n_out of them filled (fewer when fewer are eligible).  COX_ERR_INVALID_ARG: a NULL pointer (scores may be NULL when n is 0),
 * keep outside 1 .. COX_ALIGN_MAX_KEEP.  No GPU needed. */
int cox_align_select(const cox_align_score* scores, uint64_t n, uint32_t min_corr, uint32_t keep, uint32_t* idx_out, uint32_t* n_out);

/* Coarse to fine: level 0 sweeps cox_align_grid(center, half_extent, step) and keeps K; each further level halves the step (double)
 * and tau (float, not below tau_min) and sweeps the 3-per-unfrozen-axis grids around the kept poses, concatenated in selection
 * order (duplicates stay).  poses_out[4 K] and scores_out[K] get the last level's kept poses and records, best first; *n_found how
 * many (0: no candidate met min_corr at some level, which ends the search).  trace: NULL or levels + 1 entries.
 * COX_ERR_INVALID_ARG: a NULL pointer, what cox_align_grid and cox_align_select refuse, tau or tau_min non-finite or <= 0,
 * levels > COX_ALIGN_MAX_LEVELS. */
int cox_align_search(cox_align_t* h, const double pose_read[4], const cox_align_search_config* cfg, double* poses_out, cox_align_score* scores_out,
                     uint32_t* n_found, cox_align_level* trace);

/* device time of the sweeps' kernels since creation or the last reset (HIP events), and how many sweeps */
int cox_align_kernel_time(cox_align_t* h, double* ms, uint64_t* sweeps, int reset);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_ALIGN_H_ */
