/* An ESDF that follows a TSDF layer on the GPU (coxgraph_amd/csrc/cox_esdf.hip): voxblox's
 * EsdfIntegrator::updateFromTsdfLayer, which the reference runs on a timer in every client's tsdf_server
 * (coxgraph/launch/firefly/tsdf_client.launch:32-36, update_esdf_every_n_sec 0.5) and keeps bound to the combined map
 * (coxgraph/include/coxgraph/client/map_server.h:92-94).  cox_esdf_update brings the handle's ESDF layer to exactly what
 * cox_esdf_from_tsdf(tsdf, cfg) would return at that moment -- the same words, bit for bit.  Every update reads every block once
 * (the classification compares TSDF and ESDF words, 96 KB per block); the relaxation sweeps visit only the blocks that the changes
 * since the previous update can reach.  Rule, proof sketch, kernels: DESIGN.md section 7l.
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_map.h: these entry points have no counterpart in the CPU checker
 * of the test suite.  Conventions are those of coxgraph_hip_map.h (COX_OK or a negative cox_status; no usable GPU ->
 * COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG).  One call at a time per handle. */
#ifndef COXGRAPH_HIP_ESDF_H_
#define COXGRAPH_HIP_ESDF_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_esdf cox_esdf_t;

typedef struct cox_esdf_update_stats {
  uint64_t n_blocks;         /* blocks of the TSDF (and now of the ESDF) */
  uint64_t n_new_blocks;     /* blocks the ESDF gained in this update */
  uint64_t n_dirty_blocks;   /* blocks in which the classification changed a word */
  uint64_t n_swept_blocks;   /* distinct blocks a raise or lower sweep loaded */
  uint64_t n_raise_sweeps;   /* launches that had an active block */
  uint64_t n_lower_sweeps;
  uint64_t n_reset_voxels;   /* voxels the raise put back to +-default_distance */
  uint64_t n_changed_voxels; /* voxels whose words the classification changed, plus voxels the lower sweeps moved (a voxel that
                                moves in several sweeps counts once per sweep) */
  uint32_t rebuilt;          /* 1: started from an empty ESDF (first update, cox_esdf_invalidate, the TSDF lost blocks or a pool
                                slot of it changed its block) */
  uint32_t pad;
  double ms;                 /* host wall time of the call */
} cox_esdf_update_stats;

/* An empty ESDF bound to `tsdf` (which must outlive the handle; it may be written, cleared and may grow between updates).
 * cfg NULL: cox_esdf_config_default.  COX_ERR_INVALID_ARG as cox_esdf_from_tsdf: a distance that is not > 0. */
int cox_esdf_create(cox_layer_t* tsdf, const cox_esdf_config* cfg, cox_esdf_t** out);
void cox_esdf_destroy(cox_esdf_t* h);
/* Orders behind every frame enqueued on the TSDF so far (integrators' submission threads are drained first); complete on return.
 * stats may be NULL.  After an error the next update rebuilds. */
int cox_esdf_update(cox_esdf_t* h, cox_esdf_update_stats* stats);
/* The ESDF layer (TSDF wire layout: distance, weight 1 = observed, colour word 1 = fixed), owned by the handle: valid, and current
 * as of the last update, until cox_esdf_destroy.  An ordinary layer for every reader (queries, rendering, view gain, collision
 * checks, registration, download, clone); do not write or destroy it. */
int cox_esdf_layer(cox_esdf_t* h, cox_layer_t** layer);
/* the next update starts from an empty ESDF (voxblox's updateFromTsdfLayerBatch) */
int cox_esdf_invalidate(cox_esdf_t* h);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_ESDF_H_ */
