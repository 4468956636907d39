/* Filters on the disparity image of dense stereo (coxgraph_hip_stereo.h, coxgraph_amd/csrc/cox_stereo.hip and
 * cox_stereo_filter.hpp): a 3 x 3 median over the valid values (step 7a) and a speckle filter (step 7b), between the left-right
 * check and the depth.  What the matcher leaves after uniqueness and the left-right check still holds small islands of confidently
 * wrong disparities; fused into a TSDF such a speckle is a floater in free space, and an obstacle to everything that plans on the
 * map.  The rule is integer arithmetic and is stated in DESIGN.md section 7n; tests/stereo_filter_ref.py restates it in numpy and
 * the kernels owe it every bit.
 *
 *   7a  a valid pixel that is not on the image border takes rank (n - 1) / 2 of the n valid values of its 3 x 3 window, sorted
 *       ascending (the median, the lower one for even n); every other pixel keeps its value; nothing is filled
 *   7b  4-neighbours link when both are valid and differ by at most speckle_range16 (in 1/16 px); every pixel of a connected
 *       component of at most speckle_window pixels becomes invalid; a component's label is its least index y * w + x
 *
 * A handle has both filters off until told otherwise; with both off a frame is the frame of coxgraph_hip_stereo.h, launch for
 * launch and bit for bit, and no buffer of this header exists.  The buffers (about 12 bytes per pixel) are allocated when a filter
 * is first switched on; a filtered frame allocates nothing and waits for the host nowhere.  Kept apart from coxgraph_hip_stereo.h,
 * whose symbol list and layouts are pinned.  Conventions as there: COX_OK or a negative cox_status, no usable GPU ->
 * COX_ERR_NO_DEVICE checked first, then COX_ERR_INVALID_ARG.  Not done: other median sizes, 8-connectivity, hole filling. */
#ifndef COXGRAPH_HIP_STEREO_FILTER_H_
#define COXGRAPH_HIP_STEREO_FILTER_H_
#include "coxgraph_hip_stereo.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_stereo_filter_config {
  int32_t median_size;     /* 0: off, or 3 */
  int32_t speckle_window;  /* 0: off; components of at most this many pixels are removed; up to 2^31 - 1 */
  int32_t speckle_range16; /* 0 .. 0xFFFE: the largest difference, in 1/16 px, that links two neighbours */
  uint32_t reserved;       /* 0 */
} cox_stereo_filter_config;

typedef struct cox_stereo_filter_stats {
  uint64_t n_median_changed;     /* valid pixels whose value 7a changed */
  uint64_t n_components;         /* of 7b's graph */
  uint64_t n_speckle_components; /* of size <= speckle_window */
  uint64_t n_speckle_pixels;     /* pixels 7b invalidated */
  double median_ms;              /* HIP-event times of the last frame's two stages */
  double speckle_ms;
} cox_stereo_filter_stats;

/* what cox_stereo_filter_download gives */
typedef enum cox_stereo_filter_buffer {
  COX_STEREO_FILTER_DISPARITY_RAW = 0,    /* u16 [h][w]: the disparity before 7a */
  COX_STEREO_FILTER_DISPARITY_MEDIAN = 1, /* u16 [h][w]: after 7a (the same image when the median is off) */
  COX_STEREO_FILTER_LABELS = 2            /* u32 [h][w]: 7b's labels, 0xFFFFFFFF at invalid pixels */
} cox_stereo_filter_buffer;

/* 0, 0, 16, 0: both filters off, a range of one pixel */
void cox_stereo_filter_config_default(cox_stereo_filter_config* cfg);

/* Holds from the next frame; waits for the handle's stream first.  cfg NULL: both off.  COX_ERR_INVALID_ARG: a median size other
 * than 0 or 3, a negative window, a range outside 0 .. 0xFFFE, reserved != 0; COX_ERR_OUT_OF_MEMORY: no room for the buffers.
 * After either the handle is usable, with its previous setting. */
int cox_stereo_set_filters(cox_stereo_t* h, const cox_stereo_filter_config* cfg);
int cox_stereo_get_filters(cox_stereo_t* h, cox_stereo_filter_config* out);
/* of the last frame (waits for it); all zero before the first frame and when the last frame ran unfiltered.  In a filtered frame
 * cox_stereo_stats.depth_ms stays steps 6 and 8 (the two stages here are not in it) and frame_ms, first to last, includes them. */
int cox_stereo_filter_last_stats(cox_stereo_t* h, cox_stereo_filter_stats* out);
/* The last frame's filter stages (waits for the frame): `which` is a cox_stereo_filter_buffer.  Statuses as cox_stereo_download;
 * COX_ERR_INVALID_ARG also when the last frame ran unfiltered, and for the labels when it ran without 7b.  The final image is
 * cox_stereo_download(COX_STEREO_DISPARITY). */
int cox_stereo_filter_download(cox_stereo_t* h, int which, void* buf, uint64_t cap_bytes);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_STEREO_FILTER_H_ */
