/* Dense stereo on the GPU (coxgraph_amd/csrc/cox_stereo.hip): a raw 8-bit image pair to a depth image by rectification and
 * semi-global matching.  coxgraph's EuRoC experiment has no depth camera: coxgraph/launch/euroc/vins_client_euroc.launch:18-47 runs
 * image_undistort's dense_stereo_node on cam0 / cam1 of coxgraph/config/euroc/euroc_camchain.yaml and every tsdf_client integrates
 * its output.  The depth image written here has the layout of the renderer, the tracker and cox_depthfuse_integrate_dev (w * h
 * floats, row-major, z-depth in metres, NaN where there is nothing, K = {fx, fy, cx, cy}), so pair -> depth -> fusion stays on
 * the device.  The rule of one frame (steps R and 1-8) is integer arithmetic from the census to the disparity and is stated in
 * DESIGN.md section 7n; tests/stereo_ref.py restates it in numpy and the kernels owe it every bit.  A median and a speckle filter
 * on the disparity are switched on through coxgraph_hip_stereo_filter.h.  Not done: a minimum disparity other than 0, an adaptive
 * P2, colour inputs, fisheye models, OpenCV StereoSGBM parity.
 *
 * Kept apart from coxgraph_hip.h on purpose, like coxgraph_hip_depthfuse.h: these entry points have no counterpart in the CPU
 * checker of the test suite.  Conventions are those of coxgraph_hip_map.h (COX_OK or a negative cox_status; where a device is
 * needed, no usable GPU -> COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG).  One call at a time per handle. */
#ifndef COXGRAPH_HIP_STEREO_H_
#define COXGRAPH_HIP_STEREO_H_
#include "coxgraph_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cox_stereo cox_stereo_t;

#define COX_STEREO_MAX_SIDE (1 << 15)       /* w, h */
#define COX_STEREO_MAX_COST_CELLS (1ull << 31) /* w * h * n_disparities */

typedef struct cox_stereo_config {
  int32_t n_disparities;      /* 64, 128 or 256; disparities 0 .. n - 1 are searched */
  int32_t n_paths;            /* 4 or 8 */
  int32_t p1;                 /* 0 <= p1 <= p2 <= 255 */
  int32_t p2;
  int32_t uniqueness_percent; /* 0 .. 99 */
  int32_t lr_max_diff;        /* in whole disparities; < 0: no left-right check */
  float min_depth_m;          /* 0: no lower limit */
  float max_depth_m;          /* +inf: no upper limit */
  uint32_t reserved;          /* 0 */
} cox_stereo_config;

typedef struct cox_stereo_stats {
  uint64_t n_valid_pixels;        /* pixels with a depth */
  uint64_t n_rejected_uniqueness; /* usable pixels step 5 rejected */
  uint64_t n_rejected_lr;         /* usable pixels that passed step 5 and were rejected by step 6 */
  uint64_t n_rejected_depth;      /* pixels with a valid disparity whose depth is outside the limits */
  double remap_ms;                /* HIP-event times of the last frame: step 1 (with the upload of the pair, from host arrays) */
  double census_ms;               /* step 2 */
  double paths_ms;                /* steps 3-4 */
  double winner_ms;               /* steps 5 and 7, and dR of step 6 */
  double depth_ms;                /* steps 6 and 8 (with the download of the outputs, to host arrays) */
  double frame_ms;                /* first to last */
} cox_stereo_stats;

/* one camera of a kalibr camchain */
typedef struct cox_stereo_camera {
  int32_t camera_model;           /* 0 pinhole; anything else: COX_ERR_UNSUPPORTED */
  int32_t distortion_model;       /* 0 radtan; anything else (1 equidistant, 2 fov ...): COX_ERR_UNSUPPORTED */
  double intrinsics[4];           /* fx, fy, cx, cy */
  double distortion_coeffs[4];    /* k1, k2, p1, p2 */
} cox_stereo_camera;

typedef struct cox_stereo_calibration {
  cox_stereo_camera cam[2];
  double T_cn_cnm1[16];           /* cam1's, 4 x 4 row-major: p_c1 = R p_c0 + t */
} cox_stereo_calibration;

/* what cox_stereo_download gives */
typedef enum cox_stereo_buffer {
  COX_STEREO_RECT_LEFT = 0,  /* u8 [h][w] */
  COX_STEREO_RECT_RIGHT = 1, /* u8 [h][w] */
  COX_STEREO_COST_SUM = 2,   /* u16 [h][w][n_disparities]: S of step 4 */
  COX_STEREO_DISPARITY = 3   /* u16 [h][w]: 1/16 px, 0xFFFF where invalid */
} cox_stereo_buffer;

/* 128 disparities, 8 paths, P1 7, P2 86, uniqueness 10 %, left-right difference 1, no depth limits (0, +inf) */
void cox_stereo_config_default(cox_stereo_config* cfg);

/* Step R, on the host, in float64: needs NO GPU.  map0_xy / map1_xy get 2 floats per pixel of the w x h rectified images (where
 * to read cam0 / cam1, NaN where the pixel looks behind the camera), K_rect = {f, f, cx, cy} with f = scale * the mean of the
 * four focal lengths, *baseline_m = |t|, T_c0_rect = {qw, qx, qy, qz, 0, 0, 0}: the rectified left camera in cam0.
 * COX_ERR_INVALID_ARG: a NULL pointer, w or h < 1 or > 2^15, a scale that is not finite and > 0, numbers that are not finite,
 * focal lengths that are not > 0, a baseline of zero.  COX_ERR_UNSUPPORTED: another camera or distortion model. */
int cox_stereo_rectify_maps(const cox_stereo_calibration* calib, int w, int h, double scale, float* map0_xy, float* map1_xy, float K_rect[4],
                            float* baseline_m, float T_c0_rect[7]);

/* A matcher for w x h pairs on `device`.  map0_xy / map1_xy: host arrays as cox_stereo_rectify_maps writes them, copied; both
 * NULL: the pairs are already rectified.  K_rect and baseline_m turn disparities into depths.  Every device buffer a frame needs
 * is allocated here (about w * h * (2 * n_disparities + 56) bytes): a frame allocates nothing.  cfg NULL: the defaults.
 * COX_ERR_INVALID_ARG: w or h < 1 or > 2^15, w * h * n_disparities > 2^31, a configuration outside the ranges above, one map
 * without the other, K_rect[0] or baseline_m not finite and > 0, a device that does not exist. */
int cox_stereo_create(int device, int w, int h, const cox_stereo_config* cfg, const float* map0_xy, const float* map1_xy, const float K_rect[4],
                      float baseline_m, cox_stereo_t** out);
/* waits for the handle's stream first */
void cox_stereo_destroy(cox_stereo_t* h);

/* One frame from host arrays: left, right 8-bit gray [h][w]; depth float [h][w]; rgba [h][w][4] (the rectified left gray g as
 * g, g, g, 255) and disparity u16 [h][w] may be NULL.  Everything is enqueued on the handle's stream; the outputs are complete,
 * and the inputs no longer needed, after cox_stereo_sync. */
int cox_stereo_compute(cox_stereo_t* h, const uint8_t* left, const uint8_t* right, float* depth, uint8_t* rgba_or_null, uint16_t* disparity_or_null);
/* The same with device arrays on the handle's GPU, with the stream ordering of cox_depthfuse_integrate_dev: the frame orders behind
 * what producer_stream (a hipStream_t; NULL: the null stream) holds at the call, and producer_stream then waits until the frame has
 * read left and right, so they may be reused or freed in stream order on it.  Waits for the host nowhere.  The outputs are complete
 * after cox_stereo_sync, or in stream order behind an event recorded on cox_stereo_stream.  rgba_dev is written as 32-bit words: 4-byte aligned. */
int cox_stereo_compute_dev(cox_stereo_t* h, const uint8_t* left_dev, const uint8_t* right_dev, float* depth_dev, uint8_t* rgba_dev_or_null,
                           uint16_t* disparity_dev_or_null, void* producer_stream);
/* the handle's hipStream_t (NULL for a NULL handle): consumers order behind a frame without the host */
void* cox_stereo_stream(cox_stereo_t* h);
/* waits for every frame of this handle */
int cox_stereo_sync(cox_stereo_t* h);
/* of the last frame (waits for it); all zero before the first */
int cox_stereo_last_stats(cox_stereo_t* h, cox_stereo_stats* out);
/* The last frame's intermediates, for tests and debugging (waits for the frame): `which` is a cox_stereo_buffer.
 * COX_ERR_BUFFER_TOO_SMALL when cap_bytes is less than the buffer, COX_ERR_INVALID_ARG before the first frame. */
int cox_stereo_download(cox_stereo_t* h, int which, void* buf, uint64_t cap_bytes);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_STEREO_H_ */
