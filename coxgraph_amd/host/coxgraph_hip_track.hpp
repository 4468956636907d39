// Scan-to-map registration in C++ (header-only, C++14) on top of include/coxgraph_hip_track.h: where was the sensor, relative to the
// map a scan is about to be fused into?  The place voxblox's tsdf_server gives its ICP refinement and voxgraph its scan-to-map
// registerer; the cost here is this engine's own (point-to-implicit-surface on the TSDF).
#pragma once
#include <string>

#include "../../include/coxgraph_hip_track.h"
#include "coxgraph_hip_adapters.hpp"

namespace coxgraph_hip {

class ScanToMapRegisterer {
 public:
  struct Config : cox_track_config {
    Config() { cox_track_config_default(this); }
  };

  // the layer must outlive the registerer; it may be written and may grow between calls
  explicit ScanToMapRegisterer(cox_layer_t* layer, const Config& config = Config()) : config_(config) {
    check(cox_track_create(layer, &config_, &track_), "ScanToMapRegisterer");
  }
  ~ScanToMapRegisterer() { cox_track_destroy(track_); }
  ScanToMapRegisterer(const ScanToMapRegisterer&) = delete;
  ScanToMapRegisterer& operator=(const ScanToMapRegisterer&) = delete;

  const Config& config() const { return config_; }
  cox_track_t* handle() const { return track_; }

  // Refine T_prior (T_G_C) with the sensor-frame points of a scan.  True when the loop converged or ran out of iterations (a
  // step was taken each time); false when the scan is lost or the system degenerate -- T_refined is then the pose the last
  // iteration started from (the prior, if it was the first).  result (optional): counts, costs, step norms and the float64 pose.
  bool refineSensorPose(const Pointcloud& points_C, const Transformation& T_prior, Transformation* T_refined, cox_track_result* result = nullptr) {
    float prior[7], refined[7];
    T_prior.pack(prior);
    cox_track_result r;
    check(cox_track_refine(track_, prior, points_C.empty() ? nullptr : points_C[0].data(), points_C.size(), refined, &r), "refineSensorPose");
    unpack(refined, T_refined);
    if (result) *result = r;
    return r.status == COX_TRACK_CONVERGED || r.status == COX_TRACK_MAX_ITERATIONS;
  }
  // the same with a depth image already on the GPU (the layout of integrateDepth / renderView's depth), K = {fx, fy, cx, cy}
  bool refineSensorPoseFromDepthDevice(const float* depth_dev, int width, int height, const float K[4], const Transformation& T_prior,
                                       Transformation* T_refined, cox_track_result* result = nullptr) {
    float prior[7], refined[7];
    T_prior.pack(prior);
    cox_track_result r;
    check(cox_track_refine_depth_dev(track_, prior, depth_dev, width, height, K, refined, &r), "refineSensorPoseFromDepthDevice");
    unpack(refined, T_refined);
    if (result) *result = r;
    return r.status == COX_TRACK_CONVERGED || r.status == COX_TRACK_MAX_ITERATIONS;
  }

  static const char* statusString(int status) {
    switch (status) {
      case COX_TRACK_CONVERGED: return "converged";
      case COX_TRACK_MAX_ITERATIONS: return "max iterations";
      case COX_TRACK_LOST: return "lost";
      case COX_TRACK_DEGENERATE: return "degenerate";
    }
    return "?";
  }

 private:
  static void unpack(const float T[7], Transformation* out) {
    if (!out) return;
    for (int k = 0; k < 4; ++k) out->q[k] = T[k];
    for (int k = 0; k < 3; ++k) out->t[k] = T[4 + k];
  }
  Config config_;
  cox_track_t* track_ = nullptr;
};

}  // namespace coxgraph_hip
