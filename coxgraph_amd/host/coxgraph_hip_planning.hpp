// View scoring for an exploration planner in C++ (header-only, C++14) on top of include/coxgraph_hip_gain.h: the place
// active_3d_planning gives its ray-casting sensor model and its VoxelWeightEvaluator (coxgraph_sim/config/reconstruction_planner.yaml),
// here for a whole batch of candidate poses in one call on the GPU.  Rules and arithmetic: DESIGN.md section 7j.
#pragma once
#include <cmath>
#include <vector>

#include "../../include/coxgraph_hip_gain.h"
#include "coxgraph_hip_adapters.hpp"

namespace coxgraph_hip {

// The planner's camera as a ray grid: a width x height pinhole camera of the given focal length, every `downsampling_factor`-th
// pixel a ray (rounded up), principal point at the centre of the grid, rays of ray_length metres.
struct RayCasterSensor {
  int rays_x, rays_y;
  float K[4];  // fx, fy, cx, cy of the ray grid
  float ray_length, min_range;
  float ray_step;  // 0: the map's voxel size

  RayCasterSensor(int width = 172, int height = 480, float focal_length = 320.0f, float downsampling_factor = 5.0f, float ray_length_m = 5.0f)
      : rays_x(static_cast<int>(std::ceil(static_cast<float>(width) / downsampling_factor))),
        rays_y(static_cast<int>(std::ceil(static_cast<float>(height) / downsampling_factor))),
        ray_length(ray_length_m), min_range(0.0f), ray_step(0.0f) {
    K[0] = K[1] = focal_length / downsampling_factor;
    K[2] = static_cast<float>(rays_x / 2), K[3] = static_cast<float>(rays_y / 2);
  }
};

// active_3d_planning's VoxelWeightEvaluator (behind a ContinuousYawPlanningEvaluator) on a layer of this engine
class VoxelWeightEvaluator {
 public:
  struct Config {  // the yaml's names and values (reconstruction_planner.yaml:71-91)
    float frontier_voxel_weight, new_voxel_weight, min_impact_factor, ray_angle_x, ray_angle_y;
    bool accurate_frontiers, surface_frontiers;
    // bounding_volume_args: voxels whose centre lies outside do not count
    bool use_bounding_volume;
    Point bounding_volume_min, bounding_volume_max;
    // this engine's: which voxels are observed / occupied, and the cap of the GPU workspace (0: 256 MiB)
    float min_weight, surface_distance;
    uint64_t workspace_bytes;
    Config()
        : frontier_voxel_weight(1.0f), new_voxel_weight(0.0f), min_impact_factor(0.01f), ray_angle_x(0.002454f), ray_angle_y(0.002681f),
          accurate_frontiers(true), surface_frontiers(true), use_bounding_volume(false), bounding_volume_min{{0.0f, 0.0f, 0.0f}},
          bounding_volume_max{{0.0f, 0.0f, 0.0f}}, min_weight(0.0f), surface_distance(0.0f), workspace_bytes(0) {}
  };

  // the layer must outlive the evaluator; it may be written and may grow between calls
  VoxelWeightEvaluator(cox_layer_t* layer, const RayCasterSensor& sensor = RayCasterSensor(), const Config& config = Config())
      : sensor_(sensor), config_(config) {
    cox_viewgain_config c;
    cox_viewgain_config_default(&c);
    c.w = sensor.rays_x, c.h = sensor.rays_y;
    for (int k = 0; k < 4; ++k) c.K[k] = sensor.K[k];
    c.min_range = sensor.min_range, c.ray_length = sensor.ray_length, c.ray_step = sensor.ray_step;
    c.min_weight = config.min_weight, c.surface_distance = config.surface_distance;
    c.frontier_voxel_weight = config.frontier_voxel_weight, c.new_voxel_weight = config.new_voxel_weight;
    c.min_impact_factor = config.min_impact_factor;
    c.ray_angle_x = config.ray_angle_x, c.ray_angle_y = config.ray_angle_y;
    c.accurate_frontiers = config.accurate_frontiers ? 1 : 0, c.surface_frontiers = config.surface_frontiers ? 1 : 0;
    c.use_box = config.use_bounding_volume ? 1 : 0;
    for (int k = 0; k < 3; ++k) c.box_min[k] = config.bounding_volume_min[k], c.box_max[k] = config.bounding_volume_max[k];
    c.workspace_bytes = config.workspace_bytes;
    check(cox_viewgain_create(layer, &c, &h_), "VoxelWeightEvaluator");
  }
  ~VoxelWeightEvaluator() { cox_viewgain_destroy(h_); }
  VoxelWeightEvaluator(const VoxelWeightEvaluator&) = delete;
  VoxelWeightEvaluator& operator=(const VoxelWeightEvaluator&) = delete;

  const Config& config() const { return config_; }
  const RayCasterSensor& sensor() const { return sensor_; }
  cox_viewgain_t* handle() const { return h_; }

  // one record per pose (T_G_C of the camera: z forward, x right, y down), in one call; stats optional
  std::vector<cox_view_gain> computeGains(const std::vector<Transformation>& poses, cox_viewgain_stats* stats = nullptr) const {
    std::vector<float> T(7 * poses.size());
    for (size_t i = 0; i < poses.size(); ++i) poses[i].pack(&T[7 * i]);
    std::vector<cox_view_gain> out(poses.size());
    if (stats) stats->n_samples = stats->n_chunks = 0, stats->kernel_ms = 0.0;
    check(cox_viewgain_evaluate(h_, T.data(), poses.size(), out.data(), stats), "computeGains");
    return out;
  }

  // ContinuousYawPlanningEvaluator: the camera poses at `position` under n_directions yaws, k * 2 pi / n_directions about the
  // world z axis from `yaw_offset`; at yaw 0 the camera looks along +x with the image's x axis along -y
  static std::vector<Transformation> yawSweep(const Point& position, int n_directions, double yaw_offset = 0.0) {
    std::vector<Transformation> out(n_directions > 0 ? n_directions : 0);
    const double pi = 3.14159265358979323846;
    for (int k = 0; k < n_directions; ++k) {
      const double yaw = yaw_offset + 2.0 * pi * k / n_directions;
      const double hw = std::cos(0.5 * yaw), hz = std::sin(0.5 * yaw);
      const double o[4] = {0.5, -0.5, 0.5, -0.5};  // optical frame (z forward, x right, y down) in a body frame x forward, z up
      Transformation& T = out[k];
      T.q[0] = static_cast<float>(hw * o[0] - hz * o[3]);
      T.q[1] = static_cast<float>(hw * o[1] - hz * o[2]);
      T.q[2] = static_cast<float>(hw * o[2] + hz * o[1]);
      T.q[3] = static_cast<float>(hw * o[3] + hz * o[0]);
      for (int a = 0; a < 3; ++a) T.t[a] = position[a];
    }
    return out;
  }

 private:
  RayCasterSensor sensor_;
  Config config_;
  cox_viewgain_t* h_ = nullptr;
};

}  // namespace coxgraph_hip
