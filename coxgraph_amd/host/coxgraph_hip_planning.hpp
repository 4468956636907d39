// What an exploration planner asks of the map, in C++ (header-only, C++14), as coxgraph configures active_3d_planning
// (coxgraph_sim/config/reconstruction_planner.yaml), each for a whole batch in one call on the GPU:
//   view scoring -- its ray-casting sensor model and VoxelWeightEvaluator, on include/coxgraph_hip_gain.h;
//   collision checking -- its VoxbloxMap, the RRTStar generator's segment checks and crop, and the RecheckCollision updater, on
//   include/coxgraph_hip_collide.h.
#pragma once
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/coxgraph_hip_collide.h"
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

// system_constraints of the yaml (reconstruction_planner.yaml:20-25)
struct SystemConstraints {
  float v_max, a_max, yaw_rate_max, yaw_accel_max, collision_radius;
  SystemConstraints() : v_max(1.0f), a_max(0.5f), yaw_rate_max(0.5f), yaw_accel_max(0.5f), collision_radius(2.0f) {}
};

// active_3d_planning's VoxbloxMap on an ESDF (or TSDF) layer of this engine: isTraversable / isObserved, one point or a batch
class VoxbloxMap {
 public:
  // the layer must outlive the map; it may be written and may grow between calls
  explicit VoxbloxMap(cox_layer_t* layer, const SystemConstraints& constraints = SystemConstraints()) : constraints_(constraints) {
    cox_collide_config c;
    cox_collide_config_default(&c);
    c.collision_radius = constraints.collision_radius;
    check(cox_collide_create(layer, &c, &h_), "VoxbloxMap");
  }
  ~VoxbloxMap() { cox_collide_destroy(h_); }
  VoxbloxMap(const VoxbloxMap&) = delete;
  VoxbloxMap& operator=(const VoxbloxMap&) = delete;

  const SystemConstraints& constraints() const { return constraints_; }
  cox_collide_t* handle() const { return h_; }

  // COX_C_* of every position, in one call
  std::vector<uint8_t> states(const std::vector<Point>& positions) const {
    std::vector<uint8_t> st(positions.size(), 0);
    check(cox_collide_points(h_, positions.empty() ? nullptr : positions[0].data(), positions.size(), st.data(), nullptr), "VoxbloxMap::states");
    return st;
  }
  std::vector<bool> isTraversable(const std::vector<Point>& positions) const { return bit(states(positions), COX_C_TRAVERSABLE); }
  std::vector<bool> isObserved(const std::vector<Point>& positions) const { return bit(states(positions), COX_C_OBSERVED); }
  // (the orientation argument of the planner's isTraversable is ignored there too)
  bool isTraversable(const Point& position) const { return isTraversable(std::vector<Point>(1, position))[0]; }
  bool isObserved(const Point& position) const { return isObserved(std::vector<Point>(1, position))[0]; }

 private:
  static std::vector<bool> bit(const std::vector<uint8_t>& st, unsigned mask) {
    std::vector<bool> out(st.size());
    for (size_t i = 0; i < st.size(); ++i) out[i] = (st[i] & mask) != 0;
    return out;
  }
  SystemConstraints constraints_;
  cox_collide_t* h_ = nullptr;
};

// The map side of active_3d_planning's RRTStar trajectory generator and of its RecheckCollision updater
class RRTStarCollision {
 public:
  struct Config {  // the yaml's names and values (trajectory_generator, reconstruction_planner.yaml:27-41)
    bool collision_optimistic;
    float clearing_radius;
    bool crop_segments;
    float crop_margin, crop_min_length, max_extension_range, sampling_rate;
    uint32_t max_samples;  // this engine's: sampling intervals a segment may have
    Config()
        : collision_optimistic(false), clearing_radius(0.0f), crop_segments(true), crop_margin(0.3f), crop_min_length(0.5f), max_extension_range(1.5f),
          sampling_rate(20.0f), max_samples(4096) {}
  };
  // the stored trajectories of a tree's segments in CSR form and each segment's parent (-1: the root)
  struct Tree {
    std::vector<uint64_t> offsets;  // n + 1
    std::vector<Point> points;
    std::vector<int32_t> parent;    // n
    Tree() : offsets(1, 0) {}
    size_t size() const { return parent.size(); }
    void addSegment(int32_t parent_index, const std::vector<Point>& trajectory) {
      points.insert(points.end(), trajectory.begin(), trajectory.end());
      offsets.push_back(points.size());
      parent.push_back(parent_index);
    }
  };

  RRTStarCollision(cox_layer_t* layer, const SystemConstraints& constraints = SystemConstraints(), const Config& config = Config())
      : constraints_(constraints), config_(config) {
    cox_collide_config c;
    cox_collide_config_default(&c);
    c.collision_radius = constraints.collision_radius;
    c.collision_optimistic = config.collision_optimistic ? 1 : 0;
    c.clearing_radius = config.clearing_radius;
    c.sample_spacing = constraints.v_max / config.sampling_rate;
    c.max_samples = config.max_samples;
    c.max_extension_range = config.max_extension_range;
    c.crop = config.crop_segments ? 1 : 0;
    c.crop_margin = config.crop_margin, c.crop_min_length = config.crop_min_length;
    check(cox_collide_create(layer, &c, &h_), "RRTStarCollision");
  }
  ~RRTStarCollision() { cox_collide_destroy(h_); }
  RRTStarCollision(const RRTStarCollision&) = delete;
  RRTStarCollision& operator=(const RRTStarCollision&) = delete;

  const Config& config() const { return config_; }
  cox_collide_t* handle() const { return h_; }
  // the clearing sphere follows the robot
  void setRobotPosition(const Point& position) { check(cox_collide_set_clearing_centre(h_, position.data()), "setRobotPosition"); }

  // one record per straight segment starts[i] -> goals[i]
  std::vector<cox_collide_record> checkSegments(const std::vector<Point>& starts, const std::vector<Point>& goals) const {
    if (starts.size() != goals.size()) throw std::runtime_error("checkSegments: starts and goals differ in size");
    std::vector<cox_collide_record> out(starts.size());
    check(cox_collide_segments(h_, starts.empty() ? nullptr : starts[0].data(), goals.empty() ? nullptr : goals[0].data(), starts.size(), out.data()),
          "checkSegments");
    return out;
  }
  // connectPoses: the straight segment is traversable at every sample (after the cut to max_extension_range)
  std::vector<bool> connectPoses(const std::vector<Point>& starts, const std::vector<Point>& goals) const {
    const std::vector<cox_collide_record> rec = checkSegments(starts, goals);
    std::vector<bool> out(rec.size());
    for (size_t i = 0; i < rec.size(); ++i) out[i] = (rec[i].flags & COX_SEG_FEASIBLE) != 0;
    return out;
  }
  // adjustGoalPosition: the goal itself when the segment is free, the cropped goal when enough of it is; success[i] tells
  std::vector<Point> adjustGoalPositions(const std::vector<Point>& starts, const std::vector<Point>& goals, std::vector<bool>* success) const {
    const std::vector<cox_collide_record> rec = checkSegments(starts, goals);
    std::vector<Point> out(rec.size());
    if (success) success->assign(rec.size(), false);
    for (size_t i = 0; i < rec.size(); ++i) {
      for (int k = 0; k < 3; ++k) out[i][k] = rec[i].goal[k];
      if (success) (*success)[i] = (rec[i].flags & COX_SEG_GOAL) != 0;
    }
    return out;
  }
  // RecheckCollision: which segments of the tree survive the current map (a collided segment goes with its subtree); keep[i] is
  // COX_TREE_KEEP, 0 or COX_TREE_INVALID
  std::vector<uint8_t> recheckCollision(const Tree& tree, std::vector<cox_collide_record>* records = nullptr) const {
    const size_t n = tree.size();
    if (tree.offsets.size() != n + 1) throw std::runtime_error("recheckCollision: offsets and parents differ in size");
    std::vector<uint8_t> keep(n, 0);
    if (records) records->assign(n, cox_collide_record());
    check(cox_collide_tree(h_, tree.offsets.data(), tree.parent.data(), n, tree.points.empty() ? nullptr : tree.points[0].data(), tree.points.size(),
                           records ? records->data() : nullptr, keep.data()),
          "recheckCollision");
    return keep;
  }

 private:
  SystemConstraints constraints_;
  Config config_;
  cox_collide_t* h_ = nullptr;
};

}  // namespace coxgraph_hip
