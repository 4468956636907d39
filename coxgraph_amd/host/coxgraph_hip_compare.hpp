// Comparing layers and submaps in C++ (header-only, C++14) on top of include/coxgraph_hip_compare.h: voxblox's
// utils::evaluateLayersRmse with its VoxelEvaluationMode / VoxelEvaluationDetails, and the dense check of loop-closure candidates
// by free-space conflicts that the server runs between proposeLoopClosure (coxgraph_hip_align.hpp) and addLoopClosureMeasurement.
// Rule: DESIGN.md section 7p.
#pragma once
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "../../include/coxgraph_hip_compare.h"
#include "coxgraph_hip_align.hpp"
#include "coxgraph_hip_submap.hpp"

namespace coxgraph_hip {

// voxblox::utils::VoxelEvaluationMode
enum class VoxelEvaluationMode {
  kEvaluateAllVoxels = COX_COMPARE_ALL,
  kIgnoreErrorBehindTestSurface = COX_COMPARE_IGNORE_BEHIND_TEST,
  kIgnoreErrorBehindGtSurface = COX_COMPARE_IGNORE_BEHIND_GT,
  kIgnoreErrorBehindAllSurfaces = COX_COMPARE_IGNORE_BEHIND_ALL
};

// voxblox::utils::VoxelEvaluationDetails (errors in metres, quantised to 2^-16 m and saturated at 16 m: DESIGN.md 7p)
struct VoxelEvaluationDetails {
  double rmse = 0.0;
  double max_error = 0.0;
  double min_error = 0.0;
  size_t num_evaluated_voxels = 0u;
  size_t num_ignored_voxels = 0u;
  size_t num_overlapping_voxels = 0u;
  size_t num_non_overlapping_voxels = 0u;  // 4096 * blocks(test) - overlapping, as voxblox counts it
  std::string toString() const {
    return "rmse " + std::to_string(rmse) + " m, errors " + std::to_string(min_error) + " .. " + std::to_string(max_error) + " m, " + std::to_string(num_evaluated_voxels) +
           " evaluated, " + std::to_string(num_ignored_voxels) + " ignored, " + std::to_string(num_overlapping_voxels) + " overlapping, " +
           std::to_string(num_non_overlapping_voxels) + " non-overlapping voxels";
  }
};

// the root mean square of |e| in metres from one record; 0 when nothing was evaluated
inline double compareRmse(const cox_compare_stats& s) {
  if (s.n_evaluated == 0) return 0.0;
  const double total = std::ldexp(static_cast<double>(s.sum_q2_hi), 20) + static_cast<double>(s.sum_q2_lo);
  return std::sqrt(total / static_cast<double>(s.n_evaluated)) / static_cast<double>(COX_COMPARE_Q_PER_METRE);
}

// test layer A against reference layer B; both must outlive the comparer
class LayerComparer {
 public:
  struct Config : cox_compare_config {
    Config() { cox_compare_config_default(this); }
  };
  LayerComparer(const cox_layer_t* A, const cox_layer_t* B, const Config& config = Config()) {
    check(cox_compare_create(A, B, &config, &h_), "LayerComparer");
    check(cox_compare_get_config(h_, &config_), "LayerComparer");
  }
  ~LayerComparer() { cox_compare_destroy(h_); }
  LayerComparer(const LayerComparer&) = delete;
  LayerComparer& operator=(const LayerComparer&) = delete;

  const cox_compare_config& config() const { return config_; }  // defaults resolved
  cox_compare_t* handle() const { return h_; }

  // the same-frame compare
  cox_compare_stats run(VoxelEvaluationMode mode = VoxelEvaluationMode::kEvaluateAllVoxels, cox_compare_sample sample = COX_COMPARE_NEAREST) {
    cox_compare_stats s;
    check(cox_compare_run(h_, nullptr, 1, static_cast<int>(mode), sample, &s), "LayerComparer::run");
    return s;
  }
  // one record per transform T_B_A
  std::vector<cox_compare_stats> run(const std::vector<Transformation>& T_B_A, VoxelEvaluationMode mode = VoxelEvaluationMode::kEvaluateAllVoxels,
                                     cox_compare_sample sample = COX_COMPARE_NEAREST) {
    std::vector<float> T(7 * T_B_A.size());
    for (size_t i = 0; i < T_B_A.size(); ++i) T_B_A[i].pack(&T[7 * i]);
    std::vector<cox_compare_stats> out(T_B_A.size());
    check(cox_compare_run(h_, T.empty() ? nullptr : T.data(), out.size(), static_cast<int>(mode), sample, out.data()), "LayerComparer::run");
    return out;
  }
  // voxblox's error layer (T_B_A null: same frame)
  std::shared_ptr<LayerHandle> errorLayer(const Transformation* T_B_A, VoxelEvaluationMode mode = VoxelEvaluationMode::kEvaluateAllVoxels,
                                          cox_compare_sample sample = COX_COMPARE_NEAREST) {
    float T[7];
    if (T_B_A) T_B_A->pack(T);
    cox_layer_t* e = nullptr;
    check(cox_compare_error_layer(h_, T_B_A ? T : nullptr, static_cast<int>(mode), sample, &e), "LayerComparer::errorLayer");
    return std::make_shared<LayerHandle>(e);
  }
  double kernelTimeMs(uint64_t* runs = nullptr, bool reset = false) {
    double ms = 0.0;
    check(cox_compare_kernel_time(h_, &ms, runs, reset ? 1 : 0), "kernelTimeMs");
    return ms;
  }

 private:
  cox_compare_config config_;
  cox_compare_t* h_ = nullptr;
};

// voxblox::utils::evaluateLayersRmse(layer_test, layer_gt, mode, &details, &error_layer): both layers in one frame, every voxel of
// the test layer against the voxel of the ground-truth layer that contains its centre (the ground truth may be finer).  Returns
// the RMSE in metres.  error_layer (optional) receives a new layer with the test layer's blocks.
inline double evaluateLayersRmse(const TsdfLayer& layer_test, const TsdfLayer& layer_gt, VoxelEvaluationMode mode = VoxelEvaluationMode::kEvaluateAllVoxels,
                                 VoxelEvaluationDetails* details = nullptr, std::shared_ptr<LayerHandle>* error_layer = nullptr) {
  LayerComparer cmp(layer_test.handle(), layer_gt.handle());
  const cox_compare_stats s = cmp.run(mode);
  const double rmse = compareRmse(s);
  if (details) {
    details->rmse = rmse;
    details->max_error = static_cast<double>(s.max_q) / COX_COMPARE_Q_PER_METRE;
    details->min_error = static_cast<double>(s.min_q) / COX_COMPARE_Q_PER_METRE;
    details->num_evaluated_voxels = s.n_evaluated;
    details->num_ignored_voxels = s.n_ignored;
    details->num_overlapping_voxels = s.n_overlap;
    details->num_non_overlapping_voxels = 4096u * layer_test.getNumberOfAllocatedBlocks() - s.n_overlap;
  }
  if (error_layer) *error_layer = cmp.errorLayer(nullptr, mode);
  return rmse;
}

// The dense check of relative-pose candidates of two submaps: surface of A where B has observed free space, and the other way round.
class SubmapConsistency {
 public:
  struct Report {
    Transformation T_B_A;
    cox_compare_stats stats;
    double conflict_ratio = 0.0;  // (a-surface-in-b-free + b-surface-in-a-free) / (near a + near b); 0 when nothing is near a surface
    double agree_ratio = 0.0;     // agreeing / overlapping voxels; 0 without overlap
    double rmse = 0.0;
  };

  // T_B_A of two 4-DoF poses x, y, z, yaw given in one frame: composed in double, then narrowed to float
  static Transformation relativeTransformation(const double pose_a[4], const double pose_b[4]) {
    const double c = std::cos(pose_b[3]), s = std::sin(pose_b[3]);
    const double d[3] = {pose_a[0] - pose_b[0], pose_a[1] - pose_b[1], pose_a[2] - pose_b[2]};
    const double rel[4] = {c * d[0] + s * d[1], -s * d[0] + c * d[1], d[2], pose_a[3] - pose_b[3]};
    return transformationFromPose4(rel);
  }
  static Report report(const Transformation& T_B_A, const cox_compare_stats& s) {
    Report r;
    r.T_B_A = T_B_A;
    r.stats = s;
    const uint64_t near = s.n_near_a + s.n_near_b;
    r.conflict_ratio = near ? static_cast<double>(s.n_a_surface_in_b_free + s.n_b_surface_in_a_free) / static_cast<double>(near) : 0.0;
    r.agree_ratio = s.n_overlap ? static_cast<double>(s.n_agree) / static_cast<double>(s.n_overlap) : 0.0;
    r.rmse = compareRmse(s);
    return r;
  }

  // One report per candidate, in the candidates' order: candidate poses are poses of submap A as SubmapAligner searches them,
  // against submap B at pose_b (the aligner's origin by default).  The TSDF layers of the two submaps are compared.
  static std::vector<Report> check(const VoxgraphSubmap& submap_a, const VoxgraphSubmap& submap_b, const std::vector<SubmapAligner::Candidate>& candidates,
                                   const LayerComparer::Config& config = LayerComparer::Config(), cox_compare_sample sample = COX_COMPARE_TRILINEAR,
                                   const double* pose_b = nullptr) {
    static const double origin[4] = {0.0, 0.0, 0.0, 0.0};
    std::vector<Report> out;
    if (candidates.empty()) return out;
    std::vector<Transformation> T(candidates.size());
    for (size_t i = 0; i < candidates.size(); ++i) T[i] = relativeTransformation(candidates[i].pose, pose_b ? pose_b : origin);
    LayerComparer cmp(submap_a.getReadingLayer(false), submap_b.getReadingLayer(false), config);
    const std::vector<cox_compare_stats> stats = cmp.run(T, VoxelEvaluationMode::kEvaluateAllVoxels, sample);
    for (size_t i = 0; i < stats.size(); ++i) out.push_back(report(T[i], stats[i]));
    return out;
  }
};

// What a candidate must meet.  No defaults: nobody has measured good values, the caller sets all three.
struct LoopClosureCriteria {
  uint64_t min_overlap_voxels;
  double max_conflict_ratio;
  double min_agree_ratio;
  LoopClosureCriteria(uint64_t min_overlap_voxels_in, double max_conflict_ratio_in, double min_agree_ratio_in)
      : min_overlap_voxels(min_overlap_voxels_in), max_conflict_ratio(max_conflict_ratio_in), min_agree_ratio(min_agree_ratio_in) {}
  bool accepts(const SubmapConsistency::Report& r) const {
    return r.stats.n_overlap >= min_overlap_voxels && r.conflict_ratio <= max_conflict_ratio && r.agree_ratio >= min_agree_ratio;
  }
};

// The first candidate, in the aligner's order, that meets the criteria: its index, or -1.  *T_A_B (optional) is what
// addLoopClosureMeasurement(a, b, T_A_B) takes; reports (optional) receives every candidate's report.
inline int verifyLoopClosure(const VoxgraphSubmap& submap_a, const VoxgraphSubmap& submap_b, const std::vector<SubmapAligner::Candidate>& candidates,
                             const LoopClosureCriteria& criteria, Transformation* T_A_B = nullptr, std::vector<SubmapConsistency::Report>* reports = nullptr,
                             const LayerComparer::Config& config = LayerComparer::Config()) {
  const std::vector<SubmapConsistency::Report> all = SubmapConsistency::check(submap_a, submap_b, candidates, config);
  if (reports) *reports = all;
  for (size_t i = 0; i < all.size(); ++i)
    if (criteria.accepts(all[i])) {
      if (T_A_B) *T_A_B = inverse(all[i].T_B_A);
      return static_cast<int>(i);
    }
  return -1;
}

}  // namespace coxgraph_hip
