// Aligning two submaps without a prior in C++ (header-only, C++14) on top of include/coxgraph_hip_align.h: where does submap A
// sit relative to submap B when no visual loop closure says so?  The place coxgraph's server gets T_A_B from a MapFusion message
// (coxgraph/src/server/coxgraph_server.cpp:396-476); here geometry alone proposes it, and addLoopClosureMeasurement /
// addForceRegistrationConstraint take it from there.  Rule: DESIGN.md section 7o.
#pragma once
#include <cmath>
#include <vector>

#include "../../include/coxgraph_hip_align.h"
#include "coxgraph_hip_submap.hpp"

namespace coxgraph_hip {

class SubmapAligner {
 public:
  struct Config : cox_align_config {
    Config() { cox_align_config_default(this); }
  };
  // the search, and which products of the two submaps it reads (as PoseGraphInterface::RegistrationConfig chooses them)
  struct SearchConfig : cox_align_search_config {
    RegistrationPointType registration_point_type = RegistrationPointType::kIsosurfacePoints;
    bool use_esdf_distance = true;
    double no_correspondence_cost = 0.0;
    double min_corr_ratio = 0.25;  // min_corr == 0: this share of the reference points
    SearchConfig() {
      const double half[4] = {2.0, 2.0, 0.4, M_PI}, st[4] = {0.4, 0.4, 0.4, M_PI / 18.0};
      for (int k = 0; k < 4; ++k) center[k] = 0.0, half_extent[k] = half[k], step[k] = st[k];
      inlier_distance = 0.4f, tau_min = 0.1f;
      levels = 4, keep = 8, min_corr = 0, pad = 0;
    }
  };
  struct Candidate {
    double pose[4];  // x, y, z, yaw of the reference submap
    cox_align_score score;
  };

  // both must outlive the aligner; the layer may be written and may grow between calls
  SubmapAligner(const cox_regpoints_t* reference, const cox_layer_t* reading, const Config& config = Config()) : config_(config) {
    check(cox_align_create(reference, reading, &config_, &h_), "SubmapAligner");
  }
  ~SubmapAligner() { cox_align_destroy(h_); }
  SubmapAligner(const SubmapAligner&) = delete;
  SubmapAligner& operator=(const SubmapAligner&) = delete;

  const Config& config() const { return config_; }
  cox_align_t* handle() const { return h_; }

  void setSamples(const std::vector<uint32_t>& sample_idx) {
    static const uint32_t none = 0;
    check(cox_align_set_samples(h_, sample_idx.empty() ? &none : sample_idx.data(), sample_idx.size()), "setSamples");
  }
  void clearSamples() { check(cox_align_set_samples(h_, nullptr, 0), "clearSamples"); }

  // one record per candidate reference pose (4 doubles each); inlier_distance 0: the config's
  std::vector<cox_align_score> sweep(const std::vector<double>& poses_ref, const double pose_read[4], float inlier_distance = 0.0f) {
    std::vector<cox_align_score> out(poses_ref.size() / 4);
    check(cox_align_sweep(h_, pose_read, poses_ref.data(), out.size(), inlier_distance > 0.0f ? inlier_distance : config_.inlier_distance, out.data()), "sweep");
    return out;
  }
  // the kept candidates of the last level, best first; empty when none met min_corr.  trace (optional): one entry per level run.
  std::vector<Candidate> search(const cox_align_search_config& cfg, const double pose_read[4], std::vector<cox_align_level>* trace = nullptr) {
    double poses[4 * COX_ALIGN_MAX_KEEP];
    cox_align_score scores[COX_ALIGN_MAX_KEEP];
    uint32_t n = 0;
    std::vector<cox_align_level> levels(trace ? cfg.levels + 1u : 0u);
    check(cox_align_search(h_, pose_read, &cfg, poses, scores, &n, trace && cfg.levels <= COX_ALIGN_MAX_LEVELS ? levels.data() : nullptr), "search");
    if (trace) {
      while (!levels.empty() && levels.back().n_candidates == 0) levels.pop_back();
      trace->swap(levels);
    }
    std::vector<Candidate> out(n);
    for (uint32_t j = 0; j < n; ++j) {
      for (int k = 0; k < 4; ++k) out[j].pose[k] = poses[4 * j + k];
      out[j].score = scores[j];
    }
    return out;
  }
  double kernelTimeMs(uint64_t* sweeps = nullptr, bool reset = false) {
    double ms = 0.0;
    check(cox_align_kernel_time(h_, &ms, sweeps, reset ? 1 : 0), "kernelTimeMs");
    return ms;
  }

  static std::vector<double> grid(const double center[4], const double half_extent[4], const double step[4]) {
    uint64_t n = 0;
    check(cox_align_grid(center, half_extent, step, nullptr, 0, &n), "grid");
    std::vector<double> out(4 * n);
    check(cox_align_grid(center, half_extent, step, out.data(), n, &n), "grid");
    return out;
  }
  static std::vector<uint32_t> select(const std::vector<cox_align_score>& scores, uint32_t min_corr, uint32_t keep) {
    std::vector<uint32_t> idx(COX_ALIGN_MAX_KEEP);
    uint32_t n = 0;
    check(cox_align_select(scores.data(), scores.size(), min_corr, keep, idx.data(), &n), "select");
    idx.resize(n);
    return idx;
  }

 private:
  Config config_;
  cox_align_t* h_ = nullptr;
};

// the inverse of a 4-DoF pose x, y, z, yaw, in double
inline void inversePose4(const double p[4], double out[4]) {
  const double c = std::cos(p[3]), s = std::sin(p[3]);
  out[0] = -(c * p[0] + s * p[1]);
  out[1] = -(-s * p[0] + c * p[1]);
  out[2] = -p[2];
  out[3] = -p[3];
}

// Proposes the relative pose of two finished submaps from their geometry: A's registration points against B's distance field, as
// makeRegistrationConstraint pairs them.  The search runs over the pose of A in B's frame (cfg.center / half_extent / step are
// in that frame); *T_A_B is the inverse of the best candidate, what addLoopClosureMeasurement(a, b, T_A_B) takes.  False when
// no candidate had min_corr correspondences (*T_A_B is left alone).  best (optional): the candidate itself.
inline bool proposeLoopClosure(const VoxgraphSubmap& a, const VoxgraphSubmap& b, const SubmapAligner::SearchConfig& cfg, Transformation* T_A_B,
                               SubmapAligner::Candidate* best = nullptr) {
  const std::shared_ptr<RegistrationPointSet> pts = a.getRegistrationPoints(cfg.registration_point_type);
  SubmapAligner::Config ac;
  ac.inlier_distance = cfg.inlier_distance;
  ac.no_correspondence_cost = cfg.no_correspondence_cost;
  SubmapAligner aligner(pts->handle(), b.getReadingLayer(cfg.use_esdf_distance), ac);
  cox_align_search_config sc = cfg;
  if (sc.min_corr == 0) sc.min_corr = static_cast<uint32_t>(cfg.min_corr_ratio * static_cast<double>(pts->size()));
  const double origin[4] = {0.0, 0.0, 0.0, 0.0};
  const std::vector<SubmapAligner::Candidate> found = aligner.search(sc, origin);
  if (found.empty()) return false;
  if (best) *best = found[0];
  if (T_A_B) {
    double inv[4];
    inversePose4(found[0].pose, inv);
    *T_A_B = transformationFromPose4(inv);
  }
  return true;
}

}  // namespace coxgraph_hip
