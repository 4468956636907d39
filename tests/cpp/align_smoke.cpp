// Submap alignment without a prior from C++ (coxgraph_amd/host/coxgraph_hip_align.hpp) on the GPU: the analytic room (a box
// with a sphere in it) is written into two submaps through the C ABI, one in the room's frame (B), one in a frame that sits
// at a known pose in it (A).  SubmapAligner and proposeLoopClosure must find that pose from A's isosurface points and B's TSDF
// to within one final grid step per axis, and the pose graph must take the result as a loop closure.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../coxgraph_amd/host/coxgraph_hip_align.hpp"
#include "../../coxgraph_amd/host/coxgraph_hip_posegraph.hpp"

using namespace coxgraph_hip;

static const double kRoomMin[3] = {-4.0, -3.0, 0.0}, kRoomMax[3] = {4.0, 3.0, 3.0}, kSphereC[3] = {2.5, 0.5, 1.0}, kSphereR = 0.75;
static const float kVoxel = 0.2f;
static const double kTruncation = 0.6;

static double roomDistance(const double p[3]) {  // positive in free space
  double d = 1e30;
  for (int k = 0; k < 3; ++k) d = std::min(d, std::min(kRoomMax[k] - p[k], p[k] - kRoomMin[k]));
  const double s[3] = {p[0] - kSphereC[0], p[1] - kSphereC[1], p[2] - kSphereC[2]};
  return std::min(d, std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) - kSphereR);
}

// the room as a TSDF in a frame that sits at `pose` (x, y, z, yaw) in the room's frame: every voxel within truncation + one
// voxel of a surface is observed with weight 2
static void uploadRoom(const double pose[4], TsdfLayer* layer) {
  const float bs = kVoxel * 16.0f;
  const double c = std::cos(pose[3]), s = std::sin(pose[3]), band = kTruncation + kVoxel;
  std::vector<int32_t> idx;
  std::vector<uint32_t> words;
  std::vector<uint32_t> block(4096 * 3);
  const float two = 2.0f;
  uint32_t w_bits;
  std::memcpy(&w_bits, &two, 4);
  for (int bz = -2; bz <= 2; ++bz)
    for (int by = -4; by <= 3; ++by)
      for (int bx = -4; bx <= 3; ++bx) {
        bool any = false;
        const int b[3] = {bx, by, bz};
        for (int lin = 0; lin < 4096; ++lin) {
          const int v[3] = {lin & 15, (lin >> 4) & 15, lin >> 8};
          double q[3];
          for (int k = 0; k < 3; ++k) q[k] = static_cast<float>(b[k]) * bs + (static_cast<float>(v[k]) + 0.5f) * kVoxel;
          const double p[3] = {c * q[0] - s * q[1] + pose[0], s * q[0] + c * q[1] + pose[1], q[2] + pose[2]};
          const double d = roomDistance(p);
          const bool obs = std::fabs(d) <= band;
          const float df = static_cast<float>(std::max(-kTruncation, std::min(kTruncation, d)));
          std::memcpy(&block[3 * lin], &df, 4);
          block[3 * lin + 1] = obs ? w_bits : 0u;
          block[3 * lin + 2] = 0u;
          any = any || obs;
        }
        if (!any) continue;
        idx.insert(idx.end(), b, b + 3);
        words.insert(words.end(), block.begin(), block.end());
      }
  check(cox_layer_upload(layer->handle(), idx.data(), words.data(), idx.size() / 3, 0), "uploadRoom");
}

static bool withinOneStep(const double pose[4], const double truth[4], const double final_step[4]) {
  for (int k = 0; k < 4; ++k) {
    const double d = k == 3 ? normalizeAngle(pose[k] - truth[k]) : pose[k] - truth[k];
    if (!(std::fabs(d) <= final_step[k])) return false;
  }
  return true;
}

int main() {
  const double T_B_A[4] = {0.7, -0.5, 0.2, 2.2};  // where A sits in B: what the search has to find
  const double origin[4] = {0.0, 0.0, 0.0, 0.0};
  VoxgraphSubmap::Config sm_cfg;
  sm_cfg.tsdf_voxel_size = kVoxel;
  sm_cfg.capacity_blocks = 256;
  sm_cfg.esdf.max_distance_m = sm_cfg.esdf.default_distance_m = 2.0f;
  VoxgraphSubmap a(Transformation(), 0, sm_cfg), b(Transformation(), 1, sm_cfg);
  uploadRoom(T_B_A, a.getTsdfMapPtr()->getTsdfLayerPtr());
  uploadRoom(origin, b.getTsdfMapPtr()->getTsdfLayerPtr());
  a.finishSubmap();
  b.finishSubmap();
  const std::shared_ptr<RegistrationPointSet> pts = a.getRegistrationPoints(RegistrationPointType::kIsosurfacePoints);
  std::printf("submaps: %zu and %zu blocks, %zu isosurface points in A\n", a.getTsdfMap().getTsdfLayer().getNumberOfAllocatedBlocks(),
              b.getTsdfMap().getTsdfLayer().getNumberOfAllocatedBlocks(), static_cast<size_t>(pts->size()));
  if (pts->size() < 1000) return 10;

  SubmapAligner::SearchConfig cfg;
  const double half[4] = {1.2, 1.2, 0.4, 170.0 * M_PI / 180.0};
  for (int k = 0; k < 4; ++k) cfg.half_extent[k] = half[k];
  cfg.use_esdf_distance = false;
  double final_step[4];
  for (int k = 0; k < 4; ++k) final_step[k] = cfg.step[k] / 16.0;

  // ---- the class itself: grid, sweep, select, search with its trace ----
  SubmapAligner aligner(pts->handle(), b.getReadingLayer(false));
  const std::vector<double> grid = SubmapAligner::grid(cfg.center, cfg.half_extent, cfg.step);
  if (grid.size() != 4u * 7 * 7 * 3 * 35) return 11;
  const std::vector<cox_align_score> scores = aligner.sweep(grid, origin);
  const uint32_t min_corr = static_cast<uint32_t>(pts->size() / 4);
  const std::vector<uint32_t> kept = SubmapAligner::select(scores, min_corr, 8);
  if (kept.size() != 8 || scores[kept[0]].score < scores[kept[1]].score || scores[kept[0]].n_corr < min_corr) return 12;
  cox_align_search_config sc = cfg;
  sc.min_corr = min_corr;
  std::vector<cox_align_level> trace;
  const std::vector<SubmapAligner::Candidate> found = aligner.search(sc, origin, &trace);
  if (found.size() != 8 || trace.size() != 5 || trace[0].n_candidates != grid.size() / 4 || trace[4].n_candidates != 648) return 13;
  for (int j = 0; j < 8; ++j)
    if (trace[0].kept_index[j] != kept[j]) return 14;  // level 0 of the search is the sweep + select above
  std::printf("search: best %.5f %.5f %.5f %.5f (truth %.5f %.5f %.5f %.5f), score %llu, %u of %zu inliers, cost %.6g\n", found[0].pose[0], found[0].pose[1],
              found[0].pose[2], found[0].pose[3], T_B_A[0], T_B_A[1], T_B_A[2], T_B_A[3], static_cast<unsigned long long>(found[0].score.score), found[0].score.n_inlier,
              static_cast<size_t>(pts->size()), found[0].score.cost);
  if (!withinOneStep(found[0].pose, T_B_A, final_step)) return 15;
  uint64_t sweeps = 0;
  if (!(aligner.kernelTimeMs(&sweeps) > 0.0) || sweeps != 6) return 16;

  // ---- proposeLoopClosure, and the pose graph taking its result ----
  Transformation T_A_B;
  SubmapAligner::Candidate best;
  if (!proposeLoopClosure(a, b, cfg, &T_A_B, &best)) return 20;
  if (std::memcmp(best.pose, found[0].pose, sizeof(best.pose)) != 0 || std::memcmp(&best.score, &found[0].score, sizeof(best.score)) != 0) return 21;
  double back[4], want[4];
  pose4FromTransformation(inverse(T_A_B), back);  // T_B_A again, through the float transformation
  if (!withinOneStep(back, T_B_A, final_step)) return 22;
  inversePose4(best.pose, want);
  PoseGraphInterface pg;
  pg.addSubmap(0, Pose4(), 0);
  pg.addSubmap(1, Pose4(), 1);
  if (!pg.addLoopClosureMeasurement(static_cast<SubmapID>(0), static_cast<SubmapID>(1), T_A_B, false)) return 23;
  pg.optimize(false);
  const Pose4 p1 = pg.getPoseMap().at(1);
  std::printf("pose graph: submap 1 at %.5f %.5f %.5f %.5f after the loop closure (T_A_B %.5f %.5f %.5f %.5f)\n", p1.v[0], p1.v[1], p1.v[2], p1.v[3], want[0], want[1],
              want[2], want[3]);
  for (int k = 0; k < 4; ++k)
    if (std::fabs(k == 3 ? normalizeAngle(p1.v[k] - want[k]) : p1.v[k] - want[k]) > 2e-3) return 24;
  // nobody can have more correspondences than points: nothing is proposed, T_A_B stays
  SubmapAligner::SearchConfig none = cfg;
  none.min_corr = static_cast<uint32_t>(pts->size()) + 1;
  Transformation untouched;
  untouched.t[0] = 42.0f;
  if (proposeLoopClosure(a, b, none, &untouched) || untouched.t[0] != 42.0f) return 25;
  // against B's ESDF, voxgraph's default reading (reported, not judged: the rule was tried on the TSDF)
  SubmapAligner::SearchConfig esdf = cfg;
  esdf.use_esdf_distance = true;
  if (!proposeLoopClosure(a, b, esdf, nullptr, &best)) return 26;
  std::printf("against the ESDF: best %.5f %.5f %.5f %.5f, %u inliers\n", best.pose[0], best.pose[1], best.pose[2], best.pose[3], best.score.n_inlier);
  std::printf("align smoke ok\n");
  return 0;
}
