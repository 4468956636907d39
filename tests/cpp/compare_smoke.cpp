// Layer comparison from C++ (coxgraph_amd/host/coxgraph_hip_compare.hpp) on the GPU: evaluateLayersRmse on two plane layers whose
// distances differ by a dyadic delta everywhere (rmse = delta, voxblox's counts, the error layer), and SubmapConsistency +
// verifyLoopClosure on the analytic room with two candidates, of which the second is the true pose.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../coxgraph_amd/host/coxgraph_hip_compare.hpp"

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

static uint32_t bits(float v) {
  uint32_t w;
  std::memcpy(&w, &v, 4);
  return w;
}

// the room as a TSDF in a frame that sits at `pose` (x, y, z, yaw) in the room's frame: every voxel within truncation + one
// voxel of a surface is observed with weight 2
static void uploadRoom(const double pose[4], TsdfLayer* layer) {
  const float bs = kVoxel * 16.0f;
  const double c = std::cos(pose[3]), s = std::sin(pose[3]), band = kTruncation + kVoxel;
  std::vector<int32_t> idx;
  std::vector<uint32_t> words, block(4096 * 3);
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
          block[3 * lin] = bits(static_cast<float>(std::max(-kTruncation, std::min(kTruncation, d))));
          block[3 * lin + 1] = obs ? bits(2.0f) : 0u;
          block[3 * lin + 2] = 0u;
          any = any || obs;
        }
        if (!any) continue;
        idx.insert(idx.end(), b, b + 3);
        words.insert(words.end(), block.begin(), block.end());
      }
  check(cox_layer_upload(layer->handle(), idx.data(), words.data(), idx.size() / 3, 0), "uploadRoom");
}

// 2 x 2 x 2 blocks at 0.1 m holding the plane z = 0.25 rounded to multiples of 2^-6, plus shift: adding a dyadic shift is exact
static void uploadPlane(float shift, TsdfLayer* layer) {
  std::vector<int32_t> idx;
  std::vector<uint32_t> words;
  for (int bz = -1; bz <= 0; ++bz)
    for (int by = -1; by <= 0; ++by)
      for (int bx = -1; bx <= 0; ++bx) {
        const int b[3] = {bx, by, bz};
        idx.insert(idx.end(), b, b + 3);
        for (int lin = 0; lin < 4096; ++lin) {
          const double z = (16.0 * bz + (lin >> 8) + 0.5) * 0.1;
          const float base = static_cast<float>(std::round((z - 0.25) * 64.0) / 64.0);
          words.push_back(bits(base + shift));
          words.push_back(bits(1.0f));
          words.push_back(0u);
        }
      }
  check(cox_layer_upload(layer->handle(), idx.data(), words.data(), idx.size() / 3, 0), "uploadPlane");
}

int main() {
  // ---- evaluateLayersRmse on the plane pair ----
  const float delta = 0.0625f;
  TsdfLayer test(0.1f, 16, 0, 64), gt(0.1f, 16, 0, 64);
  uploadPlane(delta, &test);
  uploadPlane(0.0f, &gt);
  VoxelEvaluationDetails details;
  std::shared_ptr<LayerHandle> error_layer;
  const double rmse = evaluateLayersRmse(test, gt, VoxelEvaluationMode::kEvaluateAllVoxels, &details, &error_layer);
  std::printf("plane pair: %s\n", details.toString().c_str());
  const size_t n = 8u * 4096u;
  if (std::fabs(rmse - delta) > 1e-15 || details.rmse != rmse) return 10;
  if (details.num_evaluated_voxels != n || details.num_overlapping_voxels != n || details.num_ignored_voxels != 0 || details.num_non_overlapping_voxels != 0) return 11;
  if (details.min_error != delta || details.max_error != delta) return 12;
  uint64_t nb = 0;
  check(cox_layer_stats(error_layer->handle(), &nb, nullptr), "error layer");
  if (nb != 8) return 13;
  std::vector<int32_t> eidx(3 * nb);
  std::vector<uint32_t> ewords(nb * 12288);
  check(cox_layer_download(error_layer->handle(), eidx.data(), ewords.data(), nb, &nb), "error layer download");
  for (size_t v = 0; v < n; ++v)
    if (ewords[3 * v] != bits(delta) || ewords[3 * v + 1] != bits(1.0f) || (ewords[3 * v + 2] & COX_COMPARE_CLASS_MASK) != COX_COMPARE_CLASS_EVALUATED) return 14;
  // behind the test surface (dA < 0) nothing is evaluated: voxblox's counts move from evaluated to ignored
  VoxelEvaluationDetails behind;
  evaluateLayersRmse(test, gt, VoxelEvaluationMode::kIgnoreErrorBehindTestSurface, &behind);
  if (behind.num_ignored_voxels == 0 || behind.num_ignored_voxels + behind.num_evaluated_voxels != n || behind.rmse != rmse) return 15;
  // a test layer with one block more than the ground truth: its voxels do not overlap
  {
    const int32_t extra[3] = {5, 5, 5};
    std::vector<uint32_t> w(12288, 0u);
    for (int lin = 0; lin < 4096; ++lin) w[3 * lin + 1] = bits(1.0f);
    check(cox_layer_upload(test.handle(), extra, w.data(), 1, 0), "extra block");
    VoxelEvaluationDetails more;
    evaluateLayersRmse(test, gt, VoxelEvaluationMode::kEvaluateAllVoxels, &more);
    if (more.num_non_overlapping_voxels != 4096 || more.num_overlapping_voxels != n || more.rmse != rmse) return 16;
  }

  // ---- SubmapConsistency and verifyLoopClosure on the room ----
  const double T_B_A[4] = {0.7, -0.5, 0.2, 2.2};  // where A sits in B
  const double origin[4] = {0.0, 0.0, 0.0, 0.0};
  VoxgraphSubmap::Config sm_cfg;
  sm_cfg.tsdf_voxel_size = kVoxel;
  sm_cfg.capacity_blocks = 256;
  VoxgraphSubmap a(Transformation(), 0, sm_cfg), b(Transformation(), 1, sm_cfg);
  uploadRoom(T_B_A, a.getTsdfMapPtr()->getTsdfLayerPtr());
  uploadRoom(origin, b.getTsdfMapPtr()->getTsdfLayerPtr());
  std::vector<SubmapAligner::Candidate> candidates(2);
  std::memset(candidates.data(), 0, sizeof(SubmapAligner::Candidate) * 2);
  for (int k = 0; k < 4; ++k) candidates[0].pose[k] = candidates[1].pose[k] = T_B_A[k];
  candidates[0].pose[0] += 0.6;  // a wrong candidate first: what a self-similar wall lets score well
  const std::vector<SubmapConsistency::Report> reports = SubmapConsistency::check(a, b, candidates);
  if (reports.size() != 2) return 20;
  for (size_t i = 0; i < 2; ++i)
    std::printf("candidate %zu: overlap %llu, conflicts %llu + %llu of %llu near a surface (ratio %.4f), agree ratio %.4f, rmse %.4f m\n", i,
                static_cast<unsigned long long>(reports[i].stats.n_overlap), static_cast<unsigned long long>(reports[i].stats.n_a_surface_in_b_free),
                static_cast<unsigned long long>(reports[i].stats.n_b_surface_in_a_free), static_cast<unsigned long long>(reports[i].stats.n_near_a + reports[i].stats.n_near_b),
                reports[i].conflict_ratio, reports[i].agree_ratio, reports[i].rmse);
  if (!(reports[1].conflict_ratio < reports[0].conflict_ratio) || !(reports[1].agree_ratio > reports[0].agree_ratio) || !(reports[1].rmse < reports[0].rmse)) return 21;
  if (reports[1].stats.n_overlap < 10000) return 22;
  // the relative transformation is the candidate's pose over B at the origin, and composes in double
  const Transformation want = transformationFromPose4(T_B_A);
  if (std::memcmp(&reports[1].T_B_A, &want, sizeof(want)) != 0) return 23;
  const double pa[4] = {1.0, 2.0, 0.5, 0.3}, pb[4] = {1.0, 2.0, 0.5, 0.3};
  const Transformation same = SubmapConsistency::relativeTransformation(pa, pb);
  if (same.q[0] != 1.0f || same.q[3] != 0.0f || same.t[0] != 0.0f || same.t[1] != 0.0f || same.t[2] != 0.0f) return 24;
  // the caller's thresholds: here, halfway between what the two candidates show
  const LoopClosureCriteria criteria(10000, 0.5 * (reports[0].conflict_ratio + reports[1].conflict_ratio), 0.5 * (reports[0].agree_ratio + reports[1].agree_ratio));
  Transformation T_A_B;
  std::vector<SubmapConsistency::Report> again;
  const int chosen = verifyLoopClosure(a, b, candidates, criteria, &T_A_B, &again);
  if (chosen != 1 || again.size() != 2 || std::memcmp(&again[1].stats, &reports[1].stats, sizeof(cox_compare_stats)) != 0) return 25;
  const Transformation round_trip = inverse(T_A_B);
  for (int k = 0; k < 3; ++k)
    if (std::fabs(round_trip.t[k] - want.t[k]) > 1e-5) return 26;
  const LoopClosureCriteria nobody(1u << 30, 0.0, 1.0);
  Transformation untouched;
  untouched.t[0] = 42.0f;
  if (verifyLoopClosure(a, b, candidates, nobody, &untouched) != -1 || untouched.t[0] != 42.0f) return 27;
  if (verifyLoopClosure(a, b, std::vector<SubmapAligner::Candidate>(), criteria) != -1) return 28;
  std::printf("compare smoke ok\n");
  return 0;
}
