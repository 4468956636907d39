// VoxbloxMap and RRTStarCollision of coxgraph_amd/host/coxgraph_hip_planning.hpp on a small hand-built ESDF (the wall field
// d = 4 - x over 3 x 1 x 1 blocks of 0.1 m voxels), against the C ABI of include/coxgraph_hip_collide.h called by hand:
//   isTraversable / isObserved of single points and of a batch, adjustGoalPositions against cox_collide_segments, and
//   recheckCollision of a small tree against cox_collide_trajectories + the rule keep = feasible && keep[parent].
// Exit code 0 = all good; 77 = no GPU (the constructors fail with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_planning.hpp"

using namespace coxgraph_hip;

static Point P(float x) { return Point{{x, 0.75f, 0.75f}}; }

static bool sameRecord(const cox_collide_record& a, const cox_collide_record& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main() {
  if (cox_device_count() == 0) {
    try {
      TsdfLayer layer(0.10f);
    } catch (const std::runtime_error& e) {
      std::printf("no GPU: %s\n", e.what());
      return 77;
    }
    return 1;
  }
  // the wall: block (bx, 0, 0), voxel (x, y, z) holds 4 - centre.x, weight 1
  TsdfLayer layer(0.10f, 16, 0, 16);
  std::vector<int32_t> idx;
  std::vector<uint32_t> words;
  for (int bx = 0; bx < 3; ++bx) {
    idx.push_back(bx), idx.push_back(0), idx.push_back(0);
    for (int v = 0; v < 4096; ++v) {
      const float d = 4.0f - (static_cast<float>(bx) * 1.6f + (static_cast<float>(v & 15) + 0.5f) * 0.1f);
      const float w = 1.0f;
      uint32_t dw, ww;
      std::memcpy(&dw, &d, 4);
      std::memcpy(&ww, &w, 4);
      words.push_back(dw), words.push_back(ww), words.push_back(0u);
    }
  }
  check(cox_layer_upload(layer.handle(), idx.data(), words.data(), 3, 0), "upload");

  SystemConstraints constraints;
  if (constraints.v_max != 1.0f || constraints.collision_radius != 2.0f) return 10;
  constraints.collision_radius = 0.5f;
  VoxbloxMap map(layer.handle(), constraints);
  // free, blocked (d = 0.375), observed without a trilinear cell (half a voxel from the layer's end), unallocated
  if (!map.isTraversable(P(1.125f)) || map.isTraversable(P(3.625f)) || map.isTraversable(P(0.02f)) || map.isTraversable(P(5.0f))) return 11;
  if (!map.isObserved(P(1.125f)) || !map.isObserved(P(3.625f)) || !map.isObserved(P(0.02f)) || map.isObserved(P(5.0f))) return 12;
  const std::vector<Point> batch = {P(1.125f), P(3.625f), P(0.02f), P(5.0f), Point{{NAN, 0.0f, 0.0f}}};
  const std::vector<bool> trav = map.isTraversable(batch), obs = map.isObserved(batch);
  const bool want_t[5] = {true, false, false, false, false}, want_o[5] = {true, true, true, false, false};
  for (int i = 0; i < 5; ++i)
    if (trav[i] != want_t[i] || obs[i] != want_o[i]) return 13;
  if (map.states(batch)[4] != COX_C_INVALID || !map.isTraversable(std::vector<Point>()).empty()) return 14;

  RRTStarCollision::Config cfg;
  if (cfg.crop_margin != 0.3f || cfg.crop_min_length != 0.5f || cfg.max_extension_range != 1.5f || cfg.sampling_rate != 20.0f || !cfg.crop_segments) return 20;
  RRTStarCollision rrt(layer.handle(), constraints, cfg);
  // free; blocked from x = 3.5 on with room for a cropped goal; blocked at once; cut to 1.5 m and free
  const std::vector<Point> starts = {P(1.0f), P(2.52f), P(3.6f), P(0.5f)}, goals = {P(2.2f), P(3.92f), P(4.5f), P(3.0f)};
  std::vector<bool> success;
  const std::vector<Point> adjusted = rrt.adjustGoalPositions(starts, goals, &success);
  const std::vector<bool> connected = rrt.connectPoses(starts, goals);
  // the same through the C ABI by hand
  cox_collide_config c;
  cox_collide_config_default(&c);
  c.collision_radius = 0.5f;
  cox_collide_t* h = nullptr;
  check(cox_collide_create(layer.handle(), &c, &h), "cox_collide_create");
  std::vector<cox_collide_record> rec(4);
  check(cox_collide_segments(h, starts[0].data(), goals[0].data(), 4, rec.data()), "cox_collide_segments");
  const std::vector<cox_collide_record> rec2 = rrt.checkSegments(starts, goals);
  for (int i = 0; i < 4; ++i) {
    std::printf("segment %d: n %u first_blocked %u flags %u free_length %.4f goal %.4f\n", i, rec[i].n_samples, rec[i].first_blocked, rec[i].flags,
                rec[i].free_length, rec[i].goal[0]);
    if (!sameRecord(rec[i], rec2[i])) return 21;
    if (connected[i] != ((rec[i].flags & COX_SEG_FEASIBLE) != 0) || success[i] != ((rec[i].flags & COX_SEG_GOAL) != 0)) return 22;
    if (success[i] && std::memcmp(adjusted[i].data(), rec[i].goal, 12) != 0) return 23;
    if (!success[i] && !std::isnan(adjusted[i][0])) return 24;
  }
  if (!connected[0] || connected[1] || connected[2] || !connected[3]) return 25;
  if (!success[0] || !success[1] || success[2] || !success[3]) return 26;
  // Segment 1 is 1.4 m long in n intervals (28 or 29: 1.4 / 0.05 sits on the rounding of ceilf), sample i at x_i = 2.52 + 1.4 i / n.
  // The wall blocks from x = 3.5 on: first_blocked is the first sample beyond it, and the goal lies crop_margin before the sample
  // in front of that one.
  {
    const double n = rec[1].n_samples, fb = rec[1].first_blocked;
    if (n != 28.0 && n != 29.0) return 27;
    const double x_fb = 2.52 + 1.4 * fb / n, x_before = 2.52 + 1.4 * (fb - 1.0) / n;
    if (!(x_fb > 3.5 + 1e-3) || !(x_before < 3.5 - 1e-3)) return 27;
    if (std::fabs(adjusted[1][0] - (x_before - 0.3)) > 1e-5 || std::fabs(adjusted[0][0] - 2.2f) > 1e-5f) return 27;
  }
  if ((rec[3].flags & COX_SEG_CLAMPED) == 0 || std::fabs(adjusted[3][0] - 2.0f) > 1e-5f) return 28;

  // a tree of stored trajectories: 0 root, 1 and 2 under 0, 3 under 2, 4 under 3, 5 under 1; segment 2 runs into the wall
  RRTStarCollision::Tree tree;
  const float from[6] = {1.0f, 1.5f, 1.5f, 3.7f, 2.0f, 2.0f}, to[6] = {1.5f, 2.0f, 3.7f, 2.0f, 2.5f, 1.0f};
  const int32_t parent[6] = {-1, 0, 0, 2, 3, 1};
  for (int s = 0; s < 6; ++s) {
    std::vector<Point> traj;
    for (int i = 0; i <= 20; ++i) traj.push_back(P(from[s] + (to[s] - from[s]) * static_cast<float>(i) / 20.0f));
    tree.addSegment(parent[s], s == 5 ? std::vector<Point>() : traj);  // an empty trajectory is feasible
  }
  std::vector<cox_collide_record> tree_rec;
  const std::vector<uint8_t> keep = rrt.recheckCollision(tree, &tree_rec);
  std::vector<cox_collide_record> traj_rec(6);
  check(cox_collide_trajectories(h, tree.offsets.data(), 6, tree.points[0].data(), tree.points.size(), traj_rec.data()), "cox_collide_trajectories");
  for (int s = 0; s < 6; ++s) {
    if (!sameRecord(tree_rec[s], traj_rec[s])) return 30;
    bool want = (traj_rec[s].flags & COX_SEG_FEASIBLE) != 0;
    for (int j = parent[s]; want && j >= 0; j = parent[j]) want = (traj_rec[j].flags & COX_SEG_FEASIBLE) != 0;
    if (keep[s] != (want ? COX_TREE_KEEP : 0)) return 31;
  }
  const uint8_t want_keep[6] = {1, 1, 0, 0, 0, 1};
  if (std::memcmp(keep.data(), want_keep, 6) != 0) return 32;
  if (rrt.recheckCollision(tree) != keep || !rrt.recheckCollision(RRTStarCollision::Tree()).empty()) return 33;
  // the clearing sphere follows the robot: unallocated space next to it becomes traversable
  RRTStarCollision::Config clearing;
  clearing.clearing_radius = 1.0f;
  RRTStarCollision rrt2(layer.handle(), constraints, clearing);
  rrt2.setRobotPosition(Point{{1.0f, -0.5f, 0.75f}});
  const std::vector<Point> s2 = {Point{{1.0f, -0.6f, 0.75f}}}, g2 = {Point{{1.0f, 0.77f, 0.75f}}};
  if (rrt.connectPoses(s2, g2)[0]) return 40;
  // (within half a voxel of the layer's face the sample is observed without a distance: still blocked)
  if (rrt2.connectPoses(s2, g2)[0]) return 41;
  const std::vector<Point> g3 = {Point{{1.0f, -0.1f, 0.75f}}};
  if (!rrt2.connectPoses(s2, g3)[0] || rrt.connectPoses(s2, g3)[0]) return 42;
  cox_collide_stats_t st;
  check(cox_collide_stats(rrt.handle(), &st, 0), "cox_collide_stats");
  if (st.n_samples_evaluated == 0 || st.n_launches == 0) return 50;
  // a configuration the engine refuses
  RRTStarCollision::Config bad;
  bad.crop_margin = -1.0f;
  try {
    RRTStarCollision nope(layer.handle(), constraints, bad);
    return 51;
  } catch (const std::runtime_error&) {
  }
  cox_collide_destroy(h);
  std::printf("collide smoke ok: %llu samples evaluated, %llu skipped, %llu launches\n", static_cast<unsigned long long>(st.n_samples_evaluated),
              static_cast<unsigned long long>(st.n_samples_skipped), static_cast<unsigned long long>(st.n_launches));
  return 0;
}
