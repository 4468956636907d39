// Who walks a ray of the merged record walk (IntegratorPlan::touch_in_merge, COX_TOUCH) without a GPU: every (method, voxel size,
// queue budget).  The expectation is written down here from the rule -- the bundle merge walks exactly where the walk is on the
// ray-generation lanes (walk_on_raygen) AND no ray can outgrow the small parallel DDA (small_axis_cap), which with the reference's ray
// lengths is `merged` at 10 and 5 cm -- not taken from resolve_plan's output.  COX_TOUCH=merge|kernel wins over the rule where both
// hold and changes nothing elsewhere; the switch changes no other field of the plan.  Exit code 0 = all good.
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../coxgraph_amd/csrc/cox_plan.hpp"

using namespace cox_plan;
typedef std::map<std::string, std::string> Env;

static int g_failures = 0;
static const int kNotGiven = -1;

static cox_tsdf_config config_of(double voxel) {
  cox_tsdf_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  const bool v10 = voxel > 0.07, v5 = !v10 && voxel > 0.03, v2 = !v10 && !v5 && voxel > 0.015;
  cfg.default_truncation_distance = v10 ? 0.30f : v5 ? 0.15f : v2 ? 0.06f : 0.03f;
  cfg.max_ray_length_m = v10 ? 10.0f : v5 ? 6.0f : 3.0f;
  return cfg;
}
static IntegratorPlan resolve(int method, double voxel, const Env& env, int budget) {
  const cox_tsdf_config cfg = config_of(voxel);
  auto lookup = [&](const char* name) -> const char* {
    const auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  };
  if (budget == kNotGiven) return resolve_plan(method, cfg, static_cast<float>(voxel), lookup);
  return resolve_plan(method, cfg, static_cast<float>(voxel), lookup, budget);
}
static Env with(Env env, const char* name, const char* value) {
  env[name] = value;
  return env;
}
static std::string tag(int method, double voxel, int budget, const Env& env) {
  std::string s = std::string(method == COX_METHOD_SIMPLE ? "simple" : method == COX_METHOD_MERGED ? "merged" : "fast") + " @" + std::to_string(voxel) +
                  " budget " + (budget == kNotGiven ? std::string("-") : std::to_string(budget));
  for (const auto& kv : env) s += " " + kv.first + "=" + kv.second;
  return s;
}
static void expect(const std::string& what, bool got, bool want) {
  if (got != want) {
    std::printf("FAIL %s: touch_in_merge %d, expected %d\n", what.c_str(), got ? 1 : 0, want ? 1 : 0);
    ++g_failures;
  }
}
#define FIELD(f) \
  if (!(a.f == b.f)) { std::printf("FAIL %s: " #f " changes with COX_TOUCH\n", what.c_str()); ++g_failures; }
static void same_but_touch(const std::string& what, const IntegratorPlan& a, const IntegratorPlan& b) {
  FIELD(layer_update) FIELD(bucket_partition) FIELD(tile_shift) FIELD(wave_apply) FIELD(split_big_tiles) FIELD(big_chunk) FIELD(wave_tile_max)
  FIELD(grid_apply) FIELD(grid_apply_wave) FIELD(grid_merge) FIELD(grid_touch) FIELD(steps_max) FIELD(small_axis_cap) FIELD(record_cap)
  for (int k = 0; k < 6; ++k) FIELD(stage_stream[k])
  FIELD(alt_raygen_stream) FIELD(input_stream) FIELD(n_streams) FIELD(walk_on_raygen) FIELD(use_graphs) FIELD(submit_thread) FIELD(copy_threads)
  FIELD(h2d_kernel) FIELD(h2d_groups) FIELD(depth_convert_on_input_stream) FIELD(timeline) FIELD(debug)
  FIELD(fast.streams) FIELD(fast.rounds) FIELD(fast.cap0) FIELD(fast.cap1) FIELD(fast.relax_groups) FIELD(fast.fences) FIELD(fast.force_sequential)
}

static const int kMethods[3] = {COX_METHOD_SIMPLE, COX_METHOD_MERGED, COX_METHOD_FAST};
static const double kVoxels[4] = {0.10, 0.05, 0.02, 0.01};
static const int kBudgets[8] = {1, 2, 3, 4, 5, 8, 16, kNotGiven};

int main() {
  for (int method : kMethods)
    for (double vx : kVoxels)
      for (int b : kBudgets) {
        const bool merged = method == COX_METHOD_MERGED, coarse = vx > 0.03;
        // the default plans: the walk is on the lanes for merged at 10 and 5 cm on four queues, and those voxel sizes have the small cap
        expect(tag(method, vx, b, {}), resolve(method, vx, {}, b).touch_in_merge, merged && coarse && b == 4);
        const Env envs[] = {{}, {{"COX_WALK", "raygen"}}, {{"COX_WALK", "update"}}, {{"COX_WALK", "raygen"}, {"COX_PARTITION", "records"}},
                            {{"COX_WALK", "raygen"}, {"COX_APPLY", "records"}}, {{"COX_WALK", "raygen"}, {"COX_SUBMIT_THREAD", "0"}},
                            {{"COX_WALK", "raygen"}, {"COX_GRAPH", "1"}}, {{"COX_STREAMS", "3p"}, {"COX_PARTITION", "records"}}, {{"COX_STREAMS", "2"}},
                            {{"COX_WALK", "raygen"}, {"COX_RECORD_CAP", "100000"}}};
        for (const Env& env : envs) {
          const IntegratorPlan base = resolve(method, vx, env, b);
          // the rule, from the two fields it is made of (the walk's own placement is pinned by plan_walk_smoke.cpp) ...
          const bool allowed = base.walk_on_raygen && base.small_axis_cap;
          expect(tag(method, vx, b, env), base.touch_in_merge, allowed);
          // ... and the small cap from the voxel size: the 2 and 1 cm configurations cross more than 126 planes of an axis
          if (base.small_axis_cap != coarse) {
            std::printf("FAIL %s: small_axis_cap %d\n", tag(method, vx, b, env).c_str(), base.small_axis_cap ? 1 : 0);
            ++g_failures;
          }
          if (base.touch_in_merge && !(merged && coarse && !base.use_graphs)) {
            std::printf("FAIL %s: touch_in_merge outside merged record walks at 10 / 5 cm\n", tag(method, vx, b, env).c_str());
            ++g_failures;
          }
          const IntegratorPlan on = resolve(method, vx, with(env, "COX_TOUCH", "merge"), b), off = resolve(method, vx, with(env, "COX_TOUCH", "kernel"), b);
          expect(tag(method, vx, b, with(env, "COX_TOUCH", "merge")), on.touch_in_merge, allowed);
          expect(tag(method, vx, b, with(env, "COX_TOUCH", "kernel")), off.touch_in_merge, false);
          same_but_touch(tag(method, vx, b, with(env, "COX_TOUCH", "merge")), on, base);
          same_but_touch(tag(method, vx, b, with(env, "COX_TOUCH", "kernel")), off, base);
          // anything else is no choice: the rule holds
          expect(tag(method, vx, b, with(env, "COX_TOUCH", "lane")), resolve(method, vx, with(env, "COX_TOUCH", "lane"), b).touch_in_merge, allowed);
        }
        // chosen by hand at every budget: the walk on the lanes of a merged record walk has the merge walk at 10 and 5 cm only
        expect(tag(method, vx, b, {{"COX_WALK", "raygen"}, {"COX_PARTITION", "records"}}),
               resolve(method, vx, {{"COX_WALK", "raygen"}, {"COX_PARTITION", "records"}}, b).touch_in_merge, merged && coarse);
        expect(tag(method, vx, b, {{"COX_WALK", "update"}, {"COX_TOUCH", "merge"}}),
               resolve(method, vx, {{"COX_WALK", "update"}, {"COX_TOUCH", "merge"}}, b).touch_in_merge, false);
      }
  std::printf("%s (%d failures)\n", g_failures ? "FAILED" : "ok", g_failures);
  return g_failures ? 1 : 0;
}
