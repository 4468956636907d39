// The queue budget of coxgraph_amd/csrc/cox_plan.hpp without a GPU: whole IntegratorPlans of simple / merged / fast at 10, 5, 2 and
// 1 cm for budgets of 1, 2, 3, 4, 5, 8 and 16 hardware queues and for no budget at all.  The expected stream maps are written down
// here from the rule (the null stream keeps one queue, the engine's streams fit into the others: first the input stream goes, then
// the map steps down), not taken from resolve_plan's output.  Exit code 0 = all good.
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
  // synth.integrator_overrides(voxel): the reference's yaml values per voxel size
  cox_tsdf_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  const bool v10 = voxel > 0.07, v5 = !v10 && voxel > 0.03, v2 = !v10 && !v5 && voxel > 0.015;
  cfg.default_truncation_distance = v10 ? 0.30f : v5 ? 0.15f : v2 ? 0.06f : 0.03f;
  cfg.max_ray_length_m = v10 ? 10.0f : v5 ? 6.0f : 3.0f;
  return cfg;
}
static IntegratorPlan resolve(int method, double voxel, const Env& env, int budget = kNotGiven) {
  const cox_tsdf_config cfg = config_of(voxel);
  auto lookup = [&](const char* name) -> const char* {
    const auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  };
  if (budget == kNotGiven) return resolve_plan(method, cfg, static_cast<float>(voxel), lookup);  // the call tests/cpp/plan_smoke.cpp makes
  return resolve_plan(method, cfg, static_cast<float>(voxel), lookup, budget);
}

#define FIELD(f) \
  if (!(got.f == want.f)) { std::printf("FAIL %s: " #f "\n", what.c_str()); ++g_failures; }
static void check(const std::string& what, const IntegratorPlan& got, const IntegratorPlan& want) {
  FIELD(layer_update) FIELD(bucket_partition) FIELD(tile_shift) FIELD(wave_apply) FIELD(split_big_tiles) FIELD(big_chunk) FIELD(wave_tile_max)
  FIELD(grid_apply) FIELD(grid_apply_wave) FIELD(grid_merge) FIELD(grid_touch) FIELD(steps_max) FIELD(small_axis_cap)
  for (int k = 0; k < 6; ++k) FIELD(stage_stream[k])
  FIELD(alt_raygen_stream) FIELD(input_stream) FIELD(n_streams) FIELD(use_graphs) FIELD(submit_thread) FIELD(copy_threads) FIELD(h2d_kernel)
  FIELD(h2d_groups) FIELD(depth_convert_on_input_stream) FIELD(timeline) FIELD(debug)
  FIELD(fast.streams) FIELD(fast.rounds) FIELD(fast.cap0) FIELD(fast.cap1) FIELD(fast.relax_groups) FIELD(fast.fences) FIELD(fast.force_sequential)
}

static const int kParity[6] = {0, 0, 0, 1, 1, 2}, kHeavy[6] = {0, 0, 0, 1, 2, 3}, kFast[6] = {0, 1, 1, 2, 2, 2}, kTwo[6] = {0, 0, 0, 1, 1, 1},
                 kStaged[6] = {0, 0, 1, 2, 2, 3}, kSix[6] = {0, 1, 2, 3, 4, 5}, kOne[6] = {0, 0, 0, 0, 0, 0};
static const int kMethods[3] = {COX_METHOD_SIMPLE, COX_METHOD_MERGED, COX_METHOD_FAST};
static const double kVoxels[4] = {0.10, 0.05, 0.02, 0.01};
static const int kBudgets[8] = {1, 2, 3, 4, 5, 8, 16, kNotGiven};

static std::string tag(int method, double voxel, int budget, const Env& env = {}) {
  std::string s = std::string(method == COX_METHOD_SIMPLE ? "simple" : method == COX_METHOD_MERGED ? "merged" : "fast") + " @" + std::to_string(voxel) +
                  " budget " + (budget == kNotGiven ? std::string("-") : std::to_string(budget));
  for (const auto& kv : env) s += " " + kv.first + "=" + kv.second;
  return s;
}
// `base` with other streams: everything but the stream fields (and fast's stream count) is left alone by the budget
static IntegratorPlan with_streams(IntegratorPlan base, const int (&map)[6], bool alt, bool input) {
  for (int k = 0; k < 6; ++k) base.stage_stream[k] = map[k];
  base.alt_raygen_stream = alt;
  base.input_stream = input;
  base.n_streams = map[5] + 1 + (alt ? 1 : 0) + (input ? 1 : 0);
  return base;
}

// Today's streams: simple, and merged where no ray crosses more than 126 planes of an axis (10 and 5 cm): H P M x2 | T R | U + input = 5;
// merged with expanded pieces (2 and 1 cm): H P M | T | R | U + input = 5; fast: front | solve | update + input = 4.  With the null
// stream they need 6, 6 and 5 queues.
static IntegratorPlan expected(int method, double voxel, int budget) {
  const IntegratorPlan today = resolve(method, voxel, {});
  const bool ample = budget == kNotGiven;
  if (method == COX_METHOD_FAST) {
    if (ample || budget >= 5) return with_streams(today, kFast, false, true);
    if (budget == 4) return with_streams(today, kFast, false, false);
    IntegratorPlan p = with_streams(today, kOne, false, false);  // three stage streams or one: nothing in between
    p.fast.streams = 1;
    return p;
  }
  const bool heavy = method == COX_METHOD_MERGED && voxel < 0.03;
  if (heavy) {
    if (ample || budget >= 6) return with_streams(today, kHeavy, false, true);
    if (budget == 5) return with_streams(today, kHeavy, false, false);
    if (budget == 4) return with_streams(today, kParity, false, false);
    if (budget == 3) return with_streams(today, kTwo, false, false);
    return with_streams(today, kOne, false, false);
  }
  if (ample || budget >= 6) return with_streams(today, kParity, true, true);
  if (budget == 5) return with_streams(today, kParity, true, false);
  if (budget == 4) return with_streams(today, kTwo, true, false);  // the two ray-generation lanes + one layer-update stream
  if (budget == 3) return with_streams(today, kTwo, false, false);
  return with_streams(today, kOne, false, false);
}

static void budgets() {
  for (int method : kMethods)
    for (double vx : kVoxels) {
      const IntegratorPlan today = resolve(method, vx, {});
      // today's plans, as tests/cpp/plan_smoke.cpp pins them field by field: only the stream shape is restated here
      const bool heavy = method == COX_METHOD_MERGED && vx < 0.03, fast = method == COX_METHOD_FAST;
      check(tag(method, vx, kNotGiven) + " (today)", today, with_streams(today, fast ? kFast : heavy ? kHeavy : kParity, !fast && !heavy, true));
      check(tag(method, vx, 16) + " = today", resolve(method, vx, {}, 16), today);
      check(tag(method, vx, kAmpleQueues) + " = today", resolve(method, vx, {}, kAmpleQueues), today);
      for (int b : kBudgets) {
        const IntegratorPlan got = resolve(method, vx, {}, b);
        check(tag(method, vx, b), got, expected(method, vx, b));
        // no more streams than the budget leaves beside the null stream's queue -- one stream is the least there is
        const int room = b == kNotGiven ? 1000 : b > 1 ? b - 1 : 1;
        int distinct = got.stage_stream[5] + 1 + (got.alt_raygen_stream ? 1 : 0) + (got.input_stream ? 1 : 0);
        if (got.n_streams != distinct || got.n_streams > room) {
          std::printf("FAIL %s: %d streams (%d counted) for %d queues\n", tag(method, vx, b).c_str(), got.n_streams, distinct, b);
          ++g_failures;
        }
        for (int k = 0; k < 6; ++k)
          if (got.stage_stream[k] < 0 || (k > 0 && (got.stage_stream[k] < got.stage_stream[k - 1] || got.stage_stream[k] > got.stage_stream[k - 1] + 1))) ++g_failures;
        // COX_QUEUES is the argument, whatever the argument says
        if (b != kNotGiven) {
          const Env q = {{"COX_QUEUES", std::to_string(b)}};
          for (int other : {kNotGiven, 1, 4, 16}) check(tag(method, vx, other, q), resolve(method, vx, q, other), got);
        }
      }
      // malformed values fall back to the argument
      for (const char* bad : {"", "0", "-3", "abc", "999", "4x", "65"})
        for (int b : {kNotGiven, 4, 2}) check(tag(method, vx, b, {{"COX_QUEUES", bad}}), resolve(method, vx, {{"COX_QUEUES", bad}}, b), resolve(method, vx, {}, b));
      check(tag(method, vx, 2, {{"COX_QUEUES", "64"}}), resolve(method, vx, {{"COX_QUEUES", "64"}}, 2), today);
    }
}

// what a switch chose stays whatever the budget: the map (COX_STREAMS, COX_STREAM_MAP; COX_FAST_STREAMS for fast), the input stream
static void explicit_switches_win() {
  for (int b : kBudgets) {
    for (int method : {COX_METHOD_MERGED, COX_METHOD_SIMPLE})
      for (double vx : kVoxels) {
        const bool tight = b != kNotGiven;
        auto run = [&](const Env& env, const int (&map)[6], bool alt, bool input) {
          IntegratorPlan want = with_streams(resolve(method, vx, env), map, alt, input);  // (the layer update may depend on the switch: taken from the plan without a budget)
          check(tag(method, vx, b, env), resolve(method, vx, env, b), want);
        };
        // the map is kept; the input stream, not asked for, goes where map + input + null stream exceed the budget
        run({{"COX_STREAMS", "2"}}, kTwo, false, !tight || b >= 4);
        run({{"COX_STREAMS", "3p"}}, kTwo, true, !tight || b >= 5);
        run({{"COX_STREAMS", "4s"}}, kStaged, false, !tight || b >= 6);
        run({{"COX_STREAMS", "6"}}, kSix, false, !tight || b >= 8);
        run({{"COX_STREAM_MAP", "000000"}}, kOne, false, !tight || b >= 3);
        run({{"COX_STREAMS", "6"}, {"COX_INPUT_STREAM", "1"}}, kSix, false, true);
        run({{"COX_STREAMS", "3p"}, {"COX_INPUT_STREAM", "0"}}, kTwo, true, false);
        run({{"COX_STREAM_MAP", "001234"}, {"COX_INPUT_STREAM", "1"}}, {0, 0, 1, 2, 3, 4}, false, true);
      }
    // the input stream is kept (or stays away) and the map makes room: H P M x2 | T R | U -> H P M x2 | T R U -> H P M | T R U -> one
    for (int method : {COX_METHOD_MERGED, COX_METHOD_SIMPLE}) {
      const IntegratorPlan today = resolve(method, 0.05, {});
      const Env on = {{"COX_INPUT_STREAM", "1"}}, off = {{"COX_INPUT_STREAM", "0"}};
      const bool ample = b == kNotGiven;
      check(tag(method, 0.05, b, on), resolve(method, 0.05, on, b),
            ample || b >= 6 ? with_streams(today, kParity, true, true) : b == 5 ? with_streams(today, kTwo, true, true) : b == 4 ? with_streams(today, kTwo, false, true)
                                                                                                                                   : with_streams(today, kOne, false, true));
      check(tag(method, 0.05, b, off), resolve(method, 0.05, off, b),
            ample || b >= 5 ? with_streams(today, kParity, true, false) : b == 4 ? with_streams(today, kTwo, true, false) : b == 3 ? with_streams(today, kTwo, false, false)
                                                                                                                                    : with_streams(today, kOne, false, false));
    }
    {
      const IntegratorPlan today = resolve(COX_METHOD_FAST, 0.05, {});
      const bool tight = b != kNotGiven;
      IntegratorPlan one = with_streams(today, kOne, false, !tight || b >= 3);
      one.fast.streams = 1;
      check(tag(COX_METHOD_FAST, 0.05, b, {{"COX_FAST_STREAMS", "1"}}), resolve(COX_METHOD_FAST, 0.05, {{"COX_FAST_STREAMS", "1"}}, b), one);
      check(tag(COX_METHOD_FAST, 0.05, b, {{"COX_FAST_STREAMS", "3"}}), resolve(COX_METHOD_FAST, 0.05, {{"COX_FAST_STREAMS", "3"}}, b),
            with_streams(today, kFast, false, !tight || b >= 5));
      // COX_STREAMS / COX_STREAM_MAP are not fast's: no choice of its map
      check(tag(COX_METHOD_FAST, 0.05, b, {{"COX_STREAMS", "6"}}), resolve(COX_METHOD_FAST, 0.05, {{"COX_STREAMS", "6"}}, b), resolve(COX_METHOD_FAST, 0.05, {}, b));
    }
  }
}

// stage graphs are captured on the live streams and keep the streams they were tested with, whatever the budget; vetoed, the budget holds
static void graphs_keep_their_streams() {
  for (int method : kMethods)
    for (double vx : kVoxels)
      for (int b : kBudgets) {
        const Env on = {{"COX_GRAPH", "1"}}, vetoed = {{"COX_GRAPH", "1"}, {"COX_NO_GRAPH", "1"}};
        check(tag(method, vx, b, on), resolve(method, vx, on, b), resolve(method, vx, on));
        check(tag(method, vx, b, vetoed), resolve(method, vx, vetoed, b), expected(method, vx, b));
        if (!resolve(method, vx, on, b).use_graphs || resolve(method, vx, vetoed, b).use_graphs) ++g_failures;
      }
}

int main() {
  budgets();
  explicit_switches_win();
  graphs_keep_their_streams();
  std::printf("%s (%d failures)\n", g_failures ? "FAILED" : "ok", g_failures);
  return g_failures ? 1 : 0;
}
