// coxgraph_amd/csrc/cox_plan.hpp without a GPU: whole IntegratorPlans for given (method, configuration, voxel size, environment).
// The expected plans are written down from the decisions cox_integrator_create made before the plan existed (its defaults, clamps
// and treatment of malformed values), not from resolve_plan's output.
//   plan_smoke             checks everything, exit code 0 = all good
//   plan_smoke --switches  prints the switch table, one name per line (tests/test_plan_cpu.py compares it with DESIGN.md)
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "../../coxgraph_amd/csrc/cox_plan.hpp"

using namespace cox_plan;
typedef std::map<std::string, std::string> Env;

static int g_failures = 0;
static std::map<std::string, int> g_lookups;

static IntegratorPlan resolve(int method, double voxel, const Env& env, bool anti_grazing = false) {
  // synth.integrator_overrides(voxel): the reference's yaml values per voxel size
  cox_tsdf_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  const bool v10 = voxel > 0.07, v5 = !v10 && voxel > 0.03, v2 = !v10 && !v5 && voxel > 0.015;
  cfg.default_truncation_distance = v10 ? 0.30f : v5 ? 0.15f : v2 ? 0.06f : 0.03f;
  cfg.max_ray_length_m = v10 ? 10.0f : v5 ? 6.0f : 3.0f;
  cfg.enable_anti_grazing = anti_grazing ? 1 : 0;
  g_lookups.clear();
  return resolve_plan(method, cfg, static_cast<float>(voxel), [&](const char* name) -> const char* {
    g_lookups[name] += 1;
    const auto it = env.find(name);
    return it == env.end() ? nullptr : it->second.c_str();
  });
}

// the plan of an integrator created with an empty environment, as far as it does not depend on method or voxel size
static IntegratorPlan base(uint32_t steps_max, const int (&map)[6], bool alt) {
  IntegratorPlan p;
  p.layer_update = LayerUpdate::RecordTiles;
  p.steps_max = steps_max;
  p.small_axis_cap = (steps_max - 1) / 3 + 2 <= 128;
  p.bucket_partition = p.small_axis_cap;
  p.tile_shift = 8;
  p.wave_apply = p.split_big_tiles = true;
  p.big_chunk = 4096;
  p.wave_tile_max = 512;
  p.grid_apply = 8192;
  p.grid_apply_wave = 2048;
  p.grid_merge = 4096;
  p.grid_touch = 2048;
  for (int k = 0; k < 6; ++k) p.stage_stream[k] = map[k];
  p.alt_raygen_stream = alt;
  p.input_stream = true;
  p.n_streams = map[5] + 1 + (alt ? 1 : 0) + 1;
  p.use_graphs = false;
  p.submit_thread = true;
  p.copy_threads = 3;
  p.h2d_kernel = false;
  p.h2d_groups = 8;
  p.depth_convert_on_input_stream = false;
  p.timeline = "";
  p.debug = false;
  p.fast = FastPlan{3, 2, 8u, 16u, 128u, 1, false};
  return p;
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
  // every switch of the table is looked up, once, and nothing else is
  if (g_lookups.size() != static_cast<size_t>(kNumSwitches)) { std::printf("FAIL %s: %zu names looked up\n", what.c_str(), g_lookups.size()); ++g_failures; }
  for (int k = 0; k < kNumSwitches; ++k)
    if (g_lookups[kSwitchNames[k]] != 1) { std::printf("FAIL %s: %s looked up %d times\n", what.c_str(), kSwitchNames[k], g_lookups[kSwitchNames[k]]); ++g_failures; }
}

static const int kParity[6] = {0, 0, 0, 1, 1, 2}, kHeavy[6] = {0, 0, 0, 1, 2, 3}, kFast[6] = {0, 1, 1, 2, 2, 2}, kTwo[6] = {0, 0, 0, 1, 1, 1},
                 kStaged[6] = {0, 0, 1, 2, 2, 3}, kSix[6] = {0, 1, 2, 3, 4, 5}, kOne[6] = {0, 0, 0, 0, 0, 0};
static const double kVoxels[4] = {0.10, 0.05, 0.02, 0.01};
// 3 * (floor((max_ray + truncation) / voxel) + 3) + 1 with the float values widened to double: 105, 125, 156, 306 planes per axis
static const uint32_t kStepsMax[4] = {316, 376, 469, 919};
static uint32_t steps_of(double voxel) { return voxel > 0.07 ? 316 : voxel > 0.03 ? 376 : voxel > 0.015 ? 469 : 919; }
// merged without anti-grazing and no switch: record tiles + buckets + parity map where per_axis + 2 <= 128, expanded pieces + H P M | T | R | U beyond
static IntegratorPlan merged_default(double voxel) {
  const bool small = voxel > 0.03;
  IntegratorPlan p = base(steps_of(voxel), small ? kParity : kHeavy, small);
  if (!small) p.layer_update = LayerUpdate::PiecesExpand;
  return p;
}
static std::string tag(const char* what, double voxel, const Env& env) {
  std::string s = std::string(what) + " @" + std::to_string(voxel);
  for (const auto& kv : env) s += " " + kv.first + "=" + kv.second;
  return s;
}

static void defaults() {
  for (int i = 0; i < 4; ++i) {
    const double vx = kVoxels[i];
    const bool small = i < 2;
    if (steps_of(vx) != kStepsMax[i]) ++g_failures;
    check(tag("simple", vx, {}), resolve(COX_METHOD_SIMPLE, vx, {}), base(kStepsMax[i], kParity, true));
    check(tag("merged", vx, {}), resolve(COX_METHOD_MERGED, vx, {}), merged_default(vx));
    IntegratorPlan ag = base(kStepsMax[i], kParity, true);  // anti-grazing reads the bundle hash per step: never pieces
    check(tag("merged anti-grazing", vx, {}), resolve(COX_METHOD_MERGED, vx, {}, true), ag);
    IntegratorPlan f = base(kStepsMax[i], kFast, false);
    f.fast.rounds = small ? 2 : 8;
    f.fast.cap0 = small ? 8 : i == 2 ? 16 : 32;
    f.fast.cap1 = small ? 16 : 32;
    check(tag("fast", vx, {}), resolve(COX_METHOD_FAST, vx, {}), f);
  }
}

// tests/test_gpu_fusion.py::test_alternative_layer_update_paths_are_bit_identical (merged at 10, 5 and 2 cm)
static void layer_update_switches() {
  for (double vx : {0.10, 0.05, 0.02}) {
    const bool small = vx > 0.03;
    auto run = [&](const Env& env, const IntegratorPlan& want) { check(tag("merged", vx, env), resolve(COX_METHOD_MERGED, vx, env), want); };
    IntegratorPlan tiles = base(steps_of(vx), kParity, true), pieces = base(steps_of(vx), kHeavy, false);
    pieces.layer_update = LayerUpdate::PiecesExpand;
    IntegratorPlan p = tiles;
    p.layer_update = LayerUpdate::PiecesApply;
    run({{"COX_APPLY", "pieces"}}, p);
    p.layer_update = LayerUpdate::RecordsFullSort;
    run({{"COX_APPLY", "records"}}, p);
    run({{"COX_PARTITION", "records"}}, tiles);
    p = tiles;
    p.bucket_partition = true;
    run({{"COX_PARTITION", "records"}, {"COX_BUCKETS", "1"}}, p);
    run({{"COX_PARTITION", "pieces"}}, pieces);
    p = small ? tiles : pieces;
    p.bucket_partition = false;
    run({{"COX_BUCKETS", "0"}}, p);
    p = pieces;
    p.big_chunk = 1024;
    run({{"COX_PARTITION", "pieces"}, {"COX_BIG_CHUNK", "1024"}}, p);
    p.wave_tile_max = 256;
    run({{"COX_PARTITION", "pieces"}, {"COX_BIG_CHUNK", "1024"}, {"COX_WAVE_TILE_MAX", "256"}}, p);
    p = pieces;
    p.split_big_tiles = false;
    run({{"COX_PARTITION", "pieces"}, {"COX_SPLIT_TILES", "0"}}, p);
    p = pieces;
    p.wave_apply = false;
    run({{"COX_PARTITION", "pieces"}, {"COX_APPLY_WAVE", "0"}}, p);
  }
}

// tests/test_gpu_fusion.py::test_pipeline_configurations_give_the_same_layer (merged and simple at 5 cm)
static void pipeline_switches() {
  for (int method : {COX_METHOD_MERGED, COX_METHOD_SIMPLE}) {
    const bool merged = method == COX_METHOD_MERGED;
    auto run = [&](const Env& env, const IntegratorPlan& want) { check(tag(merged ? "merged" : "simple", 0.05, env), resolve(method, 0.05, env), want); };
    const IntegratorPlan dflt = base(376, kParity, true);
    run({{"COX_STREAMS", "2"}}, base(376, kTwo, false));
    run({{"COX_STREAMS", "4s"}}, base(376, kStaged, false));
    run({{"COX_STREAMS", "3p"}}, base(376, kTwo, true));
    run({{"COX_STREAMS", "6"}}, base(376, kSix, false));
    IntegratorPlan p = dflt;
    p.submit_thread = false;
    run({{"COX_SUBMIT_THREAD", "0"}}, p);
    p = base(376, kSix, false);
    p.submit_thread = false;
    run({{"COX_STREAMS", "6"}, {"COX_SUBMIT_THREAD", "0"}}, p);
    p = dflt;
    p.use_graphs = true;
    run({{"COX_GRAPH", "1"}}, p);
    const int custom[6] = {0, 0, 1, 2, 3, 4};
    run({{"COX_STREAM_MAP", "001234"}}, base(376, custom, false));
    p = dflt;
    if (merged) p.tile_shift = 9;  // (COX_TILE and COX_PARTITION are the merged integrator's)
    run({{"COX_TILE", "9"}}, p);
    p = merged ? base(376, kHeavy, false) : dflt;
    if (merged) p.layer_update = LayerUpdate::PiecesExpand;
    run({{"COX_PARTITION", "pieces"}}, p);
    if (merged) p.tile_shift = 9;
    run({{"COX_TILE", "9"}, {"COX_PARTITION", "pieces"}}, p);
  }
}

// test_fast_relaxation_on_the_device_and_its_sequential_fallback and test_async_host_entry_equals_the_synchronous_one (5 cm)
static void fast_and_host_input_switches() {
  auto run = [&](const Env& env, const IntegratorPlan& want) { check(tag("fast", 0.05, env), resolve(COX_METHOD_FAST, 0.05, env), want); };
  const IntegratorPlan dflt = base(376, kFast, false);
  IntegratorPlan p = dflt;
  p.fast.force_sequential = true;
  run({{"COX_FAST_SEQUENTIAL", "1"}}, p);
  p = dflt;
  p.fast.cap1 = 8;
  run({{"COX_FAST_CAP", "8,8"}}, p);
  p.fast.cap0 = 16;
  p.fast.cap1 = 32;
  run({{"COX_FAST_CAP", "16,32"}}, p);
  p.fast.cap0 = 32;
  run({{"COX_FAST_CAP", "32,32"}}, p);
  p = base(376, kOne, false);
  p.fast.streams = 1;
  run({{"COX_FAST_STREAMS", "1"}}, p);
  p = dflt;
  p.submit_thread = false;
  run({{"COX_SUBMIT_THREAD", "0"}}, p);
  for (int method : {COX_METHOD_MERGED, COX_METHOD_FAST, COX_METHOD_SIMPLE}) {
    const IntegratorPlan d = method == COX_METHOD_FAST ? dflt : base(376, kParity, true);
    auto runm = [&](const Env& env, const IntegratorPlan& want) { check(tag("host inputs", 0.05 + method, env), resolve(method, 0.05, env), want); };
    p = d;
    p.input_stream = false;
    p.n_streams -= 1;
    runm({{"COX_INPUT_STREAM", "0"}}, p);
    p = d;
    p.h2d_kernel = true;
    runm({{"COX_H2D", "kernel"}}, p);
    p = d;
    p.copy_threads = 0;
    runm({{"COX_COPY_THREADS", "0"}}, p);
  }
}

static void malformed_and_clamped() {
  auto merged = [&](double vx, const Env& env, const IntegratorPlan& want, bool ag = false) {
    check(tag(ag ? "merged anti-grazing" : "merged", vx, env), resolve(COX_METHOD_MERGED, vx, env, ag), want);
  };
  auto fast = [&](const Env& env, const IntegratorPlan& want) { check(tag("fast", 0.05, env), resolve(COX_METHOD_FAST, 0.05, env), want); };
  const IntegratorPlan d5 = base(376, kParity, true), f5 = base(376, kFast, false);
  merged(0.05, {{"COX_STREAMS", "5"}}, d5);
  IntegratorPlan p = base(469, kParity, true);  // ... but it counts as a choice: no H P M | T | R | U at 2 cm
  p.layer_update = LayerUpdate::PiecesExpand;
  merged(0.02, {{"COX_STREAMS", "5"}}, p);
  merged(0.05, {{"COX_WAVE_TILE_MAX", "300"}}, d5);
  // a stream map that is not six digits starting at 0 and non-decreasing by at most one is rejected -- the staged map is what is left
  for (const char* bad : {"123456", "002345", "00123", "0012345", "00012a", "010123", ""}) merged(0.05, {{"COX_STREAM_MAP", bad}}, base(376, kStaged, false));
  fast({{"COX_STREAM_MAP", "001234"}}, f5);
  for (const char* same : {"0", "40,40", "8,64", "x"}) fast({{"COX_FAST_CAP", same}}, f5);
  p = f5;
  p.fast.cap0 = p.fast.cap1 = 16;
  fast({{"COX_FAST_CAP", "16"}}, p);
  fast({{"COX_FAST_CAP", "16,8"}}, p);
  p = d5;
  merged(0.05, {{"COX_GRAPH", "1"}, {"COX_NO_GRAPH", "1"}}, p);
  merged(0.05, {{"COX_NO_GRAPH", "1"}}, p);
  // COX_PARTITION / COX_TILE: merged without anti-grazing and without a COX_APPLY path only
  merged(0.05, {{"COX_PARTITION", "pieces"}, {"COX_TILE", "9"}}, d5, true);
  merged(0.05, {{"COX_APPLY", "pieces"}}, d5, true);
  p = d5;
  p.layer_update = LayerUpdate::RecordsFullSort;
  merged(0.05, {{"COX_APPLY", "records"}, {"COX_PARTITION", "pieces"}, {"COX_TILE", "9"}}, p);
  merged(0.05, {{"COX_APPLY", "records"}}, p, true);
  merged(0.05, {{"COX_TILE", "7"}}, d5);
  p = f5;
  p.fast.rounds = 8;
  fast({{"COX_FAST_ROUNDS", "20"}}, p);
  p = f5;
  p.fast.relax_groups = 8;
  fast({{"COX_FAST_ROUNDS", "1"}, {"COX_FAST_GROUPS", "4"}}, p);
  p.fast.relax_groups = 256;
  p.fast.fences = 0;
  fast({{"COX_FAST_GROUPS", "1000"}, {"COX_FAST_FENCE", "0"}}, p);
  p = d5;
  p.big_chunk = 1024;
  p.grid_apply = 1;
  p.grid_apply_wave = 8;
  p.grid_merge = 7;
  p.grid_touch = 1;
  p.h2d_groups = 1;
  p.copy_threads = 15;
  merged(0.05, {{"COX_BIG_CHUNK", "100"}, {"COX_GRID_APPLY", "0"}, {"COX_GRID_APPLY_WAVE", "1"}, {"COX_GRID_MERGE", "7"}, {"COX_GRID_TOUCH", "-2"},
                {"COX_H2D_GROUPS", "0"}, {"COX_COPY_THREADS", "99"}, {"COX_H2D", "dma"}, {"COX_DEPTH_CONVERT", "frame"}}, p);
  p = d5;
  p.copy_threads = 0;
  p.depth_convert_on_input_stream = true;
  p.timeline = "/tmp/timeline.txt";
  p.debug = true;
  merged(0.05, {{"COX_COPY_THREADS", "-3"}, {"COX_DEPTH_CONVERT", "input"}, {"COX_TIMELINE", "/tmp/timeline.txt"}, {"COX_DEBUG", "1"}, {"COX_INPUT_STREAM", "1"}}, p);
}

static void predicates() {
  IntegratorPlan p;
  p.tile_shift = 9;
  p.bucket_partition = true;
  const LayerUpdate all[4] = {LayerUpdate::RecordsFullSort, LayerUpdate::RecordTiles, LayerUpdate::PiecesExpand, LayerUpdate::PiecesApply};
  const bool walks[4] = {false, false, true, true}, tiles[4] = {false, true, true, false};
  const int flags[4] = {0, 9 | 256, 0, 0}, passes[4] = {3, 1, 1, 1};
  for (int k = 0; k < 4; ++k) {
    p.layer_update = all[k];
    if (p.walks_pieces() != walks[k] || p.tile_apply() != tiles[k] || p.expands_pieces() != (k == 2) || p.emit_flags() != flags[k] || p.record_sort_passes() != passes[k]) {
      std::printf("FAIL predicates of layer update %d\n", k);
      ++g_failures;
    }
  }
  p.layer_update = LayerUpdate::RecordTiles;
  p.bucket_partition = false;
  if (p.emit_flags() != 9 || p.record_sort_passes() != 2) ++g_failures;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--switches") == 0) {
    for (int k = 0; k < kNumSwitches; ++k) std::printf("%s\n", kSwitchNames[k]);
    return 0;
  }
  defaults();
  layer_update_switches();
  pipeline_switches();
  fast_and_host_input_switches();
  malformed_and_clamped();
  predicates();
  std::printf("%s (%d failures)\n", g_failures ? "FAILED" : "ok", g_failures);
  return g_failures ? 1 : 0;
}
