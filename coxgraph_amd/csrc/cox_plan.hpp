// Everything the ray-casting integrators (simple, merged, fast) decide when they are created and never change afterwards, resolved
// ONCE by a pure function of (method, configuration, voxel size, environment, hardware queues).  Host-only C++17, no HIP: tests/cpp/plan_smoke.cpp
// builds it with a plain compiler and checks whole plans, so "which stream map / which layer-update path do I get at 2 cm with
// COX_STREAMS=3p" has an answer without a GPU.  cox_integrator.hip hands the process environment to resolve_plan and reads nothing else.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/coxgraph_hip.h"

namespace cox_plan {

// Every environment switch the integrator honours (DESIGN.md section 5 documents exactly these); each is looked up once.
#define COX_PLAN_SWITCHES(X)                                                                                                                   \
  X(APPLY) X(APPLY_WAVE) X(BIG_CHUNK) X(BUCKETS) X(COPY_THREADS) X(DEBUG) X(DEPTH_CONVERT) X(FAST_CAP) X(FAST_FENCE) X(FAST_GROUPS)             \
  X(FAST_ROUNDS) X(FAST_SEQUENTIAL) X(FAST_STREAMS) X(GRAPH) X(GRID_APPLY) X(GRID_APPLY_WAVE) X(GRID_MERGE) X(GRID_TOUCH) X(H2D) X(H2D_GROUPS) \
  X(INPUT_STREAM) X(NO_GRAPH) X(PARTITION) X(QUEUES) X(RECORD_CAP) X(SPLIT_TILES) X(STREAMS) X(STREAM_MAP) X(SUBMIT_THREAD) X(TILE) X(TIMELINE) X(TOUCH) X(WALK) \
  X(WAVE_TILE_MAX)
#define COX_PLAN_ENUM(n) k##n,
#define COX_PLAN_NAME(n) "COX_" #n,
enum Switch { COX_PLAN_SWITCHES(COX_PLAN_ENUM) kNumSwitches };
constexpr const char* kSwitchNames[kNumSwitches] = {COX_PLAN_SWITCHES(COX_PLAN_NAME)};
#undef COX_PLAN_ENUM
#undef COX_PLAN_NAME

// constants the decisions depend on; cox_integrator.hip asserts that they are the kernels' own
constexpr uint32_t kAxisCapSmall = 128;  // per-axis crossing capacity of the small parallel DDA (cox_walk.hpp)
constexpr uint32_t kTileShift = 8, kBigChunk = 4096, kBigChunkMin = 1024;  // cox_apply_tile.hpp
constexpr int kFastMaxRounds = 8;
constexpr uint32_t kFastCap0Max = 32, kFastShortMax = 32, kFastRelaxGroups = 128;  // cox_fast.hpp
constexpr int kCopyGroups = 8;                                                     // cox_frontend.hpp
constexpr int kAmpleQueues = 0;      // resolve_plan's queue budget when the caller does not give one: every stream has a queue of its own
constexpr int kMaxQueueBudget = 64;  // COX_QUEUES above this is malformed
constexpr int kNumStages = 6;  // H bundle hash | P bundling sort | M bundle boundaries + means | T offsets, touch, emit | R record partition | U apply

// The four implementations of the layer-update half (stages T, R, U) of a frame:
enum class LayerUpdate {
  RecordsFullSort,  // full stable sort of the records by voxel id + per-record kernels (k_apply_eval / k_apply_long); COX_APPLY=records
  RecordTiles,      // records partitioned by tile (one bucket pass, or the whole tile id in two) + k_apply_block
  PiecesExpand,     // the walk leaves pieces, sorted by tile and expanded into records for the tile apply (fine voxels)
  PiecesApply,      // pieces applied directly, no records (k_apply_pieces); COX_APPLY=pieces
};

struct FastPlan {
  int streams = 3;  // front / solve / update on three streams, or all on one
  int rounds = 2;   // rounds of list growth + relaxation enqueued per frame
  uint32_t cap0 = 8, cap1 = 16;  // candidate steps per ray in round 0; list length of the rays that did not get their whole walk in round 1
  uint32_t relax_groups = kFastRelaxGroups;  // workgroups of the relaxation (all resident at once)
  int fences = 1;                            // release / acquire fences in the relaxation's barrier (experiments)
  bool force_sequential = false;             // every frame is redone by k_fast_sequential (tests)
};

struct IntegratorPlan {
  // ---- layer update
  LayerUpdate layer_update = LayerUpdate::RecordTiles;
  bool bucket_partition = true;     // RecordTiles: ONE pass by tile id & 4095 (coarse voxels: few touched blocks); else the whole tile id
  uint32_t tile_shift = kTileShift;  // log2(voxels per tile) of the tile apply: 8 (one z slab of a block) or 9
  bool wave_apply = true;           // PiecesExpand: a wave per small tile (k_apply_wave) beside the workgroup per tile
  bool split_big_tiles = true;      // PiecesExpand: the largest tiles classified chunk by chunk by the whole chip
  uint32_t big_chunk = kBigChunk, wave_tile_max = 512;
  uint32_t grid_apply = 8192, grid_apply_wave = 2048, grid_merge = 4096, grid_touch = 2048;  // grid-stride kernels: any size is correct
  uint32_t steps_max = 0;       // upper bound of a ray's step count (ray_length_in_steps + 1) for this configuration
  bool small_axis_cap = false;  // no ray can cross more than kAxisCapSmall - 2 planes of one axis
  uint32_t record_cap = 0;      // records a frame may have at most (tests: COX_RECORD_CAP); 0 = the worst case of the point capacity, which no frame exceeds
  // ---- streams, in creation order: the input stream, the alternate ray-generation stream, the stage streams back to back
  int stage_stream[kNumStages] = {0, 0, 0, 1, 1, 2};  // stage -> stage stream; equal streams are adjacent
  bool alt_raygen_stream = false;  // stages H, P, M of the odd frame slots run on a stream of their own
  bool input_stream = true;        // host inputs are staged on a stream of their own
  int n_streams = 0;               // distinct streams in all
  bool walk_on_raygen = false;     // merged record walk (k_touch_wave, k_emit_wave) at the tail of stage M, on the frame's ray-generation stream;
                                   // stage T is then the binding of the frame's blocks to the layer alone
  bool touch_in_merge = false;     // walk_on_raygen with the small axis cap: the walk of a ray (k_touch_wave's work) is done by the bundle merge, on the wave
                                   // that has just produced the ray, and parked in a slot of steps_max words per ray; k_touch_wave is not launched
  // ---- host side
  bool use_graphs = false;     // stages replayed as captured HIP graphs
  bool submit_thread = true;   // stages T, R, U enqueued by a thread of the integrator's own
  int copy_threads = 3;        // helpers beside the caller for the bounce copy of pageable inputs
  bool h2d_kernel = false;     // pinned inputs read by a copy kernel of h2d_groups workgroups instead of the copy engine
  int h2d_groups = kCopyGroups;
  bool depth_convert_on_input_stream = false;
  std::string timeline;        // file the timed regions are dumped to while profiling is on (empty: none)
  bool debug = false;
  FastPlan fast;

  bool walks_pieces() const { return layer_update == LayerUpdate::PiecesExpand || layer_update == LayerUpdate::PiecesApply; }
  bool tile_apply() const { return layer_update == LayerUpdate::RecordTiles || layer_update == LayerUpdate::PiecesExpand; }
  bool expands_pieces() const { return layer_update == LayerUpdate::PiecesExpand; }
  int n_stage_streams() const { return stage_stream[kNumStages - 1] + 1; }
  // what the emit kernels are told about the record partition: the tile shift, bit 8 = buckets; 0 = full sort
  int emit_flags() const { return layer_update == LayerUpdate::RecordTiles ? static_cast<int>(tile_shift | (bucket_partition ? 256u : 0u)) : 0; }
  // sort passes (12-bit digits) the record partition enqueues
  int record_sort_passes() const { return layer_update == LayerUpdate::RecordsFullSort ? 3 : bucket_partition ? 1 : 2; }
};

// upper bound of ray_length_in_steps + 1 for any ray this configuration can cast
inline uint32_t max_steps_per_ray(const cox_tsdf_config& cfg, float voxel_size) {
  const double reach = static_cast<double>(cfg.max_ray_length_m) + static_cast<double>(cfg.default_truncation_distance);
  const double per_axis = std::floor(reach / static_cast<double>(voxel_size)) + 3.0;
  return static_cast<uint32_t>(std::min(3.0 * per_axis + 1.0, 1.0e6));
}

// env: anything callable as const char*(const char*) -- the process environment in the engine, a map in the tests.
// hw_queues: the hardware queues the process has (GPU_MAX_HW_QUEUES; the engine asks cox_internal_hw_queues()), kAmpleQueues when
// every stream may be taken to have a queue of its own.  COX_QUEUES=<n> replaces it.
template <typename Lookup>
IntegratorPlan resolve_plan(int method, const cox_tsdf_config& cfg, float voxel_size, Lookup env, int hw_queues = kAmpleQueues) {
  const char* v[kNumSwitches];
  for (int k = 0; k < kNumSwitches; ++k) v[k] = env(kSwitchNames[k]);
  auto is = [&](Switch s, const char* word) { return v[s] && std::strcmp(v[s], word) == 0; };
  auto num = [&](Switch s) { return std::atoi(v[s]); };
  const bool merged = method == COX_METHOD_MERGED, fast = method == COX_METHOD_FAST;

  IntegratorPlan p;
  p.steps_max = max_steps_per_ray(cfg, voxel_size);
  p.small_axis_cap = (p.steps_max - 1) / 3 + 2 <= kAxisCapSmall;  // steps_max = 3 * (planes per axis bound) + 1

  // ---- layer update.  Tiles by default; pieces where rays are long in voxels (the large-LDS walk: 2 cm and finer with the reference's
  // ray lengths -- 1 cm 513 -> 699 frames/s, 2 cm 2 071 -> 2 159; records otherwise: 5 cm 7 129 vs 5 323, the extra launches cost more
  // than the smaller sort saves at 4 * 10^5 records per frame).  COX_APPLY=pieces is bit-identical and in the parity tests but never the
  // default: the piece sort is 2.3x cheaper than the record sort at 1 cm, the piece apply 1.75x dearer than the record apply.
  // Buckets where a frame touches few blocks (coarse voxels: a bucket is a tile, or a few); where rays are long in voxels a frame
  // touches 10^3-10^4 blocks and the tiles of a bucket would each re-read the whole bucket, so the whole tile id is sorted there.
  const bool may_walk_pieces = merged && !cfg.enable_anti_grazing;  // anti-grazing reads the bundle hash per step: records only
  p.bucket_partition = v[kBUCKETS] ? num(kBUCKETS) != 0 : p.small_axis_cap;
  if (is(kAPPLY, "records")) {
    p.layer_update = LayerUpdate::RecordsFullSort;
  } else if (may_walk_pieces && is(kAPPLY, "pieces")) {
    p.layer_update = LayerUpdate::PiecesApply;
  } else if (may_walk_pieces) {  // (COX_PARTITION / COX_TILE are honoured here only)
    const bool pieces = v[kPARTITION] ? is(kPARTITION, "pieces") : !p.small_axis_cap;
    p.layer_update = pieces ? LayerUpdate::PiecesExpand : LayerUpdate::RecordTiles;
    // COX_TILE=9: tiles of two z slabs (512 voxels).  Half as many tiles did not help at fine voxels: the tile apply is bound by its
    // per-record work, not by the round trips per tile.
    if (v[kTILE]) p.tile_shift = num(kTILE) == 9 ? 9u : 8u;
  }
  // COX_RECORD_CAP=<n> (tests): record buffers of n records instead of the worst case, so that a frame can overflow them and be
  // dropped as a whole (kErrRecords) without a cloud of millions of points.  Record walks of simple and merged only.
  if (v[kRECORD_CAP] && !fast && !p.walks_pieces() && num(kRECORD_CAP) > 0) p.record_cap = static_cast<uint32_t>(num(kRECORD_CAP));
  if (v[kAPPLY_WAVE]) p.wave_apply = num(kAPPLY_WAVE) != 0;
  if (v[kSPLIT_TILES]) p.split_big_tiles = num(kSPLIT_TILES) != 0;
  if (v[kBIG_CHUNK]) p.big_chunk = static_cast<uint32_t>(std::max<int>(kBigChunkMin, num(kBIG_CHUNK)));
  if (v[kWAVE_TILE_MAX]) p.wave_tile_max = num(kWAVE_TILE_MAX) == 256 ? 256u : 512u;
  if (v[kGRID_APPLY]) p.grid_apply = static_cast<uint32_t>(std::max(1, num(kGRID_APPLY)));
  if (v[kGRID_APPLY_WAVE]) p.grid_apply_wave = static_cast<uint32_t>(std::max(8, num(kGRID_APPLY_WAVE)));
  if (v[kGRID_MERGE]) p.grid_merge = static_cast<uint32_t>(std::max(1, num(kGRID_MERGE)));
  if (v[kGRID_TOUCH]) p.grid_touch = static_cast<uint32_t>(std::max(1, num(kGRID_TOUCH)));

  // ---- stage -> stream.  A frame's stream is a chain of small kernels with a few microseconds between them, and the frame rate at
  // 5 cm is the length of the longest chain.  Frames/s at 5 / 2 / 1 cm: two streams 5 747 / - / -; four staged
  // 7 636 / 2 128 / 506; six 4 202 / 1 949 / 531 -- past four the hand-overs between queues cost more than the shorter chains give back.
  static const int kTwo[kNumStages] = {0, 0, 0, 1, 1, 1};          // H P M | T R U (with the alternate stream: COX_STREAMS=3p)
  static const int kStaged[kNumStages] = {0, 0, 1, 2, 2, 3};       // H P | M | T R | U (COX_STREAMS=4s)
  static const int kSix[kNumStages] = {0, 1, 2, 3, 4, 5};          // one each
  static const int kParity[kNumStages] = {0, 0, 0, 1, 1, 2};       // H P M (x2: even / odd frame slots) | T R | U: the default
  static const int kUpdateHeavy[kNumStages] = {0, 0, 0, 1, 2, 3};  // H P M | T | R | U: where the layer update is several times the ray generation
  static const int kFast[kNumStages] = {0, 1, 1, 2, 2, 2};         // front | solve | update (fast_front / fast_solve)
  static const int kOne[kNumStages] = {0, 0, 0, 0, 0, 0};
  int width = 4;  // COX_STREAMS=2|4|6 ("4s" and "3p" parse as 4 and an ignored 3)
  if (v[kSTREAMS] && (num(kSTREAMS) == 2 || num(kSTREAMS) == 4 || num(kSTREAMS) == 6)) width = num(kSTREAMS);
  const bool chosen = v[kSTREAM_MAP] || v[kSTREAMS];
  const bool three_p = is(kSTREAMS, "3p");
  const bool update_heavy = !chosen && merged && p.expands_pieces();
  // ray generation depends on the frame's input only, so two frames run it side by side on two streams
  p.alt_raygen_stream = (width == 4 || three_p) && !fast && !v[kSTREAM_MAP] && !update_heavy && !is(kSTREAMS, "4s");
  const int* map = fast ? kFast : update_heavy ? kUpdateHeavy : three_p ? kTwo : p.alt_raygen_stream ? kParity : width == 2 ? kTwo : width == 4 ? kStaged : kSix;
  int custom[kNumStages];
  if (v[kSTREAM_MAP] && !fast) {  // experiments: six digits, stage -> stream, starting at 0 and non-decreasing by at most one (e.g. 012334)
    const char* e = v[kSTREAM_MAP];
    bool ok = std::strlen(e) == kNumStages && e[0] == '0';
    for (int k = 0; ok && k < kNumStages; ++k) {
      custom[k] = e[k] - '0';
      ok = custom[k] >= 0 && custom[k] < kNumStages && (k == 0 || custom[k] == custom[k - 1] || custom[k] == custom[k - 1] + 1);
    }
    if (ok) map = custom;
  }
  if (fast) {
    p.fast.streams = (v[kFAST_STREAMS] && num(kFAST_STREAMS) == 1) ? 1 : 3;
    if (p.fast.streams == 1) map = kOne;
  }
  p.input_stream = !(v[kINPUT_STREAM] && num(kINPUT_STREAM) == 0);

  // ---- the queue budget.  The runtime gives the host's null stream a hardware queue to itself and deals every created stream onto
  // the budget - 1 others (scripts/queue_probe.hip, profiles/r05_queue_probe.txt: at 4 queues the 4th stream of a process lands on
  // the queue of the 3rd, the 5th on the 2nd's, whether streams came and went before or not), and two stages on one queue run back to
  // back.  Today's plans create 4 to 5 streams: at 4 queues H P M (even) shared a queue with T R and H P M (odd) with U, while the
  // input stream, idle on the resident path, had one to itself.  So where the streams do not fit, first the input stream goes (host
  // inputs are then copied on the frame's own ray-generation stream, COX_INPUT_STREAM=0), then the map steps down to the widest one
  // that fits.  What the map or the input stream was chosen by (COX_STREAMS, COX_STREAM_MAP, COX_FAST_STREAMS; COX_INPUT_STREAM) stays.
  // Measured at 4 queues on the commit before the budget existed, through the switches (frames/s, medians of 3-5 runs of bench.py,
  // profiles/r05_map_sweep.json; "-in" = without input stream):
  //   merged 5 cm          default 3 218 | default -in 6 421 | H P M x2 | T R U -in 7 300 | H P M | T R U 6 231, -in 6 229 | staged -in 6 432 |
  //                        H P M | T R | U -in 5 855 | one stream 2 777, -in 4 239
  //   merged 2 cm 1280x720 default 1 354 | default -in 687 | H P M | T R | U -in 1 769 | H P M | T R U -in 832 | H P M x2 | T R U -in 955 (bimodal: single
  //                        runs of most maps reach 1 600-1 800, this one did in 3 of 5)
  //   merged 1 cm          default 705 | default -in 771 | H P M | T R | U -in 793 | H P M | T R U -in 772 | H P M x2 | T R U -in 769
  //   fast 5 cm            default 2 222 | default -in 2 941 | one stream 1 332, -in 1 740
  // Budgets other than 4 follow the same rule and are covered by the parity tests, not by measurements of their own.
  // Stage graphs (COX_GRAPH, opt-in and slower) keep the streams they have always had: a stage is captured on its live stream, and
  // while one thread captures, the other thread's wait for an event last recorded on that stream is refused by the runtime.  With
  // T R U (or R U) on one stream that window is most of a frame: COX_STREAMS=2 and COX_STREAM_MAP=000112 with COX_GRAPH=1 return an
  // error on the commit before this one as well.  Graphs are out of the budget until that is mended.
  int budget = hw_queues;
  if (v[kQUEUES]) {
    char* end = nullptr;
    const long n = std::strtol(v[kQUEUES], &end, 10);
    if (end != v[kQUEUES] && *end == '\0' && n >= 1 && n <= kMaxQueueBudget) budget = static_cast<int>(n);
  }
  p.use_graphs = v[kGRAPH] != nullptr && v[kNO_GRAPH] == nullptr;
  if (budget > 0 && !p.use_graphs) {
    const int room = std::max(1, budget - 1);  // queues beside the null stream's
    const bool map_chosen = fast ? v[kFAST_STREAMS] != nullptr : chosen;
    auto streams = [&] { return map[kNumStages - 1] + 1 + (p.alt_raygen_stream ? 1 : 0) + (p.input_stream ? 1 : 0); };
    if (!v[kINPUT_STREAM] && streams() > room) p.input_stream = false;
    while (!map_chosen && streams() > room && map != kOne) {
      if (fast) {  // front | solve | update -> one stream
        map = kOne;
        p.fast.streams = 1;
      } else if (map == kUpdateHeavy) {  // H P M | T | R | U -> H P M | T R | U
        map = kParity;
      } else if (map == kParity && p.alt_raygen_stream) {  // H P M x2 | T R | U -> H P M x2 | T R U
        map = kTwo;
      } else if (p.alt_raygen_stream) {  // H P M x2 | T R U -> H P M | T R U
        p.alt_raygen_stream = false;
      } else {  // H P M | T R | U -> H P M | T R U -> one stream
        map = map == kParity ? kTwo : kOne;
      }
    }
  }
  std::copy(map, map + kNumStages, p.stage_stream);
  p.n_streams = p.n_stage_streams() + (p.alt_raygen_stream ? 1 : 0) + (p.input_stream ? 1 : 0);

  // ---- where the merged record walk runs.  Block ordinals come from a table of the frame's own (cox_walk.hpp), so the walk and emit
  // depend on the frame's rays alone and may run on the ray-generation stream; only the binding has to stay in the layer's frame
  // order.  Where T, R and U share one stream and two ray-generation lanes serve every other frame each (four queues, 10 and 5 cm),
  // that stream is the longest chain of a frame and the lanes stand half idle: the walk goes to the lanes.  With a stream each for
  // T R and U the lanes would become the longest chain, so the walk stays in stage T there.
  // COX_WALK=raygen|update replaces the rule.  Stage graphs keep the walk in stage T (a stage is captured once, and the wait for the
  // record set's previous user belongs in front of the walk).
  {
    const bool can = merged && !p.walks_pieces() && !p.use_graphs;
    const bool rule = p.alt_raygen_stream && p.stage_stream[3] == p.stage_stream[5];
    p.walk_on_raygen = can && (is(kWALK, "raygen") ? true : is(kWALK, "update") ? false : rule);
    // The lanes are what bounds the frame there, launches and gaps included, and the merge leaves the chip empty for most of its time
    // (a handful of waves finish the largest bundles): the walk of every other ray runs under that tail, one launch fewer per frame
    // (DESIGN.md section 6, round 8).  Small axis cap only: the walk's LDS scratch has to fit the merge's operand table.
    // COX_TOUCH=merge|kernel replaces the rule where the walk is on the lanes with the small axis cap, and changes nothing elsewhere.
    const bool may_touch_in_merge = p.walk_on_raygen && p.small_axis_cap;
    p.touch_in_merge = may_touch_in_merge && !is(kTOUCH, "kernel");
  }

  // ---- fast.  At 5 cm two rounds settle every frame of the benchmark stream; at 2 cm and 1 cm nine frames in ten have a ray that
  // outgrows its round-1 list, and a frame that ends so is redone by ONE lane (14 and 4 frames/s): eight rounds there, and longer lists
  // from the start (measured, frames/s at 2 cm / 1 cm: caps 8,16: 628 / 5; 16,32: 694 / 28; 32,32: - / 104).
  if (fast) {
    FastPlan& f = p.fast;
    if (v[kFAST_FENCE]) f.fences = num(kFAST_FENCE);
    f.rounds = p.small_axis_cap ? 2 : kFastMaxRounds;
    if (f.rounds > 2) {
      f.cap0 = ((p.steps_max - 1) / 3 > 200) ? 32u : 16u;
      f.cap1 = 32u;
    }
    if (v[kFAST_ROUNDS]) f.rounds = std::min(kFastMaxRounds, std::max(2, num(kFAST_ROUNDS)));
    if (v[kFAST_GROUPS]) f.relax_groups = static_cast<uint32_t>(std::min(256, std::max(8, num(kFAST_GROUPS))));
    f.force_sequential = v[kFAST_SEQUENTIAL] && num(kFAST_SEQUENTIAL) != 0;
    if (v[kFAST_CAP]) {  // candidate steps per ray: "cap0" or "cap0,cap1"
      int a = 0, b = 0;
      const int got = std::sscanf(v[kFAST_CAP], "%d,%d", &a, &b);
      if (got >= 1 && a >= 1 && a <= static_cast<int>(kFastCap0Max)) f.cap0 = static_cast<uint32_t>(a);
      f.cap1 = std::max<uint32_t>(f.cap1, f.cap0);
      if (got >= 2 && b <= static_cast<int>(kFastShortMax) && static_cast<uint32_t>(b) >= f.cap0) f.cap1 = static_cast<uint32_t>(b);
    }
  }

  // ---- host side.  Stage graphs measured slightly slower than eager launches (2 936 vs 3 117 frames/s), so opt-in (use_graphs: above).
  p.submit_thread = !(v[kSUBMIT_THREAD] && num(kSUBMIT_THREAD) == 0);
  if (v[kCOPY_THREADS]) p.copy_threads = std::min(15, std::max(0, num(kCOPY_THREADS)));
  p.h2d_kernel = is(kH2D, "kernel");
  if (v[kH2D_GROUPS]) p.h2d_groups = std::max(1, num(kH2D_GROUPS));
  p.depth_convert_on_input_stream = is(kDEPTH_CONVERT, "input");
  if (v[kTIMELINE]) p.timeline = v[kTIMELINE];
  p.debug = v[kDEBUG] != nullptr;
  return p;
}

}  // namespace cox_plan
