// MI355X (gfx950) TSDF integrator behind include/coxgraph_hip.h.
//
// Replaces the work of voxblox's TsdfIntegratorBase::integratePointCloud as coxgraph calls it
// (coxgraph/include/coxgraph/map_comm/tsdf_recover.h:75).  Design: DESIGN.md.
//
// One frame = six stages of a few kernels each, spread over four streams, and NO host round trip: every count a later kernel needs
// (rays, records, touched blocks, sort key width) stays in device memory, the host only supplies grid-size hints.
//
//   rays      simple: one ray per valid point, canonical order = voxblox "mixed" sequence number
//             merged: points bundled by terminal voxel (frame hash + stable radix sort), one ray per
//                     bundle, canonical order = (clearing?, first visit)
//   lengths   every ray knows its step count in O(1) (L1 index distance) -> exclusive scan -> each ray
//             owns a contiguous slice of the record array
//   touch     rays walk their voxels, insert block keys in the layer hash (bump-allocating pool
//             blocks) and give every block touched this frame a dense ordinal
//   emit      rays walk again and write (ordinal<<12 | linear voxel, ray id) records, ray-major
//   sort      stable partition of the records by tile (or a full radix sort by voxel id) -> per voxel, records are in canonical ray order
//   apply     per voxel: the running weighted-mean/clamp update in exactly that order
//
// This file is the integrator itself: state, allocation, the stage functions, frame enqueue and the C entry points.  What is decided
// once per integrator is cox_plan.hpp's; the kernels are in the headers below, included in the order they build on each other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include "../../include/coxgraph_hip_history.h"
#include "../../include/coxgraph_hip_selftest.h"
#include "cox_host.hpp"
#include "cox_plan.hpp"
#include "cox_sort.hpp"
#include "cox_threads.hpp"

using namespace cox;
using cox_plan::IntegratorPlan;
using cox_plan::LayerUpdate;

// ---- device side --------------------------------------------------------------------------------
#include "cox_frame.hpp"
#include "cox_raygen.hpp"
#include "cox_walk.hpp"
#include "cox_pieces.hpp"
#include "cox_fast.hpp"
#include "cox_apply_records.hpp"
#include "cox_apply_tile.hpp"
#include "cox_frontend.hpp"

static_assert(cox_plan::kAxisCapSmall == kAxisCapSmall && cox_plan::kTileShift == kTileShift && cox_plan::kBigChunk == kBigChunk &&
                  cox_plan::kBigChunkMin == kBigChunkMin && cox_plan::kFastMaxRounds == kFastMaxRounds && cox_plan::kFastShortMax == kFastShortMax &&
                  cox_plan::kFastRelaxGroups == kFastRelaxGroups && cox_plan::kCopyGroups == kCopyGroups,
              "cox_plan.hpp decides with the kernels' own constants");

// =================================================================================================
// host side
// =================================================================================================
// A frame is six pipeline stages; up to six frames are in flight, one per stage:
//   H  bundle hash                            (input only)
//   P  bundling keys + sort + bundle bounds   (input only)
//   M  sequential means                       (-> ray arrays, record offsets)
//   T  touch, emit, binding                   (allocates blocks; merged record walk: touch and emit read the frame's rays and tables
//                                              only and may run at the tail of M instead -- IntegratorPlan::walk_on_raygen)
//   R  record partition
//   U  apply                                  (writes voxels)
// (simple: H only uploads the parameter block, M is k_rays_simple.)  The stages map to FOUR streams (IntegratorPlan::stage_stream; more
// fall off a cliff): by default H P M | H P M | T R | U -- ray generation depends on the frame's input only, so
// the even and the odd frame slots run it side by side on two streams (st[0], st_alt) -- and H P M | T | R | U where the layer
// update is several times the ray generation.  The layer update stays one pipeline in frame order: T of frame t+1 beside U of frame t
// is safe (T only inserts new hash entries / bumps the pool and restamps ordinals that U never reads, U only writes voxels).
// Buffers are replicated by lifetime: what lives from H to U (parameter block, counters, ray arrays, bundle hash) x6, H..M (bundling
// sort buffers) x3, T..U (records, touched blocks, tile tables, sort info) x3.  Events order producer -> consumer (a per-frame-slot
// hand-over event between consecutive stages on different streams) and consumer -> next writer of the same copy ("done" per set).
//
// Every per-frame quantity (pose, point count, input pointers, frame id) lives in a device-side parameter block and every count in
// device counters, so the kernel arguments and grids of a stage never change.  Stages are launched eagerly; replaying each as a
// captured HIP graph is possible for the same reason but measured slower, so it is opt-in (IntegratorPlan::use_graphs).
constexpr int kStatRing = 8;
constexpr int kFrameSets = 6;  // frames in flight: one per stage
constexpr int kStageSets = 3;  // bundle sets (live H..M) and record sets (live T..U); kFrameSets is a multiple, so a frame slot fixes both
constexpr int kInputSets = kFrameSets;  // staging sets for host / depth inputs: as many as frames in flight, so that filling one never has to wait on the device
using cox_plan::kNumStages;

struct FrameSet {  // lives H .. U
  FrameParams* d_params = nullptr;
  Counters* cnt = nullptr;
  RayArrays rays{};
  u64* fh_keys = nullptr;  // [fh_cap] keys followed by [fh_cap] first-sequence numbers (one memset)
  u32* fh_first = nullptr;
  hipEvent_t done = nullptr;           // stage U of the frame that used this set
  hipEvent_t params_copied = nullptr;  // the H2D copy of the parameter block has executed (host may rewrite the pinned slot)
  hipEvent_t hand[kNumStages - 1] = {};  // hand[k]: stage k of the frame is enqueued complete (stage k + 1 on another stream waits for it)
  bool used = false;
};
struct BundleSet {  // lives H .. M
  u32 *pslot = nullptr, *skey[2] = {nullptr, nullptr}, *sval[2] = {nullptr, nullptr}, *bstart = nullptr;
  u32 *hrank = nullptr, *head = nullptr;  // bundle heads (k_bundle_keys): rank inside their tile [pcap], counts per tile [tiles][4]
  SortInfo* sort_info = nullptr;
  hipEvent_t done = nullptr;  // stage M of the frame that used this set
  bool used = false;
};
struct RecordSet {  // lives T .. U
  u32 *rec_key[2] = {nullptr, nullptr}, *rec_ray[2] = {nullptr, nullptr};
  u32 *piece_front = nullptr, *piece_back = nullptr, *piece_wsum = nullptr;
  // piece path (merged): the walk as bytes + the (ray, tile) pieces, ping-pong for their sort; the record arrays stay unallocated
  uint8_t* lin8 = nullptr;
  u32 *pkey[2] = {nullptr, nullptr}, *pstart[2] = {nullptr, nullptr}, *prl[2] = {nullptr, nullptr};
  u64* pbkey = nullptr;                   // piece partition: block key of every piece until k_piece_touch has run
  u32 *plen = nullptr, *pdest = nullptr;  // piece partition: lengths of the sorted pieces, their exclusive scan
  u32* touched_slots = nullptr;  // [layer ht_cap] slots of the blocks touched this frame, in ordinal order: of the layer's table, or (merged record walk) of ft_keys
  u64* ft_keys = nullptr;        // [layer ht_cap] merged record walk: the frame block table (cox_walk.hpp: FrameBlocks); empty between frames
  u32* ft_ord = nullptr;         // [layer ht_cap]
  int4* ord_info = nullptr;      // [layer ht_cap] (16 * block index, pool index) per block touched this frame
  u32 *blk_beg = nullptr, *blk_end = nullptr;  // [layer ht_cap * 16] record range of every tile (block apply); zero between frames
  u32 *big_of_tile = nullptr, *big_acc = nullptr;  // large tiles (cox_apply_tile.hpp: BigTiles); zero between frames
  u32* blk_list = nullptr;                         // [layer ht_cap * 16] tiles k_apply_block takes
  uint2* big_chunks = nullptr;
  u32 big_chunk_cap = 0;
  SortInfo* sort_info = nullptr;
  hipEvent_t done = nullptr;  // stage U of the frame that used this set
  bool used = false;
};

// buffers of the fast integrator (method == COX_METHOD_FAST only); see cox_fast.hpp
using cox_plan::kFastCap0Max;  // candidate steps per ray in round 0 at most (FastPlan::cap0)
struct VisitSet {  // the candidate visits of one round: ray-major arrays + their slot-sorted view
  u32 *key[2] = {nullptr, nullptr}, *val[2] = {nullptr, nullptr};  // sort ping-pong: slot, visit id
  u64 *vhash = nullptr, *shash = nullptr;                         // hash of visit v / of the visit at sorted position i
  u32 *vray = nullptr, *pos_of = nullptr, *sinfo = nullptr, *voff = nullptr;
  u32 cap = 0;                 // visits the arrays hold
  int sorted = 0;              // which ping-pong buffer holds the sorted keys
  hipEvent_t done = nullptr;   // the solve of the frame that used the set is complete
  bool used = false;
};
struct FastState {
  u64 *fhash = nullptr, *table_start = nullptr, *table_obs = nullptr;
  u32 *fresh = nullptr, *rank = nullptr;
  u32* cap[kFrameSets] = {};    // candidate-list length per ray (lives from the front to the end of the solve, like the frame set)
  u32* reach[kFrameSets] = {};  // voxels each ray updates: relaxed in place
  VisitSet vs0[2];              // round 0: written by the front of frame t (start-set stream), read by its solve -- two frames' worth
  VisitSet vs1;                 // round 1: lives inside one solve
  u32* long_list = nullptr;     // round 1: the rays with a list longer than cap1
  u32* d_stats = nullptr;       // [8] run totals: frames redone by the sequential kernel, frames with a round 1, passes of the relaxation (round 0, round 1), ...
  u64 off_start = 0, off_obs = 0;  // ApproxHashSet::offset_
  int reset_counter = 0;
  uint64_t frames = 0;
};

static std::mutex g_submitters_mutex;
static std::vector<Submitter*> g_submitters;
void cox_drain_submitters() {
  std::lock_guard<std::mutex> lk(g_submitters_mutex);
  for (Submitter* s : g_submitters) s->wait_outstanding(0);
}

struct cox_integrator {
  explicit cox_integrator(const IntegratorPlan& p) : plan(p), graphs_on(p.use_graphs) {}
  const IntegratorPlan plan;       // everything decided at creation (cox_plan.hpp)
  // what the integrator owns on the device: every slot dev_realloc / pinned_realloc / make_event has filled.  cox_integrator_destroy
  // walks these lists and nothing else, so a buffer cannot be allocated without being released.
  std::vector<void**> dev_slots, pinned_slots;
  std::vector<hipEvent_t*> event_slots;
  Submitter* submitter = nullptr;
  CopyPool* copy_pool = nullptr;   // helpers for the bounce copy of pageable inputs: created with the first such frame
  uint64_t last_big_tiles = 0, last_big_chunks = 0;  // of the last frame whose counters were folded (cox_integrator_update_stats)
  uint64_t host_ns = 0, host_wait_ns = 0, host_frames = 0;  // time the caller's thread spends inside the integrate call (enqueueing, waiting for a free slot)
  cox_projective* proj = nullptr;  // method == COX_METHOD_PROJECTIVE: everything else below stays empty
  cox_layer* layer = nullptr;
  FastState fast;
  cox_tsdf_config cfg;
  int method = 0;
  hipStream_t st[kNumStages] = {};  // stream of stage H, P, M, T, R, U (IntegratorPlan::stage_stream: equal streams adjacent)
  hipStream_t st_alt = nullptr;     // ray generation (H, P, M) of the odd frame slots runs here, beside the even slots' on st[0]
  hipStream_t st_in = nullptr;      // host inputs (copies) on a stream of their own
  FrameSet fs[kFrameSets];
  BundleSet bs[kStageSets];
  RecordSet rs[kStageSets];
  FrameParams* h_params = nullptr;  // pinned, kFrameSets entries
  u32 pcap = 0, rcap = 0, fh_cap = 0, piece_cap = 0;  // points, records, frame-hash slots, pieces the buffers hold (ensure_capacity)
  u32 layer_generation = 0;     // cox_layer::generation the layer-sized buffers (touched_slots, ord_info, graphs) belong to
  hipEvent_t timeline_ref = nullptr;
  FILE* timeline = nullptr;
  u64 blocks_seen = 0, blocks_delta_max = 0;  // pool growth: last block count seen by the host, largest increase between two looks
  SortWorkspace sort_pts, sort_pts_alt, sort_rec;  // bundling sort (even / odd frame slots: they run side by side), record / piece sort
  SortWorkspace sort_vis, sort_vis1;               // the fast integrator's visit sorts (round 0 on the front's stream, later rounds on the solve's)
  ScanWorkspace scanws_a, scanws_b, scanws_f;
  ScanWorkspace scanws_p;       // scan of the piece lengths
  ScanWorkspace scanws_h;       // piece partition: scan over the layer's hash slots (ordinals of the stamped blocks)
  // ordering against the caller's stream (cox_integrator_set_input_stream): the first stage waits for what the producer has
  // enqueued, and the producer's stream waits until the engine has read the inputs (stream-ordered allocators may then
  // recycle them)
  bool has_producer = false;
  hipStream_t producer = nullptr;
  hipEvent_t ev_producer = nullptr, ev_inputs_read = nullptr;
  // Host inputs (cox_integrate_points_async, cox_integrate_depth_async) are staged on the input stream, so the copy of frame t + 1 runs
  // beside the kernels of frame t; without one (COX_INPUT_STREAM=0) on the ray-generation stream of the frame they belong to.
  float* own_xyz[kInputSets] = {};  // staging for host / depth inputs (read by stages H .. M of the frame)
  uint8_t* own_rgba[kInputSets] = {};
  float* own_depth[kInputSets] = {};       // staging for host depth images (cox_integrate_depth_async)
  uint8_t* own_depth_rgba[kInputSets] = {};
  u32* depth_flag = nullptr;  // depth front end: valid pixels per tile
  u32* d_depth_n = nullptr;   // [kInputSets] point count of the depth image converted into each staging set: it stays on the device
  hipEvent_t in_ready[kInputSets] = {};  // staging set k has been filled (the frame's first stage waits for it)
  hipEvent_t in_free[kInputSets] = {};   // the frame that read staging set k last has read it for the last time
  bool in_used[kInputSets] = {};
  // observation record (cox_integrator_attach_history): every cloud is also marked in it, from the same device copy, on the record's
  // own stream -- beside the frame's ray generation, which therefore waits for nothing new
  cox_obs* obs = nullptr;
  hipEvent_t obs_read[kInputSets] = {};  // the record has read staging set k (created with the first attach)
  bool obs_used[kInputSets] = {};
  hipEvent_t ev_obs_read = nullptr;      // ... the caller's device buffer (cox_integrate_points_dev)
  float* pin_xyz[kInputSets] = {};       // pinned bounce buffers for pageable host inputs (a pinned caller buffer is copied from directly)
  uint8_t* pin_rgba[kInputSets] = {};
  u32 pin_cap = 0;
  Counters* h_ring = nullptr;  // pinned, kStatRing entries
  uint64_t frame_no = 0;       // frames enqueued
  cox_frame_stats last{};      // host-known part of the last frame's stats
  bool last_has_counts = false;
  bool last_count_on_device = false;  // the last frame's point count was produced on the device (fold_counters fetches it)
  // stage graphs: [stage][frame set index]
  bool graphs_on;  // plan.use_graphs until a capture fails: eager from then on
  hipGraphExec_t graphs[kNumStages][kFrameSets] = {};
  // timing of individual kernels (bench roofline); forces eager launches
  bool profiling = false;
  u32 profile_every = 1;  // time the kernels of every n-th frame
  // one (begin, end) event pair per timed region of a frame, by kernel class (cox_kernel_class in coxgraph_hip.h)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> class_events[COX_KERNEL_CLASSES];
  std::vector<hipEvent_t> event_pool[2];  // [1]: the submission thread's
  double class_ms[COX_KERNEL_CLASSES] = {};
  uint64_t class_regions[COX_KERNEL_CLASSES] = {};
};

// ---- ownership: the only ways the integrator allocates device memory, pinned memory and its fixed events ---------------------
template <typename T>
static int dev_realloc(cox_integrator* I, T** p, size_t count) {
  void** slot = reinterpret_cast<void**>(p);
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  if (count == 0) return COX_OK;
  if (std::find(I->dev_slots.begin(), I->dev_slots.end(), slot) == I->dev_slots.end()) I->dev_slots.push_back(slot);
  return cox_hip_status(hipMalloc(slot, count * sizeof(T)));
}
template <typename T>
static int pinned_realloc(cox_integrator* I, T** p, size_t count) {
  void** slot = reinterpret_cast<void**>(p);
  if (*p) (void)hipHostFree(*p);
  *p = nullptr;
  if (std::find(I->pinned_slots.begin(), I->pinned_slots.end(), slot) == I->pinned_slots.end()) I->pinned_slots.push_back(slot);
  if (hipHostMalloc(slot, count * sizeof(T), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    return COX_ERR_OUT_OF_MEMORY;
  }
  return COX_OK;
}
static int make_event(cox_integrator* I, hipEvent_t* e) {
  I->event_slots.push_back(e);
  return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess ? COX_OK : COX_ERR_NO_DEVICE;
}
static void release_owned(cox_integrator* I) {
  for (void** p : I->dev_slots)
    if (*p) (void)hipFree(*p);
  for (void** p : I->pinned_slots)
    if (*p) (void)hipHostFree(*p);
  for (hipEvent_t* e : I->event_slots)
    if (*e) (void)hipEventDestroy(*e);
}

static int alloc_sort_ws(cox_integrator* I, SortWorkspace* ws, u64 capacity) {
  ws->tiles_cap = std::max<u32>(1, sort_num_tiles(capacity));
  COX_TRY(dev_realloc(I, &ws->counts, sort_counts_words(ws->tiles_cap)));
  if (!ws->totals) {
    COX_TRY(dev_realloc(I, &ws->totals, sort_totals_words()));
    COX_HIP(hipMemset(ws->totals, 0, sizeof(u32) * sort_totals_words()));  // every sort leaves it zero again
  }
  return COX_OK;
}

// stream of a stage of the frame in frame slot `slot`
static inline hipStream_t stage_stream(const cox_integrator* I, int stage, int slot) {
  return (stage <= 2 && I->st_alt && (slot & 1)) ? I->st_alt : I->st[stage];
}

static int sync_all(cox_integrator* I) {
  if (I->submitter) {
    I->submitter->wait_outstanding(0);
    const int st = I->submitter->take_status();
    if (st != COX_OK) return st;
  }
  for (int k = 0; k < kNumStages; ++k)
    if (I->st[k] && (k == 0 || I->st[k] != I->st[k - 1])) COX_HIP(hipStreamSynchronize(I->st[k]));
  if (I->st_alt) COX_HIP(hipStreamSynchronize(I->st_alt));
  if (I->st_in) COX_HIP(hipStreamSynchronize(I->st_in));
  if (I->obs) COX_TRY(cox_internal_obs_wait(I->obs));  // (it reads the frames' input buffers)
  return COX_OK;
}

static void drop_graphs(cox_integrator* I) {
  for (auto& row : I->graphs)
    for (hipGraphExec_t& g : row) {
      if (g) (void)hipGraphExecDestroy(g);
      g = nullptr;
    }
}

// ---- buffers sized by the point capacity ---------------------------------------------------------------------------------------
// what lives from stage H to stage M, and the staging sets of host / depth inputs
static int alloc_ray_sets(cox_integrator* I, u32 cap) {
  for (FrameSet& F : I->fs) {
    RayArrays& R = F.rays;
    for (float** p : {&R.px, &R.py, &R.pz, &R.w}) COX_TRY(dev_realloc(I, p, cap));
    for (u32** p : {&R.color, &R.flags, &R.nsteps, &R.rec_off, &R.pbound, &R.piece_off}) COX_TRY(dev_realloc(I, p, cap));
    COX_TRY(dev_realloc(I, &R.key, cap));
    COX_TRY(dev_realloc(I, &R.q, static_cast<size_t>(cap) * 8));
    COX_TRY(dev_realloc(I, &F.fh_keys, static_cast<size_t>(I->fh_cap) + I->fh_cap / 2 + 1));  // u64 keys + u32 first-seq behind them
    F.fh_first = reinterpret_cast<u32*>(F.fh_keys + I->fh_cap);
    COX_HIP(hipMemset(F.fh_keys, 0xFF, sizeof(u64) * I->fh_cap + sizeof(u32) * I->fh_cap));  // empty; every frame leaves it empty again
  }
  for (BundleSet& B : I->bs) {
    for (u32** p : {&B.pslot, &B.skey[0], &B.sval[0], &B.skey[1], &B.sval[1], &B.hrank, &B.bstart}) COX_TRY(dev_realloc(I, p, cap));
    COX_TRY(dev_realloc(I, &B.head, static_cast<size_t>(4) * (cap / kHeadTile + 1)));
  }
  for (int k = 0; k < kInputSets; ++k) {
    COX_TRY(dev_realloc(I, &I->own_xyz[k], static_cast<size_t>(cap) * 3));
    COX_TRY(dev_realloc(I, &I->own_rgba[k], static_cast<size_t>(cap) * 4));
    COX_TRY(dev_realloc(I, &I->own_depth[k], cap));
    COX_TRY(dev_realloc(I, &I->own_depth_rgba[k], static_cast<size_t>(cap) * 4));
  }
  COX_TRY(dev_realloc(I, &I->depth_flag, cap));
  COX_TRY(alloc_sort_ws(I, &I->sort_pts, cap));
  COX_TRY(alloc_sort_ws(I, &I->sort_pts_alt, cap));
  for (ScanWorkspace* ws : {&I->scanws_a, &I->scanws_b, &I->scanws_f}) COX_TRY(dev_realloc(I, &ws->block_sums, scan_num_blocks(cap) + 2));
  return COX_OK;
}
// what lives from stage T to stage U: records, or pieces (+ the records they are expanded into), by the plan's layer update
static int alloc_record_sets(cox_integrator* I) {
  const bool pieces = I->plan.walks_pieces(), expand = I->plan.expands_pieces();
  const u32 rcap = I->rcap, piece_cap = I->piece_cap, wave_cap = rcap / 64 + 2;
  for (RecordSet& S : I->rs) {
    if (pieces) {
      COX_TRY(dev_realloc(I, &S.lin8, static_cast<size_t>(piece_cap) * 32));
      for (u32** p : {&S.pkey[0], &S.pstart[0], &S.prl[0], &S.pkey[1], &S.pstart[1], &S.prl[1]}) COX_TRY(dev_realloc(I, p, piece_cap));
    }
    if (expand) {
      COX_TRY(dev_realloc(I, &S.pbkey, piece_cap));
      COX_TRY(dev_realloc(I, &S.plen, piece_cap));
      COX_TRY(dev_realloc(I, &S.pdest, piece_cap));
      S.big_chunk_cap = static_cast<u32>(rcap / kBigChunkMin) + kBigCap + 1u;
      COX_TRY(dev_realloc(I, &S.big_chunks, S.big_chunk_cap));
    }
    if (!pieces || expand) {  // (expanded pieces: one buffer, the parity is the piece sort's)
      COX_TRY(dev_realloc(I, &S.rec_key[0], rcap));
      COX_TRY(dev_realloc(I, &S.rec_ray[0], rcap));
    }
    if (!pieces) {
      COX_TRY(dev_realloc(I, &S.rec_key[1], rcap));
      COX_TRY(dev_realloc(I, &S.rec_ray[1], rcap));
      COX_TRY(dev_realloc(I, &S.piece_front, wave_cap));
      COX_TRY(dev_realloc(I, &S.piece_back, wave_cap));
      COX_TRY(dev_realloc(I, &S.piece_wsum, static_cast<size_t>(wave_cap) * 2));
    }
  }
  COX_TRY(alloc_sort_ws(I, &I->sort_rec, pieces ? piece_cap : rcap));
  if (expand) COX_TRY(dev_realloc(I, &I->scanws_p.block_sums, scan_num_blocks(piece_cap) + 2));
  return COX_OK;
}
static int alloc_visit_set(cox_integrator* I, VisitSet& V, u32 vcap, u32 cap) {
  for (u32** p : {&V.key[0], &V.val[0], &V.key[1], &V.val[1], &V.vray, &V.pos_of, &V.sinfo}) COX_TRY(dev_realloc(I, p, vcap));
  COX_TRY(dev_realloc(I, &V.vhash, vcap));
  COX_TRY(dev_realloc(I, &V.shash, vcap));
  COX_TRY(dev_realloc(I, &V.voff, cap));
  V.cap = vcap;
  return COX_OK;
}
static int alloc_fast(cox_integrator* I, u32 cap) {
  FastState& X = I->fast;
  COX_TRY(dev_realloc(I, &X.fhash, cap));
  for (u32** p : {&X.fresh, &X.rank, &X.long_list}) COX_TRY(dev_realloc(I, p, cap));
  for (int k = 0; k < kFrameSets; ++k) {
    COX_TRY(dev_realloc(I, &X.cap[k], cap));
    COX_TRY(dev_realloc(I, &X.reach[k], cap));
  }
  // round 0: kFastCap0Max list slots per point; later rounds: the grown lists -- bounded (a frame whose lists do not fit is redone by
  // the sequential kernel), not sized for "every ray walks to the sensor" (5 GB at 5 cm)
  const u32 vcap0 = static_cast<u32>(std::min<u64>(static_cast<u64>(cap) * kFastCap0Max, 0xFFFFFFF0ull));
  const u32 vcap1 = static_cast<u32>(std::min<u64>(I->rcap, std::max<u64>(static_cast<u64>(cap) * 64, 1ull << 24)));
  COX_TRY(alloc_visit_set(I, X.vs0[0], vcap0, cap));
  COX_TRY(alloc_visit_set(I, X.vs0[1], vcap0, cap));
  COX_TRY(alloc_visit_set(I, X.vs1, vcap1, cap));
  COX_TRY(alloc_sort_ws(I, &I->sort_vis, vcap0));
  COX_TRY(alloc_sort_ws(I, &I->sort_vis1, vcap1));
  return COX_OK;
}
static int ensure_capacity(cox_integrator* I, u32 n) {
  if (n <= I->pcap) return COX_OK;
  COX_TRY(sync_all(I));
  drop_graphs(I);  // they hold the old pointers and grids
  const u32 cap = std::max<u32>(n, 1024);
  const u32 steps_max = I->plan.steps_max;
  I->fh_cap = next_pow2(static_cast<u64>(cap) + cap / 2);  // load factor <= 2/3 even if every point is its own bundle
  // records: the worst case (every ray at maximum length) always fits, so a frame can never overflow
  // unless that bound exceeds the 2^31 record limit of the 32-bit offsets
  I->rcap = static_cast<u32>(std::min<u64>(static_cast<u64>(cap) * steps_max, 0x7FFFFFF0ull));
  if (I->plan.record_cap) I->rcap = std::min(I->rcap, I->plan.record_cap);  // (tests: a frame with more records is dropped, as beyond 2^31)
  // pieces: every ray at the bound of the longest wave-walked ray (piece_bound); a frame of sequentially walked rays may need
  // more (one piece per step at worst) -- that frame is dropped and reported like a record overflow
  const u32 planes = (steps_max - 1) / 3;
  const u64 per_ray = static_cast<u64>(steps_max + 63) / 64 + (planes + 2) + 2 * ((planes + 2) / 16 + 1) + 4;
  I->piece_cap = static_cast<u32>(std::min<u64>(I->rcap, static_cast<u64>(cap) * per_ray));
  COX_TRY(alloc_ray_sets(I, cap));
  COX_TRY(alloc_record_sets(I));
  if (I->method == COX_METHOD_FAST) COX_TRY(alloc_fast(I, cap));
  I->pcap = cap;
  // hipMemset runs on the legacy default stream, which the engine's non-blocking streams do not wait for
  COX_HIP(hipDeviceSynchronize());
  return COX_OK;
}
// ---- buffers sized by the layer's hash capacity (one entry per block key the table can hold); device idle ----------------------
static int alloc_layer_sized(cox_integrator* I) {
  const size_t slots = I->layer->ht_cap, tiles = slots * kTilesPerBlock;
  for (RecordSet& S : I->rs) {
    COX_TRY(dev_realloc(I, &S.touched_slots, slots));
    COX_TRY(dev_realloc(I, &S.ord_info, slots));
    if (I->method == COX_METHOD_MERGED && !I->plan.walks_pieces()) {  // the frame block table: sized and re-sized with the layer's
      COX_TRY(dev_realloc(I, &S.ft_keys, slots));
      COX_TRY(dev_realloc(I, &S.ft_ord, slots));
      COX_HIP(hipMemset(S.ft_keys, 0xFF, sizeof(u64) * slots));  // empty; every frame's binding leaves it empty again
    }
    COX_TRY(dev_realloc(I, &S.blk_beg, tiles));
    COX_TRY(dev_realloc(I, &S.blk_end, tiles));
    COX_HIP(hipMemset(S.blk_beg, 0, sizeof(u32) * tiles));
    COX_HIP(hipMemset(S.blk_end, 0, sizeof(u32) * tiles));
    if (I->plan.expands_pieces()) {
      COX_TRY(dev_realloc(I, &S.big_of_tile, tiles));
      COX_TRY(dev_realloc(I, &S.blk_list, tiles));
      COX_HIP(hipMemset(S.big_of_tile, 0, sizeof(u32) * tiles));
    }
  }
  if (I->plan.expands_pieces()) COX_TRY(dev_realloc(I, &I->scanws_h.block_sums, scan_num_blocks(I->layer->ht_cap) + 2));
  I->layer_generation = I->layer->generation;
  COX_HIP(hipDeviceSynchronize());  // (the memsets ran on the legacy default stream)
  return COX_OK;
}

static FrameParams make_params(const cox_integrator* I, const float T[7], u32 n, int freespace, const float* xyz, const uint8_t* rgba) {
  const cox_tsdf_config& c = I->cfg;
  FrameParams P;
  memset(&P, 0, sizeof(P));
  P.qw = T[0];
  P.qx = T[1];
  P.qy = T[2];
  P.qz = T[3];
  P.tx = T[4];
  P.ty = T[5];
  P.tz = T[6];
  P.voxel_size = I->layer->voxel_size;
  P.voxel_size_inv = I->layer->voxel_size_inv;
  P.trunc = c.default_truncation_distance;
  {
    const double t1 = static_cast<double>(c.default_truncation_distance) * (1.0 + 4.0 * 5.9604644775390625e-08 * (1.0 + static_cast<double>(c.max_weight)));
    float f = static_cast<float>(t1);
    if (static_cast<double>(f) < t1) f = std::nextafter(f, std::numeric_limits<float>::infinity());
    P.sat1 = f;  // >= saturating_update's threshold for every update weight >= 1
  }
  P.max_weight = c.max_weight;
  P.min_ray = c.min_ray_length_m;
  P.max_ray = c.max_ray_length_m;
  P.sparsity_factor = c.sparsity_compensation_factor;
  P.start_subsampling_inv = c.start_voxel_subsampling_factor * I->layer->voxel_size_inv;
  P.n_points = n;
  P.frame_id = 0;
  P.use_const_weight = c.use_const_weight;
  P.allow_clear = c.allow_clear;
  P.carving = c.voxel_carving_enabled;
  P.use_dropoff = c.use_weight_dropoff;
  P.use_sparsity = c.use_sparsity_compensation_factor;
  P.anti_grazing = (I->method == COX_METHOD_MERGED) ? c.enable_anti_grazing : 0;
  P.freespace = freespace;
  P.cast_from_origin = (I->method == COX_METHOD_FAST) ? 0 : 1;  // the fast integrator walks from the surface towards the sensor
  P.xyz = xyz;
  P.rgba = rgba;
  P.np2 = next_pow2(static_cast<u64>(n) + 1);
  return P;
}

static inline dim3 grid_for(u32 n, u32 block = 256, u32 cap = 0x7FFFFFFFu) { return dim3(std::min<u32>(cap, std::max<u32>(1, (n + block - 1) / block))); }

// HIP-event timing of one kernel class inside a frame (bench.py roofline): begin / end on the stream the kernels run on
// classes whose regions are opened by the submission thread (stages T, R, U and the solve of fast) take their
// events from a pool of their own
static inline int event_pool_of(const cox_integrator* I, int cls) {
  if (cls == COX_KC_TOUCH_EMIT && I->plan.walk_on_raygen) return 0;  // (the walk is enqueued by the caller's thread; the binding carries no events then)
  return (I->submitter && (cls == COX_KC_APPLY || cls == COX_KC_TOUCH_EMIT || cls == COX_KC_RECORD_SORT || cls == COX_KC_FAST_SWEEPS || cls == COX_KC_FAST_ROUND1)) ? 1 : 0;
}
static thread_local u64 tl_frame_no = 0;  // the frame whose stages this thread is enqueueing (StageCtx::frame)
struct TimedRegion {
  cox_integrator* I;
  int cls;
  hipStream_t s;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  TimedRegion(cox_integrator* I_, int cls_, hipStream_t s_) : I(I_), cls(cls_), s(s_) {
    if (!(I->profiling && (tl_frame_no % I->profile_every == 0))) return;
    std::vector<hipEvent_t>& pool = I->event_pool[event_pool_of(I, cls)];
    // events come from a pool that the drain refills: creating them costs more than recording them
    auto take = [&]() -> hipEvent_t {
      if (!pool.empty()) {
        hipEvent_t e = pool.back();
        pool.pop_back();
        return e;
      }
      hipEvent_t e = nullptr;
      return hipEventCreate(&e) == hipSuccess ? e : nullptr;
    };
    e0 = take();
    e1 = take();
    if (!e0 || !e1) {
      e0 = e1 = nullptr;
      return;
    }
    (void)hipEventRecord(e0, s);
  }
  ~TimedRegion() {
    if (!e0) return;
    (void)hipEventRecord(e1, s);
    I->class_events[cls].emplace_back(e0, e1);
  }
};

// ---- the six stages; identical whether launched eagerly or captured into a graph: no argument depends on the frame ----
struct StageCtx {
  cox_integrator* I;
  FrameSet* F;
  BundleSet* B;
  RecordSet* S;
  int slot;
  u64 frame;  // frame number (which frames carry timing events)
  const u32* n_dev = nullptr;  // the frame's point count when it is known on the device only (depth front end); n_points of the parameter block is then an upper bound
};

static LayerView layer_view(const cox_layer* Lh) {
  return LayerView{Lh->voxels, Lh->ht_keys, Lh->ht_vals, Lh->ht_stamp, Lh->ht_ord, Lh->block_keys, Lh->d_nblocks, Lh->ht_cap - 1, static_cast<u32>(Lh->capacity)};
}
static int points_sort_passes(const cox_integrator* I) { return (ceil_log2(next_pow2(static_cast<u64>(I->pcap) + 1)) + 1 + 10) / 11; }

static int stage_hash(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  FrameSet& F = *c.F;
  BundleSet& B = *c.B;
  const bool by_value = (I->method == COX_METHOD_MERGED) && !I->graphs_on;
  if (!by_value) {
    COX_HIP(hipMemcpyAsync(F.d_params, &I->h_params[c.slot], sizeof(FrameParams), hipMemcpyHostToDevice, s));
    if (c.n_dev) hipLaunchKernelGGL(k_params_count, dim3(1), dim3(1), 0, s, F.d_params, c.n_dev);
  }
  COX_HIP(hipMemsetAsync(F.cnt, 0, sizeof(Counters), s));
  if (I->method == COX_METHOD_MERGED) {
    const u32 n = I->pcap;  // grids cover the capacity; the kernels stop at the frame's own point count
    {
      TimedRegion t(I, COX_KC_BUNDLE_HASH, s);
      // with anti-grazing the hash is read again by touch / emit (stage T), after this frame's pslot may have been reused:
      // that (rare) configuration keeps the memset; otherwise the frame cleans up after itself (BundleBounds, end of stage P)
      const bool self_clean = !I->cfg.enable_anti_grazing;
      if (!self_clean) COX_HIP(hipMemsetAsync(F.fh_keys, 0xFF, sizeof(u64) * I->fh_cap + sizeof(u32) * I->fh_cap, s));
      hipLaunchKernelGGL(k_bundle_insert, grid_for(n), dim3(256), 0, s, F.d_params, I->h_params[c.slot], by_value ? 1 : 0, c.n_dev, F.fh_keys, F.fh_first,
                         I->fh_cap - 1, B.pslot, F.cnt);
    }
  }
  return COX_OK;
}
static int stage_point_sort(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  FrameSet& F = *c.F;
  BundleSet& B = *c.B;
  if (I->method == COX_METHOD_MERGED) {
    const u32 n = I->pcap;
    const SortWorkspace& ws = (I->st_alt && (c.slot & 1)) ? I->sort_pts_alt : I->sort_pts;
    // The sort keys are written here, in front of the sort and on its stream, because k_bundle_keys also fills the sort workspace:
    // the histogram of pass 0, tile by tile as k_rs_hist<11> would -- as long as its tile is the sort's (rs_tile_shift == 0 for
    // every point count the buffers hold).  It stays in the bundle-hash timing class.
    const bool counted = static_cast<u64>(n) <= static_cast<u64>(kRsMaxTiles) * kRsTile;
    {
      TimedRegion t(I, COX_KC_BUNDLE_HASH, s);
      hipLaunchKernelGGL(k_bundle_keys, grid_for(n, kHeadTile), dim3(kKeysThreads), 0, s, F.d_params, F.fh_keys, F.fh_first, B.pslot, B.skey[0], B.sval[0], B.hrank, B.head,
                         B.sort_info, counted ? ws.counts : nullptr, ws.totals);
    }
    // the last scatter pass places the bundle heads: it writes the bundle starts and counts, and empties the frame hash
    const bool self_clean = !I->cfg.enable_anti_grazing;
    const BundleBounds bounds{F.d_params, B.head, B.hrank, B.pslot, B.bstart, F.cnt, self_clean ? F.fh_keys : nullptr, F.fh_first, I->fh_cap - 1};
    TimedRegion t(I, COX_KC_POINT_SORT, s);
    (void)radix_sort_pairs<11, BundleBounds>(B.skey[0], B.sval[0], B.skey[1], B.sval[1], &F.d_params->n_points, n, n, 0, true, points_sort_passes(I), ws, B.sort_info,
                                             s, nullptr, nullptr, counted, bounds);
  }
  return COX_OK;
}
// the merged record walk (RecordTiles, RecordsFullSort): few long rays, so one wave per ray (parallel DDA); the walk found by
// k_touch_wave is handed to k_emit_wave through the spare sort buffer.  Both read the frame's rays and its own tables only
// (cox_walk.hpp: FrameBlocks), so the plan may put them on the ray-generation stream (IntegratorPlan::walk_on_raygen) -- and there,
// with the small axis cap, the bundle merge does k_touch_wave's work itself (IntegratorPlan::touch_in_merge): emit is all that is left.
static FrameBlocks frame_blocks(const cox_integrator* I, const RecordSet& S) { return FrameBlocks{S.ft_keys, S.ft_ord, S.touched_slots, I->layer->ht_cap - 1}; }
static void record_walk(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  const IntegratorPlan& P = I->plan;
  FrameSet& F = *c.F;
  RecordSet& S = *c.S;
  const u32 fh_mask = I->fh_cap - 1;
  const FrameBlocks FB = frame_blocks(I, S);
  if (P.touch_in_merge) {
    // (done by stage_merge: the paths are parked in slots of steps_max words per ray)
  } else if (P.small_axis_cap)
    hipLaunchKernelGGL(k_touch_wave<kAxisCapSmall>, dim3(P.grid_touch), dim3(256), 0, s, F.d_params, F.rays, FB, S.rec_key[1], I->rcap, F.cnt, F.fh_keys, fh_mask);
  else
    hipLaunchKernelGGL(k_touch_wave<kAxisCapLarge>, dim3(2048), dim3(256), 0, s, F.d_params, F.rays, FB, S.rec_key[1], I->rcap, F.cnt, F.fh_keys, fh_mask);
  hipLaunchKernelGGL(k_emit_wave, dim3(P.grid_touch), dim3(256), 0, s, F.d_params, F.rays, FB, S.rec_key[1], S.rec_key[0], S.rec_ray[0], I->rcap, F.cnt, S.sort_info,
                     F.fh_keys, fh_mask, P.emit_flags(), P.touch_in_merge ? P.steps_max : 0u);
}
// one thread per block the frame touched (a few hundred at 5 cm, a few thousand at 2 cm); the grid strides.  Where the tile apply
// follows (RecordTiles), the binding is done at the head of stage U by k_block_starts_bind instead: one launch less on the chain.
static bool binds_in_apply(const cox_integrator* I) { return I->method == COX_METHOD_MERGED && I->plan.layer_update == LayerUpdate::RecordTiles; }
static void bind_blocks(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  if (binds_in_apply(I)) return;
  hipLaunchKernelGGL(k_bind_blocks, dim3(16), dim3(256), 0, s, layer_view(I->layer), frame_blocks(I, *c.S), c.S->ord_info, c.F->cnt, I->layer->d_err);
}
static int stage_merge(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  FrameSet& F = *c.F;
  BundleSet& B = *c.B;
  const u32 n = I->pcap;
  if (I->method == COX_METHOD_MERGED) {
    BundleView V{{B.skey[0], B.skey[1]}, {B.sval[0], B.sval[1]}, B.sort_info};
    {  // (the bundle boundaries were written by the sort's last pass)
      TimedRegion t(I, COX_KC_MERGE, s);
      if (I->plan.touch_in_merge) {  // the merge walks every ray it produces: it writes the record set's frame block table and path buffer
        const RecordSet& S = *c.S;
        const MergeWalk walk{frame_blocks(I, S), S.rec_key[1], I->plan.steps_max, I->rcap, F.fh_keys, I->fh_cap - 1};
        hipLaunchKernelGGL(k_bundle_merge<true>, dim3(I->plan.grid_merge), dim3(256), 0, s, F.d_params, V, B.bstart, F.rays, F.cnt, 0u, walk);
      } else {
        hipLaunchKernelGGL(k_bundle_merge<false>, dim3(I->plan.grid_merge), dim3(256), 0, s, F.d_params, V, B.bstart, F.rays, F.cnt,
                           I->plan.walks_pieces() ? (I->plan.small_axis_cap ? kAxisCapSmall : kAxisCapLarge) : 0u,  // (pieces: the rays' piece bounds)
                           MergeWalk{});
      }
    }
    // record offsets (and piece slots) of the rays: scanned here, on the ray-generation stream -- two frames' worth of it run
    // side by side, the layer-update chain is the one that bounds the frame rate
    const bool odd = I->st_alt && (c.slot & 1);
    const ScanWorkspace& ws = odd ? I->scanws_a : I->scanws_b;
    if (!I->plan.walks_pieces()) {
      hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, s, F.rays.nsteps, F.rays.rec_off, &F.cnt->n_ray_slots, I->pcap, &F.cnt->n_records);
    } else if (I->plan.small_axis_cap) {  // a few thousand bundles: one launch, one workgroup
      hipLaunchKernelGGL(k_scan_small2, dim3(1), dim3(1024), 0, s, F.rays.nsteps, F.rays.rec_off, &F.cnt->n_records, F.rays.pbound, F.rays.piece_off,
                         &F.cnt->n_piece_slots, &F.cnt->n_ray_slots, I->pcap);
    } else {  // fine voxels, 10^4-10^5 bundles: the three-kernel scans (the one-workgroup scan took 75 us at 1 cm)
      exclusive_scan_u32(F.rays.nsteps, F.rays.rec_off, &F.cnt->n_ray_slots, I->pcap, I->pcap, &F.cnt->n_records, ws, s);
      exclusive_scan_u32(F.rays.pbound, F.rays.piece_off, &F.cnt->n_ray_slots, I->pcap, I->pcap, &F.cnt->n_piece_slots, ws, s);
    }
  } else {
    hipLaunchKernelGGL(k_rays_simple, grid_for(n), dim3(256), 0, s, F.d_params, F.rays, F.cnt);
  }
  return COX_OK;
}
static int stage_touch(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  const IntegratorPlan& P = I->plan;
  FrameSet& F = *c.F;
  RecordSet& S = *c.S;
  const LayerView L = layer_view(I->layer);
  const u32 fh_mask = I->fh_cap - 1;
  if (P.walk_on_raygen) {  // the walk ran at the tail of stage M: the binding is all that is left (nothing, where the tile apply binds)
    bind_blocks(c, s);
    return COX_OK;
  }
  TimedRegion t_walk(I, COX_KC_TOUCH_EMIT, s);
  if (P.walks_pieces()) {
    const PieceArrays PA{S.pkey[0], S.pstart[0], S.prl[0], S.pbkey};
#define COX_LAUNCH_WALK(CAP, DEFER)                                                                                                                       \
  hipLaunchKernelGGL((k_touch_pieces<CAP, DEFER>), dim3(2048), dim3(256), 0, s, F.d_params, F.rays, L, S.touched_slots, S.lin8, PA, I->rcap, I->piece_cap, \
                     F.cnt, I->layer->d_err)
    if (P.expands_pieces()) {  // the walk defers the block touches: per piece, then ordinals by a scan over the layer's hash slots
      if (P.small_axis_cap)
        COX_LAUNCH_WALK(kAxisCapSmall, true);
      else
        COX_LAUNCH_WALK(kAxisCapLarge, true);
      hipLaunchKernelGGL(k_piece_touch, dim3(2048), dim3(256), 0, s, F.d_params, L, PA, I->rcap, I->piece_cap, S.touched_slots, F.cnt, I->layer->d_err);
      const u32 ht_cap = I->layer->ht_cap;
      hipLaunchKernelGGL(k_ord_flags, grid_for(ht_cap, 256, 4096), dim3(256), 0, s, F.d_params, L);
      exclusive_scan_u32(L.ht_ord, L.ht_ord, nullptr, ht_cap, ht_cap, &F.cnt->n_touched, I->scanws_h, s);
      hipLaunchKernelGGL(k_ord_scatter, grid_for(ht_cap, 256, 4096), dim3(256), 0, s, F.d_params, L, S.touched_slots);
    } else if (P.small_axis_cap) {
      COX_LAUNCH_WALK(kAxisCapSmall, false);
    } else {
      COX_LAUNCH_WALK(kAxisCapLarge, false);
    }
#undef COX_LAUNCH_WALK
    hipLaunchKernelGGL(k_piece_keys, dim3(1024), dim3(256), 0, s, L, S.pkey[0], I->rcap, I->piece_cap, F.cnt, S.sort_info, S.touched_slots, S.ord_info,
                       P.expands_pieces() ? P.tile_shift - kTileShift : 0u);
    return COX_OK;
  }
  if (I->method == COX_METHOD_MERGED) {  // (the record offsets are scanned at the end of stage M, off the layer-update chain)
    record_walk(c, s);
    bind_blocks(c, s);  // (behind emit, which still looks the ordinals up in the table the binding empties)
  } else {
    exclusive_scan_u32(F.rays.nsteps, F.rays.rec_off, &F.cnt->n_ray_slots, I->pcap, I->pcap, &F.cnt->n_records, I->scanws_b, s);
    hipLaunchKernelGGL(k_touch, grid_for(I->pcap, 256, 8192), dim3(256), 0, s, F.d_params, F.rays, L, S.touched_slots, F.cnt, I->layer->d_err, F.fh_keys, fh_mask);
    hipLaunchKernelGGL(k_emit, grid_for(I->pcap, 256, 8192), dim3(256), 0, s, F.d_params, F.rays, L, S.rec_key[0], S.rec_ray[0], I->rcap, F.cnt, S.sort_info,
                       F.fh_keys, fh_mask, S.touched_slots, S.ord_info, P.emit_flags());
  }
  return COX_OK;
}
static int stage_record_sort(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  const IntegratorPlan& P = I->plan;
  FrameSet& F = *c.F;
  RecordSet& S = *c.S;
  TimedRegion t_sort(I, COX_KC_RECORD_SORT, s);
  if (P.walks_pieces()) {
    // 4 + ceil(log2(touched blocks + 1)) key bits: one pass up to 255 touched blocks, two beyond
    (void)radix_sort_pairs<12>(S.pkey[0], S.pstart[0], S.pkey[1], S.pstart[1], &F.cnt->n_piece_slots, I->piece_cap, std::min<u32>(I->piece_cap, 1u << 21), 0,
                               true, 2, I->sort_rec, S.sort_info, s, S.prl[0], S.prl[1]);
    if (P.expands_pieces()) {  // sorted pieces -> records in tile order
      const u32 hint = std::min<u32>(I->piece_cap, 1u << 22);
      hipLaunchKernelGGL(k_piece_lens, grid_for(hint, 256, 8192), dim3(256), 0, s, S.pkey[0], S.pkey[1], S.prl[0], S.prl[1], S.sort_info, S.plen, F.cnt);
      exclusive_scan_u32(S.plen, S.pdest, &F.cnt->n_piece_slots, I->piece_cap, hint, &F.cnt->n_expanded, I->scanws_p, s);
      hipLaunchKernelGGL(k_piece_expand, dim3(8192), dim3(256), 0, s, S.pkey[0], S.pkey[1], S.pstart[0], S.pstart[1], S.prl[0], S.prl[1], S.sort_info, S.pdest,
                         S.lin8, S.rec_key[0], S.rec_ray[0], F.cnt);
      hipLaunchKernelGGL(k_piece_tile_ranges, grid_for(hint, 256, 8192), dim3(256), 0, s, S.pkey[0], S.pkey[1], S.sort_info, S.plen, S.pdest, S.blk_beg, S.blk_end, F.cnt,
                         P.tile_shift - kTileShift);
    }
    return COX_OK;
  }
  // 12 + ceil(log2(touched blocks + 1)) key bits, known on the device only: digits of up to 12 bits, so a full sort takes two passes
  // up to 4095 touched blocks (23 bits = 12 + 12 at 5 cm), three beyond.  Grid hint: ~2 M records keep every CU busy; larger frames
  // grid-stride.  Tile apply: ONE stable pass on the low 12 bits of the tile id (block ordinal, z slab) whatever the number of touched
  // blocks -- a partition into 4096 buckets; beyond 255 touched blocks several tiles share a bucket and the apply takes them in turn
  // (k_block_starts) -- or two passes on the whole tile id.
  (void)radix_sort_pairs<12>(S.rec_key[0], S.rec_ray[0], S.rec_key[1], S.rec_ray[1], &F.cnt->n_records, I->rcap, std::min<u32>(I->rcap, 1u << 21), 0, true,
                             P.record_sort_passes(), I->sort_rec, S.sort_info, s);
  return COX_OK;
}
// k_apply_block<ray lines left by the merge, log2(voxels per tile), buckets>: the instantiations in use
static void launch_apply_block(const StageCtx& c, hipStream_t s, const LayerView& L, const RecordView& V, bool merged, u32 tile_shift, bool bucket,
                               u32 min_records = 0, const BigTiles& big = BigTiles{nullptr, nullptr, nullptr, 0, 0, nullptr, 0}) {
  const cox_integrator* I = c.I;
#define COX_LAUNCH_APPLY(Q, TS, BUCKET)                                                                                                                    \
  hipLaunchKernelGGL((k_apply_block<Q, TS, BUCKET>), dim3(I->plan.grid_apply), dim3(kBT), 0, s, c.F->d_params, c.F->rays, L, c.S->ord_info, V, c.S->blk_beg, \
                     c.S->blk_end, c.F->cnt, I->layer->d_err, I->layer->h_nblocks, min_records, big)
  if (merged && tile_shift == 9 && !bucket)
    COX_LAUNCH_APPLY(true, 9, false);
  else if (merged && !bucket)
    COX_LAUNCH_APPLY(true, 8, false);
  else if (merged && tile_shift == 9)
    COX_LAUNCH_APPLY(true, 9, true);
  else if (merged)
    COX_LAUNCH_APPLY(true, 8, true);
  else if (bucket)  // (simple, fast: tiles of one z slab only)
    COX_LAUNCH_APPLY(false, 8, true);
  else
    COX_LAUNCH_APPLY(false, 8, false);
#undef COX_LAUNCH_APPLY
}
static int stage_apply(const StageCtx& c, hipStream_t s) {
  cox_integrator* I = c.I;
  const IntegratorPlan& P = I->plan;
  FrameSet& F = *c.F;
  RecordSet& S = *c.S;
  const LayerView L = layer_view(I->layer);
  const RecordView V{{S.rec_key[0], S.rec_key[1]}, {S.rec_ray[0], S.rec_ray[1]}, S.sort_info, &F.cnt->n_records};
  TimedRegion t(I, COX_KC_APPLY, s);
  switch (P.layer_update) {
    case LayerUpdate::RecordsFullSort:
      hipLaunchKernelGGL(k_apply_eval, dim3(4096), dim3(256), 0, s, F.d_params, F.rays, L, S.ord_info, V, S.piece_front, S.piece_back, S.piece_wsum, F.cnt);
      hipLaunchKernelGGL(k_apply_long, dim3(2048), dim3(256), 0, s, F.d_params, F.rays, L, S.ord_info, V, S.piece_front, S.piece_back, S.piece_wsum, F.cnt,
                         I->layer->d_err, I->layer->h_nblocks);
      break;
    case LayerUpdate::RecordTiles:
      if (binds_in_apply(I))
        hipLaunchKernelGGL(k_block_starts_bind, dim3(1024), dim3(256), 0, s, V, S.blk_beg, S.blk_end, F.cnt, P.tile_shift, P.bucket_partition ? 4095u : 0xFFFFFFFFu, L,
                           frame_blocks(I, S), S.ord_info, I->layer->d_err);
      else
        hipLaunchKernelGGL(k_block_starts, dim3(1024), dim3(256), 0, s, V, S.blk_beg, S.blk_end, F.cnt, P.tile_shift, P.bucket_partition ? 4095u : 0xFFFFFFFFu);
      launch_apply_block(c, s, L, V, I->method == COX_METHOD_MERGED, P.tile_shift, P.bucket_partition);
      break;
    case LayerUpdate::PiecesExpand: {  // (the tile ranges came with the expansion: k_piece_tile_ranges)
      const RecordView EV{{S.rec_key[0], S.rec_key[0]}, {S.rec_ray[0], S.rec_ray[0]}, S.sort_info, &F.cnt->n_expanded};  // one buffer: the parity is the piece sort's
      // fine voxels (cox_apply_tile.hpp): the largest tiles classified chunk by chunk by the whole chip, a workgroup per tile for the
      // large ones, a wave per tile for the rest
      const bool waves = P.tile_shift == 8 && P.wave_apply;
      const u32 min_records = waves ? P.wave_tile_max + 1 : 0;
      BigTiles big{nullptr, nullptr, nullptr, 0, 0, nullptr, 0};
      if (waves && P.split_big_tiles && S.big_chunks) {
        big = BigTiles{S.big_of_tile, S.big_acc, S.big_chunks, S.big_chunk_cap, P.big_chunk, S.blk_list, P.wave_tile_max};
        hipLaunchKernelGGL(k_big_tiles, dim3(512), dim3(256), 0, s, S.blk_beg, S.blk_end, S.ord_info, F.cnt, big);
        hipLaunchKernelGGL((k_big_classify<true>), dim3(P.grid_apply), dim3(kBT), 0, s, F.d_params, F.rays, S.ord_info, EV, S.blk_end, F.cnt, big);
      }
      launch_apply_block(c, s, L, EV, true, P.tile_shift, false, min_records, big);
      const dim3 gw(std::max(8u, P.grid_apply_wave & ~7u)), bw(kWaveTileWaves * 64);
      if (waves && P.wave_tile_max == 256)
        hipLaunchKernelGGL((k_apply_wave<256>), gw, bw, 0, s, F.d_params, F.rays, L, S.ord_info, EV, S.blk_beg, S.blk_end, F.cnt, I->layer->d_err, I->layer->h_nblocks);
      else if (waves)
        hipLaunchKernelGGL((k_apply_wave<512>), gw, bw, 0, s, F.d_params, F.rays, L, S.ord_info, EV, S.blk_beg, S.blk_end, F.cnt, I->layer->d_err, I->layer->h_nblocks);
      break;
    }
    case LayerUpdate::PiecesApply: {
      const RecordView KV{{S.pkey[0], S.pkey[1]}, {nullptr, nullptr}, S.sort_info, &F.cnt->n_piece_slots};
      const PieceView PV{{S.pkey[0], S.pkey[1]}, {S.pstart[0], S.pstart[1]}, {S.prl[0], S.prl[1]}, S.sort_info};
      hipLaunchKernelGGL(k_block_starts, dim3(1024), dim3(256), 0, s, KV, S.blk_beg, S.blk_end, F.cnt, 0u, 0xFFFFFFFFu);
      hipLaunchKernelGGL(k_apply_pieces, dim3(16384), dim3(kPT), 0, s, F.d_params, F.rays, L, S.ord_info, PV, S.lin8, S.blk_beg, S.blk_end, F.cnt, I->layer->d_err,
                         I->layer->h_nblocks);
      break;
    }
  }
  return COX_OK;
}
typedef int (*StageFn)(const StageCtx&, hipStream_t);
static const StageFn kStages[kNumStages] = {stage_hash, stage_point_sort, stage_merge, stage_touch, stage_record_sort, stage_apply};

// launch stage k of the frame in ctx on its stream: replay its graph (capturing it first if needed) or go eager
static int run_stage(int k, const StageCtx& c) {
  cox_integrator* I = c.I;
  hipStream_t s = stage_stream(I, k, c.slot);
  tl_frame_no = c.frame;
  if (!I->graphs_on || I->profiling || (k == 0 && c.n_dev)) return kStages[k](c, s);
  hipGraphExec_t& gx = I->graphs[k][c.slot];
  if (!gx) {
    hipGraph_t g = nullptr;
    COX_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    const int st = kStages[k](c, s);
    const hipError_t e = hipStreamEndCapture(s, &g);
    if (st != COX_OK || e != hipSuccess || !g) {
      if (g) (void)hipGraphDestroy(g);
      (void)hipGetLastError();
      I->graphs_on = false;  // capture not possible here: stay eager from now on
      return kStages[k](c, s);
    }
    const hipError_t ei = hipGraphInstantiate(&gx, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
      gx = nullptr;
      (void)hipGetLastError();
      I->graphs_on = false;
      return kStages[k](c, s);
    }
  }
  COX_HIP(hipGraphLaunch(gx, s));
  return COX_OK;
}

// ---- fast: one frame = three chains, each on a stream of its own, each in frame order (cox_fast.hpp):
//   front   (st[0], caller's thread)      start set -> ray list -> round-0 candidate lists (kFastCap0 steps per ray), sorted by slot;
//                                         touches the start table and this frame's own buffers only
//   solve   (st[1], submission thread)    relaxation of the observed set over the capped lists, whole walks for the rays that got
//                                         through them, relaxation again, commit to the observed table; frame t + 1's solve needs
//                                         the table frame t leaves, so this chain sets the frame rate
//   update  (st[3], submission thread)    the record pipeline of `simple` over every ray's first reach[r] voxels
// No host round trip anywhere: convergence, growth and overflow are decided on the device, the sweep launches of a round are
// enqueued speculatively (they return at once behind a launch that moved nothing), and a frame whose relaxation did not settle
// within them is redone by k_fast_sequential, exactly.
struct FastJob {
  FastFrame FF;
  bool wipe_obs = false;  // ApproxHashSet::resetApproxSet reached its full_reset_threshold: the table is zeroed
  int vs = 0;             // which round-0 visit set the front filled
};
static int fast_front(const StageCtx& c, FastJob* job) {
  cox_integrator* I = c.I;
  FrameSet& F = *c.F;
  BundleSet& B = *c.B;
  FastState& X = I->fast;
  const hipStream_t s = I->st[0];
  // FastTsdfIntegrator::integratePointCloud: both sets are reset every clear_checks_every_n_frames frames;
  // ApproxHashSet::resetApproxSet bumps the offset and wipes the table every 10 000 resets
  if (++X.reset_counter >= I->cfg.clear_checks_every_n_frames) {
    X.reset_counter = 0;
    if (++X.off_start >= kFastFullReset) {
      COX_HIP(hipMemsetAsync(X.table_start, 0, sizeof(u64) * kFastSlots, s));
      X.off_start = 0;
    }
    if (++X.off_obs >= kFastFullReset) {
      job->wipe_obs = true;  // (on the solve's stream, between the previous frame's commit and this frame's sweeps)
      X.off_obs = 0;
    }
  }
  const FastFrame FF{X.off_start, X.off_obs, I->cfg.max_consecutive_ray_collisions};
  job->FF = FF;
  job->vs = static_cast<int>(X.frames & 1u);
  X.frames += 1;
  VisitSet& V0 = X.vs0[job->vs];
  if (V0.used) COX_HIP(hipStreamWaitEvent(s, V0.done, 0));  // the solve of frame t-2 is done with this visit set
  const u32 n = I->pcap;
  const dim3 gp = grid_for(n, 256, 4096), gw(4096);  // gw: one wave per ray, grid-stride
  COX_HIP(hipMemcpyAsync(F.d_params, &I->h_params[c.slot], sizeof(FrameParams), hipMemcpyHostToDevice, s));
  if (c.n_dev) hipLaunchKernelGGL(k_params_count, dim3(1), dim3(1), 0, s, F.d_params, c.n_dev);
  COX_HIP(hipMemsetAsync(F.cnt, 0, sizeof(Counters), s));
  {
    // start set: sort the points by slot (21 key bits: slot + "not integrated"), compare neighbours
    TimedRegion t(I, COX_KC_FAST_START, s);
    hipLaunchKernelGGL(k_fast_points, gp, dim3(256), 0, s, F.d_params, FF, X.fhash, B.skey[0], B.sval[0], F.cnt);
    const int pp = radix_sort_pairs<11>(B.skey[0], B.sval[0], B.skey[1], B.sval[1], &F.d_params->n_points, n, n, kFastSlotBits + 1, false, 2, I->sort_pts, nullptr, s);
    hipLaunchKernelGGL(k_fast_start_flags, gp, dim3(256), 0, s, F.d_params, B.skey[pp], B.sval[pp], X.fhash, X.table_start, X.fresh);
    hipLaunchKernelGGL(k_fast_start_commit, gp, dim3(256), 0, s, F.d_params, B.skey[pp], B.sval[pp], X.fhash, X.table_start);
    exclusive_scan_u32(X.fresh, X.rank, &F.d_params->n_points, n, n, &F.cnt->n_rays, I->scanws_a, s);
    hipLaunchKernelGGL(k_fast_rays, gp, dim3(256), 0, s, F.d_params, X.fresh, X.rank, F.rays, X.cap[c.slot], X.reach[c.slot], I->plan.fast.cap0, V0.cap, F.cnt);
  }
  {
    // round 0's candidate visits: the first kFastCap0 voxels of every ray's walk, sorted by slot of the observed set (they depend on
    // this frame's rays only, so they are made here, beside the previous frame's solve)
    TimedRegion t(I, COX_KC_FAST_VISITS, s);
    if (I->plan.small_axis_cap)
      hipLaunchKernelGGL(k_fast_visits<kAxisCapSmall>, gw, dim3(256), 0, s, F.d_params, FF, F.rays, V0.vhash, V0.key[0], V0.val[0], V0.vray, V0.voff, X.cap[c.slot],
                         I->plan.fast.cap0, 0, F.cnt);
    else
      hipLaunchKernelGGL(k_fast_visits<kAxisCapLarge>, gw, dim3(256), 0, s, F.d_params, FF, F.rays, V0.vhash, V0.key[0], V0.val[0], V0.vray, V0.voff, X.cap[c.slot],
                         I->plan.fast.cap0, 0, F.cnt);
    V0.sorted = radix_sort_pairs<11>(V0.key[0], V0.val[0], V0.key[1], V0.val[1], &F.cnt->fast.n_visits[0], V0.cap, std::min<u32>(V0.cap, 1u << 19), kFastSlotBits + 1,
                                     false, 2, I->sort_vis, nullptr, s);
    hipLaunchKernelGGL(k_fast_inverse, dim3(512), dim3(256), 0, s, V0.key[V0.sorted], V0.val[V0.sorted], V0.vray, V0.vhash, V0.voff, V0.pos_of, V0.sinfo, V0.shash,
                       &F.cnt->fast.n_visits[0], V0.cap);
  }
  return COX_OK;
}
static inline FastVisits fast_view(const VisitSet& V) { return FastVisits{V.key[V.sorted], V.sinfo, V.shash, V.voff, V.pos_of}; }
static int fast_solve(const StageCtx& c, const FastJob& job) {
  cox_integrator* I = c.I;
  FrameSet& F = *c.F;
  FastState& X = I->fast;
  const hipStream_t s = I->st[1];
  const FastFrame FF = job.FF;
  VisitSet& V0 = X.vs0[job.vs];
  VisitSet& V1 = X.vs1;
  u32* cap = X.cap[c.slot];
  u32* reach = X.reach[c.slot];
  FastCtl* ctl = &F.cnt->fast;
  const u32* n_rays = &F.cnt->n_rays;
  const int mc = I->cfg.max_consecutive_ray_collisions;
  const dim3 gr = grid_for(I->pcap, 256, 1024), gw(4096);
  if (job.wipe_obs) COX_HIP(hipMemsetAsync(X.table_obs, 0, sizeof(u64) * kFastSlots, s));
  {
    TimedRegion t(I, COX_KC_FAST_SWEEPS, s);
    hipLaunchKernelGGL(k_fast_relax, dim3(I->plan.fast.relax_groups), dim3(kFastRelaxThreads), 0, s, fast_view(V0), mc, cap, F.rays.nsteps, X.table_obs, reach, ctl, 0,
                       X.long_list, n_rays, I->plan.fast.fences);
  }
  for (int round = 1; round < I->plan.fast.rounds; ++round) {
    // round 1 (every kernel returns at once when round 0 left nobody at the end of a capped list): whole walks for those rays, all
    // lists sorted again, relaxation from round 0's fixed point; further rounds (fine voxels: COX_FAST_ROUNDS) the same for the rays
    // that have outgrown their lists since
    TimedRegion t(I, COX_KC_FAST_ROUND1, s);
    hipLaunchKernelGGL(k_fast_grow, gr, dim3(256), 0, s, F.rays.nsteps, cap, reach, ctl, round, I->plan.fast.cap1, X.long_list, n_rays);
    if (I->pcap <= (1u << 15) || I->plan.fast.rounds == 2) {
      // one workgroup, 4 096 rays at a time: a frame at coarse voxels starts a few thousand rays (the three-launch scan and its
      // bookkeeping kernel were four of the solve chain's eighteen launches; a frame in which every point of a large cloud starts a ray
      // pays 0.2 ms here instead)
      hipLaunchKernelGGL(k_fast_scan_caps, dim3(1), dim3(1024), 0, s, cap, V1.voff, ctl, round, I->pcap, V1.cap);
    } else {  // (rays by the ten thousand, fine voxels: the three-launch scan; it covers scan_n rays, none without growth)
      exclusive_scan_u32(cap, V1.voff, &ctl->scan_n[round], I->pcap, I->pcap, &ctl->n_visits[round], I->scanws_f, s);
      hipLaunchKernelGGL(k_fast_scan_caps_done, dim3(1), dim3(1), 0, s, ctl, round, V1.cap);
    }
    if (I->plan.small_axis_cap)
      hipLaunchKernelGGL(k_fast_visits<kAxisCapSmall>, gw, dim3(256), 0, s, F.d_params, FF, F.rays, V1.vhash, V1.key[0], V1.val[0], V1.vray, V1.voff, cap, 0u, round,
                         F.cnt);
    else
      hipLaunchKernelGGL(k_fast_visits<kAxisCapLarge>, gw, dim3(256), 0, s, F.d_params, FF, F.rays, V1.vhash, V1.key[0], V1.val[0], V1.vray, V1.voff, cap, 0u, round,
                         F.cnt);
    V1.sorted = radix_sort_pairs<11>(V1.key[0], V1.val[0], V1.key[1], V1.val[1], &ctl->n_visits[round], V1.cap, std::min<u32>(V1.cap, 1u << 19), kFastSlotBits + 1, false,
                                     2, I->sort_vis1, nullptr, s);
    hipLaunchKernelGGL(k_fast_inverse, dim3(512), dim3(256), 0, s, V1.key[V1.sorted], V1.val[V1.sorted], V1.vray, V1.vhash, V1.voff, V1.pos_of, V1.sinfo, V1.shash,
                       &ctl->n_visits[round], V1.cap);
    hipLaunchKernelGGL(k_fast_relax, dim3(I->plan.fast.relax_groups), dim3(kFastRelaxThreads), 0, s, fast_view(V1), mc, cap, F.rays.nsteps, X.table_obs, reach, ctl, round,
                       X.long_list, n_rays, I->plan.fast.fences);
  }
  // (the relaxation packs (ray, step) into one word: a configuration whose walks or ray counts do not fit takes the sequential kernel)
  const bool packed_ok = I->plan.steps_max <= kFastStepMask && I->pcap <= (1u << (32 - kFastStepBits));
  hipLaunchKernelGGL(k_fast_sequential, dim3(1), dim3(64), 0, s, F.d_params, FF, F.rays, X.table_obs, reach, ctl, (I->plan.fast.force_sequential || !packed_ok) ? 1 : 0, n_rays);
  hipLaunchKernelGGL(k_fast_obs_commit, dim3(512), dim3(256), 0, s, fast_view(V0), fast_view(V1), reach, X.table_obs, ctl, V0.cap, V1.cap, X.d_stats, F.rays, F.cnt);
  COX_HIP(hipEventRecord(V0.done, s));
  V0.used = true;
  return COX_OK;
}

// Layer::allocateBlockPtrByIndex never fails in voxblox.  The last kernel of every frame leaves the block count in a pinned
// word; once the pool is half full (or the recent rate of allocation says it will be) it is doubled before the next frame is
// enqueued (a frame that still runs out reports
// COX_ERR_POOL_EXHAUSTED at sync, and so does every later frame that meets one of its blocks).  The buffers sized by the
// layer's hash capacity follow the layer whenever it has been reallocated (by this or by cox_layer_reserve / upload).
static int follow_layer(cox_integrator* I) {
  cox_layer* Lh = I->layer;
  // The count the host sees is up to a dozen frames old (frames in flight), so "half full" alone reacts too late when frames
  // allocate fast (2 cm: hundreds of blocks per frame): the largest increase seen between two looks, times the frames that may
  // be in flight, has to fit as well (found by the 600-frame soak test with a small pool).
  const u64 n_seen = *Lh->h_nblocks;
  if (n_seen > I->blocks_seen) I->blocks_delta_max = std::max<u64>(I->blocks_delta_max, n_seen - I->blocks_seen);
  I->blocks_seen = n_seen;
  const u64 need = std::max<u64>(2 * n_seen, n_seen + 12 * I->blocks_delta_max);  // (host ahead of stage H by <= 6 frames, H ahead of U by <= 6)
  if (Lh->auto_grow && need > Lh->capacity && Lh->capacity < (1ull << 26)) {
    COX_TRY(sync_all(I));
    u64 cap = Lh->capacity;
    while (cap < need && cap < (1ull << 26)) cap *= 2;
    const int st = cox_internal_layer_reserve(Lh, std::min<u64>(cap, 1ull << 26));
    if (st != COX_OK && st != COX_ERR_OUT_OF_MEMORY) return st;  // out of memory: carry on with what there is
    if (st == COX_ERR_OUT_OF_MEMORY) Lh->auto_grow = false;
  }
  if (I->layer_generation != Lh->generation) {
    COX_TRY(sync_all(I));
    drop_graphs(I);
    COX_TRY(alloc_layer_sized(I));
  }
  return COX_OK;
}

// Ordering of one frame's inputs against whoever produces them (the engine's own input stream: staged host buffers, converted depth
// images), besides the caller's stream of cox_integrator_set_input_stream:
//   ready      the frame's first stage waits for it                 consumed   recorded once the inputs have been read for the last time
//   n_dev      the point count, where only the device knows it (n is then an upper bound)
struct FrameInput {
  hipEvent_t ready = nullptr, consumed = nullptr;
  const u32* n_dev = nullptr;
  int staging_set = -1;  // the staging set the inputs are in (an attached observation record orders itself against its events)
};
// enqueue the whole frame; xyz / rgba are device pointers that must stay valid until the frame's stage M is done
static int integrate_device(cox_integrator* I, const float T[7], const float* xyz, const uint8_t* rgba, u32 n, int freespace, bool caller_waits = false,
                            const FrameInput& in = FrameInput()) {
  cox_layer* Lh = I->layer;
  struct HostTimer {
    cox_integrator* I;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~HostTimer() {
      I->host_ns += static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count());
      I->host_frames += 1;
    }
  } host_timer{I};
  // every frame but the previous one has been enqueued completely: the events this frame waits for (F.done of frame t-6,
  // B.done of t-3) are recorded, and the sets frame t-3 used are not touched by the submission thread any more
  {
    const auto w0 = std::chrono::steady_clock::now();
    if (I->submitter) I->submitter->wait_outstanding(1);
    I->host_wait_ns += static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - w0).count());
  }
  // (first: a projective integrator that wrote last settles its frames here and may grow the layer, which follow_layer picks up)
  const bool foreign_writer = (n != 0 || I->method == COX_METHOD_FAST) && cox_layer_order_writer(Lh, I);
  COX_TRY(ensure_capacity(I, n));
  COX_TRY(follow_layer(I));
  I->last = cox_frame_stats{};
  I->last.n_points = n;
  I->last_has_counts = false;
  // (an empty cloud still resets the fast integrator's two sets, as FastTsdfIntegrator::integratePointCloud does before it looks at a point)
  if (n == 0 && I->method != COX_METHOD_FAST) return COX_OK;
  I->frame_no += 1;
  const int slot = static_cast<int>(I->frame_no % kFrameSets);
  FrameSet& F = I->fs[slot];
  BundleSet& B = I->bs[slot % kStageSets];
  RecordSet& S = I->rs[slot % kStageSets];
  const StageCtx ctx{I, &F, &B, &S, slot, I->frame_no, in.n_dev};
  tl_frame_no = I->frame_no;
  I->last_count_on_device = in.n_dev != nullptr;
  // the pinned parameter slot is free once the copy of the frame that used it last (t-6) has run
  if (F.used) {
    const auto w0 = std::chrono::steady_clock::now();
    COX_HIP(hipEventSynchronize(F.params_copied));
    I->host_wait_ns += static_cast<uint64_t>(std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - w0).count());
  }
  FrameParams P = make_params(I, T, n, freespace, xyz, rgba);
  P.frame_id = ++Lh->frame_id;
  I->h_params[slot] = P;

  if (I->has_producer) {  // inputs written on the caller's stream: stage H starts after them
    COX_HIP(hipEventRecord(I->ev_producer, I->producer));
    COX_HIP(hipStreamWaitEvent(stage_stream(I, 0, slot), I->ev_producer, 0));
  }
  if (in.ready) COX_HIP(hipStreamWaitEvent(stage_stream(I, 0, slot), in.ready, 0));
  if (I->obs && n) {  // the record marks the same cloud on its own stream: behind the inputs' producer, beside everything else
    const int k = in.staging_set;
    hipEvent_t read = k >= 0 ? I->obs_read[k] : I->ev_obs_read;
    COX_TRY(cox_internal_obs_record(I->obs, T, xyz, n, freespace, I->cfg.min_ray_length_m, I->cfg.max_ray_length_m, I->cfg.allow_clear,
                                    I->has_producer ? I->ev_producer : nullptr, k >= 0 ? I->in_ready[k] : nullptr, read, false));
    if (k >= 0) I->obs_used[k] = true;
    if (I->has_producer) COX_HIP(hipStreamWaitEvent(I->producer, read, 0));  // the caller's stream may overwrite / free the cloud after that
  }
  if (I->method == COX_METHOD_FAST) {  // front on st[0] (this thread), solve on st[1] and update on st[3] (submission thread): fast_front / fast_solve
    if (F.used) COX_HIP(hipStreamWaitEvent(I->st[0], F.done, 0));  // frame t-6 is done with this frame set
    FastJob job;
    COX_TRY(fast_front(ctx, &job));
    COX_HIP(hipEventRecord(F.params_copied, I->st[0]));
    COX_HIP(hipEventRecord(F.hand[0], I->st[0]));
    if (I->has_producer) {  // the inputs are read by the front only
      COX_HIP(hipEventRecord(I->ev_inputs_read, I->st[0]));
      COX_HIP(hipStreamWaitEvent(I->producer, I->ev_inputs_read, 0));
    }
    if (in.consumed) COX_HIP(hipEventRecord(in.consumed, I->st[0]));
    COX_HIP(hipGetLastError());
    auto back = [ctx, job, foreign_writer]() -> int {
      cox_integrator* I = ctx.I;
      FrameSet& F = *ctx.F;
      RecordSet& S = *ctx.S;
      cox_layer* Lh = I->layer;
      tl_frame_no = ctx.frame;
      COX_HIP(hipStreamWaitEvent(I->st[1], F.hand[0], 0));
      COX_TRY(fast_solve(ctx, job));
      COX_HIP(hipEventRecord(F.hand[2], I->st[1]));
      COX_HIP(hipStreamWaitEvent(I->st[3], F.hand[2], 0));
      if (foreign_writer) cox_layer_wait_writes(Lh, I->st[3]);  // another integrator wrote this layer last
      COX_TRY(run_stage(3, ctx));  // touch / emit, record partition, apply on st[3] == st[4] == st[5]
      COX_TRY(run_stage(4, ctx));
      COX_TRY(run_stage(5, ctx));
      COX_HIP(hipEventRecord(F.done, I->st[5]));
      COX_HIP(hipEventRecord(S.done, I->st[5]));
      COX_HIP(hipEventRecord(Lh->last_write, I->st[5]));
      Lh->has_write = true;
      F.used = true;
      S.used = true;
      COX_HIP(hipGetLastError());
      return COX_OK;
    };
    if (I->submitter && !caller_waits) {
      I->submitter->post(back);
    } else {
      if (I->submitter) I->submitter->wait_outstanding(0);
      COX_TRY(back());
    }
    I->last_has_counts = true;
    return COX_OK;
  }
  // stage k + 1 of a frame follows stage k: in stream order, or behind the frame slot's hand-over event when on another stream
  auto chain = [](const StageCtx& x, int k) -> int {  // run stage k behind stage k - 1
    cox_integrator* I = x.I;
    const hipStream_t sk = stage_stream(I, k, x.slot);
    if (k > 0 && sk != stage_stream(I, k - 1, x.slot)) COX_HIP(hipStreamWaitEvent(sk, x.F->hand[k - 1], 0));
    COX_TRY(run_stage(k, x));
    if (k + 1 < kNumStages && stage_stream(I, k + 1, x.slot) != sk) COX_HIP(hipEventRecord(x.F->hand[k], sk));
    return COX_OK;
  };
  const hipStream_t s_h = stage_stream(I, 0, slot), s_m = stage_stream(I, 2, slot);
  // H, P, M (ray generation: depends on the frame's input only)
  if (F.used && s_h != I->st[5]) COX_HIP(hipStreamWaitEvent(s_h, F.done, 0));  // frame t-6 is done with this frame set
  if (B.used && (I->st_alt || s_h != s_m)) COX_HIP(hipStreamWaitEvent(s_h, B.done, 0));  // frame t-3's merge (on the other ray-generation stream, or on M's) is done with this bundle set
  COX_TRY(chain(ctx, 0));
  COX_HIP(hipEventRecord(F.params_copied, s_h));
  COX_TRY(chain(ctx, 1));
  // Where the merge does the walk (touch_in_merge) it writes the frame's record set -- the frame block table and the parked paths -- so
  // the wait for the apply of the frame that used the set last, t-3, stands in front of stage M instead of in front of the walk (below;
  // the same reasoning makes S.done and S.used safe to read here).  B.done and the inputs-read events are then recorded behind that wait.
  if (I->plan.touch_in_merge && S.used) COX_HIP(hipStreamWaitEvent(s_m, S.done, 0));
  COX_TRY(chain(ctx, 2));
  COX_HIP(hipEventRecord(B.done, s_m));
  B.used = true;
  if (I->has_producer) {  // the inputs are not read after the merge: later work on the caller's stream may overwrite / free them
    COX_HIP(hipEventRecord(I->ev_inputs_read, s_m));
    COX_HIP(hipStreamWaitEvent(I->producer, I->ev_inputs_read, 0));
  }
  if (in.consumed) COX_HIP(hipEventRecord(in.consumed, s_m));
  // The record walk, where the plan puts it on the ray-generation stream (behind everything above: the bundle set and the inputs are
  // not kept waiting for it).  It writes the frame's record set from this thread, so it follows the apply of the frame that used the
  // set last, t-3.  That frame's stage U has been enqueued -- the submission thread is at most one frame behind (wait_outstanding(1)
  // above) -- so S.done is recorded and S.used is there to read.  Three record sets: the lanes run at most three frames ahead of
  // the update.
  if (I->plan.walk_on_raygen) {
    if (S.used && !I->plan.touch_in_merge) COX_HIP(hipStreamWaitEvent(s_m, S.done, 0));
    {
      TimedRegion t_walk(I, COX_KC_TOUCH_EMIT, s_m);  // (touch_in_merge: emit alone; the touch is in the merge's class)
      record_walk(ctx, s_m);
    }
    if (stage_stream(I, 3, slot) != s_m) COX_HIP(hipEventRecord(F.hand[2], s_m));  // stage T waits for the walk, not only for the merge
  }
  COX_HIP(hipGetLastError());
  // T, R, U (layer update): on the submission thread when there is one
  auto stage_b = [ctx, chain, foreign_writer]() -> int {
    cox_integrator* I = ctx.I;
    FrameSet& F = *ctx.F;
    RecordSet& S = *ctx.S;
    cox_layer* Lh = I->layer;
    if (S.used && I->st[3] != I->st[5]) COX_HIP(hipStreamWaitEvent(I->st[3], S.done, 0));  // frame t-3's apply is done with this record set
    if (foreign_writer) cox_layer_wait_writes(Lh, I->st[3]);  // another integrator wrote this layer last: stage T (block touches) follows its frames
    COX_TRY(chain(ctx, 3));
    COX_TRY(chain(ctx, 4));
    COX_TRY(chain(ctx, 5));
    COX_HIP(hipEventRecord(F.done, I->st[5]));
    COX_HIP(hipEventRecord(S.done, I->st[5]));
    COX_HIP(hipEventRecord(Lh->last_write, I->st[5]));
    Lh->has_write = true;
    F.used = true;
    S.used = true;
    COX_HIP(hipGetLastError());
    return COX_OK;
  };
  if (I->submitter && !caller_waits) {
    I->submitter->post(stage_b);
  } else {  // a caller that waits for the frame anyway (cox_integrate_points) gains nothing from the hand-over
    if (I->submitter) I->submitter->wait_outstanding(0);
    COX_TRY(stage_b());
  }
  I->last_has_counts = true;
  return COX_OK;
}

// the last frame's device counters are fetched when somebody asks (sync / last_stats), not once per frame: its frame
// set is not reused before five more frames have been enqueued.  Call with all streams idle.
static int fold_counters(cox_integrator* I) {
  if (!I->last_has_counts) return COX_OK;
  Counters& c = I->h_ring[I->frame_no % kStatRing];
  COX_HIP(hipMemcpy(&c, I->fs[I->frame_no % kFrameSets].cnt, sizeof(Counters), hipMemcpyDeviceToHost));
  if (I->last_count_on_device) {  // (depth front end: the host never saw the frame's point count)
    u32 np = 0;
    COX_HIP(hipMemcpy(&np, &I->fs[I->frame_no % kFrameSets].d_params->n_points, sizeof(u32), hipMemcpyDeviceToHost));
    I->last.n_points = np;
  }
  u64 sh[5] = {0, 0, 0, 0, 0};
  u32 max_bundle = 0, max_run = 0;
  for (int s = 0; s < 64; ++s) {
    for (int k = 0; k < 5; ++k) sh[k] += c.shard[s][k];
    max_bundle = std::max(max_bundle, c.shard[s][kShMaxBundle]);
    max_run = std::max(max_run, c.shard[s][kShMaxRun]);
  }
  I->last.max_bundle_points = max_bundle;
  I->last.max_voxel_updates = max_run;
  I->last.n_valid = sh[kShValid];
  I->last.n_rays = (I->method == COX_METHOD_SIMPLE) ? sh[kShRays] : c.n_rays;
  I->last.n_updates = sh[kShUpdates];
  I->last.n_touched_voxels = sh[kShVoxels];
  I->last.n_touched_blocks = c.n_touched;
  I->last.n_new_blocks = c.n_new_blocks;
  I->last_big_tiles = c.n_big_tiles;
  I->last_big_chunks = c.n_big_chunks;
  I->last_has_counts = false;  // folded; I->last keeps the numbers
  return COX_OK;
}

// COX_TIMELINE=<file>: every timed region as "class start_ms end_ms" relative to the moment profiling was switched on
// (hipEventElapsedTime works across streams) -- how the stages of neighbouring frames overlap, without a profiler attached
static void drain_events(std::vector<std::pair<hipEvent_t, hipEvent_t>>& evs, double* ms_acc, uint64_t* n_acc, std::vector<hipEvent_t>* pool, int cls = -1,
                         hipEvent_t ref = nullptr, FILE* timeline = nullptr) {
  for (auto& ev : evs) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
      *ms_acc += ms;
      *n_acc += 1;
    }
    if (timeline && ref) {
      float a = 0.0f, b = 0.0f;
      if (hipEventElapsedTime(&a, ref, ev.first) == hipSuccess && hipEventElapsedTime(&b, ref, ev.second) == hipSuccess)
        fprintf(timeline, "%d %.4f %.4f\n", cls, a, b);
    }
    pool->push_back(ev.first);
    pool->push_back(ev.second);
  }
  evs.clear();
}

// wait for all stages, fold the last frame's counters into the stats, return deferred errors
static int integrator_finish(cox_integrator* I) {
  COX_TRY(sync_all(I));
  COX_TRY(fold_counters(I));
  // errors of every frame since the last sync are sticky in the layer's device error word; report them once
  u32 lerr = 0;
  COX_HIP(hipMemcpy(&lerr, I->layer->d_err, sizeof(u32), hipMemcpyDeviceToHost));
  if (lerr) {
    COX_HIP(hipMemset(I->layer->d_err, 0, sizeof(u32)));
    COX_HIP(hipDeviceSynchronize());  // default-stream memset: the engine's streams would not wait for it
  }
  for (int k = 0; k < COX_KERNEL_CLASSES; ++k)
    drain_events(I->class_events[k], &I->class_ms[k], &I->class_regions[k], &I->event_pool[event_pool_of(I, k)], k, I->timeline_ref, I->timeline);
  if (I->timeline) fflush(I->timeline);
  return err_bits_to_status(lerr);
}

cox_layer* cox_internal_integrator_layer(cox_integrator_t* integ) { return integ->layer; }

// streams (in the order that is load-bearing, see below), events and every buffer that does not depend on the point capacity
static int integrator_init(cox_integrator* I) {
  const IntegratorPlan& P = I->plan;
  // Creation order is load-bearing, and what it buys depends on the queue budget (scripts/queue_probe.hip):
  //  * Ample queues (16, after cox_runtime_prepare()): every stream has a hardware queue of its own, and the queues of a process are
  //    spread over the four pipes of the compute micro-engine in creation order.  Four stage streams created back to back sit on four
  //    different pipes; the input stream (host buffers -> staging sets), created FIRST and directly in front of them, lands on the
  //    pipe of the LAST of them -- the apply's (two long kernels per frame), the partner that minds least (sharing with T/R costs
  //    35 %, with a ray-generation stream 45 %).  `fast` has three stage streams: its input stream has a pipe to itself.
  //  * A tight budget (4 queues, the runtime's default): the null stream keeps one queue and the created streams are dealt onto the
  //    other three -- the fourth stream of the process onto the queue of the third, the fifth onto the second's.  The plan then has at
  //    most three streams and NO input stream (an idle stream created first would take one of the three queues for nothing), so the
  //    streams below have a queue each whenever this integrator's are the first streams the process creates; host inputs are copied
  //    on the frame's own ray-generation stream.
  if (P.input_stream) COX_HIP(hipStreamCreateWithFlags(&I->st_in, hipStreamNonBlocking));
  if (P.alt_raygen_stream) COX_HIP(hipStreamCreateWithFlags(&I->st_alt, hipStreamNonBlocking));
  for (int k = 0; k < kNumStages; ++k) {
    if (k > 0 && P.stage_stream[k] == P.stage_stream[k - 1])
      I->st[k] = I->st[k - 1];
    else
      COX_HIP(hipStreamCreateWithFlags(&I->st[k], hipStreamNonBlocking));
  }
  for (int k = 0; k < kInputSets; ++k) {
    COX_TRY(make_event(I, &I->in_ready[k]));
    COX_TRY(make_event(I, &I->in_free[k]));
  }
  COX_TRY(make_event(I, &I->ev_producer));
  COX_TRY(make_event(I, &I->ev_inputs_read));
  for (FrameSet& F : I->fs) {
    COX_TRY(make_event(I, &F.done));
    COX_TRY(make_event(I, &F.params_copied));
    for (hipEvent_t& h : F.hand) COX_TRY(make_event(I, &h));
    COX_TRY(dev_realloc(I, &F.cnt, 1));
    COX_TRY(dev_realloc(I, &F.d_params, 1));
  }
  for (BundleSet& B : I->bs) {
    COX_TRY(make_event(I, &B.done));
    COX_TRY(dev_realloc(I, &B.sort_info, 1));
    COX_HIP(hipMemset(B.sort_info, 0, sizeof(SortInfo)));
  }
  for (RecordSet& S : I->rs) {
    COX_TRY(make_event(I, &S.done));
    COX_TRY(dev_realloc(I, &S.sort_info, 1));
    COX_HIP(hipMemset(S.sort_info, 0, sizeof(SortInfo)));
    if (P.expands_pieces()) {
      COX_TRY(dev_realloc(I, &S.big_acc, static_cast<size_t>(kBigCap) * 2 * kTileVox));
      COX_HIP(hipMemset(S.big_acc, 0, sizeof(u32) * kBigCap * 2 * kTileVox));
    }
  }
  COX_TRY(alloc_layer_sized(I));
  COX_TRY(pinned_realloc(I, &I->h_ring, kStatRing));
  COX_TRY(pinned_realloc(I, &I->h_params, kFrameSets));
  memset(I->h_ring, 0, sizeof(Counters) * kStatRing);
  memset(I->h_params, 0, sizeof(FrameParams) * kFrameSets);
  COX_TRY(dev_realloc(I, &I->d_depth_n, kInputSets));
  if (I->method == COX_METHOD_FAST) {
    FastState& X = I->fast;
    COX_TRY(dev_realloc(I, &X.table_start, kFastSlots));
    COX_TRY(dev_realloc(I, &X.table_obs, kFastSlots));
    COX_TRY(dev_realloc(I, &X.d_stats, 16));
    COX_HIP(hipMemset(X.table_start, 0, sizeof(u64) * kFastSlots));
    COX_HIP(hipMemset(X.table_obs, 0, sizeof(u64) * kFastSlots));
    COX_HIP(hipMemset(X.d_stats, 0, sizeof(u32) * 16));
    COX_TRY(make_event(I, &X.vs0[0].done));
    COX_TRY(make_event(I, &X.vs0[1].done));
  }
  COX_TRY(ensure_capacity(I, 640 * 480));
  // the initialising hipMemsets above ran on the legacy default stream; the engine's streams are non-blocking and do not
  // wait for it (found by the fuzz campaign: a table read before it had been cleared, once in 1 500 cases)
  COX_HIP(hipDeviceSynchronize());
  return COX_OK;
}
static void start_submitter(cox_integrator* I) {
  I->submitter = new (std::nothrow) Submitter();
  if (!I->submitter) return;
  I->submitter->device = I->layer->device;
  I->submitter->th = std::thread([sub = I->submitter] { sub->run(); });
  {
    // the thread's first HIP call initialises per-thread runtime state: let it finish before the caller goes on making
    // HIP calls of its own (a caller's next call once failed with a stray "invalid device ordinal" right after a create)
    std::unique_lock<std::mutex> lk(I->submitter->m);
    I->submitter->cv_done.wait(lk, [&] { return I->submitter->ready; });
  }
  std::lock_guard<std::mutex> lk(g_submitters_mutex);
  g_submitters.push_back(I->submitter);
}
static void stop_submitter(cox_integrator* I) {
  if (!I->submitter) return;
  {
    std::lock_guard<std::mutex> lk(g_submitters_mutex);
    g_submitters.erase(std::remove(g_submitters.begin(), g_submitters.end(), I->submitter), g_submitters.end());
  }
  {
    std::lock_guard<std::mutex> lk(I->submitter->m);
    I->submitter->stop = true;
  }
  I->submitter->cv_job.notify_all();
  if (I->submitter->th.joinable()) I->submitter->th.join();
  delete I->submitter;
  I->submitter = nullptr;
}

extern "C" {

int cox_integrator_create(cox_layer_t* layer, const cox_tsdf_config* cfg, int method, cox_integrator_t** out) {
  COX_ENTRY();
  if (!layer || !cfg || !out) return COX_ERR_INVALID_ARG;
  const bool projective = method == COX_METHOD_PROJECTIVE;
  if (!projective && method != COX_METHOD_SIMPLE && method != COX_METHOD_MERGED && method != COX_METHOD_FAST) return COX_ERR_INVALID_ARG;
  if (!projective && cfg->integration_order_mode != 0) return COX_ERR_UNSUPPORTED;
  if (method == COX_METHOD_FAST) {
    // reproduced: the reference at integrator_threads = 1 (with more threads its two lossy sets race and the result is
    // not reproducible even by itself).  Not reproduced: a wall-clock budget, and the oracle-only exact-set variant.
    if (cfg->max_integration_time_s < 3.0e38f || cfg->fast_exact_sets != 0) return COX_ERR_UNSUPPORTED;
    if (cfg->clear_checks_every_n_frames < 1 || cfg->max_consecutive_ray_collisions < 0 || !(cfg->start_voxel_subsampling_factor > 0.0f)) return COX_ERR_INVALID_ARG;
  }
  if (!(cfg->default_truncation_distance > 0.0f) || !(cfg->max_weight > 0.0f) || !(cfg->max_ray_length_m > 0.0f)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(layer->device));
  // (the environment, then the queue budget -- a trailing argument that tests/cpp/plan_smoke.cpp leaves out)
  const int hw_queues = cox_internal_hw_queues();
  cox_integrator* I = new (std::nothrow) cox_integrator(projective ? IntegratorPlan() : cox_plan::resolve_plan(method, *cfg, layer->voxel_size, (std::getenv), hw_queues));
  if (!I) return COX_ERR_OUT_OF_MEMORY;
  I->layer = layer;
  I->cfg = *cfg;
  I->method = method;
  const int st = projective ? cox_proj_create(layer, cfg, &I->proj) : integrator_init(I);
  if (st != COX_OK) {
    cox_integrator_destroy(I);
    return st;
  }
  if (!projective && I->plan.submit_thread) start_submitter(I);
  (void)hipGetLastError();  // nothing of ours stays in the thread's sticky error slot (other HIP users in the process check it after their own calls)
  *out = I;
  return COX_OK;
}

void cox_integrator_destroy(cox_integrator_t* I) {
  if (!I) return;
  if (I->proj) {
    cox_proj_destroy(I->proj);
    delete I;
    return;
  }
  (void)hipSetDevice(I->layer->device);
  (void)sync_all(I);
  stop_submitter(I);
  delete I->copy_pool;
  drop_graphs(I);
  // profiling events come and go with the frames; everything else is in the ownership lists
  for (auto& evs : I->class_events)
    for (auto& e : evs) {
      (void)hipEventDestroy(e.first);
      (void)hipEventDestroy(e.second);
    }
  for (auto& pool : I->event_pool)
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  if (I->timeline_ref) (void)hipEventDestroy(I->timeline_ref);
  if (I->timeline) fclose(I->timeline);
  release_owned(I);
  for (int k = 0; k < kNumStages; ++k)
    if (I->st[k] && (k == 0 || I->st[k] != I->st[k - 1])) (void)hipStreamDestroy(I->st[k]);
  if (I->st_alt) (void)hipStreamDestroy(I->st_alt);
  if (I->st_in) (void)hipStreamDestroy(I->st_in);
  delete I;
  (void)hipGetLastError();
}

int cox_integrate_points_dev(cox_integrator_t* I, const float T_G_C[7], const float* xyz_dev, const uint8_t* rgba_dev, uint64_t n, int freespace) {
  COX_ENTRY_NO_DRAIN();
  if (!I || !T_G_C || (n && !xyz_dev) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(I->layer->device));
  if (I->proj) return cox_proj_integrate(I->proj, T_G_C, xyz_dev, n, 0);
  return integrate_device(I, T_G_C, xyz_dev, rgba_dev, static_cast<u32>(n), freespace);
}

int cox_integrate_points_ex(cox_integrator_t* I, const float T_G_C[7], const float* xyz, const uint8_t* rgba, uint64_t n, int freespace, int deintegrate) {
  if (!I) return COX_ERR_INVALID_ARG;
  if (!deintegrate) return cox_integrate_points(I, T_G_C, xyz, rgba, n, freespace);
  COX_ENTRY();
  if (!I->proj) return COX_ERR_UNSUPPORTED;  // only the projective integrator can take a cloud out again
  if (!T_G_C || (n && !xyz) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(I->layer->device));
  return cox_proj_integrate_host(I->proj, T_G_C, xyz, n, 1);
}

// Host buffers -> staging set k of the frame about to be enqueued, on that frame's ray-generation stream, without waiting for
// anything but the staging set itself.  Pageable memory goes through a pinned bounce buffer (one CPU copy; the caller's buffer is
// free again when the call returns), pinned memory is copied from directly.
// -> the address the device reads the buffer at (pinned memory is mapped), nullptr for pageable memory
static const void* host_pointer_device_view(const void* p) {
  hipPointerAttribute_t a;
  const hipError_t e = hipPointerGetAttributes(&a, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // pageable memory is "invalid value" to the runtime
    return nullptr;
  }
  if (a.type != hipMemoryTypeHost) return nullptr;
  return a.devicePointer ? a.devicePointer : p;
}
// what k_copy_from_host is told about one array of `bytes` (a multiple of 4; both addresses 16-byte aligned): whole 16 bytes, then words
static inline HostSegment host_segment(void* dst, const void* src_dev, size_t bytes) {
  return HostSegment{static_cast<U32x4*>(dst), static_cast<const U32x4*>(src_dev), bytes / 16, static_cast<u32>((bytes & 15u) / 4)};
}
// one or two arrays (bytes a multiple of 4) from pinned host memory, seen by the device at src_dev_*, to dst_* on stream s
static int copy_pinned_to_device(const cox_integrator* I, void* dst_a, const void* src_a, const void* src_dev_a, size_t bytes_a, void* dst_b, const void* src_b,
                                 const void* src_dev_b, size_t bytes_b, hipStream_t s) {
  const bool use_memcpy = !I->plan.h2d_kernel;
  const int groups = I->plan.h2d_groups;
  auto unaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) != 0; };
  const bool two = dst_b != nullptr;
  if (use_memcpy || !src_dev_a || unaligned(src_dev_a) || unaligned(dst_a) || (bytes_a & 3u) ||
      (two && (!src_dev_b || unaligned(src_dev_b) || unaligned(dst_b) || (bytes_b & 3u)))) {
    COX_HIP(hipMemcpyAsync(dst_a, src_a, bytes_a, hipMemcpyHostToDevice, s));
    if (two) COX_HIP(hipMemcpyAsync(dst_b, src_b, bytes_b, hipMemcpyHostToDevice, s));
    return COX_OK;
  }
  const HostSegment A = host_segment(dst_a, src_dev_a, bytes_a);
  const HostSegment B = two ? host_segment(dst_b, src_dev_b, bytes_b) : HostSegment{nullptr, nullptr, 0, 0};
  hipLaunchKernelGGL(k_copy_from_host, dim3(groups), dim3(256), 0, s, A, B);
  return COX_OK;
}
// the stream the next frame's first stage will run on
static inline hipStream_t next_frame_stream(const cox_integrator* I) { return stage_stream(I, 0, static_cast<int>((I->frame_no + 1) % kFrameSets)); }
// ... and the stream host inputs are staged on: the input stream, or (COX_INPUT_STREAM=0) the frame's own
static inline hipStream_t next_input_stream(const cox_integrator* I) { return I->st_in ? I->st_in : next_frame_stream(I); }
// Staging set k was read last by the frame kInputSets frames ago (its stages H .. M, enqueued by the caller's thread: the event is
// recorded by now).  On the frame's own stream that is a device-side wait; on the input stream it is a HOST wait -- the caller can
// not be more than kFrameSets frames ahead of the device anyway (frame slots), and the input stream's queue then carries nothing
// but the copies and one event record per frame: no barrier packet that holds its pipe.
static int wait_staging_set_free(cox_integrator* I, int k, hipStream_t s_in) {
  if (!I->in_used[k]) return COX_OK;
  if (s_in == I->st_in) {
    COX_HIP(hipEventSynchronize(I->in_free[k]));
    if (I->obs_used[k]) COX_HIP(hipEventSynchronize(I->obs_read[k]));
  } else {
    COX_HIP(hipStreamWaitEvent(s_in, I->in_free[k], 0));
    if (I->obs_used[k]) COX_HIP(hipStreamWaitEvent(s_in, I->obs_read[k], 0));
  }
  return COX_OK;
}
// two host arrays (a: a_bytes per element, b: b_bytes per element or absent) -> the device buffers dst_a / dst_b
static int stage_host_inputs(cox_integrator* I, int k, const void* a, size_t a_bytes, void* dst_a, const void* b, size_t b_bytes, void* dst_b, u32 n, FrameInput* in) {
  const hipStream_t s_in = next_input_stream(I);
  // the staging set is free once the frame that used it three frames ago has read it for the last time; that frame's stages
  // H .. M are enqueued by the caller's thread, so the event is recorded by now
  COX_TRY(wait_staging_set_free(I, k, s_in));
  const void* dev_a = host_pointer_device_view(a);
  const void* dev_b = b ? host_pointer_device_view(b) : nullptr;
  const bool pinned = dev_a != nullptr && (!b || dev_b != nullptr);
  const void* src_a = a;
  const void* src_b = b;
  if (!pinned) {
    if (I->pin_cap < I->pcap) {
      COX_TRY(sync_all(I));
      I->pin_cap = 0;
      for (int q = 0; q < kInputSets; ++q) {
        COX_TRY(pinned_realloc(I, &I->pin_xyz[q], static_cast<size_t>(I->pcap) * 3));
        COX_TRY(pinned_realloc(I, &I->pin_rgba[q], static_cast<size_t>(I->pcap) * 4));
      }
      I->pin_cap = I->pcap;
    }
    // the bounce buffer's previous copy (three frames ago) has left it: in_ready[k] was recorded behind that copy
    if (I->in_used[k]) COX_HIP(hipEventSynchronize(I->in_ready[k]));
    if (!I->copy_pool) I->copy_pool = new CopyPool(I->plan.copy_threads);
    I->copy_pool->copy(I->pin_xyz[k], a, a_bytes * n);
    if (b) I->copy_pool->copy(I->pin_rgba[k], b, b_bytes * n);
    src_a = I->pin_xyz[k];
    src_b = b ? I->pin_rgba[k] : nullptr;
    dev_a = host_pointer_device_view(src_a);
    dev_b = b ? host_pointer_device_view(src_b) : nullptr;
  }
  COX_TRY(copy_pinned_to_device(I, dst_a, src_a, dev_a, a_bytes * n, b ? dst_b : nullptr, src_b, dev_b, b ? b_bytes * n : 0, s_in));
  COX_HIP(hipEventRecord(I->in_ready[k], s_in));
  I->in_used[k] = true;
  in->ready = I->st_in ? I->in_ready[k] : nullptr;  // (without an input stream: same stream as the frame's first stage, stream order)
  in->consumed = I->in_free[k];
  in->staging_set = k;
  return COX_OK;
}

int cox_integrate_points(cox_integrator_t* I, const float T_G_C[7], const float* xyz, const uint8_t* rgba, uint64_t n, int freespace) {
  COX_ENTRY_NO_DRAIN();
  if (!I || !T_G_C || (n && !xyz) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(I->layer->device));
  if (I->proj) return cox_proj_integrate_host(I->proj, T_G_C, xyz, n, 0);
  COX_TRY(ensure_capacity(I, static_cast<u32>(n)));
  if (I->submitter) I->submitter->wait_outstanding(0);
  const int k = static_cast<int>((I->frame_no + 1) % kInputSets);  // the bundle set of the frame about to be enqueued
  FrameInput in;
  if (n) {  // synchronous call: copied straight from the caller's buffers (the runtime stages pageable memory itself), the call returns after the frame
    const hipStream_t s_in = next_input_stream(I);
    COX_TRY(wait_staging_set_free(I, k, s_in));
    COX_HIP(hipMemcpyAsync(I->own_xyz[k], xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, s_in));
    if (rgba) COX_HIP(hipMemcpyAsync(I->own_rgba[k], rgba, 4 * n, hipMemcpyHostToDevice, s_in));
    COX_HIP(hipEventRecord(I->in_ready[k], s_in));
    I->in_used[k] = true;
    in.ready = I->st_in ? I->in_ready[k] : nullptr;
    in.consumed = I->in_free[k];
    in.staging_set = k;
  }
  COX_TRY(integrate_device(I, T_G_C, I->own_xyz[k], rgba ? I->own_rgba[k] : nullptr, static_cast<u32>(n), freespace, true, in));
  return integrator_finish(I);
}

int cox_integrate_points_async(cox_integrator_t* I, const float T_G_C[7], const float* xyz, const uint8_t* rgba, uint64_t n, int freespace) {
  COX_ENTRY_NO_DRAIN();
  if (!I || !T_G_C || (n && !xyz) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(I->layer->device));
  if (I->proj) return cox_proj_integrate_host(I->proj, T_G_C, xyz, n, 0);
  COX_TRY(ensure_capacity(I, static_cast<u32>(n)));
  if (I->submitter) I->submitter->wait_outstanding(1);
  const int k = static_cast<int>((I->frame_no + 1) % kInputSets);
  FrameInput in;
  if (n) COX_TRY(stage_host_inputs(I, k, xyz, sizeof(float) * 3, I->own_xyz[k], rgba, 4, I->own_rgba[k], static_cast<u32>(n), &in));
  // (the staging buffers are the engine's own: no ordering against the caller's stream for them)
  const bool producer = I->has_producer;
  I->has_producer = false;
  const int st = integrate_device(I, T_G_C, I->own_xyz[k], rgba ? I->own_rgba[k] : nullptr, static_cast<u32>(n), freespace, false, in);
  I->has_producer = producer;
  return st;
}

int cox_integrator_wait_inputs(cox_integrator_t* I) {
  COX_ENTRY_NO_DRAIN();
  if (!I) return COX_ERR_INVALID_ARG;
  if (I->proj) return COX_OK;  // (the projective integrator's host entry point is synchronous)
  COX_HIP(hipSetDevice(I->layer->device));
  for (int k = 0; k < kInputSets; ++k)
    if (I->in_used[k]) COX_HIP(hipEventSynchronize(I->in_ready[k]));
  return COX_OK;
}

// depth image (device) -> point list in staging set k on stream s; the point count lands in d_depth_n[k]
// tiles of kDepthTile pixels in an image of n, and the words of tile_sums the two kernels use (one workgroup per tile: the grid)
static inline u32 depth_tiles(u32 n) { return std::max<u32>(1, (n + kDepthTile - 1) / kDepthTile); }
// the two launches of the depth front end; grid 0: one workgroup per tile (both kernels stride over the tiles with any grid)
static void launch_depth_convert(const float* depth_dev, const uint8_t* rgba_dev, int w, int h, const float K[4], u32 grid, u32* tile_sums, float* xyz,
                                 uint8_t* rgba_out, u32* n_out, hipStream_t s) {
  const u32 n = static_cast<u32>(w) * static_cast<u32>(h);
  const dim3 gt(grid ? grid : depth_tiles(n));
  hipLaunchKernelGGL(k_depth_count, gt, dim3(256), 0, s, depth_dev, n, tile_sums);
  hipLaunchKernelGGL(k_depth_points, gt, dim3(256), 0, s, depth_dev, rgba_dev, w, h, K[0], K[1], K[2], K[3], tile_sums, xyz, rgba_out, n_out);
}
static void convert_depth(cox_integrator* I, int k, const float* depth_dev, const uint8_t* rgba_dev, int w, int h, const float K[4], hipStream_t s) {
  u32* tile_sums = I->depth_flag + static_cast<size_t>(k) * (I->pcap / kDepthTile + 1);  // one set per staging set: consecutive frames convert on different streams
  launch_depth_convert(depth_dev, rgba_dev, w, h, K, 0, tile_sums, I->own_xyz[k], I->own_rgba[k], I->d_depth_n + k, s);
}

int cox_integrate_depth_dev(cox_integrator_t* I, const float T_G_C[7], const float* depth_dev, const uint8_t* rgba_dev, int w, int h, const float K[4]) {
  COX_ENTRY_NO_DRAIN();
  if (!I || !T_G_C || !depth_dev || !K || w <= 0 || h <= 0 || static_cast<uint64_t>(w) * h > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  if (I->proj) return COX_ERR_UNSUPPORTED;  // the projective integrator takes point clouds (it builds its own range image)
  if (I->obs) return COX_ERR_UNSUPPORTED;   // a history records point clouds (the depth front end keeps its point list to itself)
  COX_HIP(hipSetDevice(I->layer->device));
  const u32 n = static_cast<u32>(w) * static_cast<u32>(h);
  COX_TRY(ensure_capacity(I, n));
  // Frames stay in flight and nothing comes back to the host: the point list goes to the staging set of the frame's bundle set
  // (read by its stages H .. M), converted on the frame's ray-generation stream, and the point count -- which the "mixed" visiting
  // order is a function of -- stays in device memory: the frame's first kernel takes it from there (k_bundle_insert / k_params_count).
  if (I->submitter) I->submitter->wait_outstanding(1);
  const int k = static_cast<int>((I->frame_no + 1) % kInputSets);
  const hipStream_t s = next_frame_stream(I);  // (not the input stream: a wait for the caller's stream would sit in its queue)
  COX_TRY(wait_staging_set_free(I, k, s));
  if (I->has_producer) {  // the images were written on the caller's stream
    COX_HIP(hipEventRecord(I->ev_producer, I->producer));
    COX_HIP(hipStreamWaitEvent(s, I->ev_producer, 0));
  }
  convert_depth(I, k, depth_dev, rgba_dev, w, h, K, s);
  if (I->has_producer) {  // the images are not read after this: later work on the caller's stream may overwrite / free them
    COX_HIP(hipEventRecord(I->ev_inputs_read, s));
    COX_HIP(hipStreamWaitEvent(I->producer, I->ev_inputs_read, 0));
  }
  COX_HIP(hipEventRecord(I->in_ready[k], s));
  I->in_used[k] = true;
  FrameInput in;
  in.consumed = I->in_free[k];
  in.n_dev = I->d_depth_n + k;
  // (the staging buffers are the engine's own: no producer ordering for them)
  const bool producer = I->has_producer;
  I->has_producer = false;
  const int st = integrate_device(I, T_G_C, I->own_xyz[k], I->own_rgba[k], n, 0, false, in);
  I->has_producer = producer;
  return st;
}

int cox_integrate_depth_async(cox_integrator_t* I, const float T_G_C[7], const float* depth, const uint8_t* rgba, int w, int h, const float K[4]) {
  COX_ENTRY_NO_DRAIN();
  if (!I || !T_G_C || !depth || !K || w <= 0 || h <= 0 || static_cast<uint64_t>(w) * h > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  if (I->proj || I->obs) return COX_ERR_UNSUPPORTED;
  COX_HIP(hipSetDevice(I->layer->device));
  const u32 n = static_cast<u32>(w) * static_cast<u32>(h);
  COX_TRY(ensure_capacity(I, n));
  if (I->submitter) I->submitter->wait_outstanding(1);
  const int k = static_cast<int>((I->frame_no + 1) % kInputSets);
  FrameInput in;
  COX_TRY(stage_host_inputs(I, k, depth, sizeof(float), I->own_depth[k], rgba, 4, I->own_depth_rgba[k], n, &in));
  // the conversion (two kernels) runs on the frame's own stream behind the copies' event: the input stream shares the apply's pipe for
  // `merged`, and kernels there cost more than 25 us on the ray-generation chain do (640x480 images, frames/s: 6 380 vs 5 170; `fast`,
  // whose input stream has a pipe of its own: 2 780 vs 2 830).  COX_DEPTH_CONVERT=input puts it on the input stream.
  if (I->st_in && !I->plan.depth_convert_on_input_stream) {
    COX_HIP(hipStreamWaitEvent(next_frame_stream(I), I->in_ready[k], 0));
    in.ready = nullptr;
    convert_depth(I, k, I->own_depth[k], rgba ? I->own_depth_rgba[k] : nullptr, w, h, K, next_frame_stream(I));
  } else {
    convert_depth(I, k, I->own_depth[k], rgba ? I->own_depth_rgba[k] : nullptr, w, h, K, next_input_stream(I));
    if (I->st_in) COX_HIP(hipEventRecord(I->in_ready[k], I->st_in));  // (recorded again: behind the conversion)
  }
  in.n_dev = I->d_depth_n + k;
  const bool producer = I->has_producer;
  I->has_producer = false;
  const int st = integrate_device(I, T_G_C, I->own_xyz[k], I->own_rgba[k], n, 0, false, in);
  I->has_producer = producer;
  return st;
}

int cox_integrator_set_input_stream(cox_integrator_t* I, void* hip_stream, int enable) {
  COX_ENTRY();
  if (!I) return COX_ERR_INVALID_ARG;
  I->has_producer = enable != 0;
  I->producer = static_cast<hipStream_t>(hip_stream);
  return COX_OK;
}

int cox_integrator_attach_history(cox_integrator_t* I, cox_obs_t* obs) {
  COX_ENTRY();
  if (!I) return COX_ERR_INVALID_ARG;
  if (obs && !cox_internal_obs_matches(obs, I->layer)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(I->layer->device));
  if (I->proj) return cox_proj_attach_history(I->proj, obs);
  COX_TRY(sync_all(I));  // the record that is attached so far has read every cloud handed to it
  if (obs && !I->ev_obs_read) {
    COX_TRY(make_event(I, &I->ev_obs_read));
    for (hipEvent_t& e : I->obs_read) COX_TRY(make_event(I, &e));
  }
  I->obs = obs;
  for (bool& u : I->obs_used) u = false;
  return COX_OK;
}

int cox_integrator_sync(cox_integrator_t* I) {
  COX_ENTRY();
  if (!I) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(I->layer->device));
  if (I->proj) return cox_proj_sync(I->proj);
  return integrator_finish(I);
}

int cox_integrator_last_stats(cox_integrator_t* I, cox_frame_stats* stats) {
  COX_ENTRY();
  if (!I || !stats) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(I->layer->device));
  if (I->proj) return cox_proj_last_stats(I->proj, stats);
  COX_TRY(sync_all(I));
  COX_TRY(fold_counters(I));
  *stats = I->last;
  return COX_OK;
}

int cox_integrator_set_profiling(cox_integrator_t* I, int on) {
  COX_ENTRY();
  if (!I) return COX_ERR_INVALID_ARG;
  I->profiling = on > 0;
  I->profile_every = on > 1 ? static_cast<u32>(on) : 1u;
  if (on > 0 && !I->proj && !I->timeline && !I->plan.timeline.empty()) {
    I->timeline = fopen(I->plan.timeline.c_str(), "a");
    if (I->timeline && hipEventCreate(&I->timeline_ref) == hipSuccess) {
      COX_HIP(hipSetDevice(I->layer->device));
      COX_TRY(sync_all(I));
      COX_HIP(hipEventRecord(I->timeline_ref, I->st[0]));
      fprintf(I->timeline, "# integrator %p method %d\n", static_cast<void*>(I), I->method);
    }
  }
  return COX_OK;
}

int cox_integrator_kernel_time(cox_integrator_t* I, double* apply_ms, uint64_t* apply_launches, int reset) {
  COX_ENTRY();
  if (!I) return COX_ERR_INVALID_ARG;
  if (I->proj) return COX_ERR_UNSUPPORTED;
  COX_HIP(hipSetDevice(I->layer->device));
  int st = integrator_finish(I);
  if (apply_ms) *apply_ms = I->class_ms[COX_KC_APPLY];
  if (apply_launches) *apply_launches = I->class_regions[COX_KC_APPLY];
  if (reset) {
    I->class_ms[COX_KC_APPLY] = 0.0;
    I->class_regions[COX_KC_APPLY] = 0;
  }
  return st;
}

int cox_selftest_division(int device, uint64_t n, uint64_t seed, uint64_t* mismatches) {
  COX_ENTRY();
  if (!mismatches) return COX_ERR_INVALID_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return COX_ERR_NO_DEVICE;
  COX_HIP(hipSetDevice(device));
  DevBuf<u32> d;
  COX_TRY(d.alloc(1));
  COX_HIP(hipMemset(d, 0, sizeof(u32)));
  hipLaunchKernelGGL(k_selftest_division, dim3(4096), dim3(256), 0, nullptr, n, seed, d.p);
  u32 h = 0;
  COX_HIP(hipMemcpy(&h, d, sizeof(u32), hipMemcpyDeviceToHost));
  *mismatches = h;
  return COX_OK;
}

// The one-workgroup scans of the ray-generation chain on caller-supplied inputs (tests/test_gpu_sort_scan.py).  It lives here, not in
// cox_selftest.hip, because k_scan_small and k_scan_small2 are ordinary kernels of cox_frontend.hpp: one translation unit only.
int cox_selftest_scan_small(int device, const uint32_t* in_a, const uint32_t* in_b, uint32_t len, uint32_t n_max, uint32_t d_n, uint32_t sentinel,
                            uint32_t* out1_a, uint32_t* out1_b, uint32_t* out2_a, uint32_t* out2_b, uint32_t totals[4]) {
  COX_ENTRY();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return COX_ERR_NO_DEVICE;
  if (!totals || len < std::min(d_n, n_max) || (len && (!in_a || !in_b || !out1_a || !out1_b || !out2_a || !out2_b))) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(device));
  // one allocation: in_a, in_b, four outputs, the count, four totals
  const size_t words = std::max<size_t>(len, 1);
  DevBuf<u32> buf;
  COX_TRY(buf.alloc(6 * words + 5));
  u32* d = buf.p;
  u32 *d_in[2] = {d, d + words}, *d_out = d + 2 * words, *d_cnt = d + 6 * words, *d_tot = d_cnt + 1;
  if (len) {
    COX_HIP(hipMemcpy(d_in[0], in_a, len * sizeof(u32), hipMemcpyHostToDevice));
    COX_HIP(hipMemcpy(d_in[1], in_b, len * sizeof(u32), hipMemcpyHostToDevice));
  }
  COX_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d_out), static_cast<int>(sentinel), 4 * words));
  COX_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d_tot), static_cast<int>(sentinel), 4));
  COX_HIP(hipMemcpy(d_cnt, &d_n, sizeof(u32), hipMemcpyHostToDevice));
  COX_HIP(hipDeviceSynchronize());
  hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, nullptr, d_in[0], d_out, d_cnt, n_max, d_tot);
  hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, nullptr, d_in[1], d_out + words, d_cnt, n_max, d_tot + 1);
  hipLaunchKernelGGL(k_scan_small2, dim3(1), dim3(1024), 0, nullptr, d_in[0], d_out + 2 * words, d_tot + 2, d_in[1], d_out + 3 * words, d_tot + 3, d_cnt, n_max);
  COX_HIP(hipGetLastError());
  COX_HIP(hipDeviceSynchronize());
  uint32_t* outs[4] = {out1_a, out1_b, out2_a, out2_b};
  for (int k = 0; k < 4 && len; ++k) COX_HIP(hipMemcpy(outs[k], d_out + k * words, len * sizeof(u32), hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(totals, d_tot, 4 * sizeof(u32), hipMemcpyDeviceToHost));
  return COX_OK;
}

// words of a 64-word guard on the device that no longer hold the sentinel
constexpr u32 kSelftestGuard = 64;
static int selftest_guard_touched(const u32* d_guard, u32 sentinel, uint32_t* touched) {
  u32 g[kSelftestGuard];
  COX_HIP(hipMemcpy(g, d_guard, sizeof(g), hipMemcpyDeviceToHost));
  *touched = 0;
  for (u32 v : g) *touched += v != sentinel ? 1u : 0u;
  return COX_OK;
}

// The depth front end on a caller-supplied image (tests/test_gpu_frontend.py), launched by the code convert_depth launches it with.
int cox_selftest_depth_points(int device, const float* depth, const uint8_t* rgba, int w, int h, const float K[4], uint32_t grid, int want_rgba,
                              uint32_t sentinel, float* xyz_out, uint8_t* rgba_out, uint32_t* tile_sums_out, uint32_t* n_out, uint32_t guard_touched[3]) {
  COX_ENTRY();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return COX_ERR_NO_DEVICE;
  if (!depth || !K || w <= 0 || h <= 0 || static_cast<uint64_t>(w) * h > (1ull << 24) || grid > 65535u || !xyz_out || !rgba_out || !tile_sums_out ||
      !n_out || !guard_touched)
    return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(device));
  // one allocation of words: depth, colours in, then every output with its guard behind it, the count last
  const size_t n = static_cast<size_t>(w) * h, tiles = depth_tiles(static_cast<u32>(n)), G = kSelftestGuard;
  const size_t o_rgba_in = n, o_xyz = 2 * n, o_rgba = o_xyz + 3 * n + G, o_tiles = o_rgba + n + G, o_n = o_tiles + tiles + G, words = o_n + 1;
  DevBuf<u32> buf;
  COX_TRY(buf.alloc(words));
  u32* d = buf.p;
  COX_HIP(hipMemcpy(d, depth, n * sizeof(float), hipMemcpyHostToDevice));
  if (rgba) COX_HIP(hipMemcpy(d + o_rgba_in, rgba, n * 4, hipMemcpyHostToDevice));
  COX_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d + o_xyz), static_cast<int>(sentinel), words - o_xyz));
  COX_HIP(hipDeviceSynchronize());
  launch_depth_convert(reinterpret_cast<const float*>(d), rgba ? reinterpret_cast<const uint8_t*>(d + o_rgba_in) : nullptr, w, h, K, grid, d + o_tiles,
                       reinterpret_cast<float*>(d + o_xyz), want_rgba ? reinterpret_cast<uint8_t*>(d + o_rgba) : nullptr, d + o_n, nullptr);
  COX_HIP(hipGetLastError());
  COX_HIP(hipDeviceSynchronize());
  COX_HIP(hipMemcpy(xyz_out, d + o_xyz, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(rgba_out, d + o_rgba, n * 4, hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(tile_sums_out, d + o_tiles, tiles * sizeof(u32), hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(n_out, d + o_n, sizeof(u32), hipMemcpyDeviceToHost));
  COX_TRY(selftest_guard_touched(d + o_xyz + 3 * n, sentinel, &guard_touched[0]));
  COX_TRY(selftest_guard_touched(d + o_rgba + n, sentinel, &guard_touched[1]));
  COX_TRY(selftest_guard_touched(d + o_tiles + tiles, sentinel, &guard_touched[2]));
  return COX_OK;
}

// k_copy_from_host on caller-supplied arrays put into pinned host memory, with the segments copy_pinned_to_device builds.
int cox_selftest_copy_from_host(int device, const uint32_t* a, uint64_t words_a, const uint32_t* b, uint64_t words_b, int groups, uint32_t sentinel,
                                uint32_t* out_a, uint32_t* out_b, uint32_t guard_touched[2]) {
  COX_ENTRY();
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return COX_ERR_NO_DEVICE;
  constexpr uint64_t kMaxWords = 1ull << 24;
  if (groups < 1 || groups > 1024 || words_a > kMaxWords || words_b > kMaxWords || !guard_touched || (words_a && (!a || !out_a)) || (!b && words_b) ||
      (words_b && !out_b))
    return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(device));
  // both sides: a, then b from the next multiple of 16 bytes on; on the device a guard behind each
  const size_t G = kSelftestGuard, a4 = (words_a + 3) & ~static_cast<size_t>(3), b4 = (words_b + 3) & ~static_cast<size_t>(3);
  const size_t o_b = a4 + G, words = o_b + b4 + G;
  PinnedBuf<u32> host;
  COX_TRY(host.alloc(a4 + b4 + 4));
  u32* pinned = host.p;
  DevBuf<u32> buf;
  COX_TRY(buf.alloc(words));
  u32* d = buf.p;
  if (words_a) memcpy(pinned, a, words_a * sizeof(u32));
  if (words_b) memcpy(pinned + a4, b, words_b * sizeof(u32));
  const u32* pinned_dev = static_cast<const u32*>(host_pointer_device_view(pinned));
  if (!pinned_dev || (reinterpret_cast<uintptr_t>(pinned_dev) & 15u) || (reinterpret_cast<uintptr_t>(d) & 15u)) return COX_ERR_INTERNAL;
  COX_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d), static_cast<int>(sentinel), words));
  COX_HIP(hipDeviceSynchronize());
  const HostSegment A = host_segment(d, pinned_dev, words_a * sizeof(u32));
  const HostSegment B = b ? host_segment(d + o_b, pinned_dev + a4, words_b * sizeof(u32)) : HostSegment{nullptr, nullptr, 0, 0};
  hipLaunchKernelGGL(k_copy_from_host, dim3(groups), dim3(256), 0, nullptr, A, B);
  COX_HIP(hipGetLastError());
  COX_HIP(hipDeviceSynchronize());
  // (the padding words between an array's end and its guard count as guard: nothing may write them either)
  if (words_a) COX_HIP(hipMemcpy(out_a, d, words_a * sizeof(u32), hipMemcpyDeviceToHost));
  if (words_b) COX_HIP(hipMemcpy(out_b, d + o_b, words_b * sizeof(u32), hipMemcpyDeviceToHost));
  for (int k = 0; k < 2; ++k) {
    const size_t end = k ? o_b + words_b : words_a, stop = k ? words : o_b;
    std::vector<u32> g(stop - end);
    COX_HIP(hipMemcpy(g.data(), d + end, g.size() * sizeof(u32), hipMemcpyDeviceToHost));
    guard_touched[k] = 0;
    for (u32 v : g) guard_touched[k] += v != sentinel ? 1u : 0u;
  }
  return COX_OK;
}

int cox_integrator_stage_times(cox_integrator_t* I, double ms[2], uint64_t launches[2], int reset) {
  COX_ENTRY();
  if (!I || !ms || !launches) return COX_ERR_INVALID_ARG;
  if (I->proj) return COX_ERR_UNSUPPORTED;
  COX_HIP(hipSetDevice(I->layer->device));
  int st = integrator_finish(I);
  ms[0] = I->class_ms[COX_KC_MERGE];
  launches[0] = I->class_regions[COX_KC_MERGE];
  ms[1] = I->class_ms[COX_KC_APPLY];
  launches[1] = I->class_regions[COX_KC_APPLY];
  if (reset)
    for (int k : {COX_KC_MERGE, COX_KC_APPLY}) {
      I->class_ms[k] = 0.0;
      I->class_regions[k] = 0;
    }
  return st;
}

int cox_integrator_host_time(cox_integrator_t* I, double* ms_total, uint64_t* frames, int reset) {
  COX_ENTRY();
  if (!I || !ms_total || !frames) return COX_ERR_INVALID_ARG;
  *ms_total = static_cast<double>(I->host_ns - I->host_wait_ns) * 1e-6;  // enqueueing only: waits for a free slot are the GPU's time
  *frames = I->host_frames;
  if (reset) {
    I->host_ns = 0;
    I->host_wait_ns = 0;
    I->host_frames = 0;
  }
  return COX_OK;
}

int cox_integrator_fast_stats(cox_integrator_t* I, uint64_t out[10]) {
  COX_ENTRY();
  if (!I || !out) return COX_ERR_INVALID_ARG;
  if (I->method != COX_METHOD_FAST || I->proj) return COX_ERR_UNSUPPORTED;
  COX_HIP(hipSetDevice(I->layer->device));
  COX_TRY(sync_all(I));
  u32 h[16] = {};
  COX_HIP(hipMemcpy(h, I->fast.d_stats, sizeof(h), hipMemcpyDeviceToHost));
  for (int k = 0; k < 4; ++k) out[k] = h[k];
  out[4] = I->fast.frames;
  out[5] = h[4];
  out[6] = h[5];
  out[7] = h[6];
  out[8] = static_cast<uint64_t>(h[7]) * 10ull;  // ticks of 10 ns
  out[9] = static_cast<uint64_t>(h[8]) * 10ull;
  if (I->plan.debug) fprintf(stderr, "[coxgraph_hip] fast: long rays %u, visits of the last round %llu, of round 0 %llu (totals over %llu frames)\n", h[9],
                                        static_cast<unsigned long long>(h[10]) * 16ull, static_cast<unsigned long long>(h[11]) * 16ull, static_cast<unsigned long long>(I->fast.frames));
  return COX_OK;
}

int cox_integrator_update_stats(cox_integrator_t* I, uint64_t out[2]) {
  COX_ENTRY();
  if (!I || !out) return COX_ERR_INVALID_ARG;
  out[0] = out[1] = 0;
  if (I->proj) return COX_OK;
  COX_HIP(hipSetDevice(I->layer->device));
  COX_TRY(integrator_finish(I));
  out[0] = I->last_big_tiles;
  out[1] = I->last_big_chunks;
  return COX_OK;
}

int cox_integrator_class_times(cox_integrator_t* I, double ms[COX_KERNEL_CLASSES], uint64_t regions[COX_KERNEL_CLASSES], int reset) {
  COX_ENTRY();
  if (!I || !ms || !regions) return COX_ERR_INVALID_ARG;
  if (I->proj) return COX_ERR_UNSUPPORTED;
  COX_HIP(hipSetDevice(I->layer->device));
  int st = integrator_finish(I);
  for (int k = 0; k < COX_KERNEL_CLASSES; ++k) {
    ms[k] = I->class_ms[k];
    regions[k] = I->class_regions[k];
    if (reset) {
      I->class_ms[k] = 0.0;
      I->class_regions[k] = 0;
    }
  }
  return st;
}

}  // extern "C"
