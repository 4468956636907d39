// MI355X (gfx950) pose-candidate sweep behind include/coxgraph_hip_align.h: M candidate 4-DoF reference poses of one
// (registration points, reading layer) pair scored in one launch, and the coarse-to-fine search on top of the scores.
// Rule, launch shape and measurements: DESIGN.md section 7o.
//
//   k_align_sweep   grid (point chunks, candidate tiles) x 256 lanes.  A lane keeps ITS point in registers and walks the
//                   tile's candidates, whose R | t are uniform over the workgroup (scalar loads).  Per candidate the three
//                   integers and sum r^2 are reduced over the wave by shuffles and over the four waves through LDS; the
//                   integers reach the record by integer atomics (order-free), sum r^2 goes to cost_part[candidate][chunk].
//   k_align_finish  one wave per candidate sums its chunk partials (and the chunks' sums of weights) in an order that
//                   depends on the chunk count alone, and writes cost.
// The per-point value is cox_reg.hpp's reg_cell / reg_value (point_cell of cox_interp.hpp under the candidate's transform):
// the same bits as the registration cost.  The wave sums are cox_device.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/coxgraph_hip_align.h"
#include "cox_device.hpp"
#include "cox_host.hpp"
#include "cox_interp.hpp"
#include "cox_reg.hpp"

using namespace cox;

constexpr int kAlignThreads = 256;
constexpr int kAlignWaves = kAlignThreads / 64;
constexpr int kAlignTile = 4;              // candidates a workgroup walks with its points in registers
constexpr u32 kAlignMaxChunks = 1024;      // point chunks; beyond 1024 * 256 points the lanes stride (the partition depends on m alone)
constexpr u64 kAlignPartCap = 1ull << 23;  // doubles of cost_part per pass (64 MiB)
constexpr u32 kAlignMaxTiles = 65535;      // gridDim.y

struct AlignPose {  // make_rel_pose's float part
  float R[9];
  float t[3];
};

static_assert(sizeof(cox_align_score) == 24, "cox_align_score is 24 bytes");

struct AlignAcc {
  u32 k, nc, ni;
  double s;
};

// one point at one candidate: what it adds to score, n_corr, n_inlier and sum r^2
__device__ __forceinline__ void align_point(const LayerView& L, const float* R, const float* t, float px, float py, float pz, float pd, float pw, float tau,
                                            float inv, double no_corr_cost, AlignAcc& a) {
  float md[8], off[3];
  const bool has = reg_cell(L, R, t, px, py, pz, md, off);
  double r = static_cast<double>(pw) * no_corr_cost;
  if (has) {
    const float diff = pd - reg_value(md, off);
    r = static_cast<double>(diff * pw);
    const float e = fabsf(diff);
    const bool inlier = e <= tau;  // false for a NaN
    const int u = inlier ? static_cast<int>(floorf(e * inv)) : static_cast<int>(COX_ALIGN_Q);
    const int k = static_cast<int>(COX_ALIGN_Q) - u;
    a.nc += 1u;
    a.ni += inlier ? 1u : 0u;
    a.k += (inlier && k > 0) ? static_cast<u32>(k) : 0u;
  }
  a.s += r * r;
}

__global__ void __launch_bounds__(kAlignThreads) k_align_sweep(LayerView L, const float* __restrict__ pts, const u32* __restrict__ sample_idx, u32 m,
                                                               const AlignPose* __restrict__ poses, u32 n_cand, float tau, float inv, double no_corr_cost,
                                                               cox_align_score* rec, double* __restrict__ cost_part /*[n_cand][gridDim.x]*/,
                                                               double* __restrict__ w_part /*[gridDim.x]*/) {
  __shared__ double sh_s[kAlignTile][kAlignWaves];
  __shared__ u32 sh_i[kAlignTile][kAlignWaves][3];
  __shared__ double sh_w[kAlignWaves];
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const u32 chunk = blockIdx.x, n_chunks = gridDim.x;
  const u32 stride = n_chunks * kAlignThreads;
  const u32 i0 = chunk * kAlignThreads + threadIdx.x;
  // the lane's first point stays in registers over the candidates; a lane that strides (m > 1024 * 256) reloads the others
  float p0[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if (i0 < m) {
    const float* pt = pts + 5ull * (sample_idx ? sample_idx[i0] : i0);
#pragma unroll
    for (int k = 0; k < 5; ++k) p0[k] = pt[k];
  }
  if (blockIdx.y == 0) {  // the chunk's sum of weights, once
    double w = 0.0;
    if (i0 < m) w = static_cast<double>(p0[4]);
    for (u64 i = static_cast<u64>(i0) + stride; i < m; i += stride) w += static_cast<double>(pts[5ull * (sample_idx ? sample_idx[i] : i) + 4]);
    w = wave_sum_f64(w);
    if (lane == 0) sh_w[wave] = w;
    __syncthreads();
    if (threadIdx.x == 0) w_part[chunk] = ((sh_w[0] + sh_w[1]) + sh_w[2]) + sh_w[3];
  }
  const u32 c0 = blockIdx.y * kAlignTile;
  for (int cc = 0; cc < kAlignTile; ++cc) {
    const u32 c = c0 + cc;
    if (c >= n_cand) break;  // uniform
    float R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = poses[c].R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = poses[c].t[k];
    AlignAcc a{0u, 0u, 0u, 0.0};
    if (i0 < m) align_point(L, R, t, p0[0], p0[1], p0[2], p0[3], p0[4], tau, inv, no_corr_cost, a);
    for (u64 i = static_cast<u64>(i0) + stride; i < m; i += stride) {
      const float* pt = pts + 5ull * (sample_idx ? sample_idx[i] : i);
      align_point(L, R, t, pt[0], pt[1], pt[2], pt[3], pt[4], tau, inv, no_corr_cost, a);
    }
    const double s = wave_sum_f64(a.s);
    const u32 k = wave_sum_u32(a.k), nc = wave_sum_u32(a.nc), ni = wave_sum_u32(a.ni);
    if (lane == 0) {
      sh_s[cc][wave] = s;
      sh_i[cc][wave][0] = k;
      sh_i[cc][wave][1] = nc;
      sh_i[cc][wave][2] = ni;
    }
  }
  __syncthreads();
  if (threadIdx.x < kAlignTile && c0 + threadIdx.x < n_cand) {
    const u32 cc = threadIdx.x, c = c0 + cc;
    cost_part[static_cast<size_t>(c) * n_chunks + chunk] = ((sh_s[cc][0] + sh_s[cc][1]) + sh_s[cc][2]) + sh_s[cc][3];
    u32 v[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) v[q] = ((sh_i[cc][0][q] + sh_i[cc][1][q]) + sh_i[cc][2][q]) + sh_i[cc][3][q];
    // integer sums: any order gives the same record
    if (v[0]) atomicAdd(reinterpret_cast<unsigned long long*>(&rec[c].score), static_cast<unsigned long long>(v[0]));
    if (v[1]) atomicAdd(&rec[c].n_corr, v[1]);
    if (v[2]) atomicAdd(&rec[c].n_inlier, v[2]);
  }
}

// one wave per candidate: lane l adds the chunks l, l + 64, ... in that order, then the lanes pairwise
__global__ void __launch_bounds__(kAlignThreads) k_align_finish(cox_align_score* __restrict__ rec, const double* __restrict__ cost_part,
                                                                const double* __restrict__ w_part, u32 n_chunks, u32 m, u32 n_cand) {
  const u32 lane = threadIdx.x & 63u;
  const u32 c = blockIdx.x * kAlignWaves + (threadIdx.x >> 6);
  if (c >= n_cand) return;  // whole waves
  double s = 0.0, w = 0.0;
  for (u32 j = lane; j < n_chunks; j += 64) {
    s += cost_part[static_cast<size_t>(c) * n_chunks + j];
    w += w_part[j];
  }
  s = wave_sum_f64(s);
  w = wave_sum_f64(w);
  if (lane == 0) {
    const double scale = w > 0.0 ? static_cast<double>(m) / w : 0.0;
    rec[c].cost = ((0.5 * s) * scale) * scale;
  }
}

// ---- host ----------------------------------------------------------------------------------------------------
struct cox_align {
  const cox_regpoints* ref = nullptr;
  const cox_layer* reading = nullptr;
  cox_align_config cfg{};
  Stream stream;
  DevBuf<u32> d_stored;  // cox_align_set_samples
  u64 stored_samples = 0;
  bool has_stored = false;
  DevBuf<AlignPose> d_poses;
  PinnedBuf<AlignPose> h_poses;
  DevBuf<cox_align_score> d_rec;
  PinnedBuf<cox_align_score> h_rec;
  DevBuf<double> d_part;  // cost_part of a pass, then w_part
  EventPair ev;
  double ms = 0.0;
  uint64_t sweeps = 0;
};

static bool tau_ok(float tau) { return std::isfinite(tau) && tau > 0.0f; }

// up to COX_ALIGN_MAX_CANDIDATES candidates; arguments checked by the callers
static int sweep_once(cox_align* G, const double pose_read[4], const double* poses_ref, u64 M, float tau, cox_align_score* out) {
  const u64 m64 = G->has_stored ? G->stored_samples : G->ref->n;
  if (m64 == 0) {  // no points: every sum is empty
    std::memset(out, 0, sizeof(cox_align_score) * M);
    return COX_OK;
  }
  const u32 m = static_cast<u32>(m64);
  const u32 n_chunks = std::min<u32>(kAlignMaxChunks, (m + kAlignThreads - 1) / kAlignThreads);
  const u64 pass_cap = std::min<u64>(kAlignPartCap / n_chunks, static_cast<u64>(kAlignMaxTiles) * kAlignTile);
  const u64 P = std::min<u64>(M, pass_cap);
  COX_TRY(G->h_poses.grow(M));
  COX_TRY(G->h_rec.grow(M));
  COX_TRY(G->d_poses.grow(M));
  COX_TRY(G->d_rec.grow(M));
  COX_TRY(G->d_part.grow(P * n_chunks + n_chunks));
  for (u64 c = 0; c < M; ++c) {
    const RelPose R = make_rel_pose(poses_ref + 4 * c, pose_read);
    for (int k = 0; k < 9; ++k) G->h_poses.p[c].R[k] = R.R[k];
    for (int k = 0; k < 3; ++k) G->h_poses.p[c].t[k] = R.t[k];
  }
  const float inv = 1024.0f / tau;
  hipStream_t s = G->stream;
  cox_layer_wait_writes(G->reading, s);  // frames still in flight on the reading layer
  COX_HIP(hipMemcpyAsync(G->d_poses, G->h_poses, sizeof(AlignPose) * M, hipMemcpyHostToDevice, s));
  COX_HIP(G->ev.begin(s));
  COX_HIP(hipMemsetAsync(G->d_rec, 0, sizeof(cox_align_score) * M, s));
  const LayerView L = layer_view(G->reading);
  const u32* d_idx = G->has_stored ? G->d_stored.p : nullptr;
  double* w_part = G->d_part + P * n_chunks;
  for (u64 base = 0; base < M; base += P) {
    const u32 n = static_cast<u32>(std::min<u64>(P, M - base));
    hipLaunchKernelGGL(k_align_sweep, dim3(n_chunks, (n + kAlignTile - 1) / kAlignTile), dim3(kAlignThreads), 0, s, L, G->ref->pts, d_idx, m, G->d_poses + base, n, tau,
                       inv, G->cfg.no_correspondence_cost, G->d_rec + base, G->d_part, w_part);
    hipLaunchKernelGGL(k_align_finish, dim3((n + kAlignWaves - 1) / kAlignWaves), dim3(kAlignThreads), 0, s, G->d_rec + base, G->d_part, w_part, n_chunks, m, n);
  }
  COX_HIP(G->ev.end(s));
  COX_HIP(hipMemcpyAsync(G->h_rec, G->d_rec, sizeof(cox_align_score) * M, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  COX_HIP(hipGetLastError());
  std::memcpy(out, G->h_rec, sizeof(cox_align_score) * M);
  double ms = 0.0;
  if (G->ev.elapsed_ms(&ms)) {
    G->ms += ms;
    G->sweeps += 1;
  }
  return COX_OK;
}

static int sweep_all(cox_align* G, const double pose_read[4], const double* poses_ref, u64 M, float tau, cox_align_score* out) {
  for (u64 base = 0; base < M; base += COX_ALIGN_MAX_CANDIDATES)
    COX_TRY(sweep_once(G, pose_read, poses_ref + 4 * base, std::min<u64>(COX_ALIGN_MAX_CANDIDATES, M - base), tau, out + base));
  return COX_OK;
}

static bool grid_counts(const double center[4], const double half[4], const double step[4], long long mk[4], u64* count) {
  u64 n = 1;
  for (int k = 0; k < 4; ++k) {
    if (!std::isfinite(center[k]) || !std::isfinite(half[k]) || !std::isfinite(step[k]) || half[k] < 0.0 || step[k] < 0.0) return false;
    mk[k] = 0;
    if (step[k] > 0.0) {
      const double q = half[k] / step[k];
      if (!(q < static_cast<double>(COX_ALIGN_MAX_GRID))) return false;
      mk[k] = std::llround(q);
    }
    n *= static_cast<u64>(2 * mk[k] + 1);
    if (n > COX_ALIGN_MAX_GRID) return false;
  }
  *count = n;
  return true;
}
static void grid_fill(const double center[4], const double step[4], const long long mk[4], double* out) {
  for (long long jx = -mk[0]; jx <= mk[0]; ++jx)
    for (long long jy = -mk[1]; jy <= mk[1]; ++jy)
      for (long long jz = -mk[2]; jz <= mk[2]; ++jz)
        for (long long jw = -mk[3]; jw <= mk[3]; ++jw) {
          out[0] = center[0] + step[0] * static_cast<double>(jx);
          out[1] = center[1] + step[1] * static_cast<double>(jy);
          out[2] = center[2] + step[2] * static_cast<double>(jz);
          out[3] = center[3] + step[3] * static_cast<double>(jw);
          out += 4;
        }
}

static u32 select_best(const cox_align_score* scores, u64 n, u32 min_corr, u32 keep, uint32_t* idx_out) {
  std::vector<u32> el;
  for (u64 i = 0; i < n; ++i)
    if (scores[i].n_corr >= min_corr) el.push_back(static_cast<u32>(i));
  const size_t k = std::min<size_t>(keep, el.size());
  std::partial_sort(el.begin(), el.begin() + k, el.end(), [scores](u32 a, u32 b) { return scores[a].score != scores[b].score ? scores[a].score > scores[b].score : a < b; });
  for (size_t i = 0; i < k; ++i) idx_out[i] = el[i];
  return static_cast<u32>(k);
}

extern "C" {

void cox_align_config_default(cox_align_config* cfg) {
  if (!cfg) return;
  cfg->inlier_distance = 0.4f;
  cfg->pad = 0;
  cfg->no_correspondence_cost = 0.0;
}

int cox_align_create(const cox_regpoints_t* reference, const cox_layer_t* reading, const cox_align_config* cfg, cox_align_t** out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (out) *out = nullptr;
  if (!reference || !reading || !out) return COX_ERR_INVALID_ARG;
  cox_align_config c;
  cox_align_config_default(&c);
  if (cfg) c = *cfg;
  if (!tau_ok(c.inlier_distance) || std::isnan(c.no_correspondence_cost)) return COX_ERR_INVALID_ARG;
  const cox_layer* L = reinterpret_cast<const cox_layer*>(reading);
  if (L->device != reference->device || reference->n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(L->device));
  cox_align* G = new (std::nothrow) cox_align();
  if (!G) return COX_ERR_OUT_OF_MEMORY;
  G->ref = reference;
  G->reading = L;
  G->cfg = c;
  if (G->stream.create() != COX_OK || G->ev.create() != COX_OK) {
    cox_align_destroy(G);
    return COX_ERR_NO_DEVICE;
  }
  *out = G;
  return COX_OK;
}

void cox_align_destroy(cox_align_t* G) {
  if (!G) return;
  (void)hipSetDevice(G->reading->device);
  if (G->stream) (void)hipStreamSynchronize(G->stream);
  delete G;
}

int cox_align_set_samples(cox_align_t* G, const uint32_t* sample_idx, uint64_t m) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!G || m > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  if (sample_idx)
    for (uint64_t i = 0; i < m; ++i)
      if (sample_idx[i] >= G->ref->n) return COX_ERR_INVALID_ARG;  // (the stored list stands)
  COX_HIP(hipSetDevice(G->reading->device));
  G->has_stored = false;
  G->stored_samples = 0;
  if (!sample_idx) return COX_OK;  // back to "all points in order"
  COX_TRY(G->d_stored.grow(std::max<uint64_t>(m, 1)));
  if (m) COX_HIP(hipMemcpy(G->d_stored, sample_idx, sizeof(u32) * m, hipMemcpyHostToDevice));
  G->has_stored = true;
  G->stored_samples = m;
  return COX_OK;
}

int cox_align_sweep(cox_align_t* G, const double pose_read[4], const double* poses_ref, uint64_t n_candidates, float inlier_distance,
                    cox_align_score* scores_out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!G || !pose_read || !tau_ok(inlier_distance) || n_candidates > COX_ALIGN_MAX_CANDIDATES) return COX_ERR_INVALID_ARG;
  if (n_candidates == 0) return COX_OK;
  if (!poses_ref || !scores_out) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(G->reading->device));
  return sweep_once(G, pose_read, poses_ref, n_candidates, inlier_distance, scores_out);
}

int cox_align_grid(const double center[4], const double half_extent[4], const double step[4], double* poses_out, uint64_t cap, uint64_t* n_poses) {
  if (!center || !half_extent || !step || !n_poses) return COX_ERR_INVALID_ARG;
  long long mk[4];
  u64 count = 0;
  if (!grid_counts(center, half_extent, step, mk, &count)) return COX_ERR_INVALID_ARG;
  *n_poses = count;
  if (!poses_out) return COX_OK;
  if (cap < count) return COX_ERR_BUFFER_TOO_SMALL;
  grid_fill(center, step, mk, poses_out);
  return COX_OK;
}

int cox_align_select(const cox_align_score* scores, uint64_t n, uint32_t min_corr, uint32_t keep, uint32_t* idx_out, uint32_t* n_out) {
  if ((n && !scores) || !idx_out || !n_out || keep < 1 || keep > COX_ALIGN_MAX_KEEP || n > 0xFFFFFFFFull) return COX_ERR_INVALID_ARG;
  *n_out = select_best(scores, n, min_corr, keep, idx_out);
  return COX_OK;
}

int cox_align_search(cox_align_t* G, const double pose_read[4], const cox_align_search_config* cfg, double* poses_out, cox_align_score* scores_out,
                     uint32_t* n_found, cox_align_level* trace) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!G || !pose_read || !cfg || !poses_out || !scores_out || !n_found) return COX_ERR_INVALID_ARG;
  *n_found = 0;
  if (!tau_ok(cfg->inlier_distance) || !tau_ok(cfg->tau_min) || cfg->levels > COX_ALIGN_MAX_LEVELS || cfg->keep < 1 || cfg->keep > COX_ALIGN_MAX_KEEP)
    return COX_ERR_INVALID_ARG;
  long long mk[4];
  u64 count = 0;
  if (!grid_counts(cfg->center, cfg->half_extent, cfg->step, mk, &count)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(G->reading->device));
  const u32 K = cfg->keep;
  std::vector<double> cand(4 * count), kept(4 * static_cast<size_t>(K));
  std::vector<cox_align_score> rec;
  grid_fill(cfg->center, cfg->step, mk, cand.data());
  double step[4] = {cfg->step[0], cfg->step[1], cfg->step[2], cfg->step[3]};
  float tau = cfg->inlier_distance;
  u32 n_kept = 0;
  for (u32 level = 0;; ++level) {
    const u64 M = cand.size() / 4;
    rec.resize(M);
    COX_TRY(sweep_all(G, pose_read, cand.data(), M, tau, rec.data()));
    uint32_t idx[COX_ALIGN_MAX_KEEP];
    n_kept = select_best(rec.data(), M, cfg->min_corr, K, idx);
    for (u32 j = 0; j < n_kept; ++j) {
      std::memcpy(&kept[4 * j], &cand[4 * static_cast<size_t>(idx[j])], sizeof(double) * 4);
      scores_out[j] = rec[idx[j]];
    }
    if (trace) {
      cox_align_level& T = trace[level];
      std::memset(&T, 0, sizeof(T));
      T.n_candidates = M;
      T.inlier_distance = tau;
      T.n_kept = n_kept;
      for (int k = 0; k < 4; ++k) T.step[k] = step[k];
      for (u32 j = 0; j < n_kept; ++j) {
        T.kept_index[j] = idx[j];
        std::memcpy(&T.kept_pose[4 * j], &kept[4 * j], sizeof(double) * 4);
        T.kept_score[j] = scores_out[j];
      }
    }
    if (n_kept == 0 || level == cfg->levels) break;
    for (int k = 0; k < 4; ++k) step[k] = step[k] / 2;
    tau = std::max(tau / 2.0f, cfg->tau_min);
    long long m1[4];
    u64 per = 0;
    if (!grid_counts(&kept[0], step, step, m1, &per)) return COX_ERR_INVALID_ARG;  // (3 per unfrozen axis)
    cand.assign(4 * per * n_kept, 0.0);
    for (u32 j = 0; j < n_kept; ++j) grid_fill(&kept[4 * j], step, m1, &cand[4 * per * j]);
  }
  std::memcpy(poses_out, kept.data(), sizeof(double) * 4 * n_kept);
  *n_found = n_kept;
  return COX_OK;
}

int cox_align_kernel_time(cox_align_t* G, double* ms, uint64_t* sweeps, int reset) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!G) return COX_ERR_INVALID_ARG;
  if (ms) *ms = G->ms;
  if (sweeps) *sweeps = G->sweeps;
  if (reset) {
    G->ms = 0.0;
    G->sweeps = 0;
  }
  return COX_OK;
}

}  // extern "C"
