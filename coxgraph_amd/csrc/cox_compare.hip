// MI355X (gfx950): comparing two layers behind include/coxgraph_hip_compare.h -- the error statistics of voxblox's
// utils::evaluateLayersRmse and the free-space conflict counts of a loop-closure check, for a batch of transforms T_B_A in one
// launch.  Rule, window bound, launch shape and measurements: DESIGN.md section 7p.
//
//   k_compare<TRI, WRITE>  grid (blocks of A, transform chunks) x 256 lanes.  A workgroup owns ONE block of A: its 4096
//                          (distance, weight) pairs are read once, coalesced, into 32 KB of LDS and stay there for the chunk's
//                          transforms (up to kCmpMaxTile; fewer while the grid would not fill the chip).  Per transform the
//                          first 27 lanes resolve, once, the pool indices of the 3 x 3 x 3 blocks of B around the
//                          transformed block into an LDS window; every voxel's sample
//                          (tri_sample / nearest_sample of cox_interp.hpp on the WinFind finder) finds its blocks there without
//                          a hash probe, and anything outside the window asks the hash table, so the window never changes an
//                          answer.  Per-lane counts are summed over the wave (cox_device.hpp's wave sums), over the workgroup
//                          in LDS, and reach the record by one set of integer atomics per (workgroup, transform).  Everything
//                          that is summed is an integer: no order matters.  WRITE also stores the three words of the error layer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#include "../../include/coxgraph_hip_compare.h"
#include "cox_device.hpp"
#include "cox_host.hpp"
#include "cox_interp.hpp"

using namespace cox;

namespace {

constexpr int kCmpThreads = 256;
constexpr u32 kCmpMaxTile = 8;      // transforms a workgroup walks at most with its block of A in LDS
constexpr u32 kCmpFillGrid = 1024;  // workgroups that fill the chip: below that a tile is cut shorter (a record does not notice)
constexpr int kCmpWindow = 3;       // blocks of B per axis in the window (a rotated block plus the cell spans < 34 voxels)
constexpr int kCmpWindowBlocks = kCmpWindow * kCmpWindow * kCmpWindow;
constexpr int kCmpSums = 12;        // the uint64_t fields of cox_compare_stats in front of hist, in its order
constexpr int kCmpWords = kCmpSums + COX_COMPARE_HIST_BINS;  // uint64_t words of a record in front of min_q | max_q
enum : int { kNA = 0, kOV, kIG, kEV, kSQ, kLO, kHI, kNEA, kNEB, kAFB, kBFA, kAGR };

static_assert(sizeof(cox_compare_stats) == 8 * (kCmpWords + 1), "cox_compare_stats is 35 words of 8 bytes");
static_assert(offsetof(cox_compare_stats, hist) == 8 * kCmpSums && offsetof(cox_compare_stats, min_q) == 8 * kCmpWords, "field order");

struct CmpParams {
  const u32* a_voxels;
  const u64* a_keys;
  float a_voxel_size, a_block_size;
  u32 n_t, tile;
  int has_T, ignore, use_window;
  float s, f, a, min_weight;
};

// block finder on the workgroup's window: (x, y, z) -> pool index or kInvalid
struct WinFind {
  const LayerView& L;
  const u32* win;  // LDS, [x - lo.x][y - lo.y][z - lo.z]
  int lo0, lo1, lo2;
  bool on;
  __device__ __forceinline__ u32 operator()(int x, int y, int z) const {
    const u32 dx = static_cast<u32>(x - lo0), dy = static_cast<u32>(y - lo1), dz = static_cast<u32>(z - lo2);
    if (on && dx < kCmpWindow && dy < kCmpWindow && dz < kCmpWindow) return win[(dx * kCmpWindow + dy) * kCmpWindow + dz];
    return HtPool{L}(x, y, z);
  }
};

template <bool TRI, bool WRITE>
__global__ void __launch_bounds__(kCmpThreads) k_compare(LayerView B, CmpParams P, const float* __restrict__ T, cox_compare_stats* rec, u32* __restrict__ err_voxels) {
  __shared__ float sA_d[kVoxelsPerBlock], sA_w[kVoxelsPerBlock];
  __shared__ unsigned long long sh_sum[kCmpSums];
  __shared__ u32 sh_hist[COX_COMPARE_HIST_BINS];
  __shared__ u32 sh_mm[2];  // max of ~q, max of q
  __shared__ u32 sh_win[kCmpWindowBlocks];
  __shared__ int sh_lo[4];  // window corner, and whether the window is on
  const u32 tid = threadIdx.x, lane = tid & 63u;
  const u32 pool = blockIdx.x;
  {
    const u32* blk = P.a_voxels + static_cast<size_t>(pool) * kVoxelsPerBlock * kWordsPerVoxel;
    for (u32 i = tid; i < kVoxelsPerBlock * kWordsPerVoxel; i += kCmpThreads) {
      const u32 word = blk[i];
      const u32 v = i / 3u, c = i - 3u * v;
      if (c == 0u) sA_d[v] = __uint_as_float(word);
      if (c == 1u) sA_w[v] = __uint_as_float(word);
    }
  }
  int bx, by, bz;
  unpack_key(P.a_keys[pool], &bx, &by, &bz);
  const float ox = static_cast<float>(bx) * P.a_block_size, oy = static_cast<float>(by) * P.a_block_size, oz = static_cast<float>(bz) * P.a_block_size;
  const u32 t0 = blockIdx.y * P.tile;
  for (u32 tt = 0; tt < P.tile; ++tt) {
    const u32 t = t0 + tt;
    if (t >= P.n_t) break;  // uniform
    float qw = 1.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f;
    F3 tr{0.0f, 0.0f, 0.0f};
    if (P.has_T) {
      const float* p = T + 7ull * t;
      qw = p[0], qx = p[1], qy = p[2], qz = p[3];
      tr = F3{p[4], p[5], p[6]};
    }
    if (tid < kCmpSums) sh_sum[tid] = 0ull;
    if (tid < COX_COMPARE_HIST_BINS) sh_hist[tid] = 0u;
    if (tid < 2) sh_mm[tid] = 0u;
    if (tid < kCmpWindowBlocks) {
      // the corner of the window: the least transformed centre of the block's 8 corner voxels, less the reach of a cell (one
      // voxel of B below the sample) and half a voxel of slack.  Where this is off, samples fall out of the window and ask the table.
      bool on = P.use_window != 0;
      int lo[3] = {0, 0, 0};
      if (on) {
        float mn[3] = {INFINITY, INFINITY, INFINITY};
        bool finite = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const F3 cen{ox + center_coord((c & 4) ? 15 : 0, P.a_voxel_size), oy + center_coord((c & 2) ? 15 : 0, P.a_voxel_size),
                       oz + center_coord((c & 1) ? 15 : 0, P.a_voxel_size)};
          const F3 p = P.has_T ? quat_transform(qw, qx, qy, qz, tr, cen) : cen;
          const float pp[3] = {p.x, p.y, p.z};
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            finite = finite && index_in_range(pp[k] * B.block_size_inv);  // false for NaN, +-inf, beyond the keys
            mn[k] = fminf(mn[k], pp[k]);
          }
        }
        on = finite;
        if (on) {
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            lo[k] = static_cast<int>(floorf((mn[k] - 1.5f * B.voxel_size) * B.block_size_inv));
            on = on && lo[k] > -kIdxBias && lo[k] + kCmpWindow < kIdxBias;
          }
        }
      }
      u32 p = kInvalid;
      if (on) p = HtPool{B}(lo[0] + static_cast<int>(tid / 9u), lo[1] + static_cast<int>((tid / 3u) % 3u), lo[2] + static_cast<int>(tid % 3u));
      sh_win[tid] = p;
      if (tid == 0) {
        sh_lo[0] = lo[0], sh_lo[1] = lo[1], sh_lo[2] = lo[2];
        sh_lo[3] = on ? 1 : 0;
      }
    }
    __syncthreads();  // the block of A (first round), the zeroed sums, the window
    const WinFind find{B, sh_win, sh_lo[0], sh_lo[1], sh_lo[2], sh_lo[3] != 0};
    u32 acc[kCmpSums];
#pragma unroll
    for (int k = 0; k < kCmpSums; ++k) acc[k] = 0u;  // a lane adds 16 voxels: every per-lane sum stays below 2^25
    u32 mn_c = 0u, mx = 0u;
#pragma unroll 1
    for (u32 v = tid; v < kVoxelsPerBlock; v += kCmpThreads) {
      const float dA = sA_d[v], wA = sA_w[v];
      u32 cls = COX_COMPARE_CLASS_UNOBSERVED;
      float e_out = 0.0f;
      if (wA > P.min_weight) {
        acc[kNA] += 1u;
        cls = COX_COMPARE_CLASS_NO_COUNTERPART;
        const F3 cen{ox + center_coord(static_cast<int>(v & 15u), P.a_voxel_size), oy + center_coord(static_cast<int>((v >> 4) & 15u), P.a_voxel_size),
                     oz + center_coord(static_cast<int>(v >> 8), P.a_voxel_size)};
        const F3 p = P.has_T ? quat_transform(qw, qx, qy, qz, tr, cen) : cen;
        const float pos[3] = {p.x, p.y, p.z};
        float dB = 0.0f, wB = 0.0f;
        bool ok = false;
        if (point_in_range(B, pos)) ok = TRI ? tri_sample(B, find, pos, &dB, &wB, true) : nearest_sample(B, find, pos, &dB, &wB);
        if (ok && wB > P.min_weight) {
          acc[kOV] += 1u;
          const float e = dA - dB;
          const float ae = fabsf(e);
          const bool near_a = fabsf(dA) <= P.s, near_b = fabsf(dB) <= P.s;
          const bool afb = near_a && dB >= P.f, bfa = near_b && dA >= P.f;
          acc[kNEA] += near_a ? 1u : 0u;
          acc[kNEB] += near_b ? 1u : 0u;
          acc[kAFB] += afb ? 1u : 0u;
          acc[kBFA] += bfa ? 1u : 0u;
          acc[kAGR] += ae <= P.a ? 1u : 0u;
          const bool behind_a = dA < 0.0f, behind_b = dB < 0.0f;
          const bool ignored = P.ignore == COX_COMPARE_IGNORE_BEHIND_TEST  ? behind_a
                               : P.ignore == COX_COMPARE_IGNORE_BEHIND_GT  ? behind_b
                               : P.ignore == COX_COMPARE_IGNORE_BEHIND_ALL ? (behind_a && behind_b)
                                                                           : false;
          if (ignored) {
            acc[kIG] += 1u;
            cls = COX_COMPARE_CLASS_IGNORED;
          } else {
            const u32 q = ae < 16.0f ? static_cast<u32>(floorf(ae * 65536.0f)) : COX_COMPARE_Q_SATURATED;  // a NaN takes the second branch
            const u64 q2 = static_cast<u64>(q) * q;
            acc[kEV] += 1u;
            acc[kSQ] += q;
            acc[kLO] += static_cast<u32>(q2 & 0xFFFFFull);
            acc[kHI] += static_cast<u32>(q2 >> 20);
            mn_c = max(mn_c, ~q);
            mx = max(mx, q);
            atomicAdd(&sh_hist[q == 0u ? 0u : 32u - static_cast<u32>(__clz(static_cast<int>(q)))], 1u);
            cls = COX_COMPARE_CLASS_EVALUATED;
            e_out = e;
          }
          cls |= (afb ? COX_COMPARE_A_SURFACE_IN_B_FREE : 0u) | (bfa ? COX_COMPARE_B_SURFACE_IN_A_FREE : 0u);
        }
      }
      if (WRITE) {
        u32* o = err_voxels + (static_cast<size_t>(pool) * kVoxelsPerBlock + v) * kWordsPerVoxel;
        o[0] = __float_as_uint(e_out);
        o[1] = (cls & COX_COMPARE_CLASS_MASK) == COX_COMPARE_CLASS_EVALUATED ? __float_as_uint(1.0f) : 0u;
        o[2] = cls;
      }
    }
#pragma unroll
    for (int k = 0; k < kCmpSums; ++k) {
      const u32 sum = wave_sum_u32(acc[k]);  // below 2^31
      if (lane == 0 && sum) atomicAdd(&sh_sum[k], static_cast<unsigned long long>(sum));
    }
    if (mn_c) atomicMax(&sh_mm[0], mn_c);
    if (mx) atomicMax(&sh_mm[1], mx);
    __syncthreads();
    unsigned long long* r64 = reinterpret_cast<unsigned long long*>(rec + t);
    if (tid < kCmpSums) {
      if (sh_sum[tid]) atomicAdd(&r64[tid], sh_sum[tid]);
    } else if (tid < kCmpWords) {
      const u32 h = sh_hist[tid - kCmpSums];
      if (h) atomicAdd(&r64[tid], static_cast<unsigned long long>(h));
    } else if (tid == kCmpWords) {
      if (sh_mm[0]) atomicMax(&rec[t].min_q, sh_mm[0]);  // the largest ~q: the host turns it round
    } else if (tid == kCmpWords + 1) {
      if (sh_mm[1]) atomicMax(&rec[t].max_q, sh_mm[1]);
    }
    __syncthreads();  // the sums are zeroed again in the next round
  }
}

bool distance_ok(float v) { return std::isfinite(v) && v >= 0.0f; }
bool modes_ok(int ignore_mode, int sample_mode) {
  return ignore_mode >= COX_COMPARE_ALL && ignore_mode <= COX_COMPARE_IGNORE_BEHIND_ALL && (sample_mode == COX_COMPARE_NEAREST || sample_mode == COX_COMPARE_TRILINEAR);
}

}  // namespace

struct cox_compare {
  const cox_layer* A = nullptr;
  const cox_layer* B = nullptr;
  cox_compare_config cfg{};
  Stream stream;
  DevBuf<float> d_T;
  PinnedBuf<float> h_T;
  DevBuf<cox_compare_stats> d_rec;
  PinnedBuf<cox_compare_stats> h_rec;
  PinnedBuf<u32> h_nb;
  EventPair ev;
  double ms = 0.0;
  uint64_t runs = 0;
};

// n records (n >= 1) of A's first nb pool blocks against B, on G's stream; err_voxels: the block array of an error layer (n == 1) or null
static int compare_launch(cox_compare* G, const float* T, u32 n, u32 nb, int ignore_mode, int sample_mode, u32* err_voxels, cox_compare_stats* out) {
  COX_TRY(G->d_rec.grow(n));
  COX_TRY(G->h_rec.grow(n));
  hipStream_t s = G->stream;
  if (T) {
    COX_TRY(G->d_T.grow(7ull * n));
    COX_TRY(G->h_T.grow(7ull * n));
    std::memcpy(G->h_T.p, T, sizeof(float) * 7 * n);
    COX_HIP(hipMemcpyAsync(G->d_T, G->h_T, sizeof(float) * 7 * n, hipMemcpyHostToDevice, s));
  }
  const cox_layer *A = G->A, *B = G->B;
  const LayerView BV = layer_view(B);
  CmpParams P{};
  P.a_voxels = A->voxels;
  P.a_keys = A->block_keys;
  P.a_voxel_size = A->voxel_size;
  P.a_block_size = A->block_size;
  P.n_t = n;
  // as many transforms per workgroup as still leave kCmpFillGrid workgroups
  P.tile = std::min<u32>(kCmpMaxTile, std::max<u64>(1, static_cast<u64>(n) * nb / kCmpFillGrid));
  P.has_T = T ? 1 : 0;
  P.ignore = ignore_mode;
  // a block of B no smaller than a block of A: the window holds every block a transformed block of A reaches; else the hash path throughout
  P.use_window = B->block_size >= A->block_size ? 1 : 0;
  P.s = G->cfg.surface_distance, P.f = G->cfg.free_distance, P.a = G->cfg.agree_distance, P.min_weight = G->cfg.min_weight;
  COX_HIP(G->ev.begin(s));
  COX_HIP(hipMemsetAsync(G->d_rec, 0, sizeof(cox_compare_stats) * n, s));
  const dim3 grid(nb, (n + P.tile - 1) / P.tile), block(kCmpThreads);
  const bool tri = sample_mode == COX_COMPARE_TRILINEAR;
  if (err_voxels) {
    if (tri)
      hipLaunchKernelGGL((k_compare<true, true>), grid, block, 0, s, BV, P, G->d_T.p, G->d_rec.p, err_voxels);
    else
      hipLaunchKernelGGL((k_compare<false, true>), grid, block, 0, s, BV, P, G->d_T.p, G->d_rec.p, err_voxels);
  } else {
    if (tri)
      hipLaunchKernelGGL((k_compare<true, false>), grid, block, 0, s, BV, P, G->d_T.p, G->d_rec.p, static_cast<u32*>(nullptr));
    else
      hipLaunchKernelGGL((k_compare<false, false>), grid, block, 0, s, BV, P, G->d_T.p, G->d_rec.p, static_cast<u32*>(nullptr));
  }
  COX_HIP(G->ev.end(s));
  COX_HIP(hipMemcpyAsync(G->h_rec, G->d_rec, sizeof(cox_compare_stats) * n, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  COX_HIP(hipGetLastError());
  for (u32 i = 0; i < n; ++i) {
    cox_compare_stats& r = G->h_rec.p[i];
    r.min_q = r.n_evaluated ? ~r.min_q : 0u;  // the kernel keeps the largest ~q
    if (out) out[i] = r;
  }
  double ms = 0.0;
  if (G->ev.elapsed_ms(&ms)) {
    G->ms += ms;
    G->runs += 1;
  }
  return COX_OK;
}

// the block count of A behind every frame enqueued on either layer (G's stream waits for both)
static int compare_begin(cox_compare* G, u32* nb) {
  hipStream_t s = G->stream;
  cox_layer_wait_writes(G->A, s);
  cox_layer_wait_writes(G->B, s);
  COX_HIP(hipMemcpyAsync(G->h_nb, G->A->d_nblocks, sizeof(u32), hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  *nb = static_cast<u32>(std::min<u64>(*G->h_nb.p, G->A->capacity));
  return COX_OK;
}

extern "C" {

void cox_compare_config_default(cox_compare_config* cfg) {
  if (!cfg) return;
  cfg->surface_distance = 0.0f;
  cfg->free_distance = 0.0f;
  cfg->agree_distance = 0.0f;
  cfg->min_weight = 1e-6f;
}

int cox_compare_create(const cox_layer_t* A, const cox_layer_t* B, const cox_compare_config* cfg, cox_compare_t** out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (out) *out = nullptr;
  if (!A || !B || !out) return COX_ERR_INVALID_ARG;
  cox_compare_config c;
  cox_compare_config_default(&c);
  if (cfg) c = *cfg;
  if (!distance_ok(c.surface_distance) || !distance_ok(c.free_distance) || !distance_ok(c.agree_distance) || !distance_ok(c.min_weight)) return COX_ERR_INVALID_ARG;
  if (c.surface_distance == 0.0f) c.surface_distance = A->voxel_size;
  if (c.free_distance == 0.0f) c.free_distance = 2.0f * c.surface_distance;
  if (c.agree_distance == 0.0f) c.agree_distance = c.surface_distance;
  if (!std::isfinite(c.free_distance) || !(c.free_distance > c.surface_distance) || A->device != B->device) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(A->device));
  cox_compare* G = new (std::nothrow) cox_compare();
  if (!G) return COX_ERR_OUT_OF_MEMORY;
  G->A = A;
  G->B = B;
  G->cfg = c;
  if (G->stream.create() != COX_OK || G->ev.create() != COX_OK || G->h_nb.alloc(1) != COX_OK) {
    cox_compare_destroy(G);
    return COX_ERR_NO_DEVICE;
  }
  *out = G;
  return COX_OK;
}

void cox_compare_destroy(cox_compare_t* G) {
  if (!G) return;
  (void)hipSetDevice(G->A->device);
  if (G->stream) (void)hipStreamSynchronize(G->stream);
  delete G;
}

int cox_compare_get_config(const cox_compare_t* G, cox_compare_config* cfg) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!G || !cfg) return COX_ERR_INVALID_ARG;
  *cfg = G->cfg;
  return COX_OK;
}

int cox_compare_run(cox_compare_t* G, const float* T_B_A, uint64_t n, int ignore_mode, int sample_mode, cox_compare_stats* stats_out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!G || !modes_ok(ignore_mode, sample_mode) || n > COX_COMPARE_MAX_TRANSFORMS) return COX_ERR_INVALID_ARG;
  if (n == 0) return COX_OK;
  if (!stats_out || (!T_B_A && n != 1)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(G->A->device));
  u32 nb = 0;
  COX_TRY(compare_begin(G, &nb));
  if (nb == 0) {  // no voxel of A: every sum is empty
    std::memset(stats_out, 0, sizeof(cox_compare_stats) * n);
    return COX_OK;
  }
  return compare_launch(G, T_B_A, static_cast<u32>(n), nb, ignore_mode, sample_mode, nullptr, stats_out);
}

int cox_compare_error_layer(cox_compare_t* G, const float* T_B_A, int ignore_mode, int sample_mode, cox_layer_t** error_layer) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (error_layer) *error_layer = nullptr;
  if (!G || !error_layer || !modes_ok(ignore_mode, sample_mode)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(G->A->device));
  // A's blocks under A's pool indices, its keys and its hash table: the words are rewritten in place
  cox_layer* E = nullptr;
  COX_TRY(cox_layer_clone_to_device(G->A, G->A->device, 0, &E));
  u32 nb = 0, nb_clone = 0;
  int st = compare_begin(G, &nb);
  if (st == COX_OK) st = cox_hip_status(hipMemcpy(&nb_clone, E->d_nblocks, sizeof(u32), hipMemcpyDeviceToHost));
  nb = std::min(nb, nb_clone);  // the blocks the clone holds
  if (st == COX_OK && nb) st = compare_launch(G, T_B_A, 1, nb, ignore_mode, sample_mode, E->voxels, nullptr);
  if (st != COX_OK) {
    cox_layer_destroy(E);
    return st;
  }
  *error_layer = E;
  return COX_OK;
}

int cox_compare_kernel_time(cox_compare_t* G, double* ms, uint64_t* runs, int reset) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!G) return COX_ERR_INVALID_ARG;
  if (ms) *ms = G->ms;
  if (runs) *runs = G->runs;
  if (reset) {
    G->ms = 0.0;
    G->runs = 0;
  }
  return COX_OK;
}

}  // extern "C"
