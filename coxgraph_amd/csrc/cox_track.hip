// MI355X (gfx950): scan-to-map registration behind include/coxgraph_hip_track.h -- refine a sensor pose against a TSDF layer.
//
//   k_track_step<DOF>  ONE Gauss-Newton iteration per launch.  256 lanes per workgroup, a fixed number of workgroups walking the
//                      scan's candidates (every stride-th point) in passes.  A lane moves its point into the layer's frame with the
//                      integrators' transform, takes the trilinear distance d and its analytic derivative g from one 2x2x2 gather
//                      (point_cell and interp_value_gradient of cox_interp.hpp, shared with the registration cost), and fills
//                      x = sqrt(w) [J(DOF), d, 1, 0...] plus two unscaled counters.  sum x x^T is cox_normal_eq.hpp's, shared with
//                      cox_reg.hip: each wave accumulates with v_mfma_f64_16x16x4_f64, workgroup tiles go to a partials array, the
//                      workgroup that draws the last ticket sums them in workgroup order.  Its thread 0 decides (lost /
//                      degenerate / converged), solves the damped system by Cholesky and writes the next pose, the record and a
//                      `done` word.
//   cox_track_refine*  max_iterations launches back to back on the tracker's stream, no host round trip: a launch that finds
//                      `done` set returns at once (a read that is uniform per workgroup, before anything else).  One D2H at the end.
//   k_track_evaluate   the per-point seam (p_G, d, g, status) through the same device function.
//
// No float atomics (the ticket is the only atomic), no grid barrier, no graph capture: two calls on the same inputs give the same
// bits.  Rules and arithmetic: DESIGN.md section 7i.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "../../include/coxgraph_hip_track.h"
#include "cox_host.hpp"
#include "cox_interp.hpp"
#include "cox_normal_eq.hpp"

using namespace cox;

namespace {

constexpr int kTrackThreads = kNeqThreads;
constexpr u32 kTrackMaxGroups = COX_TRACK_GRID_PASS / kTrackThreads;  // 256: one per CU
constexpr int kTile = kNeqTile;                                       // one 16x16 f64 tile per workgroup
static_assert(kTrackMaxGroups * kTrackThreads == COX_TRACK_GRID_PASS, "the exported grid pass is the launch shape");

// the scan: n sensor-frame points, or the n = w * h pixels of a depth image (depth != nullptr) back-projected on the fly
struct ScanView {
  const float* xyz;
  const float* depth;
  u32 n, stride;
  u32 w;
  float fx, fy, cx, cy;
};

struct TrackParams {
  float max_abs_distance;
  u32 min_points, max_iterations;
  int update;  // 0: cox_track_normal_eq_* -- sums only
  double huber_delta, damping, tol_t, tol_r, min_inlier_ratio;
};

// device-resident state of a call: read by every workgroup at the start of a launch, written by the last one at its end
struct TrackState {
  double T[7];  // qw qx qy qz tx ty tz
  double step_t, step_r;
  double first_cost, last_cost;
  u64 first_used, first_considered, last_used, last_considered;
  u32 status, iterations, done, pad;
};

// scan point i in the sensor frame; false when it is not considered (a coordinate / the depth not finite, depth <= 0)
__device__ __forceinline__ bool scan_point(const ScanView& S, u32 i, F3* p) {
  if (S.depth) {
    const float d = S.depth[i];
    if (!(isfinite(d) && d > 0.0f)) return false;
    const u32 u = i % S.w, v = i / S.w;
    const float xn = (static_cast<float>(u) - S.cx) / S.fx;  // the depth front end's arithmetic (cox_frontend.hpp)
    const float yn = (static_cast<float>(v) - S.cy) / S.fy;
    *p = F3{d * xn, d * yn, d};
    return true;
  }
  *p = F3{S.xyz[3ull * i], S.xyz[3ull * i + 1], S.xyz[3ull * i + 2]};
  return isfinite(p->x) && isfinite(p->y) && isfinite(p->z);
}

// Steps 1 and 3 of the rule for one considered point: p_G, and when the point is used d and g.  The cell, the trilinear value
// and its derivative are the registration cost's: point_cell and interp_value_gradient of cox_interp.hpp.
__device__ __forceinline__ bool track_point(const LayerView& L, const FrameParams& P, float max_abs_distance, F3 p_C, F3* p_G, float* d_out, F3* g_out) {
  const F3 pg = transform_point(P, p_C);
  *p_G = pg;
  const float pos[3] = {pg.x, pg.y, pg.z};
  float md[8], off[3];
  if (!point_cell(L, pos, md, off)) return false;
  float val, g[3];
  interp_value_gradient(md, off, L.voxel_size_inv, &val, g);
  if (max_abs_distance > 0.0f && !(fabsf(val) <= max_abs_distance)) return false;
  *d_out = val;
  *g_out = F3{g[0], g[1], g[2]};
  return true;
}

// the float pose the points are moved with: the seven state values rounded to float
__device__ __forceinline__ FrameParams pose_params(const double* T) {
  FrameParams P{};
  P.qw = static_cast<float>(T[0]);
  P.qx = static_cast<float>(T[1]);
  P.qy = static_cast<float>(T[2]);
  P.qz = static_cast<float>(T[3]);
  P.tx = static_cast<float>(T[4]);
  P.ty = static_cast<float>(T[5]);
  P.tz = static_cast<float>(T[6]);
  return P;
}

// ---- per-point seam --------------------------------------------------------------------------------------------------------
struct PoseF {
  float v[7];
};
__global__ void __launch_bounds__(kTrackThreads) k_track_evaluate(LayerView L, ScanView S, PoseF T, float max_abs_distance, float* __restrict__ out,
                                                                  uint8_t* __restrict__ status) {
  const u32 i = blockIdx.x * kTrackThreads + threadIdx.x;
  if (i >= S.n) return;
  FrameParams P{};
  P.qw = T.v[0], P.qx = T.v[1], P.qy = T.v[2], P.qz = T.v[3], P.tx = T.v[4], P.ty = T.v[5], P.tz = T.v[6];
  const float nan = __uint_as_float(0x7FC00000u);
  F3 pc, pg = F3{nan, nan, nan}, g = F3{nan, nan, nan};
  float d = nan;
  u32 st = 0;
  if (i % S.stride == 0 && scan_point(S, i, &pc)) {
    st = COX_TRACK_CONSIDERED;
    float dv;
    F3 gv;
    if (track_point(L, P, max_abs_distance, pc, &pg, &dv, &gv)) {
      st |= COX_TRACK_USED;
      d = dv;
      g = gv;
    }
  }
  if (status) status[i] = static_cast<uint8_t>(st);
  if (out) {
    float* o = out + 7ull * i;
    o[0] = pg.x, o[1] = pg.y, o[2] = pg.z, o[3] = d, o[4] = g.x, o[5] = g.y, o[6] = g.z;
  }
}

// ---- steps 6-9 on one thread -------------------------------------------------------------------------------------------------
// D: the 16 x 16 totals (row-major, LDS), W: 64 doubles of LDS work space.  Components of x: J 0..DOF-1, r = DOF, 1 = DOF + 1,
// used = DOF + 2, considered = DOF + 3 (the last two unscaled).
template <int DOF>
__device__ void track_decide(const double* D, double* W, const TrackParams& C, TrackState* st) {
  constexpr int R = DOF, USED = DOF + 2, CONS = DOF + 3;
  const u64 n_used = static_cast<u64>(D[USED * 16 + USED] + 0.5), n_cons = static_cast<u64>(D[CONS * 16 + CONS] + 0.5);
  const double cost = D[R * 16 + R];
  const u32 it = st->iterations;
  if (it == 0) {
    st->first_used = n_used;
    st->first_considered = n_cons;
    st->first_cost = cost;
  }
  st->last_used = n_used;
  st->last_considered = n_cons;
  st->last_cost = cost;
  st->iterations = it + 1;
  if (!C.update) {
    st->done = 1u;
    return;
  }
  // 6. lost
  if (n_used < C.min_points || static_cast<double>(n_used) < C.min_inlier_ratio * static_cast<double>(n_cons)) {
    st->status = COX_TRACK_LOST;
    st->done = 1u;
    return;
  }
  // 7. (H + damping diag(H)) delta = -b: lower Cholesky, the loop order of the header comment
  double* Lc = W;            // [DOF][DOF] row-major
  double* y = W + 36;        // [DOF]
  double* delta = W + 42;    // [DOF]
  for (int j = 0; j < DOF; ++j) {
    double s = D[j * 16 + j] + C.damping * D[j * 16 + j];
    for (int k = 0; k < j; ++k) s = s - Lc[j * DOF + k] * Lc[j * DOF + k];
    if (!(s > 0.0) || !isfinite(s)) {
      st->status = COX_TRACK_DEGENERATE;
      st->done = 1u;
      return;
    }
    const double ljj = sqrt(s);
    Lc[j * DOF + j] = ljj;
    for (int i = j + 1; i < DOF; ++i) {
      double a = D[i * 16 + j];
      for (int k = 0; k < j; ++k) a = a - Lc[i * DOF + k] * Lc[j * DOF + k];
      Lc[i * DOF + j] = a / ljj;
    }
  }
  for (int i = 0; i < DOF; ++i) {
    double s = -D[i * 16 + R];
    for (int k = 0; k < i; ++k) s = s - Lc[i * DOF + k] * y[k];
    y[i] = s / Lc[i * DOF + i];
  }
  for (int i = DOF - 1; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < DOF; ++k) s = s - Lc[k * DOF + i] * delta[k];
    delta[i] = s / Lc[i * DOF + i];
  }
  // 8. t <- t + delta_t, q <- normalize(exp(omega) (x) q)
  const double wx = DOF == 6 ? delta[3] : 0.0, wy = DOF == 6 ? delta[4] : 0.0, wz = DOF == 6 ? delta[5] : delta[3];
  const double theta = sqrt((wx * wx + wy * wy) + wz * wz);
  const double half = 0.5 * theta;
  const double sc = theta > 0.0 ? sin(half) / theta : 0.5;
  const double ew = cos(half), ex = sc * wx, ey = sc * wy, ez = sc * wz;
  const double qw = st->T[0], qx = st->T[1], qy = st->T[2], qz = st->T[3];
  double nw = ((ew * qw - ex * qx) - ey * qy) - ez * qz;
  double nx = ((ew * qx + ex * qw) + ey * qz) - ez * qy;
  double ny = ((ew * qy - ex * qz) + ey * qw) + ez * qx;
  double nz = ((ew * qz + ex * qy) - ey * qx) + ez * qw;
  const double nn = sqrt(((nw * nw + nx * nx) + ny * ny) + nz * nz);
  st->T[0] = nw / nn;
  st->T[1] = nx / nn;
  st->T[2] = ny / nn;
  st->T[3] = nz / nn;
  st->T[4] = st->T[4] + delta[0];
  st->T[5] = st->T[5] + delta[1];
  st->T[6] = st->T[6] + delta[2];
  // 9. stop
  const double step_t = sqrt((delta[0] * delta[0] + delta[1] * delta[1]) + delta[2] * delta[2]);
  st->step_t = step_t;
  st->step_r = theta;
  if (step_t <= C.tol_t && theta <= C.tol_r) {
    st->status = COX_TRACK_CONVERGED;
    st->done = 1u;
  } else if (it + 1 >= C.max_iterations) {
    st->status = COX_TRACK_MAX_ITERATIONS;
    st->done = 1u;
  }
}

// ---- one iteration ---------------------------------------------------------------------------------------------------------------
template <int DOF>
__global__ void __launch_bounds__(kTrackThreads) k_track_step(LayerView L, ScanView S, TrackParams C, TrackState* st, double* partials /*[grid][256]*/,
                                                              double* out /*[256]*/, u32* ticket) {
  if (st->done) return;  // the same word for every lane of every workgroup; written by an EARLIER launch only
  __shared__ double X[kNeqWaves][16][kNeqRow];
  __shared__ double tile[kNeqWaves][kNeqTile];
  __shared__ double work[64];
  const u32 nb = gridDim.x, bx = blockIdx.x;
  const FrameParams P = pose_params(st->T);
  const double tfx = static_cast<double>(P.tx), tfy = static_cast<double>(P.ty), tfz = static_cast<double>(P.tz);
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  const u32 n_cand = S.n ? (S.n - 1u) / S.stride + 1u : 0u;
  const u32 pass = nb * kTrackThreads;
  const u32 n_pass = (n_cand + pass - 1) / pass;
  for (u32 it = 0; it < n_pass; ++it) {
    const u32 j = it * pass + bx * kTrackThreads + threadIdx.x;
    double x[16];  // components DOF + 4 .. 15 stay zero
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = 0.0;
    F3 pc;
    if (j < n_cand && scan_point(S, j * S.stride, &pc)) {
      x[DOF + 3] = 1.0;  // considered
      F3 pg, g;
      float d;
      if (track_point(L, P, C.max_abs_distance, pc, &pg, &d, &g)) {
        // 4. per-point terms in float64 from the float values
        const double ax = static_cast<double>(pg.x) - tfx, ay = static_cast<double>(pg.y) - tfy, az = static_cast<double>(pg.z) - tfz;
        const double gx = g.x, gy = g.y, gz = g.z, r = d;
        const double ad = fabs(r);
        const double w = (C.huber_delta > 0.0 && ad > C.huber_delta) ? C.huber_delta / ad : 1.0;
        const double sw = sqrt(w);
        x[0] = sw * gx;
        x[1] = sw * gy;
        x[2] = sw * gz;
        if (DOF == 6) {
          x[3] = sw * (ay * gz - az * gy);
          x[4] = sw * (az * gx - ax * gz);
          x[DOF - 1] = sw * (ax * gy - ay * gx);
        } else {
          x[3] = sw * (ax * gy - ay * gx);
        }
        x[DOF] = sw * r;
        x[DOF + 1] = sw;
        x[DOF + 2] = 1.0;  // used
      }
    }
    normal_eq_wave_step(X, x, acc);
  }
  double total;
  if (!normal_eq_finish(tile, acc, partials, ticket, bx, nb, &total)) return;
  out[threadIdx.x] = total;
  tile[0][threadIdx.x] = total;
  __syncthreads();
  if (threadIdx.x == 0) track_decide<DOF>(tile[0], work, C, st);
}

bool config_ok(const cox_track_config& c) {
  auto nonneg = [](double v) { return v >= 0.0; };  // false for NaN
  return (c.dof == 4 || c.dof == 6) && c.stride >= 1u && nonneg(c.max_abs_distance) && nonneg(c.huber_delta) && nonneg(c.damping) &&
         nonneg(c.translation_tolerance) && nonneg(c.rotation_tolerance) && nonneg(c.min_inlier_ratio) && std::isfinite(c.max_abs_distance) &&
         std::isfinite(c.huber_delta) && std::isfinite(c.damping) && std::isfinite(c.min_inlier_ratio);
}

bool pose_ok(const float T[7]) {
  if (!finite_all(T, 7)) return false;
  double nn = 0.0;
  for (int k = 0; k < 4; ++k) nn += static_cast<double>(T[k]) * T[k];
  return nn > 0.0;
}

}  // namespace

struct cox_track {
  const cox_layer* layer = nullptr;
  cox_track_config cfg;
  Stream stream;
  EventPair ev;
  DevBuf<TrackState> d_state;
  PinnedBuf<TrackState> h_state;
  DevBuf<double> d_partials;  // [kTrackMaxGroups][256]
  DevBuf<double> d_out;       // [256]
  PinnedBuf<double> h_out;    // [256]
  DevBuf<u32> d_ticket;
  DevBuf<float> d_pts;  // staging of cox_track_refine's host points

  int acquire() {
    COX_TRY(stream.create());
    COX_TRY(ev.create());
    COX_TRY(h_state.alloc(1));
    COX_TRY(h_out.alloc(kTile));
    COX_TRY(d_state.alloc(1));
    COX_TRY(d_partials.alloc(static_cast<size_t>(kTile) * kTrackMaxGroups));
    COX_TRY(d_out.alloc(kTile));
    return d_ticket.alloc(1);
  }
};

namespace {

// the launches of one call: `iterations` steps from T on scan S; the state (and with want_sums the totals) on the host afterwards
int run_steps(cox_track* K, const float T[7], const ScanView& S, u32 iterations, int update, bool want_sums) {
  const cox_track_config& c = K->cfg;
  hipStream_t s = K->stream;
  TrackState* h = K->h_state;
  std::memset(h, 0, sizeof(TrackState));
  for (int k = 0; k < 7; ++k) h->T[k] = static_cast<double>(T[k]);
  h->status = COX_TRACK_MAX_ITERATIONS;
  h->done = iterations == 0 ? 1u : 0u;
  const TrackParams C{c.max_abs_distance, c.min_points, iterations, update, c.huber_delta, c.damping, c.translation_tolerance, c.rotation_tolerance,
                      c.min_inlier_ratio};
  const LayerView V = layer_view(K->layer);  // read on every call: a layer that grew has new buffers
  const u32 n_cand = S.n ? (S.n - 1u) / S.stride + 1u : 0u;
  const u32 nb = std::max<u32>(1u, std::min<u32>(kTrackMaxGroups, (n_cand + kTrackThreads - 1) / kTrackThreads));  // from n and the config only
  cox_layer_wait_writes(K->layer, s);  // frames still in flight on the layer
  COX_HIP(hipMemsetAsync(K->d_ticket, 0, sizeof(u32), s));  // whatever an earlier, failed launch left behind
  COX_HIP(hipMemcpyAsync(K->d_state, h, sizeof(TrackState), hipMemcpyHostToDevice, s));
  COX_HIP(K->ev.begin(s));
  for (u32 it = 0; it < iterations; ++it) {
    if (c.dof == 6)
      hipLaunchKernelGGL((k_track_step<6>), dim3(nb), dim3(kTrackThreads), 0, s, V, S, C, K->d_state, K->d_partials, K->d_out, K->d_ticket);
    else
      hipLaunchKernelGGL((k_track_step<4>), dim3(nb), dim3(kTrackThreads), 0, s, V, S, C, K->d_state, K->d_partials, K->d_out, K->d_ticket);
  }
  COX_HIP(K->ev.end(s));
  COX_HIP(hipGetLastError());
  COX_HIP(hipMemcpyAsync(h, K->d_state, sizeof(TrackState), hipMemcpyDeviceToHost, s));
  if (want_sums) COX_HIP(hipMemcpyAsync(K->h_out, K->d_out, sizeof(double) * kTile, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  return COX_OK;
}

int refine_scan(cox_track* K, const float T_prior[7], const ScanView& S, float T_refined[7], cox_track_result* result) {
  COX_TRY(run_steps(K, T_prior, S, K->cfg.max_iterations, 1, false));
  const TrackState& h = *K->h_state.p;
  if (T_refined)
    for (int k = 0; k < 7; ++k) T_refined[k] = static_cast<float>(h.T[k]);
  if (result) {
    result->status = static_cast<int32_t>(h.status);
    result->iterations = h.iterations;
    result->first_n_used = h.first_used, result->first_n_considered = h.first_considered;
    result->last_n_used = h.last_used, result->last_n_considered = h.last_considered;
    result->first_cost = h.first_cost, result->last_cost = h.last_cost;
    result->last_step_translation = h.step_t, result->last_step_rotation = h.step_r;
    for (int k = 0; k < 7; ++k) result->T_G_C[k] = h.T[k];
    if (!K->ev.elapsed_ms(&result->kernel_ms)) result->kernel_ms = 0.0;
  }
  return COX_OK;
}

int normal_eq_scan(cox_track* K, const float T[7], const ScanView& S, double H[36], double b[6], double* cost, uint64_t counts[2]) {
  COX_TRY(run_steps(K, T, S, 1, 0, true));
  const int dof = K->cfg.dof;
  const double* D = K->h_out;  // D[row * 16 + col] = sum_p x[row] x[col]
  if (H)
    for (int r = 0; r < 6; ++r)
      for (int q = 0; q < 6; ++q) H[6 * r + q] = (r < dof && q < dof) ? D[r * 16 + q] : 0.0;
  if (b)
    for (int r = 0; r < 6; ++r) b[r] = r < dof ? D[r * 16 + dof] : 0.0;
  if (cost) *cost = D[dof * 16 + dof];
  if (counts) counts[0] = K->h_state.p->last_used, counts[1] = K->h_state.p->last_considered;
  return COX_OK;
}

int points_view(const float* xyz_dev, uint64_t n, u32 stride, ScanView* S) {
  if ((n && !xyz_dev) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  *S = ScanView{xyz_dev, nullptr, static_cast<u32>(n), stride, 1u, 1.0f, 1.0f, 0.0f, 0.0f};
  return COX_OK;
}

int depth_view(const float* depth_dev, int w, int h, const float K[4], u32 stride, ScanView* S) {
  if (!depth_dev || !K || w <= 0 || h <= 0 || static_cast<uint64_t>(w) * static_cast<uint64_t>(h) > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(K[k])) return COX_ERR_INVALID_ARG;
  if (K[0] == 0.0f || K[1] == 0.0f) return COX_ERR_INVALID_ARG;
  *S = ScanView{nullptr, depth_dev, static_cast<u32>(w) * static_cast<u32>(h), stride, static_cast<u32>(w), K[0], K[1], K[2], K[3]};
  return COX_OK;
}

}  // namespace

extern "C" {

void cox_track_config_default(cox_track_config* cfg) {
  if (!cfg) return;
  cfg->dof = 4;
  cfg->max_iterations = 15;
  cfg->stride = 1;
  cfg->min_points = 32;
  cfg->max_abs_distance = 0.0f;
  cfg->reserved = 0.0f;
  cfg->huber_delta = 0.0;
  cfg->damping = 1e-6;
  cfg->translation_tolerance = 1e-4;
  cfg->rotation_tolerance = 1e-4;
  cfg->min_inlier_ratio = 0.3;
}

int cox_track_create(const cox_layer_t* layer, const cox_track_config* cfg, cox_track_t** out) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!layer || !out) return COX_ERR_INVALID_ARG;
  cox_track_config c;
  if (cfg)
    c = *cfg;
  else
    cox_track_config_default(&c);
  if (!config_ok(c)) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(layer->device));
  cox_track* K = new (std::nothrow) cox_track();
  if (!K) return COX_ERR_OUT_OF_MEMORY;
  K->layer = layer;
  K->cfg = c;
  if (K->acquire() != COX_OK) {
    cox_track_destroy(K);
    return COX_ERR_NO_DEVICE;
  }
  *out = K;
  return COX_OK;
}

void cox_track_destroy(cox_track_t* K) {
  if (!K) return;
  (void)hipSetDevice(K->layer->device);
  if (K->stream) (void)hipStreamSynchronize(K->stream);
  delete K;
}

int cox_track_evaluate_dev(cox_track_t* K, const float T_G_C[7], const float* xyz_dev, uint64_t n, float* pG_d_g_dev, uint8_t* status_dev) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!K || !T_G_C || !pose_ok(T_G_C)) return COX_ERR_INVALID_ARG;
  ScanView S;
  COX_TRY(points_view(xyz_dev, n, K->cfg.stride, &S));
  if (n == 0) return COX_OK;
  COX_HIP(hipSetDevice(K->layer->device));
  PoseF P;
  for (int k = 0; k < 7; ++k) P.v[k] = T_G_C[k];
  cox_layer_wait_writes(K->layer, K->stream);
  hipLaunchKernelGGL(k_track_evaluate, dim3((S.n + kTrackThreads - 1) / kTrackThreads), dim3(kTrackThreads), 0, K->stream, layer_view(K->layer), S, P,
                     K->cfg.max_abs_distance, pG_d_g_dev, status_dev);
  COX_HIP(hipGetLastError());
  COX_HIP(hipStreamSynchronize(K->stream));
  return COX_OK;
}

int cox_track_normal_eq_dev(cox_track_t* K, const float T_G_C[7], const float* xyz_dev, uint64_t n, double H[36], double b[6], double* cost,
                            uint64_t counts[2]) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!K || !T_G_C || !pose_ok(T_G_C)) return COX_ERR_INVALID_ARG;
  ScanView S;
  COX_TRY(points_view(xyz_dev, n, K->cfg.stride, &S));
  COX_HIP(hipSetDevice(K->layer->device));
  return normal_eq_scan(K, T_G_C, S, H, b, cost, counts);
}

int cox_track_normal_eq_depth_dev(cox_track_t* K, const float T_G_C[7], const float* depth_dev, int w, int h, const float Kc[4], double H[36],
                                  double b[6], double* cost, uint64_t counts[2]) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!K || !T_G_C || !pose_ok(T_G_C)) return COX_ERR_INVALID_ARG;
  ScanView S;
  COX_TRY(depth_view(depth_dev, w, h, Kc, K->cfg.stride, &S));
  COX_HIP(hipSetDevice(K->layer->device));
  return normal_eq_scan(K, T_G_C, S, H, b, cost, counts);
}

int cox_track_refine_dev(cox_track_t* K, const float T_prior[7], const float* xyz_dev, uint64_t n, float T_refined[7], cox_track_result* result) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!K || !T_prior || !pose_ok(T_prior)) return COX_ERR_INVALID_ARG;
  ScanView S;
  COX_TRY(points_view(xyz_dev, n, K->cfg.stride, &S));
  COX_HIP(hipSetDevice(K->layer->device));
  return refine_scan(K, T_prior, S, T_refined, result);
}

int cox_track_refine(cox_track_t* K, const float T_prior[7], const float* xyz, uint64_t n, float T_refined[7], cox_track_result* result) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!K || !T_prior || !pose_ok(T_prior) || (n && !xyz) || n > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  COX_HIP(hipSetDevice(K->layer->device));
  COX_TRY(K->d_pts.grow(3 * n));
  if (n) COX_HIP(hipMemcpyAsync(K->d_pts, xyz, sizeof(float) * 3 * n, hipMemcpyHostToDevice, K->stream));
  ScanView S;
  COX_TRY(points_view(K->d_pts, n, K->cfg.stride, &S));
  return refine_scan(K, T_prior, S, T_refined, result);
}

int cox_track_refine_depth_dev(cox_track_t* K, const float T_prior[7], const float* depth_dev, int w, int h, const float Kc[4], float T_refined[7],
                               cox_track_result* result) {
  COX_ENTRY();
  COX_TRY(device_present());
  if (!K || !T_prior || !pose_ok(T_prior)) return COX_ERR_INVALID_ARG;
  ScanView S;
  COX_TRY(depth_view(depth_dev, w, h, Kc, K->cfg.stride, &S));
  COX_HIP(hipSetDevice(K->layer->device));
  return refine_scan(K, T_prior, S, T_refined, result);
}

}  // extern "C"
