// MI355X (gfx950): depth, normal and colour images of a layer seen from a pose, behind include/coxgraph_hip_render.h.
//
//   k_render  one lane per pixel, one wave per 8 x 8 pixel tile (a workgroup is 16 x 16 pixels): neighbouring lanes walk
//             neighbouring rays, so their voxel loads share cache lines and their block lookups hit the same hash slots.  A ray
//             is sphere-traced through the layer: a sample is the ADAPTIVE distance of the map queries (tri_sample of
//             cox_interp.hpp, else its containing_voxel), the next step is |d| * step_scale, an unallocated block
//             is left through its far face in one step, and a positive sample followed by a non-positive one
//             is the hit, placed by one linear interpolation.  The blocks around a sample are resolved through a per-lane
//             BlockSet (cox_interp.hpp) of the last 2 x 2 x 2 blocks, moved and filled as the ray asks (consecutive samples
//             of a ray mostly stay inside it); whatever the cache does not hold is looked up in the hash table, so the cache
//             never changes an answer.  Lanes do not wait for each other: a wave ends when its longest ray does.
//
// Rules and arithmetic: DESIGN.md section 7g.  The float expressions are those of tests/cpp/render_reference.cpp, one by one.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/coxgraph_hip_render.h"
#include "cox_host.hpp"
#include "cox_interp.hpp"

using namespace cox;

namespace {

constexpr int kRenderThreads = 256;  // 4 waves: 2 x 2 tiles of 8 x 8 pixels
constexpr int kTile = 16;

struct RenderParams {
  float qw, qx, qy, qz, ox, oy, oz;  // T_G_C
  float fx, fy, cx, cy;
  int w, h;
  u32 tiles_x;
  float min_depth, max_depth, step_scale;
  float min_step;    // min_step_voxels * voxel_size
  float half_voxel;  // 0.5 * voxel_size
  u32 max_samples;
};

__device__ __forceinline__ F3 rotate(const RenderParams& P, F3 v) { return quat_rotate(P.qw, P.qx, P.qy, P.qz, v); }

__global__ void __launch_bounds__(kRenderThreads) k_render(LayerView L, RenderParams P, float* __restrict__ depth, float* __restrict__ normal,
                                                           u32* __restrict__ rgba, uint8_t* __restrict__ status, unsigned long long* __restrict__ stats) {
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const int u = static_cast<int>((blockIdx.x % P.tiles_x) * kTile + (wave & 1u) * 8u + (lane & 7u));
  const int v = static_cast<int>((blockIdx.x / P.tiles_x) * kTile + (wave >> 1) * 8u + (lane >> 3));
  const bool inside = u < P.w && v < P.h;
  const float nan = __uint_as_float(0x7FC00000u);
  u32 st = 0u, n_samples = 0u, n_skips = 0u, color = 0u;
  float t_hit = nan, nrm[3] = {nan, nan, nan};
  if (inside) {
    const float xn = (static_cast<float>(u) - P.cx) / P.fx;
    const float yn = (static_cast<float>(v) - P.cy) / P.fy;
    const F3 dc{xn, yn, 1.0f};
    const F3 dg = rotate(P, dc);
    const float len = sqrtf(dot3(dc, dc));
    const float o[3] = {P.ox, P.oy, P.oz}, dir[3] = {dg.x, dg.y, dg.z};
    BlockSet cache = kNoBlocks;  // kept from sample to sample until the ray leaves the set
    const SetFind bc{L, cache};
    float t = P.min_depth, t_prev = 0.0f, d_prev = 0.0f;
    bool have_prev = false;
    while (t <= P.max_depth) {
      if (n_samples >= P.max_samples) {
        st = COX_R_BUDGET;
        break;
      }
      ++n_samples;
      float p[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = o[k] + t * dir[k];
      if (!point_in_range(L, p)) break;  // left the index range (or NaN): a miss
      int b[3], lo[3], span[3];
      block_window(L, p, 2, b, lo, span);  // a cell reaches g - 1 .. g + 1, one more voxel for rounding at block faces
      cache.move(lo);
      if (cache.own(L, b[0], b[1], b[2]) == kInvalid) {
        // nothing here: leave the block through its far face, plus half a voxel
        have_prev = false;
        ++n_skips;
        float t_exit = __uint_as_float(0x7F800000u);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          if (dir[k] != 0.0f) {
            const float face = static_cast<float>(dir[k] > 0.0f ? b[k] + 1 : b[k]) * L.block_size;
            t_exit = std_min(t_exit, (face - o[k]) / dir[k]);
          }
        }
        const float t_new = t_exit + P.half_voxel / len;
        t = t_new > t ? t_new : t + L.voxel_size / len;  // always forward
        continue;
      }
      cache.fill(L, span);
      float d = 0.0f;
      bool ok = tri_sample(L, bc, p, &d, nullptr, false);
      if (!ok) {
        const u32* vox = containing_voxel(L, bc, p);
        if (vox != nullptr) {
          d = __uint_as_float(vox[0]);
          ok = __uint_as_float(vox[1]) > 0.0f;
        }
      }
      if (!ok) {  // unobserved: nothing to interpolate across
        have_prev = false;
        t = t + L.voxel_size / len;
        continue;
      }
      if (have_prev && d_prev > 0.0f && d <= 0.0f) {
        t_hit = t_prev + ((t - t_prev) * d_prev) / (d_prev - d);
        st = COX_R_HIT;
        break;
      }
      t_prev = t;
      d_prev = d;
      have_prev = true;
      t = t + std_max(fabsf(d) * P.step_scale, P.min_step) / len;
    }
    if (st & COX_R_HIT) {
      float p[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = o[k] + t_hit * dir[k];
      if (point_in_range(L, p)) {
        int b[3], lo[3], span[3];
        block_window(L, p, 3, b, lo, span);  // the gradient samples reach g - 2 .. g + 2
        cache.move(lo);
        cache.fill(L, span);
        const u32* vox = containing_voxel(L, bc, p);
        if (vox != nullptr) {  // Interpolator::getGradient: getBlockPtrByCoordinates(pos)
          if (__uint_as_float(vox[1]) > 0.0f) {
            color = __builtin_bswap32(vox[2]);  // wire word a | b << 8 | g << 16 | r << 24 -> bytes r, g, b, a
            st |= COX_R_COLOR;
          }
          // central differences of the trilinear distance, g_i = ((0 + d(p - h e_i) * -1) + d(p + h e_i)) / (2 h); one copy of
          // the gather in the code
          const float h = L.voxel_size, two_h = 2.0f * L.voxel_size;
          float g[3] = {0.0f, 0.0f, 0.0f}, acc = 0.0f;
          bool okg = true;
#pragma unroll 1
          for (int k = 0; k < 6 && okg; ++k) {
            const int axis = k >> 1;
            const bool plus = (k & 1) != 0;
            const float off = plus ? h : -h;
            const float s[3] = {axis == 0 ? p[0] + off : p[0] + 0.0f, axis == 1 ? p[1] + off : p[1] + 0.0f, axis == 2 ? p[2] + off : p[2] + 0.0f};
            float dv = 0.0f;
            if (!tri_sample(L, bc, s, &dv, nullptr, false)) {
              okg = false;
            } else if (!plus) {
              acc = 0.0f + dv * -1.0f;
            } else {
              const float gi = (acc + dv) / two_h;
              g[0] = axis == 0 ? gi : g[0];
              g[1] = axis == 1 ? gi : g[1];
              g[2] = axis == 2 ? gi : g[2];
            }
          }
          if (okg) {  // Eigen normalized()
            const float z = dot3(F3{g[0], g[1], g[2]}, F3{g[0], g[1], g[2]});
            if (z > 0.0f) {
              const float s = sqrtf(z);
              g[0] = g[0] / s, g[1] = g[1] / s, g[2] = g[2] / s;
            }
            nrm[0] = g[0], nrm[1] = g[1], nrm[2] = g[2];
            st |= COX_R_NORMAL;
          }
        }
      }
    }
    // every pixel of every image is written, misses included
    const size_t i = static_cast<size_t>(v) * static_cast<size_t>(P.w) + static_cast<size_t>(u);
    if (depth) depth[i] = t_hit;
    if (normal) {
      normal[3 * i] = nrm[0];
      normal[3 * i + 1] = nrm[1];
      normal[3 * i + 2] = nrm[2];
    }
    if (rgba) rgba[i] = color;
    if (status) status[i] = static_cast<uint8_t>(st);
  }
  if (stats) {  // the same for every lane; the rays of the wave are all done here
    u32 a = n_samples, s = n_skips, hh = (st & COX_R_HIT) ? 1u : 0u, bb = (st & COX_R_BUDGET) ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off);
      s += __shfl_xor(s, off);
      hh += __shfl_xor(hh, off);
      bb += __shfl_xor(bb, off);
    }
    if (lane == 0u) {
      if (hh) atomicAdd(stats + 0, static_cast<unsigned long long>(hh));
      if (a) atomicAdd(stats + 1, static_cast<unsigned long long>(a));
      if (s) atomicAdd(stats + 2, static_cast<unsigned long long>(s));
      if (bb) atomicAdd(stats + 3, static_cast<unsigned long long>(bb));
    }
  }
}

int check_render_args(const cox_layer* L, const float* T, int w, int h, const float* K, const cox_render_config* cfg_in, RenderParams* P) {
  if (!L || !T || !K) return COX_ERR_INVALID_ARG;
  if (w <= 0 || h <= 0 || static_cast<u64>(w) * static_cast<u64>(h) > 0x7FFFFFFFull) return COX_ERR_INVALID_ARG;
  if (!finite_all(T, 7) || !finite_all(K, 4) || K[0] == 0.0f || K[1] == 0.0f) return COX_ERR_INVALID_ARG;
  cox_render_config cfg;
  if (cfg_in)
    cfg = *cfg_in;
  else
    cox_render_config_default(&cfg);
  if (!(cfg.max_depth > cfg.min_depth) || !(cfg.min_depth >= 0.0f) || !(cfg.step_scale > 0.0f)) return COX_ERR_INVALID_ARG;  // NaN fails too
  P->qw = T[0], P->qx = T[1], P->qy = T[2], P->qz = T[3], P->ox = T[4], P->oy = T[5], P->oz = T[6];
  P->fx = K[0], P->fy = K[1], P->cx = K[2], P->cy = K[3];
  P->w = w, P->h = h;
  P->tiles_x = static_cast<u32>((w + kTile - 1) / kTile);
  P->min_depth = cfg.min_depth, P->max_depth = cfg.max_depth, P->step_scale = cfg.step_scale;
  P->min_step = cfg.min_step_voxels * L->voxel_size;
  P->half_voxel = 0.5f * L->voxel_size;
  P->max_samples = cfg.max_samples;
  return COX_OK;
}

void launch_render(const cox_layer* L, const RenderParams& P, float* depth, float* normal, uint8_t* rgba, uint8_t* status, unsigned long long* stats,
                   hipStream_t s) {
  const u32 tiles_y = static_cast<u32>((P.h + kTile - 1) / kTile);
  hipLaunchKernelGGL(k_render, dim3(P.tiles_x * tiles_y), dim3(kRenderThreads), 0, s, layer_view(L), P, depth, normal, reinterpret_cast<u32*>(rgba), status,
                     stats);
}

}  // namespace

extern "C" {

void cox_render_config_default(cox_render_config* cfg) {
  if (!cfg) return;
  cfg->min_depth = 0.1f;
  cfg->max_depth = 10.0f;
  cfg->step_scale = 0.75f;
  cfg->min_step_voxels = 0.25f;
  cfg->max_samples = 4096u;
}

int cox_layer_render(cox_layer_t* L, const float T_G_C[7], int w, int h, const float K[4], const cox_render_config* cfg, float* depth, float* normal,
                     uint8_t* rgba, uint8_t* status, cox_render_stats* stats) {
  COX_ENTRY();
  COX_TRY(device_present());
  RenderParams P;
  COX_TRY(check_render_args(L, T_G_C, w, h, K, cfg, &P));
  COX_HIP(hipSetDevice(L->device));
  const size_t n = static_cast<size_t>(w) * static_cast<size_t>(h);
  // one staging allocation: counters | depth | normal | rgba | status
  const size_t b_cnt = stats ? 4 * sizeof(unsigned long long) : 0, b_d = depth ? 4 * n : 0, b_n = normal ? 12 * n : 0, b_c = rgba ? 4 * n : 0;
  DevBuf<uint8_t> buf;
  COX_TRY(buf.alloc(b_cnt + b_d + b_n + b_c + (status ? n : 0)));
  unsigned long long* d_cnt = stats ? reinterpret_cast<unsigned long long*>(buf.p) : nullptr;
  float* d_d = depth ? reinterpret_cast<float*>(buf.p + b_cnt) : nullptr;
  float* d_n = normal ? reinterpret_cast<float*>(buf.p + b_cnt + b_d) : nullptr;
  uint8_t* d_c = rgba ? buf.p + b_cnt + b_d + b_n : nullptr;
  uint8_t* d_s = status ? buf.p + b_cnt + b_d + b_n + b_c : nullptr;
  EventPair ev;
  if (stats) COX_TRY(ev.create());
  hipStream_t s = nullptr;
  cox_layer_wait_writes(L, s);  // frames still in flight on the layer
  if (stats) {
    COX_HIP(hipMemsetAsync(d_cnt, 0, b_cnt, s));
    COX_HIP(ev.begin(s));
  }
  launch_render(L, P, d_d, d_n, d_c, d_s, d_cnt, s);
  COX_HIP(hipGetLastError());
  if (stats) COX_HIP(ev.end(s));
  unsigned long long cnt[4] = {0, 0, 0, 0};
  if (stats) COX_HIP(hipMemcpyAsync(cnt, d_cnt, b_cnt, hipMemcpyDeviceToHost, s));
  if (depth) COX_HIP(hipMemcpyAsync(depth, d_d, b_d, hipMemcpyDeviceToHost, s));
  if (normal) COX_HIP(hipMemcpyAsync(normal, d_n, b_n, hipMemcpyDeviceToHost, s));
  if (rgba) COX_HIP(hipMemcpyAsync(rgba, d_c, b_c, hipMemcpyDeviceToHost, s));
  if (status) COX_HIP(hipMemcpyAsync(status, d_s, n, hipMemcpyDeviceToHost, s));
  COX_HIP(hipStreamSynchronize(s));
  if (stats) {
    if (!ev.elapsed_ms(&stats->kernel_ms)) return COX_ERR_NO_DEVICE;
    stats->n_hits = cnt[0], stats->n_samples = cnt[1], stats->n_block_skips = cnt[2], stats->n_budget = cnt[3];
  }
  return COX_OK;
}

int cox_layer_render_dev(cox_layer_t* L, const float T_G_C[7], int w, int h, const float K[4], const cox_render_config* cfg, float* depth_dev,
                         float* normal_dev, uint8_t* rgba_dev, uint8_t* status_dev, void* hip_stream) {
  COX_ENTRY();
  COX_TRY(device_present());
  RenderParams P;
  COX_TRY(check_render_args(L, T_G_C, w, h, K, cfg, &P));
  if (reinterpret_cast<uintptr_t>(rgba_dev) & 3u) return COX_ERR_INVALID_ARG;  // a pixel's colour is stored as one word
  COX_HIP(hipSetDevice(L->device));
  hipStream_t s = static_cast<hipStream_t>(hip_stream);
  cox_layer_wait_writes(L, s);
  launch_render(L, P, depth_dev, normal_dev, rgba_dev, status_dev, nullptr, s);
  COX_HIP(hipGetLastError());
  return COX_OK;
}

}  // extern "C"
