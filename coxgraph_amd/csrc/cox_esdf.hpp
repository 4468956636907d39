// The ESDF's per-voxel rules, shared by the batch (cox_submap.hip: cox_esdf_from_tsdf) and the incremental integrator
// (cox_esdf.hip): both must apply the same code for their results to agree bit for bit.  DESIGN.md sections 3 and 7l.
#pragma once
#include "cox_device.hpp"

namespace cox {

constexpr int kEsdfHalo = 18;                                     // a block and one voxel around it
constexpr int kEsdfHaloCells = kEsdfHalo * kEsdfHalo * kEsdfHalo;  // 5832
constexpr u32 kEsdfFixedFlag = 1u;                                // colour word of a fixed voxel

// What a TSDF voxel (distance d, weight w) is before any propagation: unobserved -> (0, 0, 0); inside the fixed band ->
// (d, 1, fixed); otherwise (+-default_distance by d > 0, 1, 0).  A NaN weight is observed, a NaN distance negative and free.
__device__ __forceinline__ void esdf_init_voxel(float d, float w, float min_weight, float min_distance, float default_distance, float* ed, float* ew,
                                                u32* flags) {
  *ed = 0.0f;
  *ew = 0.0f;
  *flags = 0;
  if (!(w < min_weight)) {  // observed
    *ew = 1.0f;
    if (fabsf(d) < min_distance) {
      *ed = d;
      *flags = kEsdfFixedFlag;
    } else {
      *ed = (d > 0.0f) ? default_distance : -default_distance;
    }
  }
}

// where a free voxel holding `mine` started: its sign never changes while it is free
__device__ __forceinline__ float esdf_free_init(float mine, float default_distance) { return (mine > 0.0f) ? default_distance : -default_distance; }

// what an observed source holding dn offers a neighbour `step` away (the caller has checked |dn| < max_distance)
__device__ __forceinline__ float esdf_candidate(float dn, float step) { return (dn > 0.0f) ? dn + step : dn - step; }

// Every source of tile cell c (an 18^3 tile of distances and state bytes, bit 0 = observed): f(dn, step) for each of the 26
// neighbours that is observed and holds |dn| < max_distance -- a voxel at or beyond the maximum does not propagate.
template <typename F>
__device__ __forceinline__ void esdf_for_each_source(const float* dist, const unsigned char* st, int c, float s1, float s2, float s3, float max_distance, F&& f) {
#pragma unroll
  for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int m = (dx != 0) + (dy != 0) + (dz != 0);
        if (m == 0) continue;
        const int n = c + dx + kEsdfHalo * (dy + kEsdfHalo * dz);
        if (!(st[n] & 1)) continue;
        const float dn = dist[n];
        if (!(fabsf(dn) < max_distance)) continue;
        f(dn, (m == 1) ? s1 : (m == 2) ? s2 : s3);
      }
}

// One relaxation of the free voxel at c holding `mine`: what it holds afterwards (`mine` when no source improves it).  A positive
// source can only lower a positive voxel, a non-positive source only raise a negative one; the two never both apply.
__device__ __forceinline__ float esdf_relax_voxel(const float* dist, const unsigned char* st, int c, float mine, float s1, float s2, float s3, float max_distance) {
  float best = mine;
  esdf_for_each_source(dist, st, c, s1, s2, s3, max_distance, [&](float dn, float step) {
    const float cand = esdf_candidate(dn, step);
    if (dn > 0.0f) {
      if (best > cand) best = cand;
    } else {
      if (best < cand) best = cand;
    }
  });
  return (best != mine && ((mine > 0.0f) == (best > 0.0f))) ? best : mine;
}

// whether some source offers the free voxel at c exactly the value it holds
__device__ __forceinline__ bool esdf_supported(const float* dist, const unsigned char* st, int c, float mine, float s1, float s2, float s3, float max_distance) {
  bool supported = false;
  esdf_for_each_source(dist, st, c, s1, s2, s3, max_distance, [&](float dn, float step) {
    if (esdf_candidate(dn, step) == mine) supported = true;
  });
  return supported;
}

}  // namespace cox
