// sum_p x_p x_p^T in float64 for 16-component rows x, one point per lane: the normal equations of the registration cost
// (cox_reg.hip) and of the scan-to-map tracker (cox_track.hip), and the only MFMA use in the engine.
//
// A workgroup is 4 waves of 64 lanes.  Each wave accumulates its points' outer products with v_mfma_f64_16x16x4_f64
// (normal_eq_wave_step, once per pass over the points); normal_eq_finish sums the four waves' tiles into partials[bx], and the
// workgroup that draws the last ticket sums the partials of all workgroups in workgroup order.  No float atomics: the same
// bits every run, and no second launch (a one-workgroup reduction kernel took longer than the kernel it followed).
//
// The caller declares the LDS:  __shared__ double X[kNeqWaves][16][kNeqRow];  __shared__ double tile[kNeqWaves][kNeqTile];
#pragma once
#include "cox_device.hpp"

namespace cox {

constexpr int kNeqThreads = 256;
constexpr int kNeqWaves = kNeqThreads / 64;
constexpr int kNeqTile = 256;  // one 16x16 f64 tile per workgroup
constexpr int kNeqRow = 68;    // 64 points, rows padded to 68: conflict-free writes, 2-way reads

typedef double double4_t __attribute__((ext_vector_type(4)));

// acc += sum over this wave's 64 points of x x^T.  X[wave]: 16 components x 64 points.
__device__ __forceinline__ void normal_eq_wave_step(double (&X)[kNeqWaves][16][kNeqRow], const double (&x)[16], double4_t& acc) {
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 16; ++k) X[wave][k][lane] = x[k];
  __builtin_amdgcn_wave_barrier();
  // 16 MFMA steps of K = 4 points each.
  // f64 16x16x4 operand map: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15].
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const double a = X[wave][lane & 15u][4 * t + (lane >> 4)];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, a, acc, 0, 0, 0);
  }
  __builtin_amdgcn_wave_barrier();
}

// Writes this workgroup's tile to partials[bx] (bx of nb: its place among the workgroups that share partials and ticket).
// True in the workgroup that finishes last, with *total = element threadIdx.x of the 16 x 16 sum (row-major) over all nb
// workgroups; the ticket is zero again for the next launch on the stream.
__device__ __forceinline__ bool normal_eq_finish(double (&tile)[kNeqWaves][kNeqTile], const double4_t& acc, double* partials /*[nb][256]*/, u32* ticket, u32 bx,
                                                 u32 nb, double* total) {
  const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // f64 C/D map: col = lane & 15, row = (lane >> 4) + 4 * reg
#pragma unroll
  for (int r = 0; r < 4; ++r) tile[wave][((lane >> 4) + 4 * r) * 16 + (lane & 15u)] = acc[r];
  __syncthreads();
  partials[static_cast<size_t>(bx) * kNeqTile + threadIdx.x] =
      ((tile[0][threadIdx.x] + tile[1][threadIdx.x]) + tile[2][threadIdx.x]) + tile[3][threadIdx.x];
  __shared__ u32 last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) {
    const u32 t = atomicAdd(ticket, 1u);
    last = (t == nb - 1u) ? 1u : 0u;
    if (last) *ticket = 0u;  // ready for the next launch on this stream
  }
  __syncthreads();
  if (!last) return false;
  __threadfence();
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;  // four independent chains; the order of the additions stays fixed
  u32 bq = 0;
  for (; bq + 4 <= nb; bq += 4) {
    s0 += __builtin_nontemporal_load(&partials[static_cast<size_t>(bq) * kNeqTile + threadIdx.x]);
    s1 += __builtin_nontemporal_load(&partials[static_cast<size_t>(bq + 1) * kNeqTile + threadIdx.x]);
    s2 += __builtin_nontemporal_load(&partials[static_cast<size_t>(bq + 2) * kNeqTile + threadIdx.x]);
    s3 += __builtin_nontemporal_load(&partials[static_cast<size_t>(bq + 3) * kNeqTile + threadIdx.x]);
  }
  for (; bq < nb; ++bq) s0 += __builtin_nontemporal_load(&partials[static_cast<size_t>(bq) * kNeqTile + threadIdx.x]);
  *total = (s0 + s1) + (s2 + s3);
  return true;
}

}  // namespace cox
