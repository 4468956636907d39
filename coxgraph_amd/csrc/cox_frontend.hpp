// Around the frame: depth image -> point list, pinned host inputs read by a kernel, the division self-test of the bundle merge, and
// the one-workgroup scans of the ray step counts -- part of cox_integrator.hip (included there, in this order: the kernels use what
// is defined above them in that file).
#pragma once

// ---- depth front end ----------------------------------------------------------------------------
// depth image -> point list in row-major pixel order (the order depth_image_proc produces), in two launches:
//   k_depth_count   valid pixels per tile of 2048
//   k_depth_points  every workgroup adds up the counts of the tiles before its own (a 640 x 480 image has 150), scans its tile and
//                   writes its points; the last tile leaves the frame's point count on the device -- it never visits the host
constexpr u32 kDepthTile = 2048;
__device__ __forceinline__ bool depth_valid(float d) { return isfinite(d) && d > 0.0f; }
__global__ void __launch_bounds__(256) k_depth_count(const float* __restrict__ depth, u32 n, u32* __restrict__ tile_sums) {
  __shared__ u32 lds[4];
  const u32 n_tiles = (n + kDepthTile - 1) / kDepthTile;
  for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    u32 c = 0;
#pragma unroll
    for (u32 q = 0; q < kDepthTile / 256; ++q) {
      const u32 i = tile * kDepthTile + q * 256 + threadIdx.x;
      c += (i < n && depth_valid(depth[i])) ? 1u : 0u;
    }
    u32 tot;
    (void)block_exclusive_scan<4>(c, &tot, lds);
    if (threadIdx.x == 0) tile_sums[tile] = tot;
  }
}
__global__ void __launch_bounds__(256) k_depth_points(const float* __restrict__ depth, const uint8_t* __restrict__ rgba, int w, int h, float fx, float fy,
                                                      float cx, float cy, const u32* __restrict__ tile_sums, float* __restrict__ xyz,
                                                      uint8_t* __restrict__ rgba_out, u32* __restrict__ n_out) {
  __shared__ u32 lds[4], lds2[4];
  const u32 n = static_cast<u32>(w) * static_cast<u32>(h);
  const u32 n_tiles = (n + kDepthTile - 1) / kDepthTile;
  for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    u32 below = 0;
    for (u32 t = threadIdx.x; t < tile; t += 256) below += tile_sums[t];
    u32 base;
    (void)block_exclusive_scan<4>(below, &base, lds2);
    // thread t owns the 8 consecutive pixels [tile * 2048 + 8 t, + 8)
    const u32 i0 = tile * kDepthTile + threadIdx.x * 8;
    float d[8];
    u32 c = 0;
#pragma unroll
    for (u32 q = 0; q < 8; ++q) {
      d[q] = (i0 + q < n) ? depth[i0 + q] : 0.0f;
      c += depth_valid(d[q]) ? 1u : 0u;
    }
    u32 tot;
    u32 o = base + block_exclusive_scan<4>(c, &tot, lds);
#pragma unroll
    for (u32 q = 0; q < 8; ++q) {
      if (!depth_valid(d[q])) continue;
      const u32 i = i0 + q;
      const u32 u = i % static_cast<u32>(w), v = i / static_cast<u32>(w);
      const float xn = (static_cast<float>(u) - cx) / fx;
      const float yn = (static_cast<float>(v) - cy) / fy;
      xyz[3 * o] = d[q] * xn;
      xyz[3 * o + 1] = d[q] * yn;
      xyz[3 * o + 2] = d[q];
      if (rgba_out) reinterpret_cast<u32*>(rgba_out)[o] = rgba ? reinterpret_cast<const u32*>(rgba)[i] : 0u;
      ++o;
    }
    if (tile + 1 == n_tiles && threadIdx.x == 0) *n_out = base + tot;
  }
}

// ---- host inputs: pinned host memory read by a kernel ------------------------------------------------------------------------
// hipMemcpyAsync hands a pinned-to-device copy to the SDMA engine and pays two engine hand-overs per copy on the frame's stream;
// pinned host memory is mapped into the device's address space, so an ordinary kernel can read it instead.  The grid is SMALL on
// purpose: every lane of a copy kernel sits on a PCIe read (microseconds), and a chip-filling grid of them holds the vector-memory
// queues of every CU — kernels of neighbouring frames ran 5-8 x longer beside it (k_rs_scatter 14 -> 117 us, k_bundle_count 10 ->
// 86 us in the kernel trace).  kCopyGroups workgroups with four 16-B loads in flight per lane (COX_H2D_GROUPS x 256 x 64 B) cover
// the link's bandwidth-delay product (~55 GB/s x ~2 us) and leave the other CUs alone.  Two segments (points, colours) per launch.
typedef u32 U32x4 __attribute__((ext_vector_type(4)));
constexpr int kCopyGroups = 8;
struct HostSegment {
  U32x4* dst;
  const U32x4* src;
  size_t n16;
  u32 tail_words;  // 4-byte words behind the last whole 16 bytes
};
__device__ __forceinline__ void copy_segment_from_host(const HostSegment& g) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  for (; i + 3 * stride < g.n16; i += 4 * stride) {
    const U32x4 a = __builtin_nontemporal_load(&g.src[i]);
    const U32x4 b = __builtin_nontemporal_load(&g.src[i + stride]);
    const U32x4 c = __builtin_nontemporal_load(&g.src[i + 2 * stride]);
    const U32x4 d = __builtin_nontemporal_load(&g.src[i + 3 * stride]);
    g.dst[i] = a;
    g.dst[i + stride] = b;
    g.dst[i + 2 * stride] = c;
    g.dst[i + 3 * stride] = d;
  }
  for (; i < g.n16; i += stride) g.dst[i] = __builtin_nontemporal_load(&g.src[i]);
  if (blockIdx.x == 0 && threadIdx.x < g.tail_words)
    reinterpret_cast<u32*>(g.dst + g.n16)[threadIdx.x] = reinterpret_cast<const u32*>(g.src + g.n16)[threadIdx.x];
}
__global__ void __launch_bounds__(256) k_copy_from_host(const HostSegment a, const HostSegment b) {
  copy_segment_from_host(a);
  if (b.dst) copy_segment_from_host(b);
}

// ---- self-test: the hoisted-reciprocal division of k_bundle_merge against the compiler's IEEE '/' -----------------
__global__ void __launch_bounds__(256) k_selftest_division(u64 n, u64 seed, u32* __restrict__ mismatches) {
  u64 bad = 0;
  for (u64 i = blockIdx.x * static_cast<u64>(blockDim.x) + threadIdx.x; i < n; i += static_cast<u64>(gridDim.x) * blockDim.x) {
    // splitmix64 -> two floats: divisor like the merge's (small integers and arbitrary values in 2^-40..2^40), arbitrary numerator
    u64 z = seed + 0x9E3779B97F4A7C15ull * (i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const u32 a = static_cast<u32>(z), b = static_cast<u32>(z >> 32);
    float D, N;
    if ((i & 3) == 0) {
      D = static_cast<float>((b % 200000u) + 1u);  // W + w with unit weights
    } else {
      D = __uint_as_float(((b & 0x007FFFFFu) | (((b >> 23) % 80u + 87u) << 23)));  // exponent -40..39
    }
    N = __uint_as_float((a & 0x807FFFFFu) | ((((a >> 23) & 0xFFu) % 80u + 87u) << 23));
    const float r0 = __builtin_amdgcn_rcpf(D);
    const float r = __builtin_fmaf(__builtin_fmaf(-D, r0, 1.0f), r0, r0);
    const float q0 = N * r;
    const float e0 = __builtin_fmaf(-D, q0, N);
    const float q1 = __builtin_fmaf(e0, r, q0);
    const float e1 = __builtin_fmaf(-D, q1, N);
    const float q = __builtin_fmaf(e1, r, q1);
    const float ref = N / D;
    if (__float_as_uint(q) != __float_as_uint(ref)) ++bad;
  }
  if (bad) atomicAdd(mismatches, static_cast<u32>(bad > 0xFFFFFFFFull ? 0xFFFFFFFFull : bad));
}

// exclusive scan of at most a few thousand ray step counts in ONE launch (the three-launch scan is latency-bound there)
__global__ void __launch_bounds__(1024) k_scan_small(const u32* __restrict__ in, u32* __restrict__ out, const u32* __restrict__ d_n, u32 n_max,
                                                     u32* __restrict__ d_total) {
  __shared__ u32 lds[16];
  const u32 n = min(*d_n, n_max);
  u32 carry = 0;
  for (u32 base = 0; base < n; base += 1024 * 4) {
    const u32 i0 = base + threadIdx.x * 4;
    u32 v[4], sum = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      v[q] = (i0 + q < n) ? in[i0 + q] : 0u;
      sum += v[q];
    }
    u32 total;
    u32 ex = carry + block_exclusive_scan<16>(sum, &total, lds);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (i0 + q < n) out[i0 + q] = ex;
      ex += v[q];
    }
    carry += total;
  }
  if (threadIdx.x == 0) *d_total = carry;
}

// piece path: the step counts and the piece bounds of the rays, both scanned in one launch
__global__ void __launch_bounds__(1024) k_scan_small2(const u32* __restrict__ in_a, u32* __restrict__ out_a, u32* __restrict__ total_a, const u32* __restrict__ in_b,
                                                      u32* __restrict__ out_b, u32* __restrict__ total_b, const u32* __restrict__ d_n, u32 n_max) {
  __shared__ u32 lds[16];
  const u32 n = min(*d_n, n_max);
  for (int which = 0; which < 2; ++which) {
    const u32* __restrict__ in = which ? in_b : in_a;
    u32* __restrict__ out = which ? out_b : out_a;
    u32 carry = 0;
    for (u32 base = 0; base < n; base += 1024 * 4) {
      const u32 i0 = base + threadIdx.x * 4;
      u32 v[4], sum = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        v[q] = (i0 + q < n) ? in[i0 + q] : 0u;
        sum += v[q];
      }
      u32 total;
      u32 ex = carry + block_exclusive_scan<16>(sum, &total, lds);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (i0 + q < n) out[i0 + q] = ex;
        ex += v[q];
      }
      carry += total;
    }
    if (threadIdx.x == 0) *(which ? total_b : total_a) = carry;
  }
}
