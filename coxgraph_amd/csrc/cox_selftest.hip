// MI355X (gfx950): test-side entry points into the device-wide primitives of cox_sort.hpp -- the stable LSD radix sort and the
// three-launch exclusive scan -- so that the suite can hold them to their contracts directly and not only through whole frames
// (tests/test_gpu_sort_scan.py, reference tests/sort_ref.py).  Nothing here is on a product path.  The
// kernels of cox_sort.hpp are static or templates, so this second translation unit gets its own copies; the one-workgroup scans
// of cox_frontend.hpp are neither, and their entry (cox_selftest_scan_small) lives in cox_integrator.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/coxgraph_hip_selftest.h"
#include "cox_host.hpp"
#include "cox_sort.hpp"
#include "cox_stereo_filter.hpp"

using namespace cox;

namespace {

constexpr size_t kGuardWords = size_t{16} << kRsMaxDigitBits;  // sixteen rows of the widest digit behind the counts matrix

using DevWords = DevBuf<u32>;

int fill(u32* p, u32 value, size_t words) {
  if (words) COX_HIP(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), static_cast<int>(value), words));
  return COX_OK;
}
int upload(u32* dst, const u32* src, size_t words) {
  if (words) COX_HIP(hipMemcpy(dst, src, words * sizeof(u32), hipMemcpyHostToDevice));
  return COX_OK;
}
int download(u32* dst, const u32* src, size_t words) {
  if (words) COX_HIP(hipMemcpy(dst, src, words * sizeof(u32), hipMemcpyDeviceToHost));
  return COX_OK;
}

int select_device(int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    return COX_ERR_NO_DEVICE;
  }
  COX_HIP(hipSetDevice(device));
  return COX_OK;
}

// The hook protocol of k_rs_scatter (cox_sort.hpp, RsNoHook) without BundleBounds: every third value is wanted, what fetch reads
// and where the pair went are both recorded per value, and so is the number of commits: a hook that also ran in an earlier pass
// would have its position overwritten by the last one, but not its count.
struct SelfTestHook {
  static constexpr bool kActive = true;
  static constexpr u32 kLdsWords = 1;
  const u32* aux;
  u32* pos_out;
  u32* aux_out;
  u32* count_out;
  struct Fetched {
    u32 a, val;
  };
  __device__ __forceinline__ void begin(u32, u32*) const {}
  __device__ __forceinline__ bool wants(u32, u32 val, const u32*) const { return val % 3u == 0u; }
  __device__ __forceinline__ Fetched fetch(u32, u32 val, const u32*) const { return Fetched{aux[val], val}; }
  __device__ __forceinline__ void commit(const Fetched& f, u32 pos) const {
    pos_out[f.val] = pos;
    aux_out[f.val] = f.a;
    count_out[f.val] += 1u;  // one thread per pair and pass, passes in stream order: no atomic needed
  }
};

struct SortCall {
  u32 *k0, *v0, *k1, *v1, *x0, *x1;
  const u32* d_n;
  u32 n_max, n_hint;
  int host_bits;
  bool bits_on_device;
  int max_passes;
  SortWorkspace ws;
  SortInfo* info;
  bool pass0_counted;
};

template <int RB, class Hook>
int run_sort(const SortCall& c, Hook hook) {
  if (c.pass0_counted) {  // what the producer of the keys would have left: the counts and digit totals of pass 0
    const u32 nt = sort_num_tiles(c.n_hint ? c.n_hint : 1);
    const u32 grid = std::min<u32>(1024, std::max<u32>(1, nt));
    hipLaunchKernelGGL(k_rs_hist<RB>, dim3(grid), dim3(kRsThreads), 0, nullptr, c.k0, c.k1, c.d_n, c.n_max, 0, c.info,
                       c.bits_on_device ? -1 : c.host_bits, c.ws.counts, c.ws.tiles_cap, c.ws.totals);
  }
  return radix_sort_pairs<RB, Hook>(c.k0, c.v0, c.k1, c.v1, c.d_n, c.n_max, c.n_hint, c.host_bits, c.bits_on_device, c.max_passes, c.ws, c.info, nullptr,
                                    c.x0, c.x1, c.pass0_counted, hook);
}

}  // namespace

int cox_selftest_sort(int device, cox_selftest_sort_args* a) {
  COX_ENTRY();
  COX_TRY(select_device(device));
  if (!a || (a->rb != 11 && a->rb != 12) || a->repeat < 1 || a->nbits > 32) return COX_ERR_INVALID_ARG;
  const size_t cap = a->n_max;
  const size_t hook_words = std::max<size_t>(cap, 1);
  if (cap && (!a->keys || !a->vals || !a->k0 || !a->v0 || !a->k1 || !a->v1)) return COX_ERR_INVALID_ARG;
  if (cap && a->extra && (!a->x0 || !a->x1)) return COX_ERR_INVALID_ARG;
  if (a->hook && (!a->aux || !a->hook_pos || !a->hook_aux || !a->hook_count)) return COX_ERR_INVALID_ARG;
  if (a->bits_on_device && (a->max_passes < 1 || a->max_passes > kRsMaxPasses || a->base > 32 || a->base + a->nbits > 32)) return COX_ERR_INVALID_ARG;
  for (int r = 0; a->repeat_nbits && r < a->repeat; ++r)
    if (a->repeat_nbits[r] > 32 || (a->bits_on_device && a->base + a->repeat_nbits[r] > 32)) return COX_ERR_INVALID_ARG;
  const u32 n = a->use_d_n ? std::min(a->d_n, a->n_max) : a->n_max;
  const bool has_x = a->extra != nullptr;

  DevWords k0, v0, k1, v1, x0, x1, dn, info, counts, totals, aux, hpos, haux, hcount;
  for (DevWords* b : {&k0, &v0, &k1, &v1}) COX_TRY(b->alloc(cap));
  if (has_x) {
    COX_TRY(x0.alloc(cap));
    COX_TRY(x1.alloc(cap));
  }
  COX_TRY(dn.alloc(1));
  COX_TRY(info.alloc(sizeof(SortInfo) / sizeof(u32)));
  SortCall c{};
  c.ws.tiles_cap = std::min<u32>(kRsMaxTiles, std::max<u32>(1, sort_num_tiles(a->n_max)));  // beyond kRsMaxTiles tiles the tile doubles
  const size_t counts_words = sort_counts_words(c.ws.tiles_cap);
  COX_TRY(counts.alloc(counts_words + kGuardWords));  // the workspace proper, then the guard
  COX_TRY(fill(counts.p + counts_words, a->sentinel, kGuardWords));
  COX_TRY(totals.alloc(sort_totals_words()));
  COX_HIP(hipMemset(totals.p, 0, sizeof(u32) * sort_totals_words()));  // once: every sort leaves it zero again
  c.ws.counts = counts.p;
  c.ws.totals = totals.p;
  if (a->hook) {
    COX_TRY(aux.alloc(hook_words));
    COX_TRY(hpos.alloc(hook_words));
    COX_TRY(haux.alloc(hook_words));
    COX_TRY(hcount.alloc(hook_words));
    COX_TRY(upload(aux.p, a->aux, hook_words));
  }
  COX_TRY(upload(dn.p, &a->d_n, 1));
  c.k0 = k0.p, c.v0 = v0.p, c.k1 = k1.p, c.v1 = v1.p;
  c.x0 = has_x ? x0.p : nullptr, c.x1 = has_x ? x1.p : nullptr;
  c.d_n = a->use_d_n ? dn.p : nullptr;
  c.n_max = a->n_max, c.n_hint = a->n_hint;
  c.bits_on_device = a->bits_on_device != 0;
  c.max_passes = a->bits_on_device ? a->max_passes : 0;
  c.info = reinterpret_cast<SortInfo*>(info.p);
  c.pass0_counted = a->pass0_counted != 0;

  int returned = 0;
  for (int r = 0; r < a->repeat; ++r) {
    const u32 nbits = a->repeat_nbits ? a->repeat_nbits[r] : a->nbits;
    c.host_bits = static_cast<int>(nbits);
    const SortInfo h_info{nbits, 0u, a->bits_on_device ? a->base : 0u, 0u};
    COX_HIP(hipMemcpy(info.p, &h_info, sizeof(h_info), hipMemcpyHostToDevice));
    COX_TRY(upload(k0.p, a->keys, n));
    COX_TRY(upload(v0.p, a->vals, n));
    for (u32* b : {k0.p, v0.p}) COX_TRY(fill(b + n, a->sentinel, cap - n));
    for (u32* b : {k1.p, v1.p}) COX_TRY(fill(b, a->sentinel, cap));
    if (has_x) {
      COX_TRY(upload(x0.p, a->extra, n));
      COX_TRY(fill(x0.p + n, a->sentinel, cap - n));
      COX_TRY(fill(x1.p, a->sentinel, cap));
    }
    if (a->hook) {
      COX_TRY(fill(hpos.p, a->sentinel, hook_words));
      COX_TRY(fill(haux.p, a->sentinel, hook_words));
      COX_TRY(fill(hcount.p, 0u, hook_words));
    }
    COX_HIP(hipDeviceSynchronize());
    if (a->hook) {
      const SelfTestHook hook{aux.p, hpos.p, haux.p, hcount.p};
      returned = a->rb == 11 ? run_sort<11>(c, hook) : run_sort<12>(c, hook);
    } else {
      returned = a->rb == 11 ? run_sort<11>(c, RsNoHook{}) : run_sort<12>(c, RsNoHook{});
    }
    COX_HIP(hipGetLastError());
    COX_HIP(hipDeviceSynchronize());
  }

  COX_TRY(download(a->k0, k0.p, cap));
  COX_TRY(download(a->v0, v0.p, cap));
  COX_TRY(download(a->k1, k1.p, cap));
  COX_TRY(download(a->v1, v1.p, cap));
  if (has_x) {
    COX_TRY(download(a->x0, x0.p, cap));
    COX_TRY(download(a->x1, x1.p, cap));
  }
  if (a->hook) {
    COX_TRY(download(a->hook_pos, hpos.p, hook_words));
    COX_TRY(download(a->hook_aux, haux.p, hook_words));
    COX_TRY(download(a->hook_count, hcount.p, hook_words));
  }
  if (a->bits_on_device) {
    SortInfo got{};
    COX_HIP(hipMemcpy(&got, info.p, sizeof(got), hipMemcpyDeviceToHost));
    a->result_buffer = static_cast<int32_t>(got.parity);
  } else {
    a->result_buffer = returned;
  }
  std::vector<u32> h_totals(sort_totals_words());
  COX_TRY(download(h_totals.data(), totals.p, h_totals.size()));
  a->totals_nonzero = static_cast<u32>(std::count_if(h_totals.begin(), h_totals.end(), [](u32 w) { return w != 0; }));
  std::vector<u32> h_guard(kGuardWords);
  COX_TRY(download(h_guard.data(), counts.p + counts_words, h_guard.size()));
  a->guard_touched = static_cast<u32>(std::count_if(h_guard.begin(), h_guard.end(), [&](u32 w) { return w != a->sentinel; }));
  return COX_OK;
}

int cox_selftest_scan(int device, const uint32_t* in, uint32_t n_max, int use_d_n, uint32_t d_n, uint32_t n_hint, int in_place, int want_total,
                      uint32_t sentinel, uint32_t* out, uint32_t* total) {
  COX_ENTRY();
  COX_TRY(select_device(device));
  if (!total || (n_max && (!in || !out))) return COX_ERR_INVALID_ARG;
  DevWords d_in, d_out, dn, d_total, sums;
  COX_TRY(d_in.alloc(n_max));
  if (!in_place) COX_TRY(d_out.alloc(n_max));
  COX_TRY(dn.alloc(1));
  COX_TRY(d_total.alloc(1));
  COX_TRY(sums.alloc(std::max<u32>(1, scan_num_blocks(n_max))));
  COX_TRY(upload(d_in.p, in, n_max));
  if (!in_place) COX_TRY(fill(d_out.p, sentinel, n_max));
  COX_TRY(upload(dn.p, &d_n, 1));
  COX_TRY(fill(d_total.p, sentinel, 1));
  COX_HIP(hipDeviceSynchronize());
  ScanWorkspace ws;
  ws.block_sums = sums.p;
  u32* d_result = in_place ? d_in.p : d_out.p;
  exclusive_scan_u32(d_in.p, d_result, use_d_n ? dn.p : nullptr, n_max, n_hint, want_total ? d_total.p : nullptr, ws, nullptr);
  COX_HIP(hipGetLastError());
  COX_HIP(hipDeviceSynchronize());
  COX_TRY(download(out, d_result, n_max));
  COX_TRY(download(total, d_total.p, 1));
  return COX_OK;
}

// Steps 7a and 7b of dense stereo on a caller's disparity image, through the two launch functions of cox_stereo_filter.hpp that
// cox_stereo.hip uses.  One allocation of words: the input, then every output with its guard behind it, the sizes, the counters.
int cox_selftest_stereo_filters(int device, const uint16_t* disparity, int w, int h, const cox_stereo_filter_config* cfg, uint16_t* median_out,
                                uint32_t* labels_out, uint16_t* filtered_out, uint64_t counts[4], uint32_t guard_touched[3]) {
  COX_ENTRY();
  COX_TRY(select_device(device));
  if (!disparity || !median_out || !labels_out || !filtered_out || !counts || !guard_touched) return COX_ERR_INVALID_ARG;
  if (w < 1 || h < 1 || w > COX_STEREO_MAX_SIDE || h > COX_STEREO_MAX_SIDE || static_cast<u64>(w) * static_cast<u64>(h) > (1ull << 24))
    return COX_ERR_INVALID_ARG;
  cox_stereo_filter_config c{0, 0, 16, 0};
  if (cfg) c = *cfg;
  if (!cox_stf::stf_config_ok(c.median_size, c.speckle_window, c.speckle_range16, c.reserved)) return COX_ERR_INVALID_ARG;
  constexpr size_t G = 64;
  constexpr int kFill = 0xA5;
  const size_t n = static_cast<size_t>(w) * h, half = (n + 1) / 2;
  const size_t o_med = half, o_lab = o_med + half + G, o_filt = o_lab + n + G, o_size = o_filt + half + G, o_cnt = o_size + n;
  const size_t words = o_cnt + cox_stf::kCntWords;
  DevWords buf;
  COX_TRY(buf.alloc(words));
  u32* d = buf.p;
  COX_HIP(hipMemset(d, kFill, words * sizeof(u32)));
  COX_HIP(hipMemset(d + o_cnt, 0, cox_stf::kCntWords * sizeof(u32)));
  COX_HIP(hipMemcpy(d, disparity, n * sizeof(uint16_t), hipMemcpyHostToDevice));
  COX_HIP(hipDeviceSynchronize());
  const bool median = c.median_size == 3, speckle = c.speckle_window > 0;
  const uint16_t* image = reinterpret_cast<const uint16_t*>(d);
  uint16_t* d_med = reinterpret_cast<uint16_t*>(d + o_med);
  uint16_t* d_filt = reinterpret_cast<uint16_t*>(d + o_filt);
  if (median) {
    cox_stf::stf_launch_median(image, w, h, d_med, nullptr, d + o_cnt, nullptr);
    image = d_med;
  }
  if (speckle) cox_stf::stf_launch_speckle(image, w, h, c.speckle_window, c.speckle_range16, d + o_lab, d + o_size, d_filt, nullptr, d + o_cnt, nullptr);
  COX_HIP(hipGetLastError());
  COX_HIP(hipDeviceSynchronize());
  COX_HIP(hipMemcpy(median_out, image, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(labels_out, d + o_lab, n * sizeof(u32), hipMemcpyDeviceToHost));
  COX_HIP(hipMemcpy(filtered_out, speckle ? d_filt : image, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
  u32 h_counts[cox_stf::kCntWords];
  COX_TRY(download(h_counts, d + o_cnt, cox_stf::kCntWords));
  for (int k = 0; k < cox_stf::kCntWords; ++k) counts[k] = h_counts[k];
  // a guard runs from the last element of its array to the next array: the half word behind an odd image counts as guard
  const size_t first[3] = {o_med * 4 + n * 2, (o_lab + n) * 4, o_filt * 4 + n * 2}, stop[3] = {o_lab * 4, o_filt * 4, o_size * 4};
  for (int k = 0; k < 3; ++k) {
    std::vector<uint8_t> g(stop[k] - first[k]);
    COX_HIP(hipMemcpy(g.data(), reinterpret_cast<const uint8_t*>(d) + first[k], g.size(), hipMemcpyDeviceToHost));
    guard_touched[k] = static_cast<u32>(std::count_if(g.begin(), g.end(), [](uint8_t b) { return b != kFill; }));
  }
  return COX_OK;
}
