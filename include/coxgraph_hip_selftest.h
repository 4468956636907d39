/* Self-test entry points into the device-wide primitives of libcoxgraph_hip.so: the stable LSD radix sort and the three-launch
 * exclusive scan (coxgraph_amd/csrc/cox_sort.hpp), and the two one-workgroup scans of the ray-generation chain
 * (coxgraph_amd/csrc/cox_frontend.hpp); the input side of a frame, also of cox_frontend.hpp: the depth front end (k_depth_count,
 * k_depth_points) and the kernel that reads pinned host inputs (k_copy_from_host); the depth integrator's candidate
 * box; and, last, the two filters on the disparity of dense stereo (coxgraph_amd/csrc/cox_stereo_filter.hpp).  Only the test suite
 * calls them (tests/test_gpu_sort_scan.py, tests/test_gpu_frontend.py, tests/test_depthfuse_abi_cpu.py, tests/test_gpu_depthfuse.py,
 * tests/test_gpu_stereo_filter.py); no product path does.  The two input-side entries follow the rules below as well: host arrays in
 * and out, the null stream, COX_ERR_NO_DEVICE checked first, then COX_ERR_INVALID_ARG (a missing array, an empty image, a size
 * above 2^24, a grid above 65535, groups outside 1..1024).
 *
 * Kept apart from coxgraph_hip.h on purpose: these symbols have no counterpart in the CPU checker.  Every sort or scan entry takes host arrays,
 * allocates what it needs on `device`, runs the primitive on the null stream exactly as the engine's call sites do, copies back
 * and frees.  COX_OK or a negative cox_status; no usable GPU -> COX_ERR_NO_DEVICE, checked first; then COX_ERR_INVALID_ARG.
 * The entries stay inside the primitives' contracts: a call that would break one (base + nbits above 32, a digit width other
 * than 11 or 12, a missing array) is refused with COX_ERR_INVALID_ARG before anything is launched. */
#ifndef COXGRAPH_HIP_SELFTEST_H_
#define COXGRAPH_HIP_SELFTEST_H_
#include "coxgraph_hip.h"
#include "coxgraph_hip_depthfuse.h"
#include "coxgraph_hip_stereo_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One radix_sort_pairs<rb> call (or `repeat` of them on one workspace).  n = min(d_n, n_max) when use_d_n, else n_max.
 * Before every sort buffer 0 holds the first n input pairs and `sentinel` in [n, n_max), buffer 1 holds `sentinel` throughout,
 * hook_pos and hook_aux hold `sentinel` and hook_count holds 0; what is returned is the state after the last sort.  The workspace
 * is sized as the engine's callers size it (tiles_cap = min(kRsMaxTiles, max(1, ceil(n_max / 2048)))) and its totals are zeroed
 * once.  Behind the counts matrix the entry keeps a guard of its own, filled with `sentinel`: a sort that needs more rows than
 * tiles_cap shows up in guard_touched, not in somebody else's memory. */
typedef struct cox_selftest_sort_args {
  /* ---- the sort ---- */
  int32_t rb;              /* digit width the sort is instantiated with: 11 or 12 */
  uint32_t n_max;          /* capacity of every array below */
  int32_t use_d_n;         /* 0: d_n == nullptr; 1: the count lives on the device */
  uint32_t d_n;            /* the device-side count (may exceed n_max: the kernels clamp) */
  uint32_t n_hint;         /* sizes the grids only */
  int32_t bits_on_device;  /* 0: host_bits path; 1: SortInfo{nbits, parity = 0, base} on the device, max_passes enqueued */
  uint32_t nbits;          /* key bits (host_bits on the host path) */
  uint32_t base;           /* device path only; base + nbits <= 32 */
  int32_t max_passes;      /* device path only, 1..4 */
  int32_t pass0_counted;   /* the entry runs k_rs_hist<rb> for pass 0 itself, then sorts with the flag */
  int32_t hook;            /* 1: sort with the test hook (below) */
  int32_t repeat;          /* >= 1 sorts on the same workspace, inputs restored before each */
  const uint32_t* repeat_nbits; /* NULL, or [repeat]: nbits of each repeat (overrides nbits) */
  uint32_t sentinel;
  uint32_t pad0;
  /* ---- inputs, [n_max] ---- */
  const uint32_t* keys;
  const uint32_t* vals;
  const uint32_t* extra;   /* NULL: no second value array (x0 == x1 == nullptr) */
  const uint32_t* aux;     /* hook only: [max(n_max, 1)], what fetch() reads */
  /* ---- outputs, [n_max] each; x0/x1 only with extra; hook_* only with hook, [max(n_max, 1)] each ---- */
  uint32_t* k0;
  uint32_t* v0;
  uint32_t* x0;
  uint32_t* k1;
  uint32_t* v1;
  uint32_t* x1;
  uint32_t* hook_pos;
  uint32_t* hook_aux;
  uint32_t* hook_count;    /* commits per value, over all passes of the last sort */
  int32_t result_buffer;   /* host path: what radix_sort_pairs returned; device path: info->parity afterwards */
  uint32_t totals_nonzero; /* nonzero words in the whole totals array after the last sort */
  uint32_t guard_touched;  /* words of the guard behind the counts matrix that no longer hold the sentinel */
  uint32_t pad1;
} cox_selftest_sort_args;

/* The test hook: kActive, begin() does nothing, wants(key, val) = (val % 3 == 0), fetch() reads aux[val], commit(f, pos) writes
 * hook_pos[val] = pos and hook_aux[val] = f and counts the commit in hook_count[val].  Values of wanted pairs must be below
 * max(n_max, 1). */
int cox_selftest_sort(int device, cox_selftest_sort_args* args);

/* exclusive_scan_u32 over in[0, n), n as above.  out [n_max]: pre-filled with `sentinel`, or with the input when in_place (then
 * the scan runs with out == in).  *total: the word d_total points at, pre-filled with `sentinel`; want_total == 0 passes
 * d_total == nullptr, so the sentinel must come back. */
int cox_selftest_scan(int device, const uint32_t* in, uint32_t n_max, int use_d_n, uint32_t d_n, uint32_t n_hint, int in_place,
                      int want_total, uint32_t sentinel, uint32_t* out, uint32_t* total);

/* k_scan_small on in_a, k_scan_small on in_b, and one k_scan_small2 on both, each over min(d_n, n_max) elements of arrays of
 * `len` words (len >= min(d_n, n_max)).  Outputs are pre-filled with `sentinel`.  totals = {small a, small b, small2 a, small2 b}. */
int cox_selftest_scan_small(int device, const uint32_t* in_a, const uint32_t* in_b, uint32_t len, uint32_t n_max, uint32_t d_n,
                            uint32_t sentinel, uint32_t* out1_a, uint32_t* out1_b, uint32_t* out2_a, uint32_t* out2_b,
                            uint32_t totals[4]);

/* The depth front end: k_depth_count, then k_depth_points, on the w x h image `depth` (row-major; rgba NULL: no colour image), launched
 * by the code the integrator launches them with.  grid 0: the engine's grid, one workgroup per tile of 2048 pixels; any other grid
 * (up to 65535) makes both kernels stride over the tiles.  xyz_out [3 w h], rgba_out [w h] words, tile_sums_out
 * [max(1, ceil(w h / 2048))] and *n_out are pre-filled with `sentinel`; want_rgba == 0 hands the kernel no colour output, so rgba_out
 * comes back as sentinels.  Every output array has a guard of 64 sentinel words behind it: guard_touched = the words of each that
 * changed, in the order xyz, rgba, tile_sums.  w h is at most 2^24. */
int cox_selftest_depth_points(int device, const float* depth, const uint8_t* rgba, int w, int h, const float K[4], uint32_t grid, int want_rgba,
                              uint32_t sentinel, float* xyz_out, uint8_t* rgba_out, uint32_t* tile_sums_out, uint32_t* n_out,
                              uint32_t guard_touched[3]);

/* k_copy_from_host with `groups` workgroups (1..1024) on a [words_a] and b [words_b] (b NULL with words_b == 0: no second segment),
 * both copied to pinned host memory first; the segments are built by the code the integrator builds them with.  The destinations
 * are pre-filled with `sentinel` and come back in out_a [words_a], out_b [words_b]; guard_touched = the words that changed among the
 * 64 behind each destination (the guard of b is there without b, too).  words_a, words_b at most 2^24. */
int cox_selftest_copy_from_host(int device, const uint32_t* a, uint64_t words_a, const uint32_t* b, uint64_t words_b, int groups, uint32_t sentinel,
                                uint32_t* out_a, uint32_t* out_b, uint32_t guard_touched[2]);

/* The box of candidate blocks a frame of the depth integrator (coxgraph_hip_depthfuse.h, cox_depthfuse.hip) would visit, computed
 * on the host: the one entry here that needs no GPU and checks for none.  lo[3] is the box's lowest block index, dims[3] its extent
 * per axis (x, y, z); candidate i is block (lo.x + i % dims.x, lo.y + (i / dims.x) % dims.y, lo.z + i / (dims.x * dims.y)).  cfg
 * NULL: the defaults.  Statuses as cox_depthfuse_create and cox_depthfuse_integrate give for the same arguments
 * (COX_ERR_INVALID_ARG, COX_ERR_INDEX_RANGE). */
int cox_selftest_depthfuse_box(float voxel_size, const cox_depthfuse_config* cfg, const float T_G_C[7], int w, int height, const float K[4],
                               int32_t lo[3], uint32_t dims[3]);

/* Steps 7a and 7b of dense stereo (coxgraph_hip_stereo_filter.h, coxgraph_amd/csrc/cox_stereo_filter.hpp) on a w x h disparity image
 * the caller supplies (u16, 1/16 px, 0xFFFF invalid), launched by the two functions the matcher launches them with, on the null
 * stream: whole frames cannot be made to produce the images that try a labelling.  cfg as cox_stereo_set_filters takes it (NULL:
 * both off).  median_out [w h]: the image after 7a (the input when the median is off); labels_out [w h]: 7b's labels; filtered_out
 * [w h]: the image after 7b; counts: n_median_changed, n_components, n_speckle_components, n_speckle_pixels.  With 7b off nothing
 * is labelled: labels_out comes back as its pre-fill, filtered_out is the image after 7a and the last three counts are 0.  The
 * outputs are pre-filled with 0xA5 bytes, with 64 guard words of the same behind each: guard_touched = the bytes of each guard that
 * changed, in the order median, labels, filtered.  COX_ERR_INVALID_ARG: a missing array, w or h outside 1 .. 2^15, w h above 2^24,
 * a configuration cox_stereo_set_filters refuses. */
int cox_selftest_stereo_filters(int device, const uint16_t* disparity, int w, int h, const cox_stereo_filter_config* cfg, uint16_t* median_out,
                                uint32_t* labels_out, uint16_t* filtered_out, uint64_t counts[4], uint32_t guard_touched[3]);

#ifdef __cplusplus
}
#endif
#endif /* COXGRAPH_HIP_SELFTEST_H_ */
