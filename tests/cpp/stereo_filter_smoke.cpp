// The disparity filters of DenseStereo (coxgraph_amd/host/coxgraph_hip_stereo.hpp):
//   host  -> FilterConfig is default-constructed through the C entry: both filters off, a range of 16
//   GPU   -> a pattern shifted by 8 px: filters off, then on, then off again.  On: nothing is filled, the disparity of every pixel
//            left is within half a pixel of the shift, depth follows the filtered disparity, the counts add up; a window of the
//            whole image removes everything; off again is the first frame bit for bit and the filter counts are zero
// Exit code 0 = all good; 77 = the host part passed and there is no GPU.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_stereo.hpp"

using namespace coxgraph_hip;

int main() {
  const DenseStereo::FilterConfig off;
  if (off.median_size != 0 || off.speckle_window != 0 || off.speckle_range16 != 16 || off.reserved != 0) return 2;
  if (sizeof(cox_stereo_filter_config) != 16 || sizeof(cox_stereo_filter_stats) != 48) return 3;
  const int sw = 96, sh = 40, shift = 8;
  const float Ks[4] = {120.f, 120.f, 48.f, 20.f};
  const float Bs = 0.11f;
  DenseStereo::Config cfg;
  cfg.n_disparities = 64;
  if (cox_device_count() == 0) {
    try {
      DenseStereo none(sw, sh, Ks, Bs, cfg);
    } catch (const std::runtime_error& e) {
      std::printf("host part ok; no GPU: %s\n", e.what());
      return 77;
    }
    return 1;
  }
  std::vector<uint8_t> left(static_cast<size_t>(sw) * sh), right(left.size());
  uint32_t s = 12345u;
  for (uint8_t& v : left) s = s * 1664525u + 1013904223u, v = static_cast<uint8_t>(s >> 24);
  for (uint8_t& v : right) s = s * 1664525u + 1013904223u, v = static_cast<uint8_t>(s >> 24);
  for (int y = 0; y < sh; ++y)
    for (int x = shift; x < sw; ++x) right[static_cast<size_t>(y) * sw + x - shift] = left[static_cast<size_t>(y) * sw + x];
  DenseStereo stereo(sw, sh, Ks, Bs, cfg);
  const DenseStereo::FilterConfig at_first = stereo.filters();
  if (at_first.median_size != 0 || at_first.speckle_window != 0 || at_first.speckle_range16 != 16) return 4;
  StereoFrame plain, filtered, none, again;
  stereo.compute(left.data(), right.data(), &plain);
  cox_stereo_filter_stats fs = stereo.filterStats();
  if (fs.n_median_changed || fs.n_components || fs.n_speckle_components || fs.n_speckle_pixels || fs.median_ms != 0.0 || fs.speckle_ms != 0.0) return 5;

  DenseStereo::FilterConfig on;
  on.median_size = 3, on.speckle_window = 20;
  stereo.setFilters(on);
  const DenseStereo::FilterConfig now = stereo.filters();
  if (now.median_size != 3 || now.speckle_window != 20 || now.speckle_range16 != 16) return 6;
  stereo.compute(left.data(), right.data(), &filtered);
  fs = stereo.filterStats();
  const cox_stereo_stats st = stereo.lastStats();
  const cox_stereo_filter_stats on_stats = fs;
  const float fB16 = static_cast<float>(static_cast<double>(Ks[0]) * static_cast<double>(Bs) * 16.0);
  size_t n_valid = 0, n_valid_plain = 0, n_right = 0;
  for (size_t i = 0; i < filtered.depth.size(); ++i) {
    n_valid_plain += plain.disparity[i] != 0xFFFF;
    if (filtered.color[i].r != left[i] || filtered.color[i].a != 255) return 10;
    if (filtered.disparity[i] == 0xFFFF) {
      if (!std::isnan(filtered.depth[i])) return 11;
      continue;
    }
    if (plain.disparity[i] == 0xFFFF) return 12;  // nothing is filled
    ++n_valid;
    if (filtered.depth[i] != fB16 / static_cast<float>(filtered.disparity[i])) return 13;
    if (std::abs(static_cast<int>(filtered.disparity[i]) - 16 * shift) <= 8) ++n_right;
  }
  if (n_valid != st.n_valid_pixels || n_valid + fs.n_speckle_pixels != n_valid_plain || fs.n_components < 1 ||
      fs.n_speckle_components > fs.n_components || fs.n_speckle_pixels > 20 * fs.n_speckle_components || n_valid < filtered.depth.size() / 2 ||
      n_right * 100 < n_valid * 95) {
    std::printf("valid %zu (stats %llu, unfiltered %zu), at the shift %zu, speckle pixels %llu\n", n_valid, static_cast<unsigned long long>(st.n_valid_pixels),
                n_valid_plain, n_right, static_cast<unsigned long long>(fs.n_speckle_pixels));
    return 14;
  }
  const std::vector<uint8_t> disp = stereo.download(COX_STEREO_DISPARITY);
  if (std::memcmp(disp.data(), filtered.disparity.data(), disp.size()) != 0) return 15;

  on.median_size = 0, on.speckle_window = sw * sh;  // every component is small enough
  stereo.setFilters(on);
  stereo.compute(left.data(), right.data(), &none);
  for (size_t i = 0; i < none.depth.size(); ++i)
    if (none.disparity[i] != 0xFFFF || !std::isnan(none.depth[i])) return 16;
  if (stereo.lastStats().n_valid_pixels != 0 || stereo.filterStats().n_speckle_pixels != n_valid_plain) return 17;

  on.median_size = 5;  // refused, and the handle keeps its setting
  try {
    stereo.setFilters(on);
    return 18;
  } catch (const std::runtime_error&) {
  }
  if (stereo.filters().median_size != 0 || stereo.filters().speckle_window != sw * sh) return 19;

  stereo.setFilters(off);
  stereo.compute(left.data(), right.data(), &again);
  if (std::memcmp(again.depth.data(), plain.depth.data(), plain.depth.size() * sizeof(float)) != 0 || again.disparity != plain.disparity) return 20;
  fs = stereo.filterStats();
  if (fs.n_median_changed || fs.n_components || fs.n_speckle_pixels) return 21;
  std::printf("stereo filter smoke ok: %zu of %zu valid pixels left, %llu components, %llu speckles\n", n_valid, n_valid_plain,
              static_cast<unsigned long long>(on_stats.n_components), static_cast<unsigned long long>(on_stats.n_speckle_components));
  return 0;
}
