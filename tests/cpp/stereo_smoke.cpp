// DenseStereo of coxgraph_amd/host/coxgraph_hip_stereo.hpp:
//   host  -> StereoRectification::fromCalibration gives the maps of cox_stereo_rectify_maps, bit for bit; an ideal pair gives identity maps
//   GPU   -> a noise pattern shifted by 8 px comes back as disparity 128 (1/16 px) within half a pixel, with depth f B 16 / d16;
//            raw pairs through the maps of an ideal calibration give the same frame
// Exit code 0 = all good; 77 = the host part passed and there is no GPU (the constructor fails with COX_ERR_NO_DEVICE, nothing falls back).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../coxgraph_amd/host/coxgraph_hip_stereo.hpp"

using namespace coxgraph_hip;

int main() {
  // the EuRoC camchain, at a quarter of its size
  cox_stereo_calibration cal;
  std::memset(&cal, 0, sizeof(cal));
  const double k0[4] = {458.654, 457.296, 367.215, 248.375}, d0[4] = {-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05};
  const double k1[4] = {457.587, 456.134, 379.999, 255.238}, d1[4] = {-0.28368365, 0.07451284, -0.00010473, -3.55590700e-05};
  const double T[16] = {0.9999972565,  0.0023120672,  0.0003760081, -0.1100738081, -0.0023171357, 0.9998980485, 0.0140898358, 0.0003991215,
                        -0.0003433931, -0.0140906685, 0.9999006626, -0.0008537025, 0.0,           0.0,          0.0,          1.0};
  for (int i = 0; i < 4; ++i) {
    cal.cam[0].intrinsics[i] = k0[i], cal.cam[0].distortion_coeffs[i] = d0[i];
    cal.cam[1].intrinsics[i] = k1[i], cal.cam[1].distortion_coeffs[i] = d1[i];
  }
  for (int i = 0; i < 16; ++i) cal.T_cn_cnm1[i] = T[i];
  const int w = 188, h = 120;
  const StereoRectification rect = StereoRectification::fromCalibration(cal, w, h, 0.25);
  std::vector<float> m0(2 * static_cast<size_t>(w) * h), m1(m0.size());
  float K[4], B = 0.f, Tq[7];
  if (cox_stereo_rectify_maps(&cal, w, h, 0.25, m0.data(), m1.data(), K, &B, Tq) != COX_OK) return 2;
  if (std::memcmp(m0.data(), rect.map0.data(), m0.size() * sizeof(float)) != 0 || std::memcmp(m1.data(), rect.map1.data(), m1.size() * sizeof(float)) != 0) return 3;
  if (std::memcmp(K, rect.K, sizeof(K)) != 0 || B != rect.baseline_m || std::fabs(B - 0.110078f) > 1e-6f || std::fabs(K[0] - 114.35444f) > 1e-3f) return 4;
  for (int k = 0; k < 4; ++k)
    if (Tq[k] != rect.T_c0_rect.q[k]) return 5;
  if (!(Tq[0] > 0.9999f) || rect.T_c0_rect.t[0] != 0.f) return 5;
  Transformation T_G_C0;  // a quarter turn about z, somewhere
  T_G_C0.q[0] = T_G_C0.q[3] = std::sqrt(0.5f), T_G_C0.q[1] = T_G_C0.q[2] = 0.f, T_G_C0.t[0] = 1.f, T_G_C0.t[1] = 2.f, T_G_C0.t[2] = 3.f;
  const Transformation T_G_rect = rect.cameraPose(T_G_C0), same = rect.cameraPose(Transformation());
  float norm2 = 0.f;
  for (int k = 0; k < 4; ++k) {
    if (same.q[k] != rect.T_c0_rect.q[k]) return 8;
    norm2 += T_G_rect.q[k] * T_G_rect.q[k];
  }
  if (std::fabs(norm2 - 1.f) > 1e-6f || T_G_rect.t[1] != 2.f || std::fabs(T_G_rect.q[0] - std::sqrt(0.5f) * (Tq[0] - Tq[3])) > 1e-6f) return 8;
  cal.cam[1].distortion_model = 1;  // equidistant
  try {
    StereoRectification::fromCalibration(cal, w, h);
    return 6;
  } catch (const std::runtime_error&) {
  }
  cal.cam[1].distortion_model = 0;

  // already rectified pairs: a pattern and the same pattern 8 px to the left
  const int sw = 96, sh = 40, shift = 8;
  const float Ks[4] = {120.f, 120.f, 48.f, 20.f};
  const float Bs = 0.11f;
  DenseStereo::Config cfg;
  cfg.n_disparities = 64;
  if (cfg.n_paths != 8 || cfg.p1 != 7 || cfg.p2 != 86 || cfg.uniqueness_percent != 10 || cfg.lr_max_diff != 1) return 7;
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
  StereoFrame frame;
  stereo.compute(left.data(), right.data(), &frame);
  const cox_stereo_stats st = stereo.lastStats();
  size_t n_valid = 0, n_right = 0;
  const float fB16 = static_cast<float>(static_cast<double>(Ks[0]) * static_cast<double>(Bs) * 16.0);
  for (size_t i = 0; i < frame.depth.size(); ++i) {
    if (frame.color[i].r != left[i] || frame.color[i].a != 255) return 10;
    if (frame.disparity[i] == 0xFFFF) {
      if (!std::isnan(frame.depth[i])) return 11;
      continue;
    }
    ++n_valid;
    if (frame.depth[i] != fB16 / static_cast<float>(frame.disparity[i])) return 16;
    if (std::abs(static_cast<int>(frame.disparity[i]) - 16 * shift) <= 8) ++n_right;  // within half a pixel
  }
  if (n_valid != st.n_valid_pixels || n_valid < frame.depth.size() / 2 || n_right * 100 < n_valid * 95) {
    std::printf("valid %zu (stats %llu), at the shift %zu\n", n_valid, static_cast<unsigned long long>(st.n_valid_pixels), n_right);
    return 12;
  }
  const std::vector<uint8_t> rl = stereo.download(COX_STEREO_RECT_LEFT), disp = stereo.download(COX_STEREO_DISPARITY);
  if (rl != left || std::memcmp(disp.data(), frame.disparity.data(), disp.size()) != 0) return 13;
  if (stereo.download(COX_STEREO_COST_SUM).size() != left.size() * 64 * 2) return 14;
  // raw pairs through the maps of an ideal calibration are the same frame
  cox_stereo_calibration ideal;
  std::memset(&ideal, 0, sizeof(ideal));
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 4; ++i) ideal.cam[c].intrinsics[i] = Ks[i];
  ideal.T_cn_cnm1[0] = ideal.T_cn_cnm1[5] = ideal.T_cn_cnm1[10] = ideal.T_cn_cnm1[15] = 1.0;
  ideal.T_cn_cnm1[3] = -static_cast<double>(Bs);
  DenseStereo mapped(StereoRectification::fromCalibration(ideal, sw, sh), cfg);
  StereoFrame again;
  mapped.compute(left.data(), right.data(), &again);
  if (std::memcmp(again.depth.data(), frame.depth.data(), frame.depth.size() * sizeof(float)) != 0 || again.disparity != frame.disparity) return 15;
  std::printf("stereo smoke ok: %zu of %zu pixels valid, %zu at the shift, frame %.3f ms\n", n_valid, frame.depth.size(), n_right, st.frame_ms);
  return 0;
}
