// Dense stereo in C++ (header-only, C++14) on top of include/coxgraph_hip_stereo.h: a raw 8-bit pair to the depth image the
// DepthImageIntegrator of coxgraph_hip_map.hpp fuses.  The place image_undistort's dense_stereo_node has in coxgraph's EuRoC
// launch files; the rule is this engine's own (rectification and semi-global matching).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/coxgraph_hip_stereo_filter.h"
#include "coxgraph_hip_adapters.hpp"

namespace coxgraph_hip {

// step R: what a camchain turns into, on the host (no GPU needed)
struct StereoRectification {
  int width = 0, height = 0;
  std::vector<float> map0, map1;  // 2 floats per rectified pixel: where to read cam0 / cam1
  float K[4] = {0.f, 0.f, 0.f, 0.f};  // of the rectified pair
  float baseline_m = 0.f;
  Transformation T_c0_rect;  // the rectified left camera in cam0 (a rotation)

  // T_G_C0 * T_c0_rect: the pose the depth images of this pair are fused with, from the pose of cam0
  Transformation cameraPose(const Transformation& T_G_C0) const {
    const float* a = T_G_C0.q;
    const float* b = T_c0_rect.q;
    Transformation out;
    out.q[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
    out.q[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
    out.q[2] = a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1];
    out.q[3] = a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0];
    for (int k = 0; k < 3; ++k) out.t[k] = T_G_C0.t[k];  // T_c0_rect has no translation
    return out;
  }

  static StereoRectification fromCalibration(const cox_stereo_calibration& calibration, int width, int height, double scale = 1.0) {
    StereoRectification r;
    check((width > 0 && height > 0) ? COX_OK : COX_ERR_INVALID_ARG, "StereoRectification");
    r.width = width, r.height = height;
    const size_t n = static_cast<size_t>(width) * static_cast<size_t>(height);
    r.map0.assign(2 * n, 0.f);
    r.map1.assign(2 * n, 0.f);
    float T[7];
    check(cox_stereo_rectify_maps(&calibration, width, height, scale, r.map0.data(), r.map1.data(), r.K, &r.baseline_m, T), "StereoRectification");
    for (int k = 0; k < 4; ++k) r.T_c0_rect.q[k] = T[k];
    for (int k = 0; k < 3; ++k) r.T_c0_rect.t[k] = T[4 + k];
    return r;
  }
};

// what one pair gives, on the host
struct StereoFrame {
  int width = 0, height = 0;
  std::vector<float> depth;         // z-depth in metres, NaN where there is nothing
  std::vector<Color> color;         // the rectified left image as grey
  std::vector<uint16_t> disparity;  // 1/16 px, 0xFFFF where invalid
};

class DenseStereo {
 public:
  struct Config : cox_stereo_config {
    Config() { cox_stereo_config_default(this); }
  };
  struct FilterConfig : cox_stereo_filter_config {
    FilterConfig() { cox_stereo_filter_config_default(this); }
  };

  // raw pairs, rectified with r's maps
  DenseStereo(const StereoRectification& r, const Config& config = Config(), int device = 0) : config_(config), width_(r.width), height_(r.height) {
    for (int k = 0; k < 4; ++k) K_[k] = r.K[k];
    check(cox_stereo_create(device, width_, height_, &config_, r.map0.data(), r.map1.data(), K_, r.baseline_m, &h_), "DenseStereo");
  }
  // pairs that are rectified already
  DenseStereo(int width, int height, const float K_rect[4], float baseline_m, const Config& config = Config(), int device = 0)
      : config_(config), width_(width), height_(height) {
    for (int k = 0; k < 4; ++k) K_[k] = K_rect[k];
    check(cox_stereo_create(device, width_, height_, &config_, nullptr, nullptr, K_, baseline_m, &h_), "DenseStereo");
  }
  ~DenseStereo() { cox_stereo_destroy(h_); }
  DenseStereo(const DenseStereo&) = delete;
  DenseStereo& operator=(const DenseStereo&) = delete;

  const Config& config() const { return config_; }
  const float* K() const { return K_; }
  int width() const { return width_; }
  int height() const { return height_; }
  cox_stereo_t* handle() const { return h_; }
  void* stream() const { return cox_stereo_stream(h_); }

  // one pair of 8-bit images, width * height each; waits for the result
  void compute(const uint8_t* left, const uint8_t* right, StereoFrame* out) {
    const size_t n = static_cast<size_t>(width_) * static_cast<size_t>(height_);
    out->width = width_, out->height = height_;
    out->depth.resize(n);
    out->color.resize(n);
    out->disparity.resize(n);
    check(cox_stereo_compute(h_, left, right, out->depth.data(), reinterpret_cast<uint8_t*>(out->color.data()), out->disparity.data()), "DenseStereo::compute");
    sync();
  }
  // device images on the matcher's GPU, ordered behind producer_stream (a hipStream_t; NULL: the null stream); the outputs are
  // complete after sync(), or in stream order behind stream()
  void computeDev(const uint8_t* left_dev, const uint8_t* right_dev, float* depth_dev, uint8_t* rgba_dev = nullptr, uint16_t* disparity_dev = nullptr,
                  void* producer_stream = nullptr) {
    check(cox_stereo_compute_dev(h_, left_dev, right_dev, depth_dev, rgba_dev, disparity_dev, producer_stream), "DenseStereo::computeDev");
  }
  void sync() { check(cox_stereo_sync(h_), "DenseStereo::sync"); }
  cox_stereo_stats lastStats() {
    cox_stereo_stats st;
    check(cox_stereo_last_stats(h_, &st), "DenseStereo::lastStats");
    return st;
  }
  // the median and the speckle filter on the disparity (steps 7a and 7b); both are off at first, and a setting holds from the next frame
  void setFilters(const FilterConfig& filters) { check(cox_stereo_set_filters(h_, &filters), "DenseStereo::setFilters"); }
  FilterConfig filters() const {
    FilterConfig f;
    check(cox_stereo_get_filters(h_, &f), "DenseStereo::filters");
    return f;
  }
  // of the last frame; zeros when it ran unfiltered
  cox_stereo_filter_stats filterStats() {
    cox_stereo_filter_stats st;
    check(cox_stereo_filter_last_stats(h_, &st), "DenseStereo::filterStats");
    return st;
  }
  // an intermediate of the last frame (a cox_stereo_buffer), as bytes
  std::vector<uint8_t> download(int which) {
    const size_t n = static_cast<size_t>(width_) * static_cast<size_t>(height_);
    const size_t bytes = which == COX_STEREO_COST_SUM ? 2 * n * static_cast<size_t>(config_.n_disparities) : (which == COX_STEREO_DISPARITY ? 2 * n : n);
    std::vector<uint8_t> out(bytes);
    check(cox_stereo_download(h_, which, out.data(), out.size()), "DenseStereo::download");
    return out;
  }

 private:
  Config config_;
  int width_, height_;
  float K_[4];
  cox_stereo_t* h_ = nullptr;
};

}  // namespace coxgraph_hip
