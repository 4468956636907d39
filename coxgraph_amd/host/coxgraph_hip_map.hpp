// Reading the maps back in C++ (header-only, C++14): what coxgraph's MapServer publishes and what a planner asks of it
//   MapServer::updatePastTsdf      coxgraph/src/client/map_server.cpp:61-73 (every submap merged at its pose into one TSDF)
//   MapServer::publishEsdf         map_server.cpp:94-106 (EsdfIntegrator::updateFromTsdfLayerBatch on that TSDF)
//   MapServer::publishTraversable  map_server.cpp:108-116 (createFreePointcloudFromEsdfLayer(esdf, traversability_radius))
//   voxblox::EsdfMap               getDistanceAtPosition, getDistanceAndGradientAtPosition, isObserved and the batch forms
// on top of include/coxgraph_hip_map.h.  No ROS publishing: the caller gets the layers and clouds.
#pragma once
#include <memory>
#include <vector>

#include "../../include/coxgraph_hip_depthfuse.h"
#include "../../include/coxgraph_hip_esdf.h"
#include "../../include/coxgraph_hip_map.h"
#include "../../include/coxgraph_hip_render.h"
#include "coxgraph_hip_submap.hpp"

namespace coxgraph_hip {

// voxblox::EsdfMap / TsdfMap queries over any layer handle (a TSDF, or an ESDF in TSDF wire layout).  Positions are the
// float points voxblox casts them to (position.cast<FloatingPoint>()).
class LayerQuery {
 public:
  explicit LayerQuery(cox_layer_t* layer) : layer_(layer) {}
  cox_layer_t* handle() const { return layer_; }

  // getDistanceAtPosition(position, interpolate = true, &distance)
  bool getDistanceAtPosition(const Point& position, bool interpolate, float* distance) const {
    uint8_t st = 0;
    check(cox_layer_query(layer_, position.data(), 1, interpolate ? COX_QUERY_INTERPOLATE : COX_QUERY_NEAREST, 0, distance, nullptr, nullptr, &st),
          "getDistanceAtPosition");
    return (st & COX_Q_VALUE) != 0;
  }
  bool getDistanceAtPosition(const Point& position, float* distance) const { return getDistanceAtPosition(position, true, distance); }
  // interpolate: getAdaptiveDistanceAndGradient; else the nearest distance and gradient
  bool getDistanceAndGradientAtPosition(const Point& position, bool interpolate, float* distance, Point* gradient) const {
    uint8_t st = 0;
    check(cox_layer_query(layer_, position.data(), 1, interpolate ? COX_QUERY_ADAPTIVE : COX_QUERY_NEAREST, 1, distance, nullptr, gradient->data(), &st),
          "getDistanceAndGradientAtPosition");
    return (st & COX_Q_VALUE) && (st & COX_Q_GRADIENT);
  }
  bool getDistanceAndGradientAtPosition(const Point& position, float* distance, Point* gradient) const {
    return getDistanceAndGradientAtPosition(position, true, distance, gradient);
  }
  // TsdfMap::getWeightAtPosition
  bool getWeightAtPosition(const Point& position, bool interpolate, float* weight) const {
    uint8_t st = 0;
    check(cox_layer_query(layer_, position.data(), 1, interpolate ? COX_QUERY_INTERPOLATE : COX_QUERY_NEAREST, 0, nullptr, weight, nullptr, &st),
          "getWeightAtPosition");
    return (st & COX_Q_VALUE) != 0;
  }
  // EsdfMap::isObserved: the block exists and its voxel at the position is observed
  bool isObserved(const Point& position) const {
    uint8_t st = 0;
    check(cox_layer_query(layer_, position.data(), 1, COX_QUERY_NEAREST, 0, nullptr, nullptr, nullptr, &st), "isObserved");
    return (st & COX_Q_VALUE) != 0;
  }

  // batch forms: one call for all positions; observed[i] = 1 where the answer is valid
  void batchGetDistanceAtPosition(const Pointcloud& positions, std::vector<float>* distances, std::vector<int>* observed, bool interpolate = true) const {
    std::vector<uint8_t> st;
    run(positions, interpolate ? COX_QUERY_INTERPOLATE : COX_QUERY_NEAREST, false, distances, nullptr, nullptr, &st, "batchGetDistanceAtPosition");
    observed->assign(st.begin(), st.end());
    for (int& o : *observed) o = (o & COX_Q_VALUE) ? 1 : 0;
  }
  void batchGetDistanceAndGradientAtPosition(const Pointcloud& positions, std::vector<float>* distances, Pointcloud* gradients,
                                             std::vector<int>* observed, bool interpolate = true) const {
    std::vector<uint8_t> st;
    run(positions, interpolate ? COX_QUERY_ADAPTIVE : COX_QUERY_NEAREST, true, distances, nullptr, gradients, &st, "batchGetDistanceAndGradientAtPosition");
    observed->resize(st.size());
    for (size_t i = 0; i < st.size(); ++i) (*observed)[i] = ((st[i] & COX_Q_VALUE) && (st[i] & COX_Q_GRADIENT)) ? 1 : 0;
  }
  void batchIsObserved(const Pointcloud& positions, std::vector<int>* observed) const {
    std::vector<uint8_t> st;
    run(positions, COX_QUERY_NEAREST, false, nullptr, nullptr, nullptr, &st, "batchIsObserved");
    observed->resize(st.size());
    for (size_t i = 0; i < st.size(); ++i) (*observed)[i] = (st[i] & COX_Q_VALUE) ? 1 : 0;
  }

 private:
  void run(const Pointcloud& positions, int mode, bool grad, std::vector<float>* d, std::vector<float>* w, Pointcloud* g, std::vector<uint8_t>* st,
           const char* what) const {
    const size_t n = positions.size();
    if (d) d->resize(n);
    if (w) w->resize(n);
    if (g) g->resize(n);
    st->resize(n);
    check(cox_layer_query(layer_, positions.empty() ? nullptr : positions[0].data(), n, mode, grad ? 1 : 0, d ? d->data() : nullptr, w ? w->data() : nullptr,
                          (g && n) ? (*g)[0].data() : nullptr, st->data()),
          what);
  }

  cox_layer_t* layer_;
};

// What a layer (a TSDF, or an ESDF in TSDF wire layout) looks like from a pose: cox_layer_render into host images.
struct RenderedView {
  int width = 0, height = 0;
  std::vector<float> depth;     // width * height z-depths, row-major; NaN where the ray found no surface
  std::vector<Point> normal;    // unit gradient of the distance at the hit, pointing into free space; NaN without COX_R_NORMAL
  std::vector<Color> color;     // colour of the voxel containing the hit; 0 without COX_R_COLOR
  std::vector<uint8_t> status;  // COX_R_HIT | COX_R_NORMAL | COX_R_COLOR | COX_R_BUDGET
  cox_render_stats stats;
};
// K = {fx, fy, cx, cy}; config NULL: cox_render_config_default
inline void renderView(cox_layer_t* layer, const Transformation& T_G_C, int width, int height, const float K[4], RenderedView* view,
                       const cox_render_config* config = nullptr) {
  const size_t n = (width > 0 && height > 0) ? static_cast<size_t>(width) * static_cast<size_t>(height) : 0;
  view->width = width, view->height = height;
  view->depth.resize(n), view->normal.resize(n), view->color.resize(n), view->status.resize(n);
  float T[7];
  T_G_C.pack(T);
  check(cox_layer_render(layer, T, width, height, K, config, view->depth.data(), n ? view->normal[0].data() : nullptr,
                         reinterpret_cast<uint8_t*>(view->color.data()), view->status.data(), &view->stats),
        "renderView");
}

// The other direction: a depth camera's frame into the layer (cox_depthfuse_t) -- every voxel the frustum
// reaches is projected into the depth image.  Images in renderView's layout; a writer of the layer in call order with the
// TsdfIntegrators on it.
class DepthImageIntegrator {
 public:
  typedef cox_depthfuse_config Config;
  static Config defaultConfig() {
    Config c;
    cox_depthfuse_config_default(&c);
    return c;
  }
  DepthImageIntegrator(const Config& config, cox_layer_t* layer) : h_(nullptr) { check(cox_depthfuse_create(layer, &config, &h_), "DepthImageIntegrator"); }
  DepthImageIntegrator(const Config& config, TsdfLayer* layer) : h_(nullptr) { check(cox_depthfuse_create(layer->handle(), &config, &h_), "DepthImageIntegrator"); }
  ~DepthImageIntegrator() { cox_depthfuse_destroy(h_); }
  DepthImageIntegrator(const DepthImageIntegrator&) = delete;
  DepthImageIntegrator& operator=(const DepthImageIntegrator&) = delete;

  // depth: width * height z-depths (NaN, 0, negative: nothing there); colors: as many, or empty to leave the colours alone
  void integrateDepthImage(const Transformation& T_G_C, const std::vector<float>& depth, const std::vector<Color>& colors, int width, int height,
                           const float K[4]) {
    const size_t n = (width > 0 && height > 0) ? static_cast<size_t>(width) * static_cast<size_t>(height) : 0;
    if (depth.size() != n || (!colors.empty() && colors.size() != n)) check(COX_ERR_INVALID_ARG, "integrateDepthImage");
    float T[7];
    T_G_C.pack(T);
    check(cox_depthfuse_integrate(h_, T, depth.data(), colors.empty() ? nullptr : reinterpret_cast<const uint8_t*>(colors.data()), width, height, K),
          "integrateDepthImage");
  }
  // what renderView produced, fused into this integrator's layer (colours where the view has them)
  void integrateView(const Transformation& T_G_C, const RenderedView& view, const float K[4], bool with_color = true) {
    integrateDepthImage(T_G_C, view.depth, with_color ? view.color : std::vector<Color>(), view.width, view.height, K);
  }
  // device images on the layer's GPU, ordered behind producer_stream (a hipStream_t; NULL: the null stream)
  void integrateDepthImageDev(const Transformation& T_G_C, const float* depth_dev, const uint8_t* rgba_dev, int width, int height, const float K[4],
                              void* producer_stream = nullptr) {
    float T[7];
    T_G_C.pack(T);
    check(cox_depthfuse_integrate_dev(h_, T, depth_dev, rgba_dev, width, height, K, producer_stream), "integrateDepthImageDev");
  }
  void sync() { check(cox_depthfuse_sync(h_), "DepthImageIntegrator::sync"); }
  cox_depthfuse_stats lastStats() {
    cox_depthfuse_stats st;
    check(cox_depthfuse_last_stats(h_, &st), "DepthImageIntegrator::lastStats");
    return st;
  }
  cox_depthfuse_t* handle() const { return h_; }

 private:
  cox_depthfuse_t* h_;
};

// voxblox::EsdfIntegrator bound to a TSDF layer (cox_esdf_t): what tsdf_server runs on its update_esdf_every_n_sec timer.  After
// either update the ESDF layer holds exactly the words cox_esdf_from_tsdf would return for the TSDF as it is.
class EsdfIntegrator {
 public:
  typedef cox_esdf_config Config;
  EsdfIntegrator(const Config& config, cox_layer_t* tsdf_layer) : h_(nullptr) { check(cox_esdf_create(tsdf_layer, &config, &h_), "EsdfIntegrator"); }
  EsdfIntegrator(const Config& config, TsdfLayer* tsdf_layer) : h_(nullptr) { check(cox_esdf_create(tsdf_layer->handle(), &config, &h_), "EsdfIntegrator"); }
  ~EsdfIntegrator() { cox_esdf_destroy(h_); }
  EsdfIntegrator(const EsdfIntegrator&) = delete;
  EsdfIntegrator& operator=(const EsdfIntegrator&) = delete;

  // only what the TSDF's changes since the last update can reach is visited
  cox_esdf_update_stats updateFromTsdfLayer() {
    cox_esdf_update_stats st;
    check(cox_esdf_update(h_, &st), "updateFromTsdfLayer");
    return st;
  }
  // from an empty ESDF
  cox_esdf_update_stats updateFromTsdfLayerBatch() {
    check(cox_esdf_invalidate(h_), "updateFromTsdfLayerBatch");
    return updateFromTsdfLayer();
  }
  // owned by the integrator; current as of the last update
  cox_layer_t* getEsdfLayer() const {
    cox_layer_t* e = nullptr;
    check(cox_esdf_layer(h_, &e), "getEsdfLayer");
    return e;
  }
  LayerQuery getEsdfMap() const { return LayerQuery(getEsdfLayer()); }

 private:
  cox_esdf_t* h_;
};

// coxgraph::client::MapServer without the ROS side: the combined TSDF of a submap collection, its ESDF and the traversable cloud
class MapServer {
 public:
  struct Config {  // map_server.h:26-37
    float traversability_radius;
    Config() : traversability_radius(1.0f) {}
  };

  MapServer(const VoxgraphSubmap::Config& submap_config, const Config& config = Config(), uint64_t capacity_blocks = 0)
      : submap_config_(submap_config), config_(config),
        tsdf_(new TsdfLayer(submap_config.tsdf_voxel_size, submap_config.tsdf_voxels_per_side, submap_config.device, capacity_blocks)) {}

  const Config& getConfig() const { return config_; }
  TsdfLayer* getTsdfLayerPtr() { return tsdf_.get(); }
  const TsdfLayer& getTsdfLayer() const { return *tsdf_; }

  // removeAllBlocks, then mergeLayerAintoLayerB(submap layer, submap pose, combined) for every submap in ascending id order
  void updatePastTsdf(const SubmapCollection& collection) {
    tsdf_->removeAllBlocks();
    esdf_.reset();
    for (SubmapID id : collection.getIDs()) {
      const VoxgraphSubmap::ConstPtr sm = collection.getSubmapConstPtr(id);
      mergeLayerAintoLayerB(sm->getTsdfMap().getTsdfLayer(), sm->getPose(), tsdf_.get());
    }
  }
  // EsdfIntegrator::updateFromTsdfLayerBatch on the combined TSDF (VoxgraphSubmap::Config::esdf); computed once per update
  cox_layer_t* esdf() {
    if (!esdf_) {
      cox_layer_t* e = nullptr;
      check(cox_esdf_from_tsdf(tsdf_->handle(), &submap_config_.esdf, &e), "MapServer::esdf");
      esdf_.reset(new LayerHandle(e));
    }
    return esdf_->handle();
  }
  LayerQuery getEsdfMap() { return LayerQuery(esdf()); }
  LayerQuery getTsdfMap() const { return LayerQuery(tsdf_->handle()); }

  // createFreePointcloudFromEsdfLayer(esdf, radius): voxel centres and their distances
  void getTraversable(float radius, Pointcloud* points, std::vector<float>* intensity) {
    cox_layer_t* e = esdf();
    uint64_t n = 0;
    check(cox_layer_free_points(e, radius, nullptr, nullptr, 0, &n), "getTraversable");
    points->resize(n);
    intensity->resize(n);
    if (n) check(cox_layer_free_points(e, radius, (*points)[0].data(), intensity->data(), n, &n), "getTraversable");
  }
  void getTraversable(Pointcloud* points, std::vector<float>* intensity) { getTraversable(config_.traversability_radius, points, intensity); }

 private:
  VoxgraphSubmap::Config submap_config_;
  Config config_;
  std::unique_ptr<TsdfLayer> tsdf_;
  std::unique_ptr<LayerHandle> esdf_;
};

}  // namespace coxgraph_hip
