// Test-side reference of the pinhole depth integrator: a single-threaded float32 restatement of the rule of one frame as
// DESIGN.md section 7m writes it down, steps 1-9, in that operation order.  Wire arrays in, wire arrays out (block indices plus
// 3 x u32 voxels, in POOL order), so it composes with the checker's layers.  Every voxel of every block of a generous box
// around the frustum is visited: no culling, no early exit, no parallelism -- nothing here is shared with any GPU code.
// Build: g++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off -fno-fast-math (tests/depthfuse_ref.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace {

struct Config {
  float truncation_distance, max_weight, min_depth_m, max_depth_m;
  int32_t voxel_carving_enabled, use_const_weight, use_weight_dropoff, interpolation_scheme;
  float adaptive_gap_m;
  uint32_t reserved;
};
struct Stats {
  uint64_t n_valid_pixels, n_candidate_blocks, n_touched_blocks, n_new_blocks, n_updated_voxels, n_coloured_voxels;
  double kernel_ms;
};
struct V3 {
  float x, y, z;
};
struct Block {
  int32_t idx[3];
  std::vector<uint32_t> words;  // 4096 * 3
};
struct RefLayer {
  float voxel_size;
  std::vector<Block> pool;
  std::map<std::tuple<int32_t, int32_t, int32_t>, size_t> index;  // (z, y, x) -> pool position
};

V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// A.1: uv = q.vec x p; uv += uv; p + w uv + q.vec x uv
V3 rotate(const float q[4], V3 p) {
  const V3 qv{q[1], q[2], q[3]};
  V3 uv = cross(qv, p);
  uv = V3{uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
  const V3 c = cross(qv, uv);
  return V3{(p.x + q[0] * uv.x) + c.x, (p.y + q[0] * uv.y) + c.y, (p.z + q[0] * uv.z) + c.z};
}
bool valid_depth(float d) { return std::isfinite(d) && d > 0.0f; }
float bits_to_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
uint32_t float_to_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
// Color::blendTwoColors on wire words a | b << 8 | g << 16 | r << 24
uint32_t blend(uint32_t c1, float w1, uint32_t c2, float w2) {
  const float tot = w1 + w2;
  w1 /= tot;
  w2 /= tot;
  uint32_t out = 0;
  for (int sh = 0; sh < 32; sh += 8) {
    const float a = static_cast<float>((c1 >> sh) & 255u), b = static_cast<float>((c2 >> sh) & 255u);
    out |= (static_cast<uint32_t>(static_cast<int>(std::round(a * w1 + b * w2))) & 255u) << sh;
  }
  return out;
}

// step 4
bool depth_lookup(const Config& cfg, const float* depth, int w, int h, float u, float v, float* D, int* pu, int* pv) {
  int un = static_cast<int>(std::floor(u + 0.5f)), vn = static_cast<int>(std::floor(v + 0.5f));
  un = std::min(std::max(un, 0), w - 1);
  vn = std::min(std::max(vn, 0), h - 1);
  *pu = un;
  *pv = vn;
  const float nearest = depth[static_cast<size_t>(vn) * w + un];
  const int u0 = static_cast<int>(std::floor(u)), v0 = static_cast<int>(std::floor(v));
  const bool cell = cfg.interpolation_scheme != 0 && u0 >= 0 && v0 >= 0 && u0 + 1 <= w - 1 && v0 + 1 <= h - 1;
  if (!cell) {
    *D = nearest;
    return valid_depth(nearest);
  }
  const float a = depth[static_cast<size_t>(v0) * w + u0], b = depth[static_cast<size_t>(v0) * w + u0 + 1];
  const float c = depth[static_cast<size_t>(v0 + 1) * w + u0], d = depth[static_cast<size_t>(v0 + 1) * w + u0 + 1];
  std::vector<float> ok;
  for (float p : {a, b, c, d})
    if (valid_depth(p)) ok.push_back(p);
  if (cfg.interpolation_scheme == 1) {
    if (ok.empty()) return false;
    *D = *std::min_element(ok.begin(), ok.end());
    return true;
  }
  if (cfg.interpolation_scheme == 3 && !ok.empty()) {
    const float mn = *std::min_element(ok.begin(), ok.end()), mx = *std::max_element(ok.begin(), ok.end());
    if (mx - mn > cfg.adaptive_gap_m) {
      *D = mn;
      return true;
    }
  }
  if (ok.size() != 4) {
    *D = nearest;
    return valid_depth(nearest);
  }
  const float du = u - static_cast<float>(u0), dv = v - static_cast<float>(v0);
  *D = (a * (1.0f - dv) + c * dv) * (1.0f - du) + (b * (1.0f - dv) + d * dv) * du;
  return true;
}

}  // namespace

extern "C" {

void* depthfuse_ref_create(float voxel_size, uint64_t n, const int32_t* idx, const uint32_t* vox) {
  RefLayer* L = new RefLayer();
  L->voxel_size = voxel_size;
  for (uint64_t i = 0; i < n; ++i) {
    Block b;
    std::memcpy(b.idx, idx + 3 * i, 12);
    b.words.assign(vox + i * 12288, vox + (i + 1) * 12288);
    L->index[{b.idx[2], b.idx[1], b.idx[0]}] = L->pool.size();
    L->pool.push_back(std::move(b));
  }
  return L;
}
void depthfuse_ref_free(void* h) { delete static_cast<RefLayer*>(h); }
uint64_t depthfuse_ref_size(void* h) { return static_cast<RefLayer*>(h)->pool.size(); }
void depthfuse_ref_download(void* h, int32_t* idx, uint32_t* vox) {  // pool order
  const RefLayer* L = static_cast<RefLayer*>(h);
  for (size_t i = 0; i < L->pool.size(); ++i) {
    std::memcpy(idx + 3 * i, L->pool[i].idx, 12);
    std::memcpy(vox + i * 12288, L->pool[i].words.data(), 12288 * 4);
  }
}

// one frame; rgba may be NULL; max_blocks < 0: unlimited, else the pool's capacity (returns -4 with the layer unchanged)
int depthfuse_ref_frame(void* h, const Config* cfgp, const float T[7], const float* depth, const uint8_t* rgba, int w, int hgt, const float K[4],
                        int64_t max_blocks, Stats* stats) {
  RefLayer* L = static_cast<RefLayer*>(h);
  const Config cfg = *cfgp;
  const float vs = L->voxel_size, trunc = cfg.truncation_distance;
  Stats st{};
  // step 1
  for (size_t i = 0; i < static_cast<size_t>(w) * hgt; ++i) st.n_valid_pixels += valid_depth(depth[i]) ? 1 : 0;
  // T_G_C^-1 = (q*, -rotate(q*, t))
  const float qi[4] = {T[0], -T[1], -T[2], -T[3]};
  const V3 rt = rotate(qi, V3{T[4], T[5], T[6]});
  const V3 ti{-rt.x, -rt.y, -rt.z};
  // a box of blocks that holds every voxel within max_depth / cos(half angle) of the camera, one block to spare
  const double ax = std::max(std::fabs((-0.5 - K[2]) / K[0]), std::fabs((w - 0.5 - K[2]) / K[0]));
  const double ay = std::max(std::fabs((-0.5 - K[3]) / K[1]), std::fabs((hgt - 0.5 - K[3]) / K[1]));
  const double reach = cfg.max_depth_m * std::sqrt(1.0 + ax * ax + ay * ay);
  const double bs = 16.0 * static_cast<double>(vs);
  int64_t lo[3], hi[3];
  for (int k = 0; k < 3; ++k) {
    lo[k] = static_cast<int64_t>(std::floor((T[4 + k] - reach) / bs)) - 1;
    hi[k] = static_cast<int64_t>(std::floor((T[4 + k] + reach) / bs)) + 1;
  }
  struct Pending {
    int32_t idx[3];
    std::vector<uint32_t> words;
    bool is_new;
    size_t pool;
  };
  std::vector<Pending> touched;  // in ascending (z, y, x)
  const float u_hi = static_cast<float>(w) - 0.5f, v_hi = static_cast<float>(hgt) - 0.5f;
  for (int64_t bz = lo[2]; bz <= hi[2]; ++bz)
    for (int64_t by = lo[1]; by <= hi[1]; ++by)
      for (int64_t bx = lo[0]; bx <= hi[0]; ++bx) {
        ++st.n_candidate_blocks;
        const auto it = L->index.find({static_cast<int32_t>(bz), static_cast<int32_t>(by), static_cast<int32_t>(bx)});
        Pending p;
        p.idx[0] = static_cast<int32_t>(bx), p.idx[1] = static_cast<int32_t>(by), p.idx[2] = static_cast<int32_t>(bz);
        p.is_new = it == L->index.end();
        p.pool = p.is_new ? 0 : it->second;
        if (p.is_new)
          p.words.assign(12288, 0u);
        else
          p.words = L->pool[p.pool].words;
        uint64_t n_upd = 0, n_col = 0;
        for (int lin = 0; lin < 4096; ++lin) {
          const int gx = static_cast<int>(bx) * 16 + (lin & 15), gy = static_cast<int>(by) * 16 + ((lin >> 4) & 15), gz = static_cast<int>(bz) * 16 + (lin >> 8);
          // step 2: centre (A.2), into the camera frame
          const V3 c{(static_cast<float>(gx) + 0.5f) * vs, (static_cast<float>(gy) + 0.5f) * vs, (static_cast<float>(gz) + 0.5f) * vs};
          const V3 r = rotate(qi, c);
          const V3 q{r.x + ti.x, r.y + ti.y, r.z + ti.z};
          const float z = q.z;
          if (!(cfg.min_depth_m <= z && z <= cfg.max_depth_m)) continue;
          // step 3
          const float u = K[0] * (q.x / z) + K[2];
          const float v = K[1] * (q.y / z) + K[3];
          if (!(-0.5f <= u && u < u_hi && -0.5f <= v && v < v_hi)) continue;
          // step 4
          float D;
          int pu, pv;
          if (!depth_lookup(cfg, depth, w, hgt, u, v, &D, &pu, &pv)) continue;
          // step 5
          const float norm = std::sqrt((q.x * q.x + q.y * q.y) + q.z * q.z);
          const float sdf = (D - z) * (norm / z);
          if (sdf < -trunc) continue;
          if (!cfg.voxel_carving_enabled && sdf > trunc) continue;
          // step 6
          float uw = cfg.use_const_weight ? 1.0f : 1.0f / (D * D);
          if (cfg.use_weight_dropoff && sdf < -vs) {
            uw = uw * (trunc + sdf) / (trunc - vs);
            uw = std::max(uw, 0.0f);
          }
          // step 7
          uint32_t* word = p.words.data() + 3 * lin;
          const float d0 = bits_to_float(word[0]), w0 = bits_to_float(word[1]);
          const float nw = w0 + uw;
          if (nw < 1e-6f) continue;
          const float nsdf = (sdf * uw + d0 * w0) / nw;
          if (rgba != nullptr && std::fabs(sdf) < trunc) {
            const uint8_t* px = rgba + 4 * (static_cast<size_t>(pv) * w + pu);
            const uint32_t colour = static_cast<uint32_t>(px[3]) | (static_cast<uint32_t>(px[2]) << 8) | (static_cast<uint32_t>(px[1]) << 16) | (static_cast<uint32_t>(px[0]) << 24);
            word[2] = blend(word[2], w0, colour, uw);
            ++n_col;
          }
          word[0] = float_to_bits(nsdf > 0.0f ? std::min(trunc, nsdf) : std::max(-trunc, nsdf));
          word[1] = float_to_bits(std::min(cfg.max_weight, nw));
          ++n_upd;
        }
        if (n_upd == 0) continue;  // step 8
        st.n_updated_voxels += n_upd;
        st.n_coloured_voxels += n_col;
        st.n_touched_blocks += 1;
        st.n_new_blocks += p.is_new ? 1 : 0;
        touched.push_back(std::move(p));
      }
  if (stats) *stats = st;
  if (max_blocks >= 0 && L->pool.size() + st.n_new_blocks > static_cast<uint64_t>(max_blocks)) {
    if (stats) *stats = Stats{};
    return -4;
  }
  // step 9: new blocks to the end of the pool in ascending (z, y, x) -- the loop order above
  for (Pending& p : touched) {
    if (p.is_new) {
      Block b;
      std::memcpy(b.idx, p.idx, 12);
      b.words = std::move(p.words);
      L->index[{b.idx[2], b.idx[1], b.idx[0]}] = L->pool.size();
      L->pool.push_back(std::move(b));
    } else {
      L->pool[p.pool].words = std::move(p.words);
    }
  }
  return 0;
}

}  // extern "C"
