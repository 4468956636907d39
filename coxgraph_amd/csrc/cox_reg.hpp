// The per-point value rule of the submap registration, shared by the registration cost (cox_reg.hip) and the pose-candidate sweep
// (cox_align.hip): the relative pose reading<-reference and the transform of a reference point into the reading layer.  The
// cell and the trilinear distance there are cox_interp.hpp's.  One copy: both units produce the same bits for pos, has and val.
#pragma once
#include <cmath>

#include "cox_interp.hpp"

// relative pose reading<-reference: float for the per-point transform, double for the Jacobians
struct RelPose {
  float R[9];
  float t[3];
  double cf, sf, cr, sr;
  double tf[3], tr[3];
};

static inline RelPose make_rel_pose(const double ref[4], const double read[4]) {
  RelPose P;
  P.cf = std::cos(ref[3]);
  P.sf = std::sin(ref[3]);
  P.cr = std::cos(read[3]);
  P.sr = std::sin(read[3]);
  for (int k = 0; k < 3; ++k) {
    P.tf[k] = ref[k];
    P.tr[k] = read[k];
  }
  const double c = P.cr * P.cf + P.sr * P.sf, s = P.cr * P.sf - P.sr * P.cf;
  const double Rd[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
  for (int i = 0; i < 9; ++i) P.R[i] = static_cast<float>(Rd[i]);
  const double dx = ref[0] - read[0], dy = ref[1] - read[1], dz = ref[2] - read[2];
  P.t[0] = static_cast<float>(P.cr * dx + P.sr * dy);
  P.t[1] = static_cast<float>(-P.sr * dx + P.cr * dy);
  P.t[2] = static_cast<float>(dz);
  return P;
}

namespace cox {

// The reference point (px, py, pz) in the reading layer under R, t and the 2x2x2 cell around it there (point_cell of
// cox_interp.hpp).  False without a correspondence.
__device__ __forceinline__ bool reg_cell(const LayerView& L, const float* R, const float* t, float px, float py, float pz, float md[8], float off[3]) {
  const float pos[3] = {(R[0] * px + R[1] * py) + R[2] * pz + t[0], (R[3] * px + R[4] * py) + R[5] * pz + t[1], (R[6] * px + R[7] * py) + R[8] * pz + t[2]};
  return point_cell(L, pos, md, off);
}

// the interpolated distance of reg_cell's cell: q . md
__device__ __forceinline__ float reg_value(const float md[8], const float off[3]) {
  float q[8];
  interp_q(off, q);
  return interp_dot(q, md);
}

}  // namespace cox
