// cloud_device.h -- what the kernels over packed export blocks share about a keyframe's points (kernels_cloud.hip, kernels_segment.hip):
// the reference's predicate of a point and the point itself (include/rgbid_cloud.h).  Device code with internal linkage.
#pragma once
#include "../../include/rgbid_cloud.h"
#include "common.h"

namespace rgbid {
namespace {

// the reference's predicate (keyframe_manager.cpp:478-481, 505-507): d = 1.f / iD is not NaN, the normal's x is not NaN, and in
// RGBID_CLOUD_NOVEL_ONLY mode the overlap mask is 0.  Returns d through `d`.
__device__ __forceinline__ bool cloud_valid(float iD, float n0, unsigned m, int mode, float& d) {
  d = 1.f / iD;   // IEEE division (hipcc's default for float '/'): NaN exactly when iD is
  return !isnan(d) && !isnan(n0) && (mode == RGBID_CLOUD_ALL || m == 0);
}

// Xworld = R (d Kinv p) + t and nworld = R n in double, every dot product ((a0 b0 + a1 b1) + a2 b2) and no contraction -- the order
// the tests' float64 restatement uses; all nine products d Kinv_ij and 1.0 * p_z are evaluated, so d = inf gives
// the reference's NaN from 0 * inf.  (The pragma marks these operations as not contractible; inlining keeps that mark.)
__device__ __forceinline__ void cloud_point(float d, int x, int y, const double* __restrict__ Ki, const double* __restrict__ R,
                                            const double* __restrict__ t, float n0, float n1, float n2, float (&o)[6]) {
  RGBID_FP_STRICT
  const double dd = (double)d, px = (double)x, py = (double)y, pz = 1.0;
  double Xc[3], Xw[3];
  for (int i = 0; i < 3; ++i) {
    const double a0 = dd * Ki[3 * i], a1 = dd * Ki[3 * i + 1], a2 = dd * Ki[3 * i + 2];
    Xc[i] = (a0 * px + a1 * py) + a2 * pz;
  }
  for (int i = 0; i < 3; ++i) Xw[i] = ((R[3 * i] * Xc[0] + R[3 * i + 1] * Xc[1]) + R[3 * i + 2] * Xc[2]) + t[i];
  const double nc0 = (double)n0, nc1 = (double)n1, nc2 = (double)n2;
  for (int i = 0; i < 3; ++i) {
    o[i] = (float)Xw[i];
    o[3 + i] = (float)((R[3 * i] * nc0 + R[3 * i + 1] * nc1) + R[3 * i + 2] * nc2);
  }
}

}  // namespace
}  // namespace rgbid
