// so3r3.h -- the pose-graph back-end's pose parameterisation, host + device: g2o's TrafoSO3R3 (SO(3) x R^3) and the EdgeSO3R3 error,
// information and Jacobians, restated in double without Eigen.  These are NOT the tracker's SE(3) maps of se3.h: here exp(upsilon, omega)
// has t = upsilon (no V * upsilon) and log returns (t, omega).
//   exp         ThirdParty/g2o-lite/g2o/types/pose_graph/trafo_so3r3.h:216-245 (Rodrigues; theta < 1e-5: I + Omega + 0.5 Omega^2)
//   log         trafo_so3r3.h:179-213 (d > 0.99999: omega = 0.5 deltaR)
//   skew, deltaR, jacobianR   so3_utils.hpp (jacobianR is the LEFT Jacobian: jacobianR(e)^-1 R_E = the right-Jacobian inverse)
//   oplus       types_six_dof_pose.h:63-67   T <- T * exp(delta), delta = (upsilon, omega), translation first
//   error       types_six_dof_pose.h:84-104  E = Z * Tj^-1 * Ti, e = log(E), Omega = (D proto^-1 D^T)^-1,
//               D = [[I, -skew(t_E)], [0, Q^-1 R_E^T]], Q = jacobianR(e_rot)
//   Jacobians   types_six_dof_pose.cpp:101-137
// Rotations are kept as row-major 3x3 matrices (g2o keeps a quaternion); a pose is R[9] | t[3].
#pragma once
#include "se3.h"

namespace rgbid {
namespace so3r3 {

// so3_utils.hpp deltaR
RGBID_HD void deltaR(const double* R, double* v) { RGBID_FP_STRICT
  v[0] = R[7] - R[5];
  v[1] = R[2] - R[6];
  v[2] = R[3] - R[1];
}

// so3_utils.hpp jacobianR: I + (1 - cos th) / th^2 Theta + (1 - sin th / th) / th^2 Theta^2; th < 1e-5: I + Theta / 2 + Theta^2 / 6
RGBID_HD void jacobianR(const double* w, double* Q) { RGBID_FP_STRICT
  double S[9], S2[9];
  se3::skew(w, S);
  se3::m3_mul(S, S, S2);
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double a, b;
  if (th < 0.00001) { a = 1.0 / 2.0; b = 1.0 / 6.0; }
  else { a = (1 - cos(th)) / (th * th); b = (1 - (sin(th) / th)) / (th * th); }
  RGBID_UNROLL for (int i = 0; i < 9; ++i) Q[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * S[i] + b * S2[i];
}

// trafo_so3r3.h:216-245 TrafoSO3R3::exp: R = Rodrigues(omega), t = upsilon
RGBID_HD void exp(const double* d, double* R, double* t) { RGBID_FP_STRICT
  const double w[3] = {d[3], d[4], d[5]};
  const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  double S[9], S2[9];
  se3::skew(w, S);
  se3::m3_mul(S, S, S2);
  double a, b;
  if (th < 0.00001) { a = 1.0; b = 0.5; }
  else { a = sin(th) / th; b = (1 - cos(th)) / (th * th); }
  RGBID_UNROLL for (int i = 0; i < 9; ++i) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * S[i] + b * S2[i];
  t[0] = d[0]; t[1] = d[1]; t[2] = d[2];
}

// trafo_so3r3.h:179-213 TrafoSO3R3::log: (t, omega); d = (tr R - 1) / 2, d > 0.99999: omega = deltaR / 2, else acos(d) / (2 sqrt(1 - d^2)) deltaR
RGBID_HD void log(const double* R, const double* t, double* e) { RGBID_FP_STRICT
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  double dR[3];
  deltaR(R, dR);
  double s;
  if (d > 0.99999) s = 0.5;
  else { const double th = acos(d); s = th / (2 * sqrt(1 - d * d)); }
  e[0] = t[0]; e[1] = t[1]; e[2] = t[2];
  e[3] = s * dR[0]; e[4] = s * dR[1]; e[5] = s * dR[2];
}

// (R1, t1) * (R2, t2)
RGBID_HD void compose(const double* R1, const double* t1, const double* R2, const double* t2, double* R, double* t) { RGBID_FP_STRICT
  double Rt[9], tt[3];
  se3::m3_mul(R1, R2, Rt);
  se3::m3_mulv(R1, t2, tt);
  RGBID_UNROLL for (int i = 0; i < 3; ++i) t[i] = tt[i] + t1[i];
  se3::m3_copy(Rt, R);
}

// types_six_dof_pose.h:63-67 VertexSO3R3::oplusImpl: T <- T * exp(delta)
RGBID_HD void oplus(double* R, double* t, const double* delta) { RGBID_FP_STRICT
  double Rd[9], td[3];
  exp(delta, Rd, td);
  compose(R, t, Rd, td, R, t);
}

// E = Z * Tj^-1 * Ti:  R_E = R_Z R_j^T R_i,  t_E = R_Z (R_j^T (t_i - t_j)) + t_Z.  mtji = R_j^T (t_i - t_j) (minus_tji of linearizeOplus)
RGBID_HD void edge_E(const double* Ri, const double* ti, const double* Rj, const double* tj, const double* RZ, const double* tZ, double* RE, double* tE,
                     double* mtji) { RGBID_FP_STRICT
  double RjT[9], A[9], dt[3], u[3];
  se3::m3_T(Rj, RjT);
  se3::m3_mul(RjT, Ri, A);
  se3::m3_mul(RZ, A, RE);
  RGBID_UNROLL for (int i = 0; i < 3; ++i) dt[i] = ti[i] - tj[i];
  se3::m3_mulv(RjT, dt, mtji);
  se3::m3_mulv(RZ, mtji, u);
  RGBID_UNROLL for (int i = 0; i < 3; ++i) tE[i] = u[i] + tZ[i];
}

// types_six_dof_pose.h:84-104 EdgeSO3R3::computeError: e = log(E); Omega = (D * proto^-1 * D^T)^-1 with D = [[I, -skew(t_E)], [0, Q^-1 R_E^T]].
// proto_inv = the inverse of the constraint's information (inverse6 of inverse6(cov), formed once per edge: it does not change).  Qinv out: Q^-1.
RGBID_HD void edge_error(const double* RE, const double* tE, const double* proto_inv, double* e, double* Omega, double* Qinv) { RGBID_FP_STRICT
  log(RE, tE, e);
  double Q[9], RET[9], B[9], S[9], D[36], C[36];
  jacobianR(e + 3, Q);
  se3::m3_inv(Q, Qinv);
  se3::m3_T(RE, RET);
  se3::m3_mul(Qinv, RET, B);
  se3::skew(tE, S);
  se3::m6_zero(D);
  RGBID_UNROLL for (int i = 0; i < 3; ++i) D[i * 6 + i] = 1.0;
  se3::m6_set_block(D, 0, 3, S, -1.0);
  se3::m6_set_block(D, 3, 3, B, 1.0);
  se3::m6_zero(C);
  se3::m6_JCJt_add(D, proto_inv, C);
  se3::inverse6(C, Omega);
}

// types_six_dof_pose.cpp:101-137 EdgeSO3R3::linearizeOplus (row-major 6x6):
//   Ji = [[R_E, 0], [0, Q^-1 R_E]],   Jj = [[-R_Z, R_Z skew(mtji)], [0, -Q^-1 R_Z]]
RGBID_HD void edge_jacobians(const double* RE, const double* RZ, const double* mtji, const double* Qinv, double* Ji, double* Jj) { RGBID_FP_STRICT
  double S[9], A[9], B[9], C[9];
  se3::m3_mul(Qinv, RE, A);
  se3::m6_zero(Ji);
  se3::m6_set_block(Ji, 0, 0, RE, 1.0);
  se3::m6_set_block(Ji, 3, 3, A, 1.0);
  se3::skew(mtji, S);
  se3::m3_mul(RZ, S, B);
  se3::m3_mul(Qinv, RZ, C);
  se3::m6_zero(Jj);
  se3::m6_set_block(Jj, 0, 0, RZ, -1.0);
  se3::m6_set_block(Jj, 0, 3, B, 1.0);
  se3::m6_set_block(Jj, 3, 3, C, -1.0);
}

}  // namespace so3r3
}  // namespace rgbid
