// gn_device.h -- the Gauss-Newton pieces of rgbid_tsdf_align.h steps 28, 30 and 31 that a second user needs (kernels_meshreg.hip): the
// fixed summation tree over a wave, its upper rounds between two workspace buffers, the damped 6 x 6 Cholesky solve and the retraction
// without transcendentals.  Double without contraction; the judges are tests/align_mirror.py's tree64, reduce_tiles, solve and update.
// kernels_tsdf.hip keeps its own copies of these (DESIGN.md section 28 says why); a change here is a change there.
// Device code with internal linkage: each including file compiles its own copy.
#pragma once
#include "common.h"

namespace rgbid {
namespace {

constexpr int GN_TERMS = 28;          // 21 of H (i <= j, row-major), 6 of b, the weighted squared residual
constexpr int GN_BLOCK = 256;         // the block of gn_upper_tree's callers: four waves

// every NaN among a record's doubles gets one bit pattern (a - b turns the sign of a NaN b here and not on every host)
__device__ __forceinline__ double gn_canonical_nan(double x) { return x != x ? __longlong_as_double(0x7FFFFFFFFFFFFFFFll) : x; }

// step 28's tree64 over the wave: v[l] + v[l ^ 1], then across bit 1, ... bit 5; every lane ends with the sum
__device__ __forceinline__ double gn_tree64(double v) {
  RGBID_FP_STRICT
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
  return v;
}

// Step 28's upper tree by a whole block of GN_BLOCK threads: the n values per term in src ([GN_TERMS][src_stride]) are replaced, round by
// round, by the tree64 of every 64 consecutive ones, ping-ponging between src and dst, until one per term is left.  On return src and
// src_stride name the buffer that holds them (at [term * src_stride]) and every thread of the block may read it.
__device__ __forceinline__ void gn_upper_tree(double*& src, size_t& src_stride, double* dst, size_t dst_stride, unsigned n) {
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  while (n > 1u) {
    const unsigned groups = (n + 63u) / 64u;
    for (unsigned item = wave; item < groups * GN_TERMS; item += GN_BLOCK / 64) {
      const unsigned term = item / groups, grp = item % groups, i = grp * 64u + lane;
      const double s = gn_tree64(i < n ? src[(size_t)term * src_stride + i] : 0.0);
      if (lane == 0) dst[(size_t)term * dst_stride + grp] = s;
    }
    __syncthreads();                                            // the round's sums are written before the next round reads them
    double* p = src; src = dst; dst = p;
    const size_t q = src_stride; src_stride = dst_stride; dst_stride = q;
    n = groups;
  }
  __syncthreads();
}

// Step 30 for one thread: the 28 sums at sums[k * stride] -> x = delta = (v, omega) and max |x_i|; false: SINGULAR
__device__ __forceinline__ bool gn_solve(const double* sums, size_t stride, double damping, double x[6], double& biggest) {
  RGBID_FP_STRICT
  double H[6][6], L[6][6], b[6], y[6];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) { H[i][j] = H[j][i] = sums[(size_t)k * stride]; ++k; }
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = sums[(size_t)(21 + i) * stride];
  }
  const double damp = 1.0 + damping;
#pragma unroll
  for (int j = 0; j < 6; ++j) H[j][j] = H[j][j] * damp;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = H[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0 && s < (double)INFINITY)) ok = false;         // NaN fails; a later column of a failed one is never used
    L[j][j] = sqrt(s);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double q = H[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) q = q - L[i][k] * L[j][k];
      L[i][j] = q / L[j][j];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = -b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  biggest = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double ax = fabs(x[i]);
    if (!(ax < (double)INFINITY)) ok = false;                   // NaN and infinity
    biggest = ax > biggest ? ax : biggest;
  }
  return ok;
}

// Step 31: the pose P = R00 .. R22 tx ty tz moved by the twist x = (v, omega) -> Q: R = dR R, t = dR t + v
__device__ __forceinline__ void gn_retract(const double P[12], const double x[6], double Q[12]) {
  RGBID_FP_STRICT
  const double hx = x[3] / 2.0, hy = x[4] / 2.0, hz = x[5] / 2.0;
  const double nn = sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz));
  const double qw = 1.0 / nn, qx = hx / nn, qy = hy / nn, qz = hz / nn;
  const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
  const double dR[9] = {1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
                        2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
                        2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Q[3 * i + j] = (dR[3 * i] * P[j] + dR[3 * i + 1] * P[3 + j]) + dR[3 * i + 2] * P[6 + j];
    Q[9 + i] = ((dR[3 * i] * P[9] + dR[3 * i + 1] * P[10]) + dR[3 * i + 2] * P[11]) + x[i];
  }
}

}  // namespace
}  // namespace rgbid
