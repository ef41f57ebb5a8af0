// kernels_loopfeat.hip -- appearance stage of loop closure (include/rgbid_loopfeat.h; LoopCloser::detectLoopClosures and
// computeRANSACTrafo3D, src/loop_closer.cpp:193-716; Keyframe::lift2DKeypointsto3DPointsWithCovariance, src/keyframe.cpp:232-274).
//
//   features  k_lf_response   Harris response per pixel: a 24 x 24 grey tile and its 22 x 22 integer derivatives in LDS, 49 products per pixel
//             k_lf_select     one workgroup per 32 x 32 cell: strict local maxima appended to an LDS list (integer LDS counter; the list's
//                             order does not matter), ranked by counting (response descending, raster index ascending); the best k go to a
//                             staging table [keyframe][cell][rank]
//             k_lf_describe   one wave per staged keypoint: the 33 x 33 patch in LDS, integer moments -> direction, 256 tests on 5 x 5 box
//                             sums assembled by 4 ballots, the 3-D point and covariance in double; the wave finds its output slot by summing
//                             the counts of the cells before its own, so the records are compact, cell-major, and no atomics touch the output
//   matching  k_lf_match      one workgroup per (query, candidate) pair: candidate descriptors in LDS, a query descriptor in 4 x 64-bit
//                             registers per thread, XOR + popcount; survivors are compacted in query order with ballots + mbcnt
//   ransac    k_lf_ransac     one workgroup per pair, one thread per hypothesis; per-match points and covariances are staged in LDS in
//                             chunks of 128 matches and read as broadcasts; block argmax (most inliers, lowest iteration); the inlier mask of
//                             the winner is written by one thread per match with the same error function
// The file is compiled without contraction: every float / double expression below is rounded operation by operation, in the order written.
#include "../../include/rgbid_loopfeat.h"
#include "../../include/rgbid_cloud.h"
#include "common.h"
#include "ctx.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#pragma clang fp contract(off)

using namespace rgbid;

static_assert(sizeof(rgbid_loopfeat_kp) == 120, "rgbid_loopfeat_kp is 120 bytes");
static_assert(offsetof(rgbid_loopfeat_kp, desc) == 16 && offsetof(rgbid_loopfeat_kp, X) == 48 && offsetof(rgbid_loopfeat_kp, cov) == 72, "record layout");
static_assert(sizeof(rgbid_loopfeat_corr) == 16, "rgbid_loopfeat_corr is 16 bytes");

namespace {

constexpr int LT = 256;                              // threads per block
constexpr int CELL = RGBID_LOOPFEAT_CELL;
constexpr int BORDER = RGBID_LOOPFEAT_BORDER;
constexpr int CELL_CAND = (CELL / 2) * (CELL / 2);   // no two 8-neighbours are both strict maxima: at most one per 2 x 2 block
constexpr int PATCH = 2 * BORDER + 1;                // 33
constexpr int RCHUNK = 128;                          // matches per LDS chunk of the vote
constexpr int HARRIS_R = 3;                          // 7 x 7 block
constexpr int RESP_MARGIN = HARRIS_R + 1;

struct LfGeom { int rows, cols, cells_x, cells_y, per_cell, max_kp; };
struct LfKinv { double m[9]; };
struct LfStaged { int idx; float resp; };

__device__ __forceinline__ unsigned lane_prefix(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- features ----
__global__ __launch_bounds__(LT) void k_lf_response(const uint8_t* __restrict__ grey, LfGeom g, float scale4, float* __restrict__ resp) {
  __shared__ int tile[24][24];
  __shared__ short dIx[22][22], dIy[22][22];
  const int kf = blockIdx.z, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int x0 = blockIdx.x * 16, y0 = blockIdx.y * 16;
  const uint8_t* img = grey + (size_t)kf * g.rows * g.cols;
  for (int i = threadIdx.x; i < 24 * 24; i += LT) {
    const int ly = i / 24, lx = i % 24;
    const int y = min(max(y0 + ly - RESP_MARGIN, 0), g.rows - 1), x = min(max(x0 + lx - RESP_MARGIN, 0), g.cols - 1);   // clamped reads feed only refused pixels
    tile[ly][lx] = img[(size_t)y * g.cols + x];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 22 * 22; i += LT) {
    const int ly = i / 22 + 1, lx = i % 22 + 1;   // tile coordinates of the derivative's centre
#define GV(dy, dx) tile[ly + (dy)][lx + (dx)]
    const int Ix = 2 * (GV(0, 1) - GV(0, -1)) + (GV(-1, 1) - GV(-1, -1)) + (GV(1, 1) - GV(1, -1));
    const int Iy = 2 * (GV(1, 0) - GV(-1, 0)) + (GV(1, -1) - GV(-1, -1)) + (GV(1, 1) - GV(-1, 1));
#undef GV
    dIx[ly - 1][lx - 1] = (short)Ix;
    dIy[ly - 1][lx - 1] = (short)Iy;
  }
  __syncthreads();
  const int x = x0 + tx, y = y0 + ty;
  if (x >= g.cols || y >= g.rows) return;
  float r = 0.f;
  if (x >= RESP_MARGIN && x < g.cols - RESP_MARGIN && y >= RESP_MARGIN && y < g.rows - RESP_MARGIN) {
    int sxx = 0, syy = 0, sxy = 0;
    for (int j = 0; j < 7; ++j)
      for (int i = 0; i < 7; ++i) {
        const int Ix = dIx[ty + j][tx + i], Iy = dIy[ty + j][tx + i];
        sxx += Ix * Ix; syy += Iy * Iy; sxy += Ix * Iy;
      }
    const float a = (float)((long long)sxx * (long long)syy), b = (float)((long long)sxy * (long long)sxy);
    const float tr = (float)(sxx + syy);
    r = (a - b) - ((0.04f * tr) * tr) * scale4;
  }
  resp[((size_t)kf * g.rows + y) * g.cols + x] = r;
}

// a beats b: larger response, or equal response and smaller raster index
__device__ __forceinline__ bool lf_beats(float ra, int ia, float rb, int ib) { return ra > rb || (ra == rb && ia < ib); }

__global__ __launch_bounds__(LT) void k_lf_select(const float* __restrict__ resp, const float* __restrict__ invdepth, LfGeom g,
                                                  LfStaged* __restrict__ staged, int* __restrict__ cell_counts) {
  __shared__ int cnt;
  __shared__ float cr[CELL_CAND];
  __shared__ int ci[CELL_CAND];
  const int kf = blockIdx.y, cell = blockIdx.x, cells = g.cells_x * g.cells_y;
  const int cx = cell % g.cells_x, cy = cell / g.cells_x;
  const float* R = resp + (size_t)kf * g.rows * g.cols;
  const float* W = invdepth + (size_t)kf * g.rows * g.cols;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  for (int p = threadIdx.x; p < CELL * CELL; p += LT) {
    const int x = cx * CELL + p % CELL, y = cy * CELL + p / CELL;
    if (x < BORDER || x >= g.cols - BORDER || y < BORDER || y >= g.rows - BORDER) continue;   // the 8 neighbours are inside the image
    const int idx = y * g.cols + x;
    const float r = R[idx];
    if (!(r > 0.f)) continue;
    bool is_max = true;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (dx == 0 && dy == 0) continue;
        const int j = idx + dy * g.cols + dx;
        is_max = is_max && lf_beats(r, idx, R[j], j);
      }
    const float w = W[idx];
    if (!is_max || !(isfinite(w) && w > 0.f)) continue;
    const int slot = atomicAdd(&cnt, 1);   // integer LDS counter: the list's order is arbitrary, the ranks below do not depend on it
    if (slot < CELL_CAND) { cr[slot] = r; ci[slot] = idx; }
  }
  __syncthreads();
  const int nc = min(cnt, CELL_CAND);
  if ((int)threadIdx.x < nc) {
    const float r = cr[threadIdx.x];
    const int idx = ci[threadIdx.x];
    int rank = 0;
    for (int j = 0; j < nc; ++j) rank += lf_beats(cr[j], ci[j], r, idx) ? 1 : 0;
    if (rank < g.per_cell) staged[((size_t)kf * cells + cell) * g.per_cell + rank] = LfStaged{idx, r};
  }
  if (threadIdx.x == 0) cell_counts[(size_t)kf * cells + cell] = min(nc, g.per_cell);
}

__device__ __forceinline__ int lf_box(const uint8_t* patch, int px, int py) {
  int s = 0;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) s += patch[(py + dy + BORDER) * PATCH + (px + dx + BORDER)];
  return s;
}

__global__ __launch_bounds__(LT) void k_lf_describe(const uint8_t* __restrict__ grey, const float* __restrict__ invdepth, LfGeom g, LfKinv Ki,
                                                    const LfStaged* __restrict__ staged, const int* __restrict__ cell_counts,
                                                    const char4* __restrict__ rotated, const double* __restrict__ bounds,
                                                    rgbid_loopfeat_kp* __restrict__ kps, int* __restrict__ counts) {
  __shared__ uint8_t patches[LT / 64][PATCH * PATCH + 7];
  const int kf = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cells = g.cells_x * g.cells_y;
  const int slot = blockIdx.x * (LT / 64) + wave;
  const int cell = slot / g.per_cell, rank = slot % g.per_cell;
  const int* cc = cell_counts + (size_t)kf * cells;
  const bool in_table = slot < cells * g.per_cell;
  int before = 0;
  if (in_table)
    for (int c = lane; c < cell; c += 64) before += cc[c];
  before = wave_sum(before);
  if (slot == 0) {   // the first wave of a keyframe also writes its keypoint count
    int total = 0;
    for (int c = lane; c < cells; c += 64) total += cc[c];
    total = wave_sum(total);
    if (lane == 0) counts[kf] = total;
  }
  const bool active = in_table && rank < cc[cell];
  uint8_t* patch = patches[wave];
  const uint8_t* img = grey + (size_t)kf * g.rows * g.cols;
  int idx = 0, x = BORDER, y = BORDER;
  float response = 0.f;
  if (active) {
    const LfStaged st = staged[((size_t)kf * cells + cell) * g.per_cell + rank];
    idx = st.idx; response = st.resp; x = idx % g.cols; y = idx / g.cols;   // BORDER <= x < cols - BORDER and the same for y: the patch is inside
    for (int i = lane; i < PATCH * PATCH; i += 64) patch[i] = img[(size_t)(y + i / PATCH - BORDER) * g.cols + (x + i % PATCH - BORDER)];
  }
  __syncthreads();
  if (!active) return;
  int m10 = 0, m01 = 0;
  for (int i = lane; i < 31 * 31; i += 64) {
    const int dy = i / 31 - 15, dx = i % 31 - 15;
    if (dx * dx + dy * dy <= 225) {
      const int v = patch[(dy + BORDER) * PATCH + dx + BORDER];
      m10 += dx * v; m01 += dy * v;
    }
  }
  m10 = wave_sum(m10); m01 = wave_sum(m01);
  // direction: the half plane, then the boundaries (2 b + 1) pi / 32, b < 16, that the moment vector has passed
  const bool upper = m01 > 0 || (m01 == 0 && m10 >= 0);
  const double mx = upper ? (double)m10 : -(double)m10, my = upper ? (double)m01 : -(double)m01;
  int passed = 0;
  for (int b = 0; b < 16; ++b) passed += (bounds[2 * b] * my - bounds[2 * b + 1] * mx > 0.0) ? 1 : 0;
  const int dir = (passed + (upper ? 0 : 16)) & 31;
  rgbid_loopfeat_kp* out = kps + (size_t)kf * g.max_kp + before + rank;
  uint8_t* desc = out->desc;
  for (int j = 0; j < 4; ++j) {
    const char4 p = rotated[dir * RGBID_LOOPFEAT_TESTS + j * 64 + lane];
    const bool bit = lf_box(patch, p.x, p.y) < lf_box(patch, p.z, p.w);
    const unsigned long long m = __ballot(bit);
    if (lane < 8) desc[j * 8 + lane] = (uint8_t)(m >> (8 * lane));
  }
  if (lane == 0) {
    out->x = x; out->y = y; out->response = response; out->direction = dir;
    const float w = invdepth[(size_t)kf * g.rows * g.cols + idx];
    const double d = (double)(1.f / w), px = (double)x, py = (double)y, pz = 1.0;
    const double inv_d = 1.0 / d;
    const double s[3] = {(double)(0.5f * 0.5f), (double)(0.5f * 0.5f), (double)(0.00025f * 0.00025f)};
    double X[3], J[3][3];
    for (int i = 0; i < 3; ++i) {
      const double a0 = d * Ki.m[3 * i], a1 = d * Ki.m[3 * i + 1], a2 = d * Ki.m[3 * i + 2];
      X[i] = (a0 * px + a1 * py) + a2 * pz;
      const double mp = (Ki.m[3 * i] * px + Ki.m[3 * i + 1] * py) + Ki.m[3 * i + 2] * pz;
      J[i][0] = inv_d * Ki.m[3 * i];
      J[i][1] = inv_d * Ki.m[3 * i + 1];
      J[i][2] = -(inv_d * inv_d) * mp;
      out->X[i] = X[i];
    }
    int k = 0;
    for (int i = 0; i < 3; ++i)
      for (int j = i; j < 3; ++j) out->cov[k++] = ((J[i][0] * s[0]) * J[j][0] + (J[i][1] * s[1]) * J[j][1]) + (J[i][2] * s[2]) * J[j][2];
  }
}

// ---- matching ----
__global__ __launch_bounds__(LT) void k_lf_match(const rgbid_loopfeat_kp* __restrict__ kps, const int* __restrict__ counts, int n_kf, int max_kp,
                                                 const int* __restrict__ pairs, float ratio, rgbid_loopfeat_corr* __restrict__ matches,
                                                 int* __restrict__ match_counts) {
  extern __shared__ unsigned long long cdesc[];   // [max_kp][4]
  __shared__ unsigned wtot[LT / 64];
  const int pair = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = pairs[2 * pair], c = pairs[2 * pair + 1];
  const bool ok = q >= 0 && q < n_kf && c >= 0 && c < n_kf;
  const int nq = ok ? min(max(counts[q], 0), max_kp) : 0, nc = ok ? min(max(counts[c], 0), max_kp) : 0;
  if (nq == 0 || nc < 2) {   // uniform over the block
    if (threadIdx.x == 0) match_counts[pair] = 0;
    return;
  }
  const rgbid_loopfeat_kp* kq = kps + (size_t)q * max_kp;
  const rgbid_loopfeat_kp* kc = kps + (size_t)c * max_kp;
  for (int i = threadIdx.x; i < nc * 4; i += LT)
    cdesc[i] = *reinterpret_cast<const unsigned long long*>(kc[i >> 2].desc + 8 * (i & 3));
  __syncthreads();
  rgbid_loopfeat_corr* out = matches ? matches + (size_t)pair * max_kp : nullptr;
  unsigned running = 0;
  for (int base = 0; base < nq; base += LT) {
    const int i = base + threadIdx.x;
    const bool valid = i < nq;
    int d0 = 1 << 20, d1 = 1 << 20, i0 = -1;
    if (valid) {
      unsigned long long a[4];
      for (int j = 0; j < 4; ++j) a[j] = *reinterpret_cast<const unsigned long long*>(kq[i].desc + 8 * j);
      for (int k = 0; k < nc; ++k) {
        const int d = __popcll(a[0] ^ cdesc[4 * k]) + __popcll(a[1] ^ cdesc[4 * k + 1]) + __popcll(a[2] ^ cdesc[4 * k + 2]) +
                      __popcll(a[3] ^ cdesc[4 * k + 3]);
        if (d < d0) { d1 = d0; d0 = d; i0 = k; }   // strict: the lower candidate index stays in front on a tie
        else if (d < d1) d1 = d;
      }
    }
    const bool keep = valid && (float)d0 < ratio * (float)d1;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wtot[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned pos = running + lane_prefix(m);
    for (int w = 0; w < wave; ++w) pos += wtot[w];
    const unsigned total = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    if (keep && out) out[pos] = rgbid_loopfeat_corr{i, i0, d0, d1};   // pos < nq <= max_kp
    running += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) match_counts[pair] = (int)running;
}

// ---- RANSAC ----
struct LfPose { double R[9], t[3]; };

// selectRandomMatches (loop_closer.cpp:555-585) without the array: entry j of the list after the first removal is (j == i0 ? m - 1 : j)
__device__ __forceinline__ void lf_sample3(const double* u, int m, int s[3]) {
  const int i0 = (int)(u[0] * (double)m);
  const int i1 = (int)(u[1] * (double)(m - 1));
  const int i2 = (int)(u[2] * (double)(m - 2));
  s[0] = i0;
  s[1] = i1 == i0 ? m - 1 : i1;
  const int last = (m - 2 == i0) ? m - 1 : m - 2;   // what moved into position i1 at the second removal
  s[2] = i2 == i1 ? last : (i2 == i0 ? m - 1 : i2);
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

// centred 3-point set -> in-plane orthonormal frame (e1 along the first delta, e2 = n x e1, n) and the points' 2-D coordinates
__device__ __forceinline__ bool lf_plane(const double (&P)[3][3], double* centroid, double (&E)[3][3], double (&xy)[3][2]) {
  double d[3][3];
  for (int a = 0; a < 3; ++a) centroid[a] = ((P[0][a] + P[1][a]) + P[2][a]) / 3.0;
  for (int i = 0; i < 3; ++i)
    for (int a = 0; a < 3; ++a) d[i][a] = P[i][a] - centroid[a];
  double n[3];
  cross3(d[0], d[1], n);
  const double l1 = sqrt(dot3(d[0], d[0])), ln = sqrt(dot3(n, n));
  if (!(l1 > 0.0 && ln > 0.0)) return false;
  for (int a = 0; a < 3; ++a) { E[0][a] = d[0][a] / l1; E[2][a] = n[a] / ln; }
  cross3(E[2], E[0], E[1]);
  for (int i = 0; i < 3; ++i) { xy[i][0] = dot3(d[i], E[0]); xy[i][1] = dot3(d[i], E[1]); }
  return true;
}

// the proper rotation that maximises sum q_i . (R c_i) for 3 correspondences: both triangles are planar, so R takes the candidate's plane
// to the query's; inside the plane the best orthogonal map is a rotation (det of the 2-D correlation >= 0) or a reflection, and the normal
// goes to +n or -n so that det R = +1.  That is U diag(1, 1, det(U V^T)) V^T of the rank-2 correlation, without a factorisation.
__device__ __forceinline__ bool lf_pose3(const double (&Q)[3][3], const double (&Cn)[3][3], LfPose& T) {
  double cq[3], cc[3], E[3][3], F[3][3], q2[3][2], c2[3][2];
  if (!lf_plane(Q, cq, E, q2) || !lf_plane(Cn, cc, F, c2)) return false;
  double sxx = 0, sxy = 0, syx = 0, syy = 0;   // sum q_a c_b
  for (int i = 0; i < 3; ++i) {
    sxx += q2[i][0] * c2[i][0]; sxy += q2[i][0] * c2[i][1];
    syx += q2[i][1] * c2[i][0]; syy += q2[i][1] * c2[i][1];
  }
  const bool rot = sxx * syy - sxy * syx >= 0.0;
  const double Cc = rot ? sxx + syy : sxx - syy, Ss = rot ? syx - sxy : sxy + syx;
  const double h = sqrt(Cc * Cc + Ss * Ss);
  if (!(h > 0.0)) return false;
  const double co = Cc / h, si = Ss / h;
  // M maps candidate plane coordinates (f1, f2, n_c) to query plane coordinates (e1, e2, n_q)
  const double M[3][3] = {{co, rot ? -si : si, 0.0}, {si, rot ? co : -co, 0.0}, {0.0, 0.0, rot ? 1.0 : -1.0}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int a = 0; a < 3; ++a) {
        const double ma = (M[a][0] * F[0][j] + M[a][1] * F[1][j]) + M[a][2] * F[2][j];
        s += E[a][i] * ma;
      }
      T.R[3 * i + j] = s;
    }
  for (int i = 0; i < 3; ++i) T.t[i] = cq[i] - dot3(&T.R[3 * i], cc);
  return true;
}

// computeNormalisedError3D (loop_closer.cpp:700-716): sqrt(v^T (R cov_a R^T + cov_b)^-1 v), v = R X_a + t - X_b; the inverse as adjugate / det.
// transpose: use R^T and -R^T t (the candidate-from-query direction)
__device__ __forceinline__ double lf_error3d(const double* Xa, const double* ca, const double* Xb, const double* cb, const LfPose& T, bool transpose) {
  double R[9], t[3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = transpose ? T.R[3 * j + i] : T.R[3 * i + j];
  for (int i = 0; i < 3; ++i) t[i] = transpose ? -dot3(&R[3 * i], T.t) : T.t[i];
  const double A[3][3] = {{ca[0], ca[1], ca[2]}, {ca[1], ca[3], ca[4]}, {ca[2], ca[4], ca[5]}};
  double v[3], RA[3][3];
  for (int i = 0; i < 3; ++i) {
    v[i] = (dot3(&R[3 * i], Xa) + t[i]) - Xb[i];
    for (int j = 0; j < 3; ++j) RA[i][j] = (R[3 * i] * A[0][j] + R[3 * i + 1] * A[1][j]) + R[3 * i + 2] * A[2][j];
  }
  double S[6];   // xx xy xz yy yz zz of R A R^T + B
  int k = 0;
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j, ++k) S[k] = dot3(RA[i], &R[3 * j]) + cb[k];
  const double a00 = S[3] * S[5] - S[4] * S[4], a01 = S[2] * S[4] - S[1] * S[5], a02 = S[1] * S[4] - S[2] * S[3];
  const double a11 = S[0] * S[5] - S[2] * S[2], a12 = S[1] * S[2] - S[0] * S[4], a22 = S[0] * S[3] - S[1] * S[1];
  const double det = (S[0] * a00 + S[1] * a01) + S[2] * a02;
  const double w0 = (a00 * v[0] + a01 * v[1]) + a02 * v[2], w1 = (a01 * v[0] + a11 * v[1]) + a12 * v[2], w2 = (a02 * v[0] + a12 * v[1]) + a22 * v[2];
  return sqrt(((v[0] * w0 + v[1] * w1) + v[2] * w2) / det);
}

__device__ __forceinline__ bool lf_inlier(const double* d, const LfPose& T, double th) {   // d: Xq[3] covq[6] Xc[3] covc[6]
  const double e_c2q = lf_error3d(d + 9, d + 12, d, d + 3, T, false);
  const double e_q2c = lf_error3d(d, d + 3, d + 9, d + 12, T, true);
  return e_c2q < th && e_q2c < th;
}

__global__ __launch_bounds__(LT) void k_lf_ransac(const rgbid_loopfeat_kp* __restrict__ kps, int n_kf, int max_kp, const int* __restrict__ pairs,
                                                  const rgbid_loopfeat_corr* __restrict__ matches, const int* __restrict__ match_counts,
                                                  const double* __restrict__ u, int iters, double th, double* __restrict__ pose,
                                                  int* __restrict__ result, uint8_t* __restrict__ mask) {
  __shared__ double chunk[RCHUNK][18];
  __shared__ int best_cnt[LT], best_it[LT];
  __shared__ LfPose best_pose;
  __shared__ int winner;
  const int pair = blockIdx.x;
  const int q = pairs[2 * pair], c = pairs[2 * pair + 1];
  const bool ok = q >= 0 && q < n_kf && c >= 0 && c < n_kf;
  const int m = ok ? min(max(match_counts[pair], 0), max_kp) : 0;
  uint8_t* mk = mask + (size_t)pair * max_kp;
  for (int i = threadIdx.x; i < max_kp; i += LT) mk[i] = 0;
  if (m < 3) {   // uniform over the block
    if (threadIdx.x < 12) pose[(size_t)pair * 12 + threadIdx.x] = __longlong_as_double(0x7ff8000000000000ll);
    if (threadIdx.x == 0) { result[2 * pair] = -1; result[2 * pair + 1] = 0; }
    return;
  }
  const rgbid_loopfeat_kp* kq = kps + (size_t)q * max_kp;
  const rgbid_loopfeat_kp* kc = kps + (size_t)c * max_kp;
  const rgbid_loopfeat_corr* mt = matches + (size_t)pair * max_kp;
  int my_cnt = 0, my_it = -1;
  LfPose my_pose;
  for (int i = 0; i < 9; ++i) my_pose.R[i] = 0.0;
  for (int i = 0; i < 3; ++i) my_pose.t[i] = 0.0;
  for (int h0 = 0; h0 < iters; h0 += LT) {
    const int h = h0 + threadIdx.x;
    LfPose T;
    bool valid = h < iters;
    if (valid) {
      int s[3];
      lf_sample3(u + 3 * h, m, s);
      double Q[3][3], Cn[3][3];
      int qi[3], ti[3];
      for (int j = 0; j < 3; ++j) {
        const rgbid_loopfeat_corr mm = mt[min(max(s[j], 0), m - 1)];
        qi[j] = min(max(mm.query, 0), max_kp - 1); ti[j] = min(max(mm.train, 0), max_kp - 1);
        for (int a = 0; a < 3; ++a) { Q[j][a] = kq[qi[j]].X[a]; Cn[j][a] = kc[ti[j]].X[a]; }
      }
      // three matches that share a keypoint give a rank-deficient correlation: no hypothesis
      valid = qi[0] != qi[1] && qi[0] != qi[2] && qi[1] != qi[2] && ti[0] != ti[1] && ti[0] != ti[2] && ti[1] != ti[2];
      valid = valid && lf_pose3(Q, Cn, T);
    }
    int cnt = 0;
    for (int k0 = 0; k0 < m; k0 += RCHUNK) {
      const int nk = min(RCHUNK, m - k0);
      __syncthreads();
      for (int i = threadIdx.x; i < nk * 18; i += LT) {
        const int k = i / 18, f = i % 18;
        const rgbid_loopfeat_corr mm = mt[k0 + k];
        const rgbid_loopfeat_kp* kp = f < 9 ? &kq[min(max(mm.query, 0), max_kp - 1)] : &kc[min(max(mm.train, 0), max_kp - 1)];
        const int ff = f % 9;
        chunk[k][f] = ff < 3 ? kp->X[ff] : kp->cov[ff - 3];
      }
      __syncthreads();
      if (valid)
        for (int k = 0; k < nk; ++k) cnt += lf_inlier(chunk[k], T, th) ? 1 : 0;
    }
    if (valid && cnt > my_cnt) { my_cnt = cnt; my_it = h; my_pose = T; }   // strict: the lowest iteration of this thread stays
  }
  best_cnt[threadIdx.x] = my_cnt; best_it[threadIdx.x] = my_it;
  __syncthreads();
  if (threadIdx.x == 0) {
    int w = -1, wc = 0, wi = -1;
    for (int i = 0; i < LT; ++i)
      if (best_it[i] >= 0 && (best_cnt[i] > wc || (best_cnt[i] == wc && best_it[i] < wi))) { w = i; wc = best_cnt[i]; wi = best_it[i]; }
    winner = w;
    result[2 * pair] = wi; result[2 * pair + 1] = wc;
  }
  __syncthreads();
  const int w = winner;
  if (w < 0) {
    if (threadIdx.x < 12) pose[(size_t)pair * 12 + threadIdx.x] = __longlong_as_double(0x7ff8000000000000ll);
    return;
  }
  if ((int)threadIdx.x == w) best_pose = my_pose;
  __syncthreads();
  if (threadIdx.x < 12) pose[(size_t)pair * 12 + threadIdx.x] = threadIdx.x < 9 ? best_pose.R[threadIdx.x] : best_pose.t[threadIdx.x - 9];
  const LfPose T = best_pose;
  for (int k = threadIdx.x; k < m; k += LT) {
    const rgbid_loopfeat_corr mm = mt[k];
    const rgbid_loopfeat_kp* a = &kq[min(max(mm.query, 0), max_kp - 1)];
    const rgbid_loopfeat_kp* b = &kc[min(max(mm.train, 0), max_kp - 1)];
    double d[18];
    for (int f = 0; f < 3; ++f) { d[f] = a->X[f]; d[9 + f] = b->X[f]; }
    for (int f = 0; f < 6; ++f) { d[3 + f] = a->cov[f]; d[12 + f] = b->cov[f]; }
    mk[k] = lf_inlier(d, T, th) ? 1 : 0;
  }
}

// ---- host ----
int lf_alloc(void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return RGBID_OK;
  (void)hipGetLastError();
  *p = nullptr;
  return e == hipErrorOutOfMemory ? RGBID_E_NOMEM : (int)e;
}

#define RGBID_HIPC(expr)                                               \
  do {                                                                 \
    hipError_t e_ = (expr);                                            \
    if (e_ != hipSuccess) { (void)hipGetLastError(); return (int)e_; } \
  } while (0)

// the project's own test pattern: xorshift32 from 0x9E3779B9; a coordinate is (next % 27) - 13; a test is (x1, y1, x2, y2) with both points
// inside the disc of radius 13 and different from each other; the first 256 accepted tests, in order
void lf_pattern(int8_t* pattern) {
  uint32_t s = 0x9E3779B9u;
  auto next = [&]() { s ^= s << 13; s ^= s >> 17; s ^= s << 5; return s; };
  int n = 0;
  while (n < RGBID_LOOPFEAT_TESTS) {
    int v[4];
    for (int i = 0; i < 4; ++i) v[i] = (int)(next() % 27u) - 13;
    if (v[0] * v[0] + v[1] * v[1] > 169 || v[2] * v[2] + v[3] * v[3] > 169 || (v[0] == v[2] && v[1] == v[3])) continue;
    for (int i = 0; i < 4; ++i) pattern[4 * n + i] = (int8_t)v[i];
    ++n;
  }
}

}  // namespace

struct rgbid_loopfeat {
  rgbid_ctx* ctx = nullptr;
  LfGeom g{};
  float* resp = nullptr;
  LfStaged* staged = nullptr;
  int* cell_counts = nullptr;
  int cap_kf = 0;
  char4* rotated = nullptr;
  double* bounds = nullptr;
  bool timing = false;
  hipEvent_t ev[8] = {};   // 0-3 extract, 4-5 match, 6-7 ransac
  bool timed[3] = {false, false, false};
  void mark(int i) { if (timing) (void)hipEventRecord(ev[i], ctx->stream); }
};

extern "C" {

int rgbid_loopfeat_tables(int8_t* pattern, int8_t* rotated, double* bounds) {
  int8_t pat[RGBID_LOOPFEAT_TESTS * 4];
  lf_pattern(pat);
  if (pattern) memcpy(pattern, pat, sizeof(pat));
  const double pi = 3.14159265358979323846;
  if (rotated)
    for (int b = 0; b < RGBID_LOOPFEAT_DIRECTIONS; ++b) {
      const double a = (double)(2 * b) * pi / 32.0, c = std::cos(a), s = std::sin(a);
      for (int t = 0; t < RGBID_LOOPFEAT_TESTS * 2; ++t) {
        const double x = (double)pat[2 * t], y = (double)pat[2 * t + 1];
        rotated[(b * RGBID_LOOPFEAT_TESTS * 2 + t) * 2] = (int8_t)std::floor((c * x - s * y) + 0.5);
        rotated[(b * RGBID_LOOPFEAT_TESTS * 2 + t) * 2 + 1] = (int8_t)std::floor((s * x + c * y) + 0.5);
      }
    }
  if (bounds)
    for (int b = 0; b < 16; ++b) {
      const double a = (double)(2 * b + 1) * pi / 32.0;
      bounds[2 * b] = std::cos(a); bounds[2 * b + 1] = std::sin(a);
    }
  return RGBID_OK;
}

int rgbid_loopfeat_create(rgbid_loopfeat** out, rgbid_ctx* ctx, int rows, int cols, int max_keypoints) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || rows < 2 * BORDER + 1 || cols < 2 * BORDER + 1 || rows > 8192 || cols > 8192) return RGBID_E_INVALID;
  const int cells_x = (cols + CELL - 1) / CELL, cells_y = (rows + CELL - 1) / CELL, cells = cells_x * cells_y;
  if (max_keypoints < cells || max_keypoints > RGBID_LOOPFEAT_MAX_KEYPOINTS) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_loopfeat* f = new (std::nothrow) rgbid_loopfeat;
  if (!f) return RGBID_E_NOMEM;
  f->ctx = ctx;
  const int per_cell = max_keypoints / cells;
  f->g = LfGeom{rows, cols, cells_x, cells_y, per_cell < RGBID_LOOPFEAT_CELL_MAX ? per_cell : RGBID_LOOPFEAT_CELL_MAX, max_keypoints};
  int8_t rot[RGBID_LOOPFEAT_DIRECTIONS * RGBID_LOOPFEAT_TESTS * 4];
  double bounds[32];
  rgbid_loopfeat_tables(nullptr, rot, bounds);
  int r = lf_alloc((void**)&f->rotated, sizeof(rot));
  if (!r) r = lf_alloc((void**)&f->bounds, sizeof(bounds));
  if (!r) {   // pageable sources: the copies have left the host buffers when the calls return
    hipError_t e = hipMemcpy(f->rotated, rot, sizeof(rot), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(f->bounds, bounds, sizeof(bounds), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipGetLastError(); r = (int)e; }
  }
  if (r) { rgbid_loopfeat_destroy(f); return r; }
  *out = f;
  return RGBID_OK;
}

int rgbid_loopfeat_destroy(rgbid_loopfeat* f) {
  if (!f) return RGBID_OK;
  (void)hipSetDevice(f->ctx->device);
  if (f->ctx->stream) (void)hipStreamSynchronize(f->ctx->stream);
  for (void* p : {(void*)f->resp, (void*)f->staged, (void*)f->cell_counts, (void*)f->rotated, (void*)f->bounds})
    if (p) (void)hipFree(p);
  for (hipEvent_t e : f->ev) if (e) (void)hipEventDestroy(e);
  (void)hipGetLastError();
  delete f;
  return RGBID_OK;
}

int rgbid_loopfeat_layout(const rgbid_loopfeat* f, int* cells_x, int* cells_y, int* per_cell) {
  if (!f) return RGBID_E_INVALID;
  if (cells_x) *cells_x = f->g.cells_x;
  if (cells_y) *cells_y = f->g.cells_y;
  if (per_cell) *per_cell = f->g.per_cell;
  return RGBID_OK;
}

int rgbid_loopfeat_extract(rgbid_loopfeat* f, const uint8_t* grey_dev, const float* invdepth_dev, int n, const float K[4],
                           rgbid_loopfeat_kp* kps_dev, int32_t* counts_dev) {
  if (!f || n < 0 || n > 65535 || !K) return RGBID_E_INVALID;
  if (n == 0) return RGBID_OK;
  if (!grey_dev || !invdepth_dev || !kps_dev || !counts_dev || (((uintptr_t)kps_dev) & 7)) return RGBID_E_INVALID;
  for (int i = 0; i < 4; ++i) if (!std::isfinite(K[i])) return RGBID_E_INVALID;
  if (K[0] == 0.f || K[1] == 0.f) return RGBID_E_INVALID;
  (void)hipSetDevice(f->ctx->device);
  hipStream_t s = f->ctx->stream;
  const LfGeom g = f->g;
  const int cells = g.cells_x * g.cells_y;
  if (n > f->cap_kf) {
    RGBID_HIPC(hipStreamSynchronize(s));
    for (void* p : {(void*)f->resp, (void*)f->staged, (void*)f->cell_counts}) if (p) (void)hipFree(p);
    f->resp = nullptr; f->staged = nullptr; f->cell_counts = nullptr; f->cap_kf = 0;
    int r = lf_alloc((void**)&f->resp, sizeof(float) * (size_t)n * g.rows * g.cols);
    if (!r) r = lf_alloc((void**)&f->staged, sizeof(LfStaged) * (size_t)n * cells * g.per_cell);
    if (!r) r = lf_alloc((void**)&f->cell_counts, sizeof(int) * (size_t)n * cells);
    if (r) return r;
    f->cap_kf = n;
  }
  LfKinv Ki;
  rgbid_cloud_kinv(K, Ki.m);
  const float scale = 1.f / (4 * 7 * 255.f);
  const float scale4 = ((scale * scale) * scale) * scale;
  f->timed[0] = false;
  f->mark(0);
  RGBID_HIPC(hipMemsetAsync(kps_dev, 0, sizeof(rgbid_loopfeat_kp) * (size_t)n * g.max_kp, s));
  hipLaunchKernelGGL(k_lf_response, dim3((g.cols + 15) / 16, (g.rows + 15) / 16, n), dim3(LT), 0, s, grey_dev, g, scale4, f->resp);
  f->mark(1);
  hipLaunchKernelGGL(k_lf_select, dim3(cells, n), dim3(LT), 0, s, f->resp, invdepth_dev, g, f->staged, f->cell_counts);
  f->mark(2);
  hipLaunchKernelGGL(k_lf_describe, dim3((cells * g.per_cell + 3) / 4, n), dim3(LT), 0, s, grey_dev, invdepth_dev, g, Ki, f->staged,
                     f->cell_counts, f->rotated, f->bounds, kps_dev, counts_dev);
  f->mark(3);
  f->timed[0] = f->timing;
  RGBID_HIPC(hipGetLastError());
  return RGBID_OK;
}

int rgbid_loopfeat_match(rgbid_loopfeat* f, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, const int32_t* pairs_dev,
                         int n_pairs, float ratio, rgbid_loopfeat_corr* matches_dev, int32_t* match_counts_dev) {
  if (!f || n_kf < 0 || n_pairs < 0 || !(std::isfinite(ratio) && ratio > 0.f)) return RGBID_E_INVALID;
  if (n_pairs == 0) return RGBID_OK;
  if (!kps_dev || !counts_dev || !pairs_dev || !match_counts_dev || n_kf == 0 || (((uintptr_t)kps_dev) & 7) || (((uintptr_t)matches_dev) & 15))
    return RGBID_E_INVALID;
  (void)hipSetDevice(f->ctx->device);
  hipStream_t s = f->ctx->stream;
  f->timed[1] = false;
  f->mark(4);
  hipLaunchKernelGGL(k_lf_match, dim3(n_pairs), dim3(LT), sizeof(unsigned long long) * 4 * (size_t)f->g.max_kp, s, kps_dev, counts_dev, n_kf,
                     f->g.max_kp, pairs_dev, ratio, matches_dev, match_counts_dev);
  f->mark(5);
  f->timed[1] = f->timing;
  RGBID_HIPC(hipGetLastError());
  return RGBID_OK;
}

int rgbid_loopfeat_ransac(rgbid_loopfeat* f, const rgbid_loopfeat_kp* kps_dev, int n_kf, const int32_t* pairs_dev, int n_pairs,
                          const rgbid_loopfeat_corr* matches_dev, const int32_t* match_counts_dev, const double* u_dev, int iters,
                          double threshold, double* pose_dev, int32_t* result_dev, uint8_t* mask_dev) {
  if (!f || n_kf < 0 || n_pairs < 0 || iters < 1 || iters > RGBID_LOOPFEAT_MAX_ITERS || !(std::isfinite(threshold) && threshold > 0.0))
    return RGBID_E_INVALID;
  if (n_pairs == 0) return RGBID_OK;
  if (!kps_dev || !pairs_dev || !matches_dev || !match_counts_dev || !u_dev || !pose_dev || !result_dev || !mask_dev || n_kf == 0 ||
      (((uintptr_t)kps_dev) & 7) || (((uintptr_t)matches_dev) & 15) || (((uintptr_t)u_dev) & 7) || (((uintptr_t)pose_dev) & 7))
    return RGBID_E_INVALID;
  (void)hipSetDevice(f->ctx->device);
  hipStream_t s = f->ctx->stream;
  f->timed[2] = false;
  f->mark(6);
  hipLaunchKernelGGL(k_lf_ransac, dim3(n_pairs), dim3(LT), 0, s, kps_dev, n_kf, f->g.max_kp, pairs_dev, matches_dev, match_counts_dev, u_dev,
                     iters, threshold, pose_dev, result_dev, mask_dev);
  f->mark(7);
  f->timed[2] = f->timing;
  RGBID_HIPC(hipGetLastError());
  return RGBID_OK;
}

int rgbid_loopfeat_timing(rgbid_loopfeat* f, int enable, float ms[5]) {
  if (!f) return RGBID_E_INVALID;
  (void)hipSetDevice(f->ctx->device);
  if (ms) {
    for (int i = 0; i < 5; ++i) ms[i] = 0.f;
    const int a[5] = {0, 1, 2, 4, 6}, grp[5] = {0, 0, 0, 1, 2};
    for (int i = 0; i < 5; ++i)
      if (f->timed[grp[i]]) {
        RGBID_HIPC(hipEventSynchronize(f->ev[a[i] + 1]));
        RGBID_HIPC(hipEventElapsedTime(&ms[i], f->ev[a[i]], f->ev[a[i] + 1]));
      }
  }
  if (enable && !f->ev[0])
    for (hipEvent_t& e : f->ev) RGBID_HIPC(hipEventCreate(&e));
  f->timing = enable != 0;
  return RGBID_OK;
}

}  // extern "C"
