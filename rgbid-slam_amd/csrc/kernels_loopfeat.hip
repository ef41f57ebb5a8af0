// kernels_loopfeat.hip -- appearance stage of loop closure (include/rgbid_loopfeat.h; LoopCloser::detectLoopClosures and
// computeRANSACTrafo3D, src/loop_closer.cpp:193-716; Keyframe::lift2DKeypointsto3DPointsWithCovariance, src/keyframe.cpp:232-274).
//
//   features  k_lf_pyramid    level l of the scale pyramid from level l - 1 (extractors of several levels): integer bilinear, 4 pixels per thread
//             the three kernels below run once over all levels: a flat grid over (level, tile | cell | slot) x keyframe, the level from a table
//             k_lf_response   Harris response per pixel: a 24 x 24 grey tile and its 22 x 22 integer derivatives in LDS, 49 products per pixel
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
#include "hip_host.h"
#include "wave_device.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#pragma clang fp contract(off)

using namespace rgbid;

static_assert(sizeof(rgbid_loopfeat_kp) == 120, "rgbid_loopfeat_kp is 120 bytes");
static_assert(offsetof(rgbid_loopfeat_kp, desc) == 16 && offsetof(rgbid_loopfeat_kp, X) == 48 && offsetof(rgbid_loopfeat_kp, cov) == 72, "record layout");
static_assert(sizeof(rgbid_loopfeat_corr) == 16, "rgbid_loopfeat_corr is 16 bytes");
static_assert(sizeof(rgbid_loopfeat_aux) == 16 && offsetof(rgbid_loopfeat_aux, level) == 12, "rgbid_loopfeat_aux is 16 bytes");

namespace {

constexpr int LT = 256;                              // threads per block
constexpr int CELL = RGBID_LOOPFEAT_CELL;
constexpr int BORDER = RGBID_LOOPFEAT_BORDER;
constexpr int CELL_CAND = (CELL / 2) * (CELL / 2);   // no two 8-neighbours are both strict maxima: at most one per 2 x 2 block
constexpr int PATCH = 2 * BORDER + 1;                // 33
constexpr int RCHUNK = 128;                          // matches per LDS chunk of the vote
constexpr int HARRIS_R = 3;                          // 7 x 7 block
constexpr int RESP_MARGIN = HARRIS_R + 1;
constexpr int MAXL = RGBID_LOOPFEAT_MAX_LEVELS;

// one pyramid level: its image, its cells and where its tiles, cells, staging slots and describe blocks start in the grids over all levels
struct LfLevel {
  int rows, cols, cells_x, cells_y, per_cell;
  float s;                                       // (float) pow(scale, level): level pixel -> level-0 pixel
  int img_off, resp_off;                         // per keyframe: bytes into the pyramid scratch (levels >= 1), floats into the response scratch
  int cell_off, slot_off;                        // cells and staging slots of the levels below
  int tiles_x, tile_off, dblock_off;             // response tiles of 16 x 16 and describe blocks of the levels below
};
struct LfGeom { int rows, cols, levels, max_kp, cells, slots, resp_stride, pyr_stride; };   // level 0's size; totals over the levels; per-keyframe strides
struct LfKinv { double m[9]; };
struct LfStaged { int idx; float resp; };

// the level whose range of a flat grid holds block b (uniform over the block: scalar loads of a table of at most 8 entries)
__device__ __forceinline__ int lf_level_of(const LfLevel* __restrict__ lv, int levels, int b, int LfLevel::*off) {
  int l = levels - 1;
  while (l > 0 && b < lv[l].*off) --l;
  return l;
}

__device__ __forceinline__ const uint8_t* lf_image(const uint8_t* grey, const uint8_t* pyr, const LfGeom& g, const LfLevel& lv, int level, int kf) {
  return level == 0 ? grey + (size_t)kf * g.rows * g.cols : pyr + (size_t)kf * g.pyr_stride + lv.img_off;
}

// ---- features ----
// level l from level l - 1: bilinear with 11-bit weights from the host's (x0, w1) tables, in int32.  A thread makes 4 consecutive pixels of the
// destination image taken as one flat array (they may run over a row end) and stores them as one word; the image's slot in the scratch is
// padded to a multiple of 4 bytes, so the last word stays inside it.
__global__ __launch_bounds__(LT) void k_lf_pyramid(const uint8_t* __restrict__ src, size_t src_stride, int srows, int scols, uint8_t* __restrict__ dst,
                                                   size_t dst_stride, int drows, int dcols, const int2* __restrict__ xtab, const int2* __restrict__ ytab) {
  const int kf = blockIdx.y, i0 = 4 * (blockIdx.x * LT + threadIdx.x), dpx = drows * dcols;
  if (i0 >= dpx) return;
  const uint8_t* S = src + (size_t)kf * src_stride;
  int y = i0 / dcols, x = i0 - y * dcols;
  unsigned word = 0;
  for (int k = 0; k < 4 && i0 + k < dpx; ++k) {
    const int2 tx = xtab[x], ty = ytab[y];
    const int x1 = min(tx.x + 1, scols - 1), y1 = min(ty.x + 1, srows - 1);
    const int w1x = tx.y, w0x = 2048 - w1x, w1y = ty.y, w0y = 2048 - w1y;
    const uint8_t* r0 = S + (size_t)ty.x * scols;
    const uint8_t* r1 = S + (size_t)y1 * scols;
    const int top = w0x * r0[tx.x] + w1x * r0[x1], bot = w0x * r1[tx.x] + w1x * r1[x1];
    const int v = (w0y * top + w1y * bot + (1 << 21)) >> 22;
    word |= (unsigned)v << (8 * k);
    if (++x == dcols) { x = 0; ++y; }
  }
  *reinterpret_cast<unsigned*>(dst + (size_t)kf * dst_stride + i0) = word;
}

// 7 waves per SIMD as with one level: without the hint the allocator takes 88 VGPRs (5 waves) for the same loops
__global__ __launch_bounds__(LT) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_lf_response(const uint8_t* __restrict__ grey, const uint8_t* __restrict__ pyr, LfGeom g,
                                                    const LfLevel* __restrict__ levels, float scale4, float* __restrict__ resp) {
  __shared__ int tile[24][24];
  __shared__ short dIx[22][22], dIy[22][22];
  const int level = lf_level_of(levels, g.levels, blockIdx.x, &LfLevel::tile_off);
  const LfLevel lv = levels[level];
  const int t = blockIdx.x - lv.tile_off;
  const int kf = blockIdx.y, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int x0 = (t % lv.tiles_x) * 16, y0 = (t / lv.tiles_x) * 16;
  const uint8_t* img = lf_image(grey, pyr, g, lv, level, kf);
  for (int i = threadIdx.x; i < 24 * 24; i += LT) {
    const int ly = i / 24, lx = i % 24;
    const int y = min(max(y0 + ly - RESP_MARGIN, 0), lv.rows - 1), x = min(max(x0 + lx - RESP_MARGIN, 0), lv.cols - 1);   // clamped reads feed only refused pixels
    tile[ly][lx] = img[(size_t)y * lv.cols + x];
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
  if (x >= lv.cols || y >= lv.rows) return;
  float r = 0.f;
  if (x >= RESP_MARGIN && x < lv.cols - RESP_MARGIN && y >= RESP_MARGIN && y < lv.rows - RESP_MARGIN) {
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
  resp[(size_t)kf * g.resp_stride + lv.resp_off + (size_t)y * lv.cols + x] = r;
}

// a beats b: larger response, or equal response and smaller raster index
__device__ __forceinline__ bool lf_beats(float ra, int ia, float rb, int ib) { return ra > rb || (ra == rb && ia < ib); }

// the level-0 pixel whose depth a keypoint at coordinate v of a level reads: (int) ((double) ((float) v * s) + 0.5); p receives the float product
__device__ __forceinline__ int lf_pixel0(int v, float s, float* p) {
  *p = (float)v * s;
  return (int)((double)*p + 0.5);
}

__global__ __launch_bounds__(LT) void k_lf_select(const float* __restrict__ resp, const float* __restrict__ invdepth, LfGeom g,
                                                  const LfLevel* __restrict__ levels, LfStaged* __restrict__ staged, int* __restrict__ cell_counts) {
  __shared__ int cnt;
  __shared__ float cr[CELL_CAND];
  __shared__ int ci[CELL_CAND];
  const int level = lf_level_of(levels, g.levels, blockIdx.x, &LfLevel::cell_off);
  const LfLevel lv = levels[level];
  const int kf = blockIdx.y, cell = blockIdx.x - lv.cell_off;
  const int cx = cell % lv.cells_x, cy = cell / lv.cells_x;
  const float* R = resp + (size_t)kf * g.resp_stride + lv.resp_off;
  const float* W = invdepth + (size_t)kf * g.rows * g.cols;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  for (int p = threadIdx.x; p < CELL * CELL; p += LT) {
    const int x = cx * CELL + p % CELL, y = cy * CELL + p / CELL;
    if (x < BORDER || x >= lv.cols - BORDER || y < BORDER || y >= lv.rows - BORDER) continue;   // the 8 neighbours are inside the image
    const int idx = y * lv.cols + x;
    const float r = R[idx];
    if (!(r > 0.f)) continue;
    bool is_max = true;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (dx == 0 && dy == 0) continue;
        const int j = idx + dy * lv.cols + dx;
        is_max = is_max && lf_beats(r, idx, R[j], j);
      }
    if (!is_max) continue;
    float pf;
    const int X0 = lf_pixel0(x, lv.s, &pf), Y0 = lf_pixel0(y, lv.s, &pf);
    if (X0 >= g.cols || Y0 >= g.rows) continue;
    const float w = W[(size_t)Y0 * g.cols + X0];
    if (!(isfinite(w) && w > 0.f)) continue;
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
    if (rank < lv.per_cell) staged[(size_t)kf * g.slots + lv.slot_off + cell * lv.per_cell + rank] = LfStaged{idx, r};
  }
  if (threadIdx.x == 0) cell_counts[(size_t)kf * g.cells + blockIdx.x] = min(nc, lv.per_cell);
}

__device__ __forceinline__ int lf_box(const uint8_t* patch, int px, int py) {
  int s = 0;
  for (int dy = -2; dy <= 2; ++dy)
    for (int dx = -2; dx <= 2; ++dx) s += patch[(py + dy + BORDER) * PATCH + (px + dx + BORDER)];
  return s;
}

__global__ __launch_bounds__(LT) void k_lf_describe(const uint8_t* __restrict__ grey, const uint8_t* __restrict__ pyr,
                                                    const float* __restrict__ invdepth, LfGeom g, const LfLevel* __restrict__ levels, LfKinv Ki,
                                                    const LfStaged* __restrict__ staged, const int* __restrict__ cell_counts,
                                                    const char4* __restrict__ rotated, const double* __restrict__ bounds,
                                                    rgbid_loopfeat_kp* __restrict__ kps, int* __restrict__ counts, rgbid_loopfeat_aux* __restrict__ aux) {
  __shared__ uint8_t patches[LT / 64][PATCH * PATCH + 7];
  const int level = lf_level_of(levels, g.levels, blockIdx.x, &LfLevel::dblock_off);
  const LfLevel lv = levels[level];
  const int kf = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = (blockIdx.x - lv.dblock_off) * (LT / 64) + wave;   // within the level
  const int cell = slot / lv.per_cell, rank = slot % lv.per_cell;
  const int* cc = cell_counts + (size_t)kf * g.cells;
  const bool in_table = slot < lv.cells_x * lv.cells_y * lv.per_cell;
  int before = 0;   // keypoints of the levels below and of this level's cells before this one
  if (in_table)
    for (int c = lane; c < lv.cell_off + cell; c += 64) before += cc[c];
  before = wave_sum(before);
  if (blockIdx.x == 0 && wave == 0) {   // the first wave of a keyframe also writes its keypoint count
    int total = 0;
    for (int c = lane; c < g.cells; c += 64) total += cc[c];
    total = wave_sum(total);
    if (lane == 0) counts[kf] = total;
  }
  const bool active = in_table && rank < cc[lv.cell_off + cell];
  uint8_t* patch = patches[wave];
  const uint8_t* img = lf_image(grey, pyr, g, lv, level, kf);
  int idx = 0, x = BORDER, y = BORDER;
  float response = 0.f;
  if (active) {
    const LfStaged st = staged[(size_t)kf * g.slots + lv.slot_off + cell * lv.per_cell + rank];
    idx = st.idx; response = st.resp; x = idx % lv.cols; y = idx / lv.cols;   // BORDER <= x < cols - BORDER and the same for y: the patch is inside
    for (int i = lane; i < PATCH * PATCH; i += 64) patch[i] = img[(size_t)(y + i / PATCH - BORDER) * lv.cols + (x + i % PATCH - BORDER)];
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
  const size_t rec = (size_t)kf * g.max_kp + before + rank;   // before + rank < sum over levels of cells x per_cell <= max_kp
  rgbid_loopfeat_kp* out = kps + rec;
  uint8_t* desc = out->desc;
  for (int j = 0; j < 4; ++j) {
    const char4 p = rotated[dir * RGBID_LOOPFEAT_TESTS + j * 64 + lane];
    const bool bit = lf_box(patch, p.x, p.y) < lf_box(patch, p.z, p.w);
    const unsigned long long m = __ballot(bit);
    if (lane < 8) desc[j * 8 + lane] = (uint8_t)(m >> (8 * lane));
  }
  if (lane == 0) {
    float pxf, pyf;
    const int X0 = lf_pixel0(x, lv.s, &pxf), Y0 = lf_pixel0(y, lv.s, &pyf);   // the select kernel has checked them against the level-0 size
    out->x = X0; out->y = Y0; out->response = response; out->direction = dir;
    if (aux) aux[rec] = rgbid_loopfeat_aux{pxf, pyf, (int16_t)x, (int16_t)y, level};
    const float w = invdepth[((size_t)kf * g.rows + Y0) * g.cols + X0];
    const double d = (double)(1.f / w), px = (double)pxf, py = (double)pyf, pz = 1.0;
    const double inv_d = 1.0 / d;
    const float var = ((lv.s * lv.s) * 0.5f) * 0.5f;   // the pixel variance 0.25 widened by scale^(2 level), formed in float
    const double s[3] = {(double)var, (double)var, (double)(0.00025f * 0.00025f)};
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
  const int pair = blockIdx.x;
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
    unsigned total;
    const unsigned pos = running + block_rank(keep, wtot, total);
    if (keep && out) out[pos] = rgbid_loopfeat_corr{i, i0, d0, d1};   // pos < nq <= max_kp
    running += total;
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


// the levels that exist and each one's cells and share of the keypoints (the header's "level geometry" and "budget per level")
struct LfPlan { int levels; int rows[MAXL], cols[MAXL], cells_x[MAXL], cells_y[MAXL], per_cell[MAXL]; float s[MAXL]; };

int lf_plan(int rows, int cols, int max_keypoints, int levels, float scale, LfPlan& p) {
  if (rows < 2 * BORDER + 1 || cols < 2 * BORDER + 1 || rows > 8192 || cols > 8192) return RGBID_E_INVALID;
  if (levels < 1 || levels > MAXL || !(scale > 1.f && scale <= 2.f)) return RGBID_E_INVALID;
  if (max_keypoints < 1 || max_keypoints > RGBID_LOOPFEAT_MAX_KEYPOINTS) return RGBID_E_INVALID;
  p.levels = 0;
  for (int l = 0; l < levels; ++l) {
    const float s = (float)std::pow((double)scale, (double)l);
    const int c = (int)(((float)cols + 0.5f) / s), r = (int)(((float)rows + 0.5f) / s);
    if (r < 2 * BORDER + 1 || c < 2 * BORDER + 1) break;
    p.rows[l] = r; p.cols[l] = c; p.s[l] = s;
    p.cells_x[l] = (c + CELL - 1) / CELL; p.cells_y[l] = (r + CELL - 1) / CELL;
    p.levels = l + 1;
  }
  const double sd = (double)scale, r = 1.0 / (sd * sd);
  double rL = 1.0;
  for (int l = 0; l < p.levels; ++l) rL *= r;
  double rl = 1.0;
  long long slots = 0;
  for (int l = 0; l < p.levels; ++l, rl *= r) {
    const int n = (int)std::floor((double)max_keypoints * (((1.0 - r) * rl) / (1.0 - rL)));   // one level: exactly max_keypoints
    const int cells = p.cells_x[l] * p.cells_y[l];
    const int k = n / cells < 1 ? 1 : n / cells;
    p.per_cell[l] = k < RGBID_LOOPFEAT_CELL_MAX ? k : RGBID_LOOPFEAT_CELL_MAX;
    slots += (long long)cells * p.per_cell[l];
  }
  return slots > max_keypoints ? RGBID_E_INVALID : RGBID_OK;
}

}  // namespace

struct rgbid_loopfeat {
  rgbid_ctx* ctx = nullptr;
  LfGeom g{};
  LfLevel lv[MAXL] = {};
  int tiles = 0, dblocks = 0;        // response tiles and describe blocks over all levels
  int tab_off[MAXL][2] = {};         // level l's column and row resize tables in `tabs`
  float* resp = nullptr;
  LfStaged* staged = nullptr;
  int* cell_counts = nullptr;
  uint8_t* pyr = nullptr;            // levels 1 .. L - 1 of cap_kf keyframes
  int cap_kf = 0;
  char4* rotated = nullptr;
  double* bounds = nullptr;
  LfLevel* levels_dev = nullptr;
  int2* tabs = nullptr;
  Buffers tables, scratch;  // what create made; what lf_reserve makes for cap_kf keyframes
  StageTimer<10> timer;     // 0-3 extract, 4-5 match, 6-7 ransac, 8-9 pyramid
  bool timed[4] = {false, false, false, false};
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

// scratch for n keyframes
int lf_reserve(rgbid_loopfeat* f, int n) {
  if (n <= f->cap_kf) return RGBID_OK;
  RGBID_HIP(hipStreamSynchronize(f->ctx->stream));
  f->scratch.release();
  f->resp = nullptr; f->staged = nullptr; f->cell_counts = nullptr; f->pyr = nullptr; f->cap_kf = 0;
  const LfGeom& g = f->g;
  int r = f->scratch.alloc(&f->resp, sizeof(float) * (size_t)n * g.resp_stride);
  if (!r) r = f->scratch.alloc(&f->staged, sizeof(LfStaged) * (size_t)n * g.slots);
  if (!r) r = f->scratch.alloc(&f->cell_counts, sizeof(int) * (size_t)n * g.cells);
  if (!r && g.pyr_stride) r = f->scratch.alloc(&f->pyr, (size_t)n * g.pyr_stride);
  if (r) return r;
  f->cap_kf = n;
  return RGBID_OK;
}

// levels 1 .. upto of n keyframes into the scratch, each from the level below
void lf_build_pyramid(rgbid_loopfeat* f, const uint8_t* grey_dev, int n, int upto) {
  const LfGeom& g = f->g;
  for (int l = 1; l <= upto; ++l) {
    const LfLevel &a = f->lv[l - 1], &b = f->lv[l];
    const uint8_t* src = l == 1 ? grey_dev : f->pyr + a.img_off;
    const size_t src_stride = l == 1 ? (size_t)g.rows * g.cols : (size_t)g.pyr_stride;
    const int words = (b.rows * b.cols + 3) / 4;
    hipLaunchKernelGGL(k_lf_pyramid, dim3((words + LT - 1) / LT, n), dim3(LT), 0, f->ctx->stream, src, src_stride, a.rows, a.cols, f->pyr + b.img_off,
                       (size_t)g.pyr_stride, b.rows, b.cols, f->tabs + f->tab_off[l][0], f->tabs + f->tab_off[l][1]);
  }
}

}  // namespace

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

int rgbid_loopfeat_resize_table(int src, int dst, int32_t* x0, int32_t* w1) {
  if (src < 1 || dst < 1 || !x0 || !w1) return RGBID_E_INVALID;
  const double ratio = (double)src / (double)dst;
  for (int d = 0; d < dst; ++d) {
    const double fx = ((double)d + 0.5) * ratio - 0.5;
    const double fl = std::floor(fx);
    int i = (int)fl, w = (int)std::floor((fx - fl) * 2048.0 + 0.5);
    if (i < 0) { i = 0; w = 0; }
    if (i >= src - 1) { i = src - 1; w = 0; }
    x0[d] = i; w1[d] = w;
  }
  return RGBID_OK;
}

int rgbid_loopfeat_plan_levels(int rows, int cols, int max_keypoints, int levels, float scale, int32_t* existing, int32_t* geometry, float* scale_l) {
  LfPlan p;
  const int r = lf_plan(rows, cols, max_keypoints, levels, scale, p);
  if (r) return r;
  if (existing) *existing = p.levels;
  for (int l = 0; l < p.levels; ++l) {
    if (geometry) {
      const int v[5] = {p.rows[l], p.cols[l], p.cells_x[l], p.cells_y[l], p.per_cell[l]};
      for (int i = 0; i < 5; ++i) geometry[5 * l + i] = v[i];
    }
    if (scale_l) scale_l[l] = p.s[l];
  }
  return RGBID_OK;
}

int rgbid_loopfeat_create(rgbid_loopfeat** out, rgbid_ctx* ctx, int rows, int cols, int max_keypoints) {
  return rgbid_loopfeat_create_levels(out, ctx, rows, cols, max_keypoints, 1, 1.2f);
}

int rgbid_loopfeat_create_levels(rgbid_loopfeat** out, rgbid_ctx* ctx, int rows, int cols, int max_keypoints, int levels, float scale) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  LfPlan p;
  if (!ctx || lf_plan(rows, cols, max_keypoints, levels, scale, p)) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_loopfeat* f = new (std::nothrow) rgbid_loopfeat;
  if (!f) return RGBID_E_NOMEM;
  f->ctx = ctx;
  LfGeom& g = f->g;
  g = LfGeom{rows, cols, p.levels, max_keypoints, 0, 0, 0, 0};
  int ntab = 0;
  for (int l = 0; l < p.levels; ++l) {
    LfLevel& v = f->lv[l];
    v = LfLevel{p.rows[l], p.cols[l], p.cells_x[l], p.cells_y[l], p.per_cell[l], p.s[l], l ? g.pyr_stride : 0, g.resp_stride, g.cells, g.slots,
                (p.cols[l] + 15) / 16, f->tiles, f->dblocks};
    const int px = p.rows[l] * p.cols[l], cells = v.cells_x * v.cells_y;
    if (l) g.pyr_stride += (px + 3) / 4 * 4;   // each image starts on a word and ends before the next one
    g.resp_stride += px; g.cells += cells; g.slots += cells * v.per_cell;
    f->tiles += v.tiles_x * ((v.rows + 15) / 16);
    f->dblocks += (cells * v.per_cell + 3) / 4;
    f->tab_off[l][0] = ntab; f->tab_off[l][1] = ntab + (l ? v.cols : 0);
    if (l) ntab += v.cols + v.rows;
  }
  int8_t rot[RGBID_LOOPFEAT_DIRECTIONS * RGBID_LOOPFEAT_TESTS * 4];
  double bounds[32];
  rgbid_loopfeat_tables(nullptr, rot, bounds);
  int2* tabs = ntab ? new (std::nothrow) int2[ntab] : nullptr;
  int32_t* tmp = ntab ? new (std::nothrow) int32_t[2 * 8192] : nullptr;
  int r = (ntab && (!tabs || !tmp)) ? RGBID_E_NOMEM : RGBID_OK;
  for (int l = 1; l < p.levels && !r; ++l)
    for (int axis = 0; axis < 2; ++axis) {
      const int src = axis ? p.rows[l - 1] : p.cols[l - 1], dst = axis ? p.rows[l] : p.cols[l];
      rgbid_loopfeat_resize_table(src, dst, tmp, tmp + 8192);
      for (int d = 0; d < dst; ++d) tabs[f->tab_off[l][axis] + d] = make_int2(tmp[d], tmp[8192 + d]);
    }
  if (!r) r = f->tables.alloc(&f->rotated, sizeof(rot));
  if (!r) r = f->tables.alloc(&f->bounds, sizeof(bounds));
  if (!r) r = f->tables.alloc(&f->levels_dev, sizeof(LfLevel) * MAXL);
  if (!r && ntab) r = f->tables.alloc(&f->tabs, sizeof(int2) * (size_t)ntab);
  if (!r) {   // pageable sources: the copies have left the host buffers when the calls return
    hipError_t e = hipMemcpy(f->rotated, rot, sizeof(rot), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(f->bounds, bounds, sizeof(bounds), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(f->levels_dev, f->lv, sizeof(LfLevel) * MAXL, hipMemcpyHostToDevice);
    if (e == hipSuccess && ntab) e = hipMemcpy(f->tabs, tabs, sizeof(int2) * (size_t)ntab, hipMemcpyHostToDevice);
    r = hip_status(e);
  }
  delete[] tabs;
  delete[] tmp;
  if (r) { rgbid_loopfeat_destroy(f); return r; }
  *out = f;
  return RGBID_OK;
}

int rgbid_loopfeat_destroy(rgbid_loopfeat* f) { return destroy_handle(f); }

int rgbid_loopfeat_layout(const rgbid_loopfeat* f, int* cells_x, int* cells_y, int* per_cell) {
  return rgbid_loopfeat_level_layout(f, 0, nullptr, nullptr, cells_x, cells_y, per_cell, nullptr);
}

int rgbid_loopfeat_level_layout(const rgbid_loopfeat* f, int level, int* rows_l, int* cols_l, int* cells_x, int* cells_y, int* per_cell,
                                float* scale_l) {
  if (!f || level < 0 || level >= f->g.levels) return RGBID_E_INVALID;
  const LfLevel& v = f->lv[level];
  if (rows_l) *rows_l = v.rows;
  if (cols_l) *cols_l = v.cols;
  if (cells_x) *cells_x = v.cells_x;
  if (cells_y) *cells_y = v.cells_y;
  if (per_cell) *per_cell = v.per_cell;
  if (scale_l) *scale_l = v.s;
  return RGBID_OK;
}

int rgbid_loopfeat_pyramid(rgbid_loopfeat* f, const uint8_t* grey_dev, int n, int level, uint8_t* out_dev) {
  if (!f || n < 0 || n > 65535 || level < 0 || level >= f->g.levels) return RGBID_E_INVALID;
  if (n == 0) return RGBID_OK;
  if (!grey_dev || !out_dev) return RGBID_E_INVALID;
  (void)hipSetDevice(f->ctx->device);
  hipStream_t s = f->ctx->stream;
  const LfGeom& g = f->g;
  if (level == 0) {
    RGBID_HIP(hipMemcpyAsync(out_dev, grey_dev, (size_t)n * g.rows * g.cols, hipMemcpyDeviceToDevice, s));
    return RGBID_OK;
  }
  const int r = lf_reserve(f, n);
  if (r) return r;
  lf_build_pyramid(f, grey_dev, n, level);
  RGBID_HIP(hipGetLastError());
  const size_t px = (size_t)f->lv[level].rows * f->lv[level].cols;
  RGBID_HIP(hipMemcpy2DAsync(out_dev, px, f->pyr + f->lv[level].img_off, (size_t)g.pyr_stride, px, (size_t)n, hipMemcpyDeviceToDevice, s));
  return RGBID_OK;
}

int rgbid_loopfeat_extract(rgbid_loopfeat* f, const uint8_t* grey_dev, const float* invdepth_dev, int n, const float K[4],
                           rgbid_loopfeat_kp* kps_dev, int32_t* counts_dev) {
  return rgbid_loopfeat_extract_levels(f, grey_dev, invdepth_dev, n, K, kps_dev, counts_dev, nullptr);
}

int rgbid_loopfeat_extract_levels(rgbid_loopfeat* f, const uint8_t* grey_dev, const float* invdepth_dev, int n, const float K[4],
                                  rgbid_loopfeat_kp* kps_dev, int32_t* counts_dev, rgbid_loopfeat_aux* aux_dev) {
  if (!f || n < 0 || n > 65535 || !K) return RGBID_E_INVALID;
  if (n == 0) return RGBID_OK;
  if (!grey_dev || !invdepth_dev || !kps_dev || !counts_dev || (((uintptr_t)kps_dev) & 7) || (((uintptr_t)aux_dev) & 3)) return RGBID_E_INVALID;
  for (int i = 0; i < 4; ++i) if (!std::isfinite(K[i])) return RGBID_E_INVALID;
  if (K[0] == 0.f || K[1] == 0.f) return RGBID_E_INVALID;
  (void)hipSetDevice(f->ctx->device);
  hipStream_t s = f->ctx->stream;
  const LfGeom g = f->g;
  const int r = lf_reserve(f, n);
  if (r) return r;
  LfKinv Ki;
  rgbid_cloud_kinv(K, Ki.m);
  const float scale = 1.f / (4 * 7 * 255.f);
  const float scale4 = ((scale * scale) * scale) * scale;
  f->timed[0] = false; f->timed[3] = false;
  if (g.levels > 1) {
    f->mark(8);
    lf_build_pyramid(f, grey_dev, n, g.levels - 1);
    f->mark(9);
  }
  f->mark(0);
  RGBID_HIP(hipMemsetAsync(kps_dev, 0, sizeof(rgbid_loopfeat_kp) * (size_t)n * g.max_kp, s));
  if (aux_dev) RGBID_HIP(hipMemsetAsync(aux_dev, 0, sizeof(rgbid_loopfeat_aux) * (size_t)n * g.max_kp, s));
  hipLaunchKernelGGL(k_lf_response, dim3(f->tiles, n), dim3(LT), 0, s, grey_dev, f->pyr, g, f->levels_dev, scale4, f->resp);
  f->mark(1);
  hipLaunchKernelGGL(k_lf_select, dim3(g.cells, n), dim3(LT), 0, s, f->resp, invdepth_dev, g, f->levels_dev, f->staged, f->cell_counts);
  f->mark(2);
  hipLaunchKernelGGL(k_lf_describe, dim3(f->dblocks, n), dim3(LT), 0, s, grey_dev, f->pyr, invdepth_dev, g, f->levels_dev, Ki, f->staged,
                     f->cell_counts, f->rotated, f->bounds, kps_dev, counts_dev, aux_dev);
  f->mark(3);
  f->timed[0] = f->timer.on;
  f->timed[3] = f->timer.on && g.levels > 1;
  RGBID_HIP(hipGetLastError());
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
  f->timed[1] = f->timer.on;
  RGBID_HIP(hipGetLastError());
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
  f->timed[2] = f->timer.on;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_loopfeat_timing_pyramid(rgbid_loopfeat* f, float* ms) {
  if (!f || !ms) return RGBID_E_INVALID;
  (void)hipSetDevice(f->ctx->device);
  *ms = 0.f;
  if (f->timed[3]) {
    RGBID_HIP(hipEventSynchronize(f->timer.ev[9]));
    RGBID_HIP(f->timer.elapsed(8, 9, ms));
  }
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
        RGBID_HIP(hipEventSynchronize(f->timer.ev[a[i] + 1]));
        RGBID_HIP(f->timer.elapsed(a[i], a[i] + 1, &ms[i]));
      }
  }
  return f->timer.enable(enable != 0);
}

}  // extern "C"
