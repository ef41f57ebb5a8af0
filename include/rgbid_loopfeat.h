/*
 * rgbid_loopfeat.h -- C-ABI of the appearance stage of loop closure: binary features of keyframes, 2-NN Hamming matching with the ratio
 * test, and the 3-point RANSAC over 3-D correspondences with covariances that starts the dense verifier (the reference's
 * LoopCloser::detectLoopClosures / computeRANSACTrafo3D, src/loop_closer.cpp:193-716, and Keyframe::lift2DKeypointsto3DPointsWithCovariance,
 * src/keyframe.cpp:232-274).  Every call is batched over keyframes or over (query, candidate) pairs, works on the context's stream, uses
 * no library sort and no floating-point atomics, and gives results that are bitwise the same from run to run and independent of the
 * batch a keyframe or a pair is computed in.
 *
 * Contract.
 *  features  On one pyramid level (the default), or on every level of a scale pyramid ("levels" below).  Harris response of a pixel at least 4 from the border: 3 x 3 Sobel-like integer derivatives Ix, Iy of
 *            the grey image over the 7 x 7 block, sxx = sum Ix Ix, syy, sxy (int32); response = ((float)(sxx syy) - (float)(sxy sxy)) -
 *            ((0.04f (float)(sxx + syy)) (float)(sxx + syy)) scale4, the two products formed in int64, scale = 1.f / (4 * 7 * 255.f),
 *            scale4 = ((scale scale) scale) scale, every float operation rounded once (no contraction).  A keypoint is a pixel at least
 *            RGBID_LOOPFEAT_BORDER from the border whose response is > 0 and beats its 8 neighbours (an equal neighbour loses when its
 *            raster index is larger) and whose inverse depth is finite and > 0.  The image is cut into cells of RGBID_LOOPFEAT_CELL
 *            pixels squared (the last row / column of cells may be cut by the border); each cell keeps its best k = min(max_keypoints /
 *            cells, RGBID_LOOPFEAT_CELL_MAX) by (response descending, raster index ascending).  Records are written cell-major, then by rank.
 *            Direction: m10 = sum x I, m01 = sum y I (integers) over the disc x x + y y <= 15 * 15; one of 32 directions, bin b centred
 *            at 2 pi b / 32 (rgbid_loopfeat_tables gives the boundary vectors).  Descriptor: bit t (byte t / 8, bit t % 8) is set when the
 *            5 x 5 box sum at the first rotated position of test t is smaller than at the second.  X = (d Kinv) p with d = 1.f / iD
 *            (float division) and cov = J diag(0.25f, 0.25f, 0.00025f 0.00025f) J^T in double, as rgbid_loopfeat_kp documents.
 *  levels    An extractor made by rgbid_loopfeat_create_levels works on L <= levels images per keyframe.  Geometry (host): s_l = (float)
 *            pow((double) scale, (double) l), cols_l = (int) (((float) cols + 0.5f) / s_l) in float, rows_l likewise; a level with rows_l
 *            or cols_l below 2 * RGBID_LOOPFEAT_BORDER + 1 does not exist, nor does any above it.  Level l is resized from level l - 1,
 *            bilinear with 11-bit weights: per destination column fx = (dx + 0.5) * ((double) src / (double) dst) - 0.5, x0 = floor(fx),
 *            w1 = (int) floor((fx - x0) * 2048 + 0.5), w0 = 2048 - w1; x0 < 0 gives x0 = 0, w1 = 0; x0 >= src - 1 gives x0 = src - 1,
 *            w1 = 0; x1 = min(x0 + 1, src - 1); rows likewise; pixel = (w0y (w0x p00 + w1x p01) + w1y (w0x p10 + w1x p11) + (1 << 21))
 *            >> 22 in int32 (rgbid_loopfeat_resize_table gives x0 and w1).  No level is blurred.  Budget (host, double): r = 1 / (s s),
 *            s = (double) scale, r^l by repeated multiplication, n_l = floor(max_keypoints * (((1 - r) r^l) / (1 - r^L))); level l has
 *            cells of RGBID_LOOPFEAT_CELL pixels on its own image and keeps per_cell_l = min(max(n_l / cells_l, 1), RGBID_LOOPFEAT_CELL_MAX)
 *            per cell; sum cells_l per_cell_l must not exceed max_keypoints.  A keypoint of level l at (x_l, y_l) satisfies the predicate
 *            above on the level's image and response, and its depth is read at the level-0 pixel X0 = (int) ((double) px + 0.5), px =
 *            (float) x_l * s_l (Y0, py likewise), which must lie inside the image and hold a finite inverse depth > 0.  Direction and
 *            descriptor come from the level's image around (x_l, y_l).  The lift uses p = ((double) px, (double) py, 1), d = 1.f /
 *            iD(Y0, X0), and the pixel variances (double) (((s_l * s_l) * 0.5f) * 0.5f), formed in float.  Records are written level-major,
 *            then cell-major, then by rank, compacted; their x, y are X0, Y0; rgbid_loopfeat_aux carries px, py, x_l, y_l and the level.
 *            With one level all of this is the single-level arithmetic above, bit for bit.
 *  matching  per query descriptor the two nearest candidate descriptors by (Hamming distance, candidate index); kept when
 *            (float) d0 < ratio * (float) d1.  A candidate keyframe with fewer than 2 keypoints gives no match.
 *  ransac    one hypothesis per iteration from 3 matches chosen by replaying selectRandomMatches on the uploaded uniform draws; the
 *            proper rotation of the 3-point correlation; inliers by both directed Mahalanobis errors below the threshold; the best is the
 *            hypothesis of most inliers, the lowest iteration on a tie.
 */
#ifndef RGBID_LOOPFEAT_H_
#define RGBID_LOOPFEAT_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_LOOPFEAT_CELL 32          /* cell edge in pixels */
#define RGBID_LOOPFEAT_CELL_MAX 64      /* most keypoints a cell keeps */
#define RGBID_LOOPFEAT_BORDER 16        /* a keypoint's distance from the image border: disc radius 15, test positions within 13 + box 2 */
#define RGBID_LOOPFEAT_DIRECTIONS 32
#define RGBID_LOOPFEAT_TESTS 256
#define RGBID_LOOPFEAT_MAX_KEYPOINTS 1536   /* a candidate's descriptors (32 B each) are staged in LDS */
#define RGBID_LOOPFEAT_MAX_ITERS 4096
#define RGBID_LOOPFEAT_MAX_LEVELS 8

/* one keypoint, 120 bytes */
typedef struct rgbid_loopfeat_kp {
  int32_t x, y;          /* pixel (column, row) */
  float response;        /* Harris response */
  int32_t direction;     /* 0 .. 31 */
  uint8_t desc[32];      /* 256 binary tests */
  double X[3];           /* camera-frame point (d Kinv) p, p = (x, y, 1), d = 1.f / iD */
  double cov[6];         /* its covariance: xx, xy, xz, yy, yz, zz.  J = [inv_d Kinv(:, 0:2) | -(inv_d inv_d) (Kinv p)], inv_d = 1.0 / d (the
                            reference's Jacobian as written, keyframe.cpp:346-361); cov_ij = ((J_i0 s0) J_j0 + (J_i1 s1) J_j1) + (J_i2 s2) J_j2 */
} rgbid_loopfeat_kp;

/* one surviving match, 16 bytes */
typedef struct rgbid_loopfeat_corr {
  int32_t query, train;        /* keypoint indices in the query and the candidate keyframe */
  int32_t distance, second;    /* Hamming distance of the nearest and of the second nearest candidate descriptor */
} rgbid_loopfeat_corr;

/* what the 120 bytes cannot say about a keypoint of a pyramid level, 16 bytes */
typedef struct rgbid_loopfeat_aux {
  float px, py;          /* level-0 position (float) lx * s_l, (float) ly * s_l: the p of the lift */
  int16_t lx, ly;        /* pixel (column, row) on its level's image */
  int32_t level;
} rgbid_loopfeat_aux;

typedef struct rgbid_loopfeat rgbid_loopfeat;

/* an extractor / matcher for keyframes of rows x cols pixels (each >= 2 * RGBID_LOOPFEAT_BORDER + 1) with up to max_keypoints
 * (cells .. RGBID_LOOPFEAT_MAX_KEYPOINTS) keypoints each.  RGBID_E_INVALID otherwise. */
int rgbid_loopfeat_create(rgbid_loopfeat** f, rgbid_ctx* ctx, int rows, int cols, int max_keypoints);
/* the same over a pyramid of up to levels (1 .. RGBID_LOOPFEAT_MAX_LEVELS) images per keyframe at 1 < scale <= 2 between neighbours; the levels'
 * cells x per_cell must fit into max_keypoints.  rgbid_loopfeat_create is levels = 1.  RGBID_E_INVALID otherwise. */
int rgbid_loopfeat_create_levels(rgbid_loopfeat** f, rgbid_ctx* ctx, int rows, int cols, int max_keypoints, int levels, float scale);
int rgbid_loopfeat_destroy(rgbid_loopfeat* f);
/* what rgbid_loopfeat_create_levels would lay out, or its refusal: existing = L; geometry[L][5] = rows_l, cols_l, cells_x, cells_y, per_cell
 * (room for RGBID_LOOPFEAT_MAX_LEVELS rows); scale_l[L].  Each output optional.  Needs no device. */
int rgbid_loopfeat_plan_levels(int rows, int cols, int max_keypoints, int levels, float scale, int32_t* existing, int32_t* geometry, float* scale_l);
/* the resize tables of one axis from src to dst pixels: x0[dst], w1[dst].  Needs no device. */
int rgbid_loopfeat_resize_table(int src, int dst, int32_t* x0, int32_t* w1);
/* host tables (each optional): pattern[256][4] = x1, y1, x2, y2 of the tests; rotated[32][256][4] = the same per direction;
 * bounds[16][2] = (cos, sin) of the bin boundaries (2 b + 1) pi / 32.  Needs no device. */
int rgbid_loopfeat_tables(int8_t* pattern, int8_t* rotated, double* bounds);
/* cells per keyframe and keypoints kept per cell (of level 0) */
int rgbid_loopfeat_layout(const rgbid_loopfeat* f, int* cells_x, int* cells_y, int* per_cell);
/* the same of one existing level, with its image size and s_l (each output optional); RGBID_E_INVALID for a level that does not exist */
int rgbid_loopfeat_level_layout(const rgbid_loopfeat* f, int level, int* rows_l, int* cols_l, int* cells_x, int* cells_y, int* per_cell,
                                float* scale_l);
/* features of n keyframes: grey_dev [n][rows][cols] uint8, invdepth_dev [n][rows][cols] float, K = fx, fy, cx, cy (host);
 * kps_dev [n][max_keypoints] records (unused ones are zeroed), counts_dev [n].  scratch is allocated for n keyframes on first use
 * and grown on demand.  Asynchronous on the context's stream. */
int rgbid_loopfeat_extract(rgbid_loopfeat* f, const uint8_t* grey_dev, const float* invdepth_dev, int n, const float K[4],
                           rgbid_loopfeat_kp* kps_dev, int32_t* counts_dev);
/* the same with aux_dev [n][max_keypoints] (optional; unused ones are zeroed) beside the records.  On an extractor of several levels
 * rgbid_loopfeat_extract is this call without aux_dev; the pyramid scratch grows with n as the other scratch does. */
int rgbid_loopfeat_extract_levels(rgbid_loopfeat* f, const uint8_t* grey_dev, const float* invdepth_dev, int n, const float K[4],
                                  rgbid_loopfeat_kp* kps_dev, int32_t* counts_dev, rgbid_loopfeat_aux* aux_dev);
/* level `level` of the pyramid of n keyframes: out_dev [n][rows_l][cols_l] uint8 (level 0 is a copy).  Asynchronous. */
int rgbid_loopfeat_pyramid(rgbid_loopfeat* f, const uint8_t* grey_dev, int n, int level, uint8_t* out_dev);
/* matches of n_pairs (query, candidate) keyframe pairs pairs_dev [n_pairs][2] over the features of n_kf keyframes (a pair naming a
 * keyframe outside 0 .. n_kf - 1 yields no match); match_counts_dev [n_pairs]; matches_dev [n_pairs][max_keypoints] in query order, or
 * NULL for the counts alone.  ratio finite and > 0.  Asynchronous. */
int rgbid_loopfeat_match(rgbid_loopfeat* f, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, const int32_t* pairs_dev,
                         int n_pairs, float ratio, rgbid_loopfeat_corr* matches_dev, int32_t* match_counts_dev);
/* RANSAC per pair over its matches: u_dev [3 * iters] uniform draws in [0, 1) (1 <= iters <= RGBID_LOOPFEAT_MAX_ITERS), threshold finite
 * and > 0.  pose_dev [n_pairs][12] = qRc row-major | t_qc of the best hypothesis (NaN when a pair has fewer than 3 matches);
 * result_dev [n_pairs][2] = best iteration (-1 when none), inlier count; mask_dev [n_pairs][max_keypoints] = 1 per inlier match.
 * Asynchronous. */
int rgbid_loopfeat_ransac(rgbid_loopfeat* f, const rgbid_loopfeat_kp* kps_dev, int n_kf, const int32_t* pairs_dev, int n_pairs,
                          const rgbid_loopfeat_corr* matches_dev, const int32_t* match_counts_dev, const double* u_dev, int iters,
                          double threshold, double* pose_dev, int32_t* result_dev, uint8_t* mask_dev);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last ones: response, select, describe, match, ransac.  Call it for ms after the work has completed. */
int rgbid_loopfeat_timing(rgbid_loopfeat* f, int enable, float ms[5]);
/* the device milliseconds the last timed extract spent building its pyramid (0 with one level) */
int rgbid_loopfeat_timing_pyramid(rgbid_loopfeat* f, float* ms);

#ifdef __cplusplus
}
#endif
#endif
