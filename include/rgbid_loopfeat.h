/*
 * rgbid_loopfeat.h -- C-ABI of the appearance stage of loop closure: binary features of keyframes, 2-NN Hamming matching with the ratio
 * test, and the 3-point RANSAC over 3-D correspondences with covariances that starts the dense verifier (the reference's
 * LoopCloser::detectLoopClosures / computeRANSACTrafo3D, src/loop_closer.cpp:193-716, and Keyframe::lift2DKeypointsto3DPointsWithCovariance,
 * src/keyframe.cpp:232-274).  Every call is batched over keyframes or over (query, candidate) pairs, works on the context's stream, uses
 * no library sort and no floating-point atomics, and gives results that are bitwise the same from run to run and independent of the
 * batch a keyframe or a pair is computed in.
 *
 * Contract.
 *  features  One pyramid level.  Harris response of a pixel at least 4 from the border: 3 x 3 Sobel-like integer derivatives Ix, Iy of
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

typedef struct rgbid_loopfeat rgbid_loopfeat;

/* an extractor / matcher for keyframes of rows x cols pixels (each >= 2 * RGBID_LOOPFEAT_BORDER + 1) with up to max_keypoints
 * (cells .. RGBID_LOOPFEAT_MAX_KEYPOINTS) keypoints each.  RGBID_E_INVALID otherwise. */
int rgbid_loopfeat_create(rgbid_loopfeat** f, rgbid_ctx* ctx, int rows, int cols, int max_keypoints);
int rgbid_loopfeat_destroy(rgbid_loopfeat* f);
/* host tables (each optional): pattern[256][4] = x1, y1, x2, y2 of the tests; rotated[32][256][4] = the same per direction;
 * bounds[16][2] = (cos, sin) of the bin boundaries (2 b + 1) pi / 32.  Needs no device. */
int rgbid_loopfeat_tables(int8_t* pattern, int8_t* rotated, double* bounds);
/* cells per keyframe and keypoints kept per cell */
int rgbid_loopfeat_layout(const rgbid_loopfeat* f, int* cells_x, int* cells_y, int* per_cell);
/* features of n keyframes: grey_dev [n][rows][cols] uint8, invdepth_dev [n][rows][cols] float, K = fx, fy, cx, cy (host);
 * kps_dev [n][max_keypoints] records (unused ones are zeroed), counts_dev [n].  scratch is allocated for n keyframes on first use
 * and grown on demand.  Asynchronous on the context's stream. */
int rgbid_loopfeat_extract(rgbid_loopfeat* f, const uint8_t* grey_dev, const float* invdepth_dev, int n, const float K[4],
                           rgbid_loopfeat_kp* kps_dev, int32_t* counts_dev);
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

#ifdef __cplusplus
}
#endif
#endif
