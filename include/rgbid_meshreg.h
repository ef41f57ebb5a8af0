/*
 * rgbid_meshreg.h -- C-ABI of the registering stage of the surface chain: a set of points (the vertices of a mesh, a keyframe cloud) is
 * brought into the frame of an indexed triangle mesh in device memory by point-to-plane ICP, so that rgbid_meshdist.h measures the distance
 * between two surfaces and not between two frames.  Every iteration finds the nearest triangle of every transformed point with the
 * truncated search of rgbid_meshdist.h, sums the normal equations of the point-to-plane residuals in the fixed tree of rgbid_tsdf_align.h
 * and solves and retracts as that header does.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/meshreg_mirror.py).  Double without contraction; only + - x / sqrt and exact
 * float32 -> double conversions; integers and comparisons decide; the sums follow one fixed tree and nothing depends on execution order.
 *  1. Target.  A mesh as in rgbid_meshdist.h step 1, planned with d_max and cell exactly as rgbid_meshdist_plan plans it.  Per triangle a
 *     normal in double from the converted float32 corners a, b, c: ab = b - a, ac = c - a, m = (ab1 ac2 - ab2 ac1, ab2 ac0 - ab0 ac2,
 *     ab0 ac1 - ab1 ac0), each product rounded, then the difference; l2 = (m0 m0 + m1 m1) + m2 m2; n = m / sqrt(l2) per component.  A
 *     triangle HAS A NORMAL iff it takes part (its nine coordinates are finite), l2 > 0 and l2 is finite.
 *  2. Source.  N points, float32 [N][3] (rgbid_meshreg_align) or rgbid_cloud_point records of which x y z are read
 *     (rgbid_meshreg_align_records).  V starts, each 12 doubles R00 .. R22 tx ty tz that map the source into the target's frame, all finite.
 *  3. Levels.  1 .. RGBID_MESHREG_MAX_LEVELS levels of (stride >= 1, iterations >= 1, reach), 0 < reach <= d_max as float32, at most
 *     RGBID_MESHREG_MAX_ITERATIONS iterations in all.  A level takes the points i = j stride, j = 0 .. n_l - 1, n_l = ceil(N / stride).
 *  4. Transformed point.  p_k = (float)(((R_k0 x + R_k1 y) + R_k2 z) + t_k), formed in double from the converted source coordinates.  The
 *     float32 p is the query of rgbid_meshdist.h steps 3 - 6; a non-finite p has no winner.
 *  5. A point is USED iff it has a winner, its float32 distance <= reach and the winning triangle has a normal.
 *  6. Terms.  With P = (double)p, r = (double)closest: e = P - r, f = (n0 e0 + n1 e1) + n2 e2, J = (n0, n1, n2, P1 n2 - P2 n1,
 *     P2 n0 - P0 n2, P0 n1 - P1 n0), w = 1 if |f| <= (double)huber, else (double)huber / |f|, a_i = w J_i.  28 doubles per used point:
 *     a_i J_j for i <= j, row-major (21), a_i f (6), (w f) f (1).  A point that is not used contributes +0.0 to each.  The used points are
 *     counted in an integer.
 *  7. Sums.  The lattice index j in groups of 64 consecutive ones, lane j & 63, lanes beyond n_l hold +0.0 (N = 0 has one such group).
 *     tree64 per group, then the upper tree of rgbid_tsdf_align.h step 28 over the group sums in ascending order.
 *  8. used < min_points (min_points >= 6): the start ends FEW.
 *  9. Solve and update: steps 30 and 31 of rgbid_tsdf_align.h, word for word: the damping on the diagonal, the column Cholesky with
 *     term-by-term subtractions, SINGULAR on a pivot that is not > 0 and finite or on a delta that is not finite; delta = (v, omega) is a
 *     twist in the target's frame, R <- dR R, t <- dR t + v.
 * 10. max |delta_i| < eps: CONVERGED for the level; the next level restarts CONVERGED starts.  FEW and SINGULAR are final, and the pose
 *     stays as it was before that iteration.  A start that uses all its iterations ends RUNNING.  The points of a stopped start are queried
 *     as NaN, so they walk nothing.
 * 11. Result per start: rgbid_meshreg_result, laid out as rgbid_tsdf_align_result (560 bytes).  Every NaN among its doubles is written with
 *     the bits RGBID_MESHREG_NAN_BITS (the arithmetic's own NaN differs between device and host in its sign).
 * 12. Apply.  out = step 4's p for any points; optionally normals as (float)((R_k0 nx + R_k1 ny) + R_k2 nz), not renormalised.
 */
#ifndef RGBID_MESHREG_H_
#define RGBID_MESHREG_H_

#include <stdint.h>
#include "rgbid.h"
#include "rgbid_cloud.h"
#include "rgbid_meshdist.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_MESHREG_MAX_STARTS 256
#define RGBID_MESHREG_MAX_QUERIES 2147483648ull   /* 2^31: the bound of max_points max_starts */
#define RGBID_MESHREG_MAX_LEVELS 4
#define RGBID_MESHREG_MAX_ITERATIONS 256          /* over all levels of a call */
#define RGBID_MESHREG_TERMS 28                    /* 21 of H, 6 of b, the weighted squared residual */
#define RGBID_MESHREG_NAN_BITS 0x7FFFFFFFFFFFFFFFull   /* bits of every NaN among the doubles of a result record */

enum {
  RGBID_MESHREG_RUNNING = 0,                      /* every iteration was used and none met eps */
  RGBID_MESHREG_CONVERGED = 1,
  RGBID_MESHREG_FEW = 2,
  RGBID_MESHREG_SINGULAR = 3
};

typedef struct rgbid_meshreg_level {
  int stride;                                     /* at least 1 */
  int iterations;                                 /* at least 1 */
  float reach;                                    /* metres, 0 < reach <= the target's d_max */
} rgbid_meshreg_level;

/* step 11: 560 bytes */
typedef struct rgbid_meshreg_result {
  double pose[12];                                /* R00 .. R22 tx ty tz, source -> target */
  int32_t status;
  int32_t iterations;                             /* systems built, over all levels */
  uint32_t used[2];                               /* used points of the first and of the last system built */
  double sums[2][RGBID_MESHREG_TERMS];            /* the 28 sums of step 7 of the first and of the last system built */
} rgbid_meshreg_result;

typedef struct rgbid_meshreg rgbid_meshreg;

/* a handle for targets of up to max_vertices vertices and max_triangles triangles whose grid holds up to max_pairs pairs (each as in
 * rgbid_meshdist_create), registered with up to max_points points from up to max_starts starts per call: max_points >= 1, max_starts in
 * 1 .. RGBID_MESHREG_MAX_STARTS, max_points max_starts <= RGBID_MESHREG_MAX_QUERIES (RGBID_E_INVALID otherwise).  It owns a rgbid_meshdist
 * of max_points max_starts queries, 24 bytes per triangle of capacity (the normals), 32 bytes per query (the transformed point and the
 * search's triangle, distance and closest point) and 29 words of 8 and 4 bytes per 64 points and start (the group sums). */
int rgbid_meshreg_create(rgbid_meshreg** h, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles,
                         unsigned long long max_pairs, unsigned long long max_points, unsigned long long max_starts);
int rgbid_meshreg_destroy(rgbid_meshreg* h);
/* step 1: arguments, outputs and refusals are rgbid_meshdist_plan's, passed through.  After a refusal before any launch the former target
 * is KEPT, after a later one it is GONE, as there.  Synchronises; the mesh may be released after the call. */
int rgbid_meshreg_target(rgbid_meshreg* h, unsigned long long n_vertices, const float* vertices_dev, unsigned long long n_triangles,
                         const uint32_t* triangles_dev, float d_max, float cell, long long grid[6], unsigned long long stats[4]);
/* steps 2 - 11 for n points (device memory, float32 [n][3], 4-byte aligned) and V starts (poses: host memory, [V][12] doubles);
 * result_dev: device memory, V records, 8-byte aligned.  RGBID_E_INVALID before any launch, nothing written and the handle usable, for: no
 * target; n above max_points; NULL or misaligned points with n > 0; V out of 1 .. max_starts; a pose that is not finite; huber (float32,
 * metres) not finite or <= 0; damping not finite or < 0; eps not finite or <= 0; min_points < 6; n_levels out of
 * 1 .. RGBID_MESHREG_MAX_LEVELS; a stride or an iteration count < 1, more than RGBID_MESHREG_MAX_ITERATIONS iterations in all; a reach that
 * is not finite, <= 0 or above the target's d_max; a NULL or misaligned result.  Asynchronous: the init and every iteration of every level
 * (transform, search, system, solve) are enqueued on the context's stream without waiting for any of them, and which starts still run is
 * decided on the device; points and result must stay valid until it has run.  The poses are copied before the call returns. */
int rgbid_meshreg_align(rgbid_meshreg* h, unsigned long long n, const float* points_dev, int V, const double* poses, float huber,
                        double damping, double eps, unsigned min_points, int n_levels, const rgbid_meshreg_level* levels,
                        rgbid_meshreg_result* result_dev);
/* the same for the positions of n records (16-byte aligned) */
int rgbid_meshreg_align_records(rgbid_meshreg* h, unsigned long long n, const rgbid_cloud_point* records_dev, int V, const double* poses,
                                float huber, double damping, double eps, unsigned min_points, int n_levels,
                                const rgbid_meshreg_level* levels, rgbid_meshreg_result* result_dev);
/* step 12 for n <= 2^31 points (device memory, float32 [n][3]) at pose (host memory, 12 doubles, all finite): points_out float32 [n][3];
 * normals_dev and normals_out (float32 [n][3]) are given together or both NULL.  Outputs may be their inputs.  RGBID_E_INVALID before any
 * launch for a NULL or misaligned buffer with n > 0, one of the two normal buffers without the other, n above 2^31 and a pose that is not
 * finite.  Asynchronous; it needs no target. */
int rgbid_meshreg_apply(rgbid_meshreg* h, unsigned long long n, const float* points_dev, const float* normals_dev, const double pose[12],
                        float* points_out, float* normals_out);
/* the search's switch (rgbid_meshdist_set_query_sort): the results do not depend on it */
int rgbid_meshreg_set_query_sort(rgbid_meshreg* h, int enable);
/* stage timing: enable != 0 records HIP events around every launch of the following rgbid_meshreg_align calls; ms (optional, host)
 * receives the device milliseconds of the last call, summed over its iterations: transform, query, system, solve.  Call it for ms after
 * the call has completed. */
int rgbid_meshreg_timing(rgbid_meshreg* h, int enable, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif
