/*
 * rgbid_colouralign.h -- C-ABI of the pose refinement of the colour chain: the world poses of the keyframes that rgbid_recolour.h and
 * rgbid_texture.h sample are moved, each by 6-DoF Gauss-Newton steps, until the grey value a keyframe shows at a mesh vertex agrees with
 * the mean over all keyframes that see the vertex (the rigid part of colour map optimisation, Zhou & Koltun 2014).  It changes no
 * geometry and no image: only what is sampled afterwards sees the new poses.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/colouralign_mirror.py).  float32 and double without contraction; only + - x /
 * sqrt and exact conversions; integers and comparisons decide; the sums follow one fixed tree and nothing depends on execution order.
 *  1. Input.  Vertices float32 [n][3] in the world frame, optional normals float32 [n][3].  V views, 1 .. RGBID_COLOURALIGN_MAX_VIEWS, as
 *     rgbid_colouralign_view: an rgbid_recolour_view (the world pose R_WC | t_WC as doubles, a colour plane uint8 [rows][cols][3], an
 *     optional surface-depth plane and an optional inverse-depth plane, float32 [rows][cols] each) and the flag `fixed`, 0 or 1.  One
 *     K = fx, fy, cx, cy, one rows and one cols for the call.  An rgbid_recolour_params with the meaning it has in rgbid_recolour_add.  A
 *     rule (rgbid_colouralign_rule): huber > 0, float32, in grey levels; damping >= 0 and eps > 0, doubles; min_pairs >= 6;
 *     min_views >= 2; rounds >= 1 and iterations >= 1 with rounds * iterations <= RGBID_COLOURALIGN_MAX_ITERATIONS; stride >= 1.  The
 *     lattice is the vertices i = j stride, j = 0 .. n_l - 1, n_l = ceil(n / stride).
 *  2. Pose on the device.  Before every pass the twelve floats cw of a view are formed from its current double pose exactly as step 1 of
 *     rgbid_render.h says: R_CW = R_WC^T, t_CW[i] = -((R[0][i] t0 + R[1][i] t1) + R[2][i] t2) in double, every entry rounded once to
 *     float32.  Only these floats enter steps 3 and 4.
 *  3. Pair class.  A (vertex, view) pair at the view's current pose has exactly one class, GATED, OUTSIDE, HIDDEN, UNMEASURED, AVERTED or
 *     TAKEN, and a TAKEN pair the weight w in 1 .. 1024: steps 3 and 4 of rgbid_recolour.h, word for word.
 *  4. Grey sample of a TAKEN pair, in integers.  Per footprint texel L = 77 R + 150 G + 29 B, 0 .. 65 280.
 *     s = (256 - ax)(256 - ay) L00 + ax (256 - ay) L10 + (256 - ax) ay L01 + ax ay L11, 0 <= s <= 65 280 * 65 536 < 2^32.
 *     Gx = (256 - ay)(L10 - L00) + ay (L11 - L01), Gy = (256 - ax)(L01 - L00) + ax (L11 - L10), signed; where x1 = x0 or y1 = y0 the
 *     differences are 0 by themselves.  g = (double)s / 16777216.0, dx = (double)Gx / 65536.0, dy = (double)Gy / 65536.0: all exact.
 *  5. Target pass, once per round, over every lattice vertex and ALL views at their current poses, the fixed ones and those that ended
 *     FEW or SINGULAR included.  Per vertex S += w s, W += w in uint64 and used += 1 in uint32 over the TAKEN pairs.  S <= V w s <=
 *     2 048 * 1 024 * 65 280 * 65 536 = 255 * 2^45 < 2^53 (that is why RGBID_COLOURALIGN_MAX_VIEWS is 2 048 and not more), so (double)S
 *     is exact.  The vertex HAS A TARGET iff used >= min_views; its target is C = (double)S / ((double)W * 16777216.0), the product exact,
 *     one rounding in the division.
 *  6. System of a RUNNING view.  A pair is USED iff it is TAKEN at the view's current pose and its vertex has a target.  With X, Y, Z the
 *     float32 camera point of step 3, p the float32 vertex, fx, fy and r_ki = cw[3 k + i], all widened to double: f = g - C; iz = 1 / Z,
 *     a = (dx fx) iz, b = (dy fy) iz, c = -((a X + b Y) iz); m_i = (r_0i a + r_1i b) + r_2i c (R_WC applied to (a, b, c));
 *     J = (-m0, -m1, -m2, -(p1 m2 - p2 m1), -(p2 m0 - p0 m2), -(p0 m1 - p1 m0)), each product rounded, then the difference: the derivative
 *     of f under the left-multiplied world-frame twist of step 7.  wh = 1 if |f| <= (double)huber, else (double)huber / |f|; a_i = wh J_i.
 *     The 28 terms are those of rgbid_meshreg.h step 6: a_i J_j for i <= j, row-major (21), a_i f (6), (wh f) f (1); a pair that is not
 *     used contributes +0.0 to each and the used pairs are counted in an integer.  The sums are those of rgbid_meshreg.h step 7 over the
 *     lattice index j: tree64 per 64 consecutive indices (lanes beyond n_l hold +0.0, n = 0 has one such group), then the upper tree of
 *     rgbid_tsdf_align.h step 28.
 *  7. Solve and update: steps 29 - 31 of rgbid_tsdf_align.h, word for word.  used < min_pairs: FEW.  A pivot that is not > 0 and finite or
 *     a delta that is not finite: SINGULAR.  Otherwise R_WC <- dR R_WC, t_WC <- dR t_WC + v for delta = (v, omega), and max |delta_i| < eps
 *     gives CONVERGED.  FEW and SINGULAR are final and leave the pose as it was.  A fixed view has the status FIXED from the start and is
 *     never updated.  The first iteration of every round sets CONVERGED views RUNNING again (their targets have moved).  Inside a round a
 *     view reads its own pose and the round's targets only: the views are independent and their order does not matter.
 *  8. Result per view: rgbid_colouralign_result, laid out as rgbid_meshreg_result (560 bytes): the pose, the status, the systems built,
 *     and `used` and the 28 sums of the first and of the last system built.  Every NaN among its doubles is written with the bits
 *     RGBID_COLOURALIGN_NAN_BITS.  The last round's S, W and used per lattice vertex can be copied out (rgbid_colouralign_targets).
 */
#ifndef RGBID_COLOURALIGN_H_
#define RGBID_COLOURALIGN_H_

#include <stdint.h>
#include "rgbid_recolour.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_COLOURALIGN_MAX_VERTICES 2147483648ull    /* 2^31 */
#define RGBID_COLOURALIGN_MAX_VIEWS 2048                /* step 5: 2 048 * 1 024 * 65 280 * 65 536 < 2^53 */
#define RGBID_COLOURALIGN_MAX_ITERATIONS 256            /* rounds * iterations of a call */
#define RGBID_COLOURALIGN_MAX_FACTOR 16                 /* the box of rgbid_colouralign_downscale */
#define RGBID_COLOURALIGN_TERMS 28                      /* 21 of H, 6 of b, the weighted squared residual */
#define RGBID_COLOURALIGN_NAN_BITS 0x7FFFFFFFFFFFFFFFull

enum {
  RGBID_COLOURALIGN_TARGET_AUTO = 0,
  RGBID_COLOURALIGN_TARGET_WALK = 1,
  RGBID_COLOURALIGN_TARGET_CHUNKS = 2
};

enum {
  RGBID_COLOURALIGN_RUNNING = 0,                        /* every iteration was used and the last one did not meet eps */
  RGBID_COLOURALIGN_CONVERGED = 1,
  RGBID_COLOURALIGN_FEW = 2,
  RGBID_COLOURALIGN_SINGULAR = 3,
  RGBID_COLOURALIGN_FIXED = 4
};

/* step 1: a view of rgbid_recolour_add and whether its pose is held */
typedef struct rgbid_colouralign_view {
  rgbid_recolour_view view;
  int fixed;
} rgbid_colouralign_view;

typedef struct rgbid_colouralign_rule {
  float huber;                                          /* grey levels (0 .. 255) */
  double damping, eps;
  unsigned min_pairs;                                   /* used pairs a system needs, at least 6 */
  unsigned min_views;                                   /* TAKEN pairs a vertex needs for a target, at least 2 */
  int rounds, iterations;                               /* target passes, and Gauss-Newton steps after each */
  int stride;
} rgbid_colouralign_rule;

/* step 8: 560 bytes */
typedef struct rgbid_colouralign_result {
  double pose[12];                                      /* R00 .. R22 tx ty tz of R_WC | t_WC */
  int32_t status;
  int32_t iterations;                                   /* systems built, over all rounds */
  uint32_t used[2];                                     /* used pairs of the first and of the last system built */
  double sums[2][RGBID_COLOURALIGN_TERMS];              /* the 28 sums of step 6 of the first and of the last system built */
} rgbid_colouralign_result;

typedef struct rgbid_colouralign rgbid_colouralign;

/* a handle for meshes of up to max_vertices (1 .. 2^31) vertices seen from up to max_views (1 .. RGBID_COLOURALIGN_MAX_VIEWS) views
 * (RGBID_E_INVALID otherwise); it works on the context's stream.  It holds 20 bytes per vertex (S, W, used), 29 words of 8 and 4 bytes per
 * 64 vertices and view (the group sums and counts, and 1/64 of that again for the upper tree) and 176 bytes per view (the view table). */
int rgbid_colouralign_create(rgbid_colouralign** h, rgbid_ctx* ctx, unsigned long long max_vertices, int max_views);
int rgbid_colouralign_destroy(rgbid_colouralign* h);
/* steps 1 - 8.  result_dev: device memory, V records, 8-byte aligned.  RGBID_E_INVALID before any launch, nothing written and the handle
 * usable, for: a NULL handle, views, K, params, rule or result; n above the capacity; V out of 1 .. max_views; rows or cols < 1 or
 * > RGBID_RASTER_MAX_DIM; z_min or z_max not finite, <= 0 or z_min > z_max; a tolerance that is not finite or < 0; min_cos not in [0, 1];
 * two_sided or a view's fixed neither 0 nor 1; a pose or intrinsic that is not finite (as double or once rounded to float32), fx or fy
 * equal to 0; a NULL colour plane; a NULL or misaligned vertex buffer with n > 0; a misaligned normals buffer, surface or inverse-depth
 * plane; huber not finite or <= 0; damping not finite or < 0; eps not finite or <= 0; min_pairs < 6; min_views < 2; rounds, iterations or
 * stride < 1; rounds * iterations > RGBID_COLOURALIGN_MAX_ITERATIONS; a misaligned result.  Asynchronous: the init and every round (target)
 * and iteration (system, solve, pose) are enqueued on the context's stream without waiting for any of them, and which views still run is
 * decided on the device; vertices, normals, planes and result must stay valid until it has run.  The view table is copied before the call
 * returns. */
int rgbid_colouralign_run(rgbid_colouralign* h, const float* vertices_dev, const float* normals_dev, unsigned long long n, int V,
                          const rgbid_colouralign_view* views, const float K[4], int rows, int cols, const rgbid_recolour_params* params,
                          const rgbid_colouralign_rule* rule, rgbid_colouralign_result* result_dev);
/* step 8: the last run's last target pass, n_l entries each, into device memory (each may be NULL): S and W uint64, 8-byte aligned, used
 * uint32, 4-byte aligned.  RGBID_E_INVALID for a NULL handle, no run yet or a misaligned output.  Asynchronous. */
int rgbid_colouralign_targets(rgbid_colouralign* h, uint64_t* S_out_dev, uint64_t* W_out_dev, uint32_t* used_out_dev);
/* the target pass's switch: RGBID_COLOURALIGN_TARGET_WALK walks all views per vertex and writes the state once,
 * RGBID_COLOURALIGN_TARGET_CHUNKS spreads chunks of 16 views over blocks that add to the cleared state with integer atomics,
 * RGBID_COLOURALIGN_TARGET_AUTO (the default) takes the chunks for more than 16 views.  The sums are integers: the results do not depend
 * on it; the switch is there for the tests and for tools/colouralign_bench.py.  RGBID_E_INVALID for a NULL handle or another value. */
int rgbid_colouralign_set_target_form(rgbid_colouralign* h, int form);
/* stage timing: enable != 0 records HIP events around every launch of the following rgbid_colouralign_run calls; ms (optional, host)
 * receives the device milliseconds of the last call, summed over its rounds and iterations: target, system, solve (the solve with the
 * pose pass that follows it).  Call it for ms after the call has completed. */
int rgbid_colouralign_timing(rgbid_colouralign* h, int enable, float ms[3]);
/* a colour plane at 1 / f of its resolution for a coarse-to-fine schedule: in_dev uint8 [rows][cols][3] -> out_dev uint8
 * [rows / f][cols / f][3], per channel (2 sum + f f) / (2 f f) in integers over the f x f box (the mean, halves rounded up); the rows and
 * columns beyond a multiple of f are cropped.  RGBID_E_INVALID for a NULL handle or plane, rows or cols < 1 or > RGBID_RASTER_MAX_DIM,
 * f out of 1 .. RGBID_COLOURALIGN_MAX_FACTOR, rows / f or cols / f < 1.  Asynchronous; in and out must not overlap. */
int rgbid_colouralign_downscale(rgbid_colouralign* h, const uint8_t* in_dev, int rows, int cols, int f, uint8_t* out_dev);

#ifdef __cplusplus
}
#endif
#endif
