/*
 * rgbid_tsdf_align.h -- the third part of the C-ABI of rgbid_tsdf.h, which includes this file at its end: depth frames aligned to the fused
 * volume.  Given a view's inverse-depth plane and an approximate world pose, Gauss-Newton on the signed distance itself (Bylow et al.,
 * RSS 2013) proposes the pose at which the frame lies on the model: no correspondence search and no intermediate image.  The reference has no
 * program text for it.  The call proposes and applies nothing: it returns the pose with the normal equations and the residuals of the
 * first and the last system, and the caller judges them.
 *
 * Contract, continued from rgbid_tsdf_raycast.h (byte-identical to tests/align_mirror.py).  float32 and float64
 * without contraction or FMA; only + - x / sqrt and conversions, so the whole chain, solve and pose update included, is reproducible bit
 * for bit; integers and comparisons decide and the sums follow one fixed tree.
 *
 * Inputs.  V views (rgbid_tsdf_view: the initial world pose as doubles and the inverse-depth plane; colour_dev is ignored), one K = fx, fy,
 * cx, cy, rows, cols, the gate 0 < z_min <= z_max, min_weight in 1 .. 65 535, huber > 0 (metres, float32), damping >= 0, eps > 0 (doubles),
 * min_pixels >= 6, and 1 .. RGBID_TSDF_ALIGN_MAX_LEVELS levels of (stride in {1, 2, 4, 8}, iterations >= 1) with at most
 * RGBID_TSDF_ALIGN_MAX_ITERATIONS iterations in all.  The volume is the handle's current state.
 * 24. Pose: per view 12 doubles R00 .. R22 tx ty tz of R_WC | t_WC.  Every iteration uses their float32 roundings (step 13).
 * 25. Pixels of a level: those with pu % stride == 0 and pv % stride == 0; their lattice coordinates are (lx, ly) = (pu / stride,
 *     pv / stride), so the lattice has ceil(cols / stride) x ceil(rows / stride) pixels.
 * 26. A pixel is USED iff m = iD[pv][pu] is measured (step 5); z = 1.f / m passes the gate z_min <= z <= z_max; with dx, dy of step 14,
 *     xc = dx z, yc = dy z, px = ((R00 xc + R01 yc) + R02 z) + tx (py, pz with rows 1 and 2) and gx = (px - ox) / voxel (gy, gz likewise)
 *     the sample at (gx, gy, gz) is defined (step 15); and fabsf(f) < trunc with f of step 16.  Its values: G = step 16's gradient, each
 *     component divided by voxel; J = (Gx, Gy, Gz, py Gz - pz Gy, pz Gx - px Gz, px Gy - py Gx), each product rounded, then the
 *     difference; w = 1.f if fabsf(f) <= huber, else huber / fabsf(f); a_i = w J_i.  All float32.
 * 27. Terms: 28 doubles per used pixel: the 21 products (double)a_i (double)J_j for i <= j, row-major (00 01 .. 05 11 12 .. 55); the 6
 *     products (double)a_i (double)f; and (double)(w f) (double)f with w f rounded to float32 first.  The products are exact.  A pixel that
 *     is not used contributes +0.0 to each.  The used pixels are counted in an integer.
 * 28. Sums, in one fixed tree.  The lattice is cut into 8 x 8 tiles; lane l = (ly & 7) 8 + (lx & 7); lanes outside the lattice hold +0.0.
 *     tree64 of 64 values v[l]: s[l] = v[l] + v[l ^ 1], then s[l] + s[l ^ 2] of those, and so on up to bit 5; every lane ends with the same
 *     value.  A tile's sum is tree64 of its lanes.  The tile sums of a view, in raster order of the tiles: while more than one value is
 *     left, the values are padded with +0.0 to a multiple of 64 and every 64 consecutive ones are replaced by their tree64.
 * 29. used < min_pixels: the view stops with the status FEW.
 * 30. Solve, in double.  H is the symmetric 6 x 6 matrix of the 21 sums, b the 6 sums.  H_jj = H_jj (1 + damping).  Lower Cholesky column
 *     by column: for j = 0 .. 5: s = H_jj, then s = s - L_jk L_jk for k = 0 .. j - 1 in this order; unless s > 0 and s is finite the view
 *     stops with SINGULAR; L_jj = sqrt(s); for i = j + 1 .. 5: s = H_ij, s = s - L_ik L_jk for ascending k, L_ij = s / L_jj.  Forward:
 *     y_i = (-b_i - L_i0 y_0 - ... - L_i,i-1 y_i-1) / L_ii for i = 0 .. 5; back: x_i = (y_i - L_i+1,i x_i+1 - ... - L_5i x_5) / L_ii for
 *     i = 5 .. 0, the subtractions term by term in ascending k.  delta = x = (v, omega).  A delta that is not finite is SINGULAR as well.
 * 31. Update, a retraction without transcendentals: h = omega / 2, n = sqrt(1 + ((hx hx + hy hy) + hz hz)), qw = 1 / n, qx = hx / n,
 *     qy = hy / n, qz = hz / n; with xx = qx qx, yy, zz, xy = qx qy, xz, yz, wx = qw qx, wy, wz:
 *       dR00 = 1 - 2 (yy + zz)   dR01 = 2 (xy - wz)       dR02 = 2 (xz + wy)
 *       dR10 = 2 (xy + wz)       dR11 = 1 - 2 (xx + zz)   dR12 = 2 (yz - wx)
 *       dR20 = 2 (xz - wy)       dR21 = 2 (yz + wx)       dR22 = 1 - 2 (xx + yy)
 *     R = dR R with every entry (dR_i0 R_0j + dR_i1 R_1j) + dR_i2 R_2j, and t_i = ((dR_i0 t_0 + dR_i1 t_1) + dR_i2 t_2) + v_i.
 * 32. max |delta_i| < eps: the view is CONVERGED for this level.  A view that has stopped is skipped by the rest of the level.  The next
 *     level sets CONVERGED views RUNNING again.  FEW and SINGULAR are final, and the pose stays as it was before that iteration.  A view
 *     that has used all its iterations ends RUNNING.
 * 33. Result per view (device memory): rgbid_tsdf_align_result.  On any state (rgbid_tsdf.h): fabsf(f) < trunc fails for a NaN or
 *     infinite f, and a fraction of 0 still multiplies its corner (0 inf and 0 NaN are NaN), so a D that is NaN or infinite never reaches a
 *     used pixel.  A huge finite D can: beside a fraction of exactly 0 it leaves f alone and makes J infinite or NaN, the sums then hold
 *     NaN and the view ends SINGULAR with its pose unchanged.  Every NaN among the doubles of the record (sums and pose) is written with
 *     the bits RGBID_TSDF_ALIGN_NAN_BITS: the arithmetic's own NaN differs between device and host in its sign (measured: a float32
 *     difference a - b turns the sign of a NaN b on the device).
 */
#ifndef RGBID_TSDF_ALIGN_H_
#define RGBID_TSDF_ALIGN_H_

#ifndef RGBID_TSDF_H_
#error "include rgbid_tsdf.h: it declares the handle and includes this file"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_TSDF_ALIGN_MAX_LEVELS 4
#define RGBID_TSDF_ALIGN_MAX_ITERATIONS 256     /* over all levels of a call */
#define RGBID_TSDF_ALIGN_TERMS 28               /* 21 of H, 6 of b, the weighted squared residual */
#define RGBID_TSDF_ALIGN_NAN_BITS 0x7FFFFFFFFFFFFFFFull   /* bits of every NaN among the doubles of a result record */

enum {
  RGBID_TSDF_ALIGN_RUNNING = 0,                 /* every iteration was used and none met eps */
  RGBID_TSDF_ALIGN_CONVERGED = 1,
  RGBID_TSDF_ALIGN_FEW = 2,
  RGBID_TSDF_ALIGN_SINGULAR = 3
};

typedef struct rgbid_tsdf_align_level {
  int stride;                                   /* 1, 2, 4 or 8 */
  int iterations;                               /* at least 1 */
} rgbid_tsdf_align_level;

/* step 33: 560 bytes */
typedef struct rgbid_tsdf_align_result {
  double pose[12];                              /* R00 .. R22 tx ty tz of R_WC | t_WC */
  int32_t status;
  int32_t iterations;                           /* systems built, over all levels */
  uint32_t used[2];                             /* used pixels of the first and of the last system built */
  double sums[2][RGBID_TSDF_ALIGN_TERMS];       /* the 28 sums of step 28 of the first and of the last system built */
} rgbid_tsdf_align_result;

/* steps 24 - 33 for V views; result_dev: device memory, V records, 8-byte aligned.  RGBID_E_INVALID before any launch, the handle usable
 * afterwards and the result untouched, for: V < 1 or above the handle's max_views; rows or cols out of 1 .. RGBID_TSDF_MAX_DIM;
 * rows cols V >= 2^31; z_min or z_max not finite, <= 0 or z_min > z_max; min_weight out of 1 .. RGBID_TSDF_MAX_WEIGHT; huber not finite
 * or <= 0; damping not finite or < 0; eps not finite or <= 0; min_pixels < 6; n_levels out of 1 .. RGBID_TSDF_ALIGN_MAX_LEVELS; a stride
 * that is not 1, 2, 4 or 8; iterations < 1 or more than RGBID_TSDF_ALIGN_MAX_ITERATIONS in all; a pose or intrinsic that is not finite (as
 * double or as float32), fx or fy equal to 0; a NULL or misaligned plane or result.  Every iteration of every level is enqueued on the
 * context's stream without waiting for any: the call is asynchronous, and planes and result must stay valid until it has run.  It reads
 * the state only: a plan of rgbid_tsdf_extract_plan survives it.  The handle holds the workspace (29 words of 8 and 4 bytes per tile and
 * view); it grows with the largest call. */
int rgbid_tsdf_align(rgbid_tsdf* v, int V, const rgbid_tsdf_view* views, const float K[4], int rows, int cols, float z_min, float z_max,
                     unsigned min_weight, float huber, double damping, double eps, unsigned min_pixels, int n_levels,
                     const rgbid_tsdf_align_level* levels, rgbid_tsdf_align_result* result_dev);
/* stage timing of the alignment, beside rgbid_tsdf_timing (they share one switch): enable != 0 records HIP events around every launch of
 * the following calls; ms (optional, host) receives the device milliseconds of the last call, summed over its launches: system
 * (k_tsdf_align_system) and solve (k_tsdf_align_solve).  Call it for ms after the call has completed. */
int rgbid_tsdf_align_timing(rgbid_tsdf* v, int enable, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
