/*
 * rgbid_recolour.h -- C-ABI of the colouring stage of the surface chain: every vertex of an indexed triangle mesh in device memory is
 * projected into the keyframes, the keyframes that see it (unoccluded, measured, facing) are sampled bilinearly at full resolution and
 * their samples are combined into the vertex's colour.  It takes the vertices of any mesh, not only the one rgbid_tsdf_extract_emit
 * writes; the triangles are not needed here (the occlusion test reads the depth planes rgbid_raster_views wrote for them).  The
 * reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/recolour_mirror.py).  Integers decide everything that is accumulated; float32
 * and double are used without contraction, division and square root are IEEE; nothing depends on execution order or on how the views
 * are split over calls.
 *  1. State.  A handle serves meshes of up to max_vertices (1 .. RGBID_RECOLOUR_MAX_VERTICES = 2^31) vertices.
 *     rgbid_recolour_begin(n_vertices, mode) clears the per-vertex state and the per-view counts and starts view numbering at 0; mode is
 *     RGBID_RECOLOUR_MEAN (0) or RGBID_RECOLOUR_BEST (1).  At most RGBID_RECOLOUR_MAX_VIEWS = 65 535 views may follow one begin.
 *  2. Input of rgbid_recolour_add.  Vertices float32 [n_v][3], optional normals float32 [n_v][3]; V >= 1 views as rgbid_recolour_view:
 *     an rgbid_render_pose (which rgbid_render_pose_cw turns into the twelve floats r00 .. r22, tx, ty, tz), a colour plane uint8
 *     [rows][cols][3] (required), an optional surface-depth plane float32 [rows][cols] (what rgbid_raster_views writes: NaN = empty)
 *     and an optional inverse-depth plane float32 [rows][cols] (the keyframe's own); one K = fx, fy, cx, cy; rows, cols in
 *     1 .. RGBID_RASTER_MAX_DIM; the parameters by pointer (rgbid_recolour_params): float32 0 < z_min <= z_max, surface_tolerance and
 *     measured_tolerance (finite, >= 0), min_cos in [0, 1], two_sided 0 or 1.  The views of one call are walked in launches of
 *     RGBID_RECOLOUR_VIEW_CHUNK = 16.  A view's global index is its position since begin.
 *  3. Vertex in a view.  Camera point X, Y, Z, the depth gate, u, v and the snapped xs, ys are exactly step 3 of rgbid_raster.h: the
 *     same float32 expressions, the same 1/256 lattice, |xs|, |ys| <= 2^23 before the conversion to int32.
 *  4. Class of a (vertex, view) pair, exactly one, tested in this order.
 *     GATED: not usable by step 3.
 *     OUTSIDE: not (0 <= xs <= 256 (cols - 1) and 0 <= ys <= 256 (rows - 1)).  Otherwise x0 = xs >> 8, ax = xs & 255,
 *       x1 = min(x0 + 1, cols - 1), and y0, ay, y1 likewise; the footprint is the four texels (x0, y0), (x1, y0), (x0, y1), (x1, y1),
 *       which coincide at the last row or column and in a 1 x 1 image.
 *     HIDDEN: the view has a surface plane and for some footprint texel d is not finite or fabsf(Z - d) > surface_tolerance.
 *     UNMEASURED: the view has an inverse-depth plane and for some footprint texel m is not finite, m <= 0, 1.f / m is not finite or
 *       fabsf(Z - 1.f / m) > measured_tolerance.
 *     AVERTED: normals are given and the vertex's normal n has a finite, non-zero squared length (n0 n0 + n1 n1) + n2 n2 in float32.
 *       c = R_CW n in float32, each row ((r0 n0 + r1 n1) + r2 n2).  In double, with the floats widened: dot = -((c0 X + c1 Y) + c2 Z),
 *       g = (c0 c0 + c1 c1) + c2 c2, r = (X X + Y Y) + Z Z, cos = dot / sqrt(g r); with two_sided, cos = |cos|.  The pair is averted
 *       iff not (cos > 0 and cos >= (double)min_cos); a NaN fails.
 *     TAKEN: everything else, with the weight w = max(1, (uint32)floor(cos * 1024.0 + 0.5)).  Without normals, or with a zero or
 *       non-finite normal, the facing test is skipped and w = 1024.
 *  5. Sample of a TAKEN pair, per channel k, in integers, c_xy the colour bytes of the footprint:
 *     s_k = (256 - ax)(256 - ay) c00_k + ax (256 - ay) c10_k + (256 - ax) ay c01_k + ax ay c11_k, so 0 <= s_k <= 255 * 65 536.
 *  6. Accumulate.  MEAN: S_k += w s_k and W += w in uint64, used += 1.  BEST: the pair with the largest key
 *     (uint64 w << 32) | (0xFFFFFFFF - global view index) keeps its s_k, used += 1: the largest weight wins, of equals the earliest view.
 *  7. rgbid_recolour_finish.  A vertex with used = 0 gets its input colour when colours_in is given and 0 0 0 otherwise.  MEAN:
 *     (2 S_k + D) / (2 D) with D = 65 536 W, in 64-bit integers.  BEST: (s_k + 32 768) >> 16.  Outputs (device memory, each may be
 *     NULL): colours uint8 [n_v][3], which may alias colours_in; views_used uint32 [n_v]; for BEST best_view uint32 [n_v], the winner's
 *     global view index, RGBID_RECOLOUR_NO_VIEW for none.  finish may be called repeatedly and more views may be added after it.
 *  8. Counts.  Six uint64 per view since begin, the pairs per class in the order of step 4; they sum to n_v.
 */
#ifndef RGBID_RECOLOUR_H_
#define RGBID_RECOLOUR_H_

#include <stdint.h>
#include "rgbid_raster.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_RECOLOUR_MAX_VERTICES 2147483648ull   /* 2^31 */
#define RGBID_RECOLOUR_MAX_VIEWS 65535              /* views after one begin at most: w * s_k summed over them stays below 2^50 */
#define RGBID_RECOLOUR_VIEW_CHUNK 16                /* views one launch handles; further views go in further launches */
#define RGBID_RECOLOUR_MEAN 0                       /* the weighted mean of the samples of all views that see the vertex */
#define RGBID_RECOLOUR_BEST 1                       /* the sample of the view with the largest weight */
#define RGBID_RECOLOUR_UNIT_WEIGHT 1024             /* the weight of cos = 1, and of a pair without a facing test */
#define RGBID_RECOLOUR_NO_VIEW 0xFFFFFFFFu          /* best_view of a vertex no view was taken for */

/* one view: the keyframe's world pose and its planes in device memory, each contiguous [rows][cols]; surface_dev and measured_dev 4-byte
 * aligned, either may be NULL */
typedef struct rgbid_recolour_view {
  rgbid_render_pose pose;
  const uint8_t* colour_dev;
  const float* surface_dev;
  const float* measured_dev;
} rgbid_recolour_view;

typedef struct rgbid_recolour_params {
  float z_min, z_max;            /* the depth gate of step 3 */
  float surface_tolerance;       /* metres between the vertex's depth and the surface plane's */
  float measured_tolerance;      /* metres between the vertex's depth and the keyframe's own */
  float min_cos;                 /* the smallest cosine between the normal and the direction to the camera */
  int two_sided;                 /* 1: a normal pointing away counts as its opposite */
} rgbid_recolour_params;

typedef struct rgbid_recolour rgbid_recolour;

/* a handle for meshes of up to max_vertices (1 .. 2^31) vertices (RGBID_E_INVALID otherwise); it works on the context's stream.  It holds
 * 36 bytes per vertex (four 64-bit sums and the count of views) and 4 MiB for the counts of RGBID_RECOLOUR_MAX_VIEWS views. */
int rgbid_recolour_create(rgbid_recolour** r, rgbid_ctx* ctx, unsigned long long max_vertices);
int rgbid_recolour_destroy(rgbid_recolour* r);
/* step 1.  RGBID_E_INVALID, the handle usable afterwards and its state as it was, for: a NULL handle, n_vertices above the capacity, a
 * mode that is neither RGBID_RECOLOUR_MEAN nor RGBID_RECOLOUR_BEST.  n_vertices = 0 is legal.  Asynchronous. */
int rgbid_recolour_begin(rgbid_recolour* r, unsigned long long n_vertices, int mode);
/* steps 2 - 6 for V further views.  RGBID_E_INVALID before any launch, the handle usable afterwards, state and counts untouched, for: a
 * NULL handle, views, K or params; V < 1 or more than RGBID_RECOLOUR_MAX_VIEWS views since begin; no begin; n_vertices other than
 * begin's; rows or cols < 1 or > RGBID_RASTER_MAX_DIM; z_min or z_max not finite, <= 0 or z_min > z_max; a tolerance that is not finite or
 * < 0; min_cos not in [0, 1]; two_sided neither 0 nor 1; a pose or intrinsic that is not finite (as double or once rounded to float32),
 * fx or fy equal to 0; a NULL colour plane; a NULL or misaligned vertex buffer with n_vertices > 0; a misaligned normals buffer, surface
 * or inverse-depth plane.  With n_vertices = 0 the views are numbered and counted (all zeros) and nothing else happens.  Asynchronous
 * on the context's stream: vertices, normals and planes must stay valid until it ran. */
int rgbid_recolour_add(rgbid_recolour* r, const float* vertices_dev, const float* normals_dev, unsigned long long n_vertices, int V,
                       const rgbid_recolour_view* views, const float K[4], int rows, int cols, const rgbid_recolour_params* params);
/* step 7 for the n_vertices of begin.  RGBID_E_INVALID before any launch, the outputs untouched, for: a NULL handle, no begin, a
 * misaligned views_used or best_view, a best_view after a begin with RGBID_RECOLOUR_MEAN.  colours_in_dev may be NULL and may be
 * colours_out_dev.  The state is not changed.  Asynchronous. */
int rgbid_recolour_finish(rgbid_recolour* r, const uint8_t* colours_in_dev, uint8_t* colours_out_dev, uint32_t* views_used_dev,
                          uint32_t* best_view_dev);
/* step 8 of the views first_view .. first_view + V - 1 since begin, which must have been added (RGBID_E_INVALID otherwise, and for a NULL
 * handle or out, first_view < 0 or V < 1): out (host) uint64 [V][6].  Synchronises. */
int rgbid_recolour_counts(rgbid_recolour* r, int first_view, int V, unsigned long long* out);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last add (accumulate, all its launches) and of the last finish (resolve).  Call it for ms after the calls have completed. */
int rgbid_recolour_timing(rgbid_recolour* r, int enable, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
