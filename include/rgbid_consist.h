/*
 * rgbid_consist.h -- C-ABI of the multi-view consistency filter over keyframe point clouds: a record goes when other keyframes, looking
 * along their own rays, measured a surface clearly BEHIND the place where the record claims to be -- they saw through it.  That removes
 * the mixed-depth "flying pixels" along depth discontinuities and the points on things that moved, which the radius filter only catches
 * where they happen to be isolated.  The reference has no such step and no program text for it; only the pose, intrinsics and record
 * conventions are the ones the project mirrors already.  It is an opt-in first section of the map chain (rgbid_cloud.h -> here ->
 * rgbid_outlier.h -> rgbid_voxel.h -> rgbid_render.h): only the unfiltered cloud still knows which keyframe a record came from.
 *
 * Contract (byte-identical to tests/consist_mirror.py).  Integers decide and nothing depends on execution order.
 * Inputs: n <= 2^31 - 1 records; V views (1 .. 65 535), each a world pose R_WC | t_WC and that keyframe's inverse-depth plane, float32
 * [rows][cols]; optionally offsets[V + 1], ascending from 0 to n: view v OWNS records offsets[v] .. offsets[v + 1] - 1 (NULL: nobody owns
 * anything); K = fx, fy, cx, cy; tolerances tol_rel, tol_abs >= 0; window half-width w (0 .. 2); depth gate 0 < z_min <= z_max;
 * min_support and max_conflicts (0 .. 65 535).
 *  1. Per view, on the host: the pose goes to twelve floats r00 .. r22, tx, ty, tz through rgbid_render_pose_cw (step 1 of rgbid_render.h).
 *  2. A record takes part iff x, y, z are finite.  One that does not has counts 0 and is never kept.
 *  3. For every view v that does not own the record, the camera point in float32 without contraction, as step 3 of rgbid_render.h:
 *     X = ((r00 x + r01 y) + r02 z) + tx, Y and Z likewise with rows 1 and 2.
 *  4. Depth gate: z_min <= Z <= z_max (NaN and infinity fail); otherwise the view is blind to the record.
 *  5. Projection: u = fx (X / Z) + cx, v = fy (Y / Z) + cy with IEEE division, one product and one sum each; pu = floorf(u + 0.5f),
 *     pv = floorf(v + 0.5f).  In float: the view is blind unless 0 <= pu <= cols - 1 and 0 <= pv <= rows - 1; only then are pu, pv
 *     converted to int (step 5 of rgbid_render.h with s = 0).
 *  6. Tolerance: d = tol_rel Z + tol_abs, one product and one sum.
 *  7. Over the (2 w + 1)^2 pixels around (pu, pv), clipped to the image: a pixel is MEASURED iff its m = iD[y][x] is finite and > 0 and
 *     z_m = 1.f / m (IEEE division) is finite; for a measured pixel e = z_m - Z.
 *  8. The view SUPPORTS the record iff some measured pixel has |e| <= d.  It CONTRADICTS it iff it does not support it, at least one pixel
 *     is measured and every measured pixel has e > d: the view measured something behind the record everywhere it looked.  In every other
 *     case -- occluded or partly occluded, holes only, out of view, out of the gate -- it is blind.
 *  9. support[i] and conflicts[i] are the numbers of supporting and contradicting views, published as one uint32: support | conflicts << 16.
 * 10. keep[i] = takes part && support[i] >= min_support && conflicts[i] <= max_conflicts.
 * 11. The output is the kept records, unchanged, in input order.
 */
#ifndef RGBID_CONSIST_H_
#define RGBID_CONSIST_H_

#include <stdint.h>
#include "rgbid_cloud.h"
#include "rgbid_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_CONSIST_MAX_POINTS 2147483647ull  /* 2^31 - 1: indices fit in 32 bits */
#define RGBID_CONSIST_MAX_VIEWS 65535           /* support and conflicts fit in 16 bits each */
#define RGBID_CONSIST_MAX_WINDOW 2              /* the largest window half-width w: (2 w + 1)^2 <= 25 pixels per record and view */
#define RGBID_CONSIST_MAX_DIM 1048576           /* 2^20: rows and cols at most, as RGBID_RENDER_MAX_DIM */
#define RGBID_CONSIST_VIEW_CHUNK 16             /* views one block of the count pass walks once V exceeds it; no result depends on it */

/* one view: the keyframe's world pose and its inverse-depth plane (device memory, float32 [rows][cols], contiguous, 4-byte aligned) */
typedef struct rgbid_consist_view {
  rgbid_render_pose pose;
  const float* depthinv_dev;
} rgbid_consist_view;

/* the decision: steps 4, 6, 7 and 10 of the contract */
typedef struct rgbid_consist_params {
  float tol_rel, tol_abs;                       /* finite, >= 0 */
  int window;                                   /* 0 .. RGBID_CONSIST_MAX_WINDOW */
  float z_min, z_max;                           /* finite, 0 < z_min <= z_max */
  unsigned min_support, max_conflicts;          /* 0 .. 65 535 */
} rgbid_consist_params;

typedef struct rgbid_consist rgbid_consist;

/* a filter for up to max_points (1 .. RGBID_CONSIST_MAX_POINTS) records and max_views (1 .. RGBID_CONSIST_MAX_VIEWS) views per plan; it
 * works on the context's stream and holds 5 bytes per record and 64 bytes per view */
int rgbid_consist_create(rgbid_consist** c, rgbid_ctx* ctx, unsigned long long max_points, int max_views);
int rgbid_consist_destroy(rgbid_consist* c);
/* count the supporting and contradicting views of n records at in_dev (device memory, 16-byte aligned) among V views and mark the records
 * that stay.  offsets: host, V + 1 entries, or NULL.  stats (optional, host): records that took part, (record, view) pairs past the gates
 * of steps 4 and 5, records with conflicts > 0, records kept; kept: the number of records the emit writes.  RGBID_E_INVALID before any
 * launch, the handle usable afterwards, for: rows or cols < 1 or > RGBID_CONSIST_MAX_DIM; V < 1 or above the handle's capacity; n above
 * the handle's capacity; a NULL or misaligned record pointer with n > 0; a window out of range; z_min or z_max not finite, <= 0 or
 * z_min > z_max; a tolerance that is not finite or negative; min_support or max_conflicts above 65 535; a pose or intrinsic that is not
 * finite (as double or once rounded to float32), fx or fy equal to 0; a NULL or misaligned plane; offsets that do not start at 0, are not
 * ascending or do not end at n.  n = 0 is no error and keeps nothing.  Synchronises. */
int rgbid_consist_plan(rgbid_consist* c, const rgbid_cloud_point* in_dev, unsigned long long n, int V, const rgbid_consist_view* views,
                       const unsigned long long* offsets, const float K[4], int rows, int cols, const rgbid_consist_params* params,
                       unsigned long long stats[4], unsigned long long* kept);
/* write support | conflicts << 16 of the last plan's n records, in input order, to counts_dev (device memory of n uint32).  Asynchronous. */
int rgbid_consist_counts(rgbid_consist* c, uint32_t* counts_dev);
/* write the kept records of the last plan to out_dev (device memory of `capacity` records, 16-byte aligned; RGBID_E_INVALID when
 * capacity < kept; nothing past `kept` records is written).  Asynchronous on the context's stream: the input records must stay valid and
 * unchanged until it has run. */
int rgbid_consist_emit(rgbid_consist* c, rgbid_cloud_point* out_dev, unsigned long long capacity);
/* stage timing: enable != 0 records HIP events around the stages of the following plans and emits; ms (optional, host) receives the
 * device milliseconds of the last ones: count (the view table's upload and the count and mark pass), scan (the count and scan of the kept
 * records), emit (the write).  Call it for ms after the emit has completed. */
int rgbid_consist_timing(rgbid_consist* c, int enable, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
