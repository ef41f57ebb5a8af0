/*
 * rgbid_outlier.h -- C-ABI of the radius outlier filter over keyframe point clouds: a record stays when enough other records lie within
 * a radius of it.  The reference has no such filter; it is an opt-in addition to the map chain (rgbid_cloud.h -> here -> rgbid_voxel.h)
 * that removes the isolated mixed-depth points a depth camera leaves along depth discontinuities before the voxel grid turns each of
 * them into a voxel of its own.
 *
 * Contract (bit-exact against tests/outlier_mirror.py).  A record takes part iff x, y, z are finite; one that does
 * not has count 0, is nobody's neighbour and is never kept.  r2 = r * r, formed once in float32.  For taking-part i != j:
 * dx = x_j - x_i, dy, dz likewise, d2 = (dx dx + dy dy) + dz dz, all in float32 without contraction; j is a neighbour of i iff
 * d2 <= r2 (a duplicate point, at distance 0, is one).  count[i] = min(number of neighbours of i, cap): the clamp lets the kernel stop
 * walking at cap.  keep[i] = takes part && count[i] >= min_neighbours.  The output is the kept records, unchanged, in input order.
 * Counts, mask and output are a function of the input alone: integer counts, no float atomics.
 *
 * Grid and its bound.  The search runs on the float32 grid of the voxel filter with cell = r * 1.0625f, inv = 1.f / cell, a point's
 * cell floorf(p_a * inv) per axis, and looks into the 3 x 3 x 3 cells around a point.  That walk provably holds every neighbour while
 * |floorf(p_a * inv)| <= RGBID_OUTLIER_MAX_CELL (2^18) for every finite point and axis, and 2^-60 <= r <= 2^60 (so that r * r and
 * r * 1.0625f are normal float32 numbers); the plan refuses anything else.  At r = 2 cm that is a box of +- 5.5 km around the origin.
 */
#ifndef RGBID_OUTLIER_H_
#define RGBID_OUTLIER_H_

#include <stdint.h>
#include "rgbid_cloud.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_OUTLIER_MAX_POINTS (1ull << 31)   /* indices fit in 32 bits */
#define RGBID_OUTLIER_MAX_CELL 262144           /* 2^18: the largest |floorf(p * inv)| of a finite point the plan accepts */
#define RGBID_OUTLIER_CELL_FACTOR 1.0625f       /* cell size / radius */
#define RGBID_OUTLIER_MIN_RADIUS 8.673617379884035e-19f   /* 2^-60 */
#define RGBID_OUTLIER_MAX_RADIUS 1152921504606846976.0f   /* 2^60 */

typedef struct rgbid_outlier rgbid_outlier;

/* a filter for up to max_points (1 .. RGBID_OUTLIER_MAX_POINTS) input records per plan; it works on the context's stream */
int rgbid_outlier_create(rgbid_outlier** o, rgbid_ctx* ctx, unsigned long long max_points);
int rgbid_outlier_destroy(rgbid_outlier* o);
/* count the neighbours of n records at in_dev (device memory, 16-byte aligned) within `radius`, clamped at cap (>= 1), and mark the
 * records of at least min_neighbours (<= cap) neighbours.  stats (optional, host): finite points, occupied cells, kept records;
 * kept: the number of records the emit writes.  RGBID_E_INVALID for a radius that is not finite, <= 0 or outside
 * [RGBID_OUTLIER_MIN_RADIUS, RGBID_OUTLIER_MAX_RADIUS], cap = 0, min_neighbours > cap, n > max_points, a misaligned pointer, and, after
 * the box of the finite points has been read back, a box that leaves the grid bound above.  Synchronises. */
int rgbid_outlier_plan(rgbid_outlier* o, const rgbid_cloud_point* in_dev, unsigned long long n, float radius, unsigned cap,
                       unsigned min_neighbours, unsigned long long stats[3], unsigned long long* kept);
/* write count[i] of the last plan's n records, in input order, to counts_dev (device memory of n uint32).  Asynchronous. */
int rgbid_outlier_counts(rgbid_outlier* o, uint32_t* counts_dev);
/* write the kept records of the last plan to out_dev (device memory of `capacity` records, 16-byte aligned; RGBID_E_INVALID when
 * capacity < kept; nothing past `kept` records is written).  Asynchronous on the context's stream: the input records must stay valid and
 * unchanged until it has run. */
int rgbid_outlier_emit(rgbid_outlier* o, rgbid_cloud_point* out_dev, unsigned long long capacity);
/* stage timing: enable != 0 records HIP events around the stages of the following plans and emits; ms (optional, host) receives the
 * device milliseconds of the last ones: box, keys + sort, cells (sorted positions and the cell table), count, emit (the plan's count and
 * scan of the kept records plus the emit's write).  Call it for ms after the emit has completed. */
int rgbid_outlier_timing(rgbid_outlier* o, int enable, float ms[5]);

#ifdef __cplusplus
}
#endif
#endif
