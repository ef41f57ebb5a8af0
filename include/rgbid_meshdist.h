/*
 * rgbid_meshdist.h -- C-ABI of the measuring stage of the surface chain: for every query point the nearest triangle of an indexed
 * triangle mesh in device memory within a truncation distance d_max, the closest point on it and the distance (cloud-to-mesh and, over
 * the vertices of a second mesh, mesh-to-mesh distance).  It takes any mesh of this form, not only the one rgbid_tsdf_extract_emit
 * writes.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/meshdist_mirror.py, a brute force over all triangles).  Integers and
 * comparisons decide; double is used without contraction, with only + - x / sqrt and exact float32 -> double conversions; nothing
 * depends on execution order or on the grid.
 *  1. Mesh.  n_v vertices float32 [n_v][3], n_t triangles uint32 [n_t][3]; both counts between 0 and the handle's capacities, the
 *     capacities at most RGBID_MESHDIST_MAX_VERTICES = RGBID_MESHDIST_MAX_TRIANGLES = 2^31; 3 t is formed in 64 bits.  A mesh with an
 *     index >= n_v is refused.  A triangle TAKES PART iff its nine coordinates are finite.  Repeated indices, duplicate and zero-area
 *     triangles are legal and take part.
 *  2. Box of a triangle.  lo_a, hi_a: the float32 minimum and maximum of its three corners on axis a.
 *  3. Box test.  For a query q with finite coordinates and a triangle that takes part: e_a = |(double)q_a - clamp((double)q_a, lo_a,
 *     hi_a)|, clamp(x, lo, hi) = min(max(x, lo), hi).  The pair PASSES iff e_a <= (double)d_max on all three axes.  In exact geometry
 *     this follows from distance <= d_max; it is part of the contract so that the grid's cover rests on comparisons only.
 *  4. Closest point.  Ericson, Real-Time Collision Detection 5.1.5, in double on the converted corners a, b, c and p = q:
 *       ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c              (per component)
 *       dot(x, y) = (x0 y0 + x1 y1) + x2 y2
 *       d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp)
 *       vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4
 *     The regions, tested in this order, the first that holds decides; r is the point returned:
 *       0  A     d1 <= 0 and d2 <= 0                              r = a, the vertex's own coordinates
 *       1  B     d3 >= 0 and d4 <= d3                             r = b
 *       2  C     d6 >= 0 and d5 <= d6                             r = c
 *       3  AB    vc <= 0 and d1 >= 0 and d3 <= 0                  v = d1 / (d1 - d3),                    r = a + v ab
 *       4  AC    vb <= 0 and d2 >= 0 and d6 <= 0                  w = d2 / (d2 - d6),                    r = a + w ac
 *       5  BC    va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0        w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), r = b + w (c - b)
 *       6  face  otherwise                                        den = 1 / ((va + vb) + vc), v = vb den, w = vc den,
 *                                                                 r = (a + v ab) + w ac
 *     e = q - r, dist2 = (e0 e0 + e1 e1) + e2 e2.  A comparison with a NaN is false, so NaNs fall through to the face.
 *  5. Competition.  A pair COMPETES iff it passes step 3, dist2 is not NaN and dist2 <= (double)d_max (double)d_max.  The winner has the
 *     smallest dist2; among equal dist2, the smallest triangle index.
 *  6. Result per query, in input order.  triangle: uint32, RGBID_MESHDIST_NONE without a winner.  distance: float32 =
 *     (float)sqrt(dist2), without a winner the NaN with the bits RGBID_RENDER_NAN_BITS.  closest (optional): float32 [n][3], the rounded
 *     r, or those NaN bits.  region (optional): uint8, 0 .. 6 as above, RGBID_MESHDIST_NO_REGION without a winner.  candidates
 *     (optional): uint32, the total length of the cell runs the query walked (see the grid); a property of the grid, which the mirror
 *     restates as well.  A query with a non-finite coordinate has no winner and candidates 0.
 *  7. Queries.  float32 [n][3] (rgbid_meshdist_query) or rgbid_cloud_point records, of which x y z are read
 *     (rgbid_meshdist_query_records).
 * Grid.  The voxel filter's float32 grid (rgbid_voxel.h) with inv = 1.f / cell over the box of the corners of the
 * triangles that take part; a coordinate's cell is floorf(p inv).  cell = 0 asks for d_max * RGBID_MESHDIST_CELL_FACTOR; a smaller cell
 * is refused.  d_max lies in RGBID_MESHDIST_MIN_DISTANCE .. RGBID_MESHDIST_MAX_DISTANCE and every |floorf(p inv)| of the box is at most
 * RGBID_MESHDIST_MAX_CELL, or the plan refuses.  A triangle that takes part is entered into every cell of [floorf(lo_a inv),
 * floorf(hi_a inv)] per axis; the (cell key, triangle) pairs are sorted by key, stably: a cell's run is in ascending triangle index.  A
 * finite query walks the runs of the 27 cells around its own that lie in the grid; a query more than one cell outside walks nothing.
 * DESIGN.md section 26 proves that every pair that passes step 3 is met.  The number of pairs is formed in 64 bits and saturates at
 * 2^64 - 1.
 */
#ifndef RGBID_MESHDIST_H_
#define RGBID_MESHDIST_H_

#include <stdint.h>
#include "rgbid.h"
#include "rgbid_cloud.h"
#include "rgbid_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_MESHDIST_MAX_VERTICES 2147483648ull    /* 2^31 */
#define RGBID_MESHDIST_MAX_TRIANGLES 2147483648ull   /* 2^31 */
#define RGBID_MESHDIST_MAX_PAIRS 2147483648ull       /* 2^31 */
#define RGBID_MESHDIST_MAX_QUERIES 2147483648ull     /* 2^31 */
#define RGBID_MESHDIST_NONE 0xFFFFFFFFu              /* triangle of a query without a winner */
#define RGBID_MESHDIST_NO_REGION 255                 /* region of a query without a winner */
#define RGBID_MESHDIST_MAX_CELL 262144               /* 2^18: the largest |floorf(p * inv)| of the mesh's box the plan accepts */
#define RGBID_MESHDIST_CELL_FACTOR 1.0625f           /* smallest cell size / d_max */
#define RGBID_MESHDIST_MIN_DISTANCE 8.673617379884035e-19f   /* 2^-60 */
#define RGBID_MESHDIST_MAX_DISTANCE 1152921504606846976.0f   /* 2^60 */

typedef struct rgbid_meshdist rgbid_meshdist;

/* a handle for meshes of up to max_vertices vertices and max_triangles triangles whose grid holds up to max_pairs (cell, triangle)
 * pairs, queried with up to max_queries points per call (each 1 .. the limit above, RGBID_E_INVALID otherwise); it works on the
 * context's stream.  It owns no bytes per vertex, 48 bytes per triangle of capacity (the nine coordinates, gathered once, as three
 * 16-byte rows) and 12 bytes per 2 048 triangles, 24 bytes per pair of capacity (the two key and the two index buffers of the sort,
 * which afterwards hold the runs, the occupied cells' keys and their starts) and 24 bytes per query of capacity (the same four buffers
 * for the queries' cell order), and per sort 1 KiB per 4 096 items and 4 bytes per 2 048 items for the tiles' tables. */
int rgbid_meshdist_create(rgbid_meshdist** h, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles,
                          unsigned long long max_pairs, unsigned long long max_queries);
int rgbid_meshdist_destroy(rgbid_meshdist* h);
/* the grid of the mesh vertices_dev (device memory, float32 [n_vertices][3]) and triangles_dev (device memory, uint32
 * [n_triangles][3]), both contiguous and 4-byte aligned, for queries up to d_max; cell = 0 asks for the default cell.
 *  -> grid[6] = min_b[3], div_b[3] as rgbid_voxel_plan gives them (zeros when no triangle takes part);
 *     stats[4] = the triangles that take part, the pairs, the occupied cells, the longest run.  Either may be NULL.
 * RGBID_E_INVALID before any launch, the handle usable, nothing written and the former plan KEPT, for: a count above the capacity; a
 * NULL or misaligned buffer with a non-zero count; triangles with n_vertices = 0; d_max not finite, <= 0 or outside the range above;
 * cell not finite, < 0, above RGBID_MESHDIST_MAX_DISTANCE * RGBID_MESHDIST_CELL_FACTOR or, when not 0, below
 * d_max * RGBID_MESHDIST_CELL_FACTOR.
 * The first launches count the triangles with an index >= n_vertices, gather the corners and take their box; with such a triangle, a box
 * outside the bounds of the grid, or more pairs than max_pairs the call returns RGBID_E_INVALID, the former plan is GONE and the handle
 * is usable; in the last case stats[1] still reports the pairs the mesh needs (the other stats as far as they are known).  Every kernel
 * tests an index before it uses it as an address.  Synchronises.  The corners are copied: the mesh may be released after the call. */
int rgbid_meshdist_plan(rgbid_meshdist* h, unsigned long long n_vertices, const float* vertices_dev, unsigned long long n_triangles,
                        const uint32_t* triangles_dev, float d_max, float cell, long long grid[6], unsigned long long stats[4]);
/* steps 3 - 6 for n query points (device memory, float32 [n][3], 4-byte aligned) against the last plan.  Outputs (device memory, each n
 * rows, or NULL): triangle_out uint32, distance_out float32, closest_out float32 [.][3], region_out uint8, candidates_out uint32.
 * RGBID_E_INVALID before any launch, nothing written, for: no plan; n above max_queries; NULL or misaligned points with n > 0; a
 * misaligned (4 bytes) triangle, distance, closest or candidates buffer.  With all outputs NULL or n = 0 nothing is launched.
 * Asynchronous: points and outputs must stay valid until it has run.  It may be called any number of times on one plan. */
int rgbid_meshdist_query(rgbid_meshdist* h, unsigned long long n, const float* points_dev, uint32_t* triangle_out, float* distance_out,
                         float* closest_out, uint8_t* region_out, uint32_t* candidates_out);
/* the same for the positions of n records (16-byte aligned) */
int rgbid_meshdist_query_records(rgbid_meshdist* h, unsigned long long n, const rgbid_cloud_point* records_dev, uint32_t* triangle_out,
                                 float* distance_out, float* closest_out, uint8_t* region_out, uint32_t* candidates_out);
/* the handle's switch: enable != 0 (the default) walks the queries in the order of their cells (one more sort per call), 0 in input
 * order.  The outputs do not depend on it. */
int rgbid_meshdist_set_query_sort(rgbid_meshdist* h, int enable);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last plan's box (index check, gather, box), pairs (count, scan, write), sort and cells (the cell table, the longest run) stages and of
 * the last query (with its sort).  Call it for ms after the calls have completed. */
int rgbid_meshdist_timing(rgbid_meshdist* h, int enable, float ms[5]);

#ifdef __cplusplus
}
#endif
#endif
