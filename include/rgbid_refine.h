/*
 * rgbid_refine.h -- C-ABI of the refinement stage of the surface chain: every edge of an indexed triangle mesh in device memory that is
 * longer than a length gets a new vertex at its midpoint and every triangle is cut by the pattern of its split edges (a conforming edge
 * split, one round per plan and emit).  It takes any mesh of this form, not only the one rgbid_tsdf_extract_emit or rgbid_holes_emit
 * writes.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/refine_mirror.py).  Only integers decide the topology; float32 and double are
 * used without contraction; every float is one rounding of a stated expression; there are no float atomics; nothing depends on
 * execution order.
 *  1. Mesh.  As rgbid_holes.h step 1: n_v vertices float32 [n_v][3], n_t triangles uint32 [n_t][3]; both counts between 0 and the
 *     handle's capacities, the capacities at most RGBID_REFINE_MAX_VERTICES = 2^31 and RGBID_REFINE_MAX_TRIANGLES = 2^29.  A mesh with an
 *     index >= n_v is refused.  Repeated indices inside a triangle, duplicate triangles, edges named by three triangles or more and
 *     vertices that no triangle names are legal.  Optional attributes: colours uint8 [n_v][3], normals float32 [n_v][3], a selection
 *     uint8 [n_t]; without a selection every triangle is selected.
 *  2. Edge table (topology only; no position is read).  A triangle with three distinct indices (a, b, c) names the undirected edges
 *     (min, max) of ab from corner 0, bc from corner 1 and ca from corner 2; a triangle with a repeated index is DEGENERATE, names none
 *     and is copied as it is.  The distinct edges in ascending (lo, hi) order are the edges 0 .. n_e - 1; every corner knows its edge.
 *  3. Mark, with L = max_edge, a finite double >= 0.  An edge is ELIGIBLE iff a triangle that names it has a selection byte != 0.  An
 *     eligible edge (a, b) is MARKED iff the six components of both positions are finite and q > L L, with d_k = (double)p_b,k -
 *     (double)p_a,k and q = (d_0 d_0 + d_1 d_1) + d_2 d_2.  (Between finite float32 positions q is finite; the comparison as written
 *     would mark an infinite q against a finite L L.)  The marked edges in edge order have the ranks r = 0 .. M - 1.
 *  4. New vertices.  The edge of rank r gives the vertex n_v + r: position (float)(((double)p_lo,k + (double)p_hi,k) / 2.0); colour
 *     (c_lo + c_hi + 1) >> 1 per channel in integers; normal unit_of(s) with s_k = (double)n_lo,k + (double)n_hi,k, as rgbid_holes.h
 *     step 5: q = (s_0 s_0 + s_1 s_1) + s_2 s_2, (float)(s_k / sqrt(q)), 0 0 0 when q is 0 or not finite.  The n_v input rows are copied
 *     as words.
 *  5. Triangles.  k(t) is the number of marked edges of t (0 for a degenerate one), m0 m1 m2 the new vertices on ab bc ca.  Row t of the
 *     output holds the first child, the other k(t) children stand at n_t + base(t) + i, base the exclusive sum of k over the triangles in
 *     order; E is the sum of k, the output has n_t + E rows.
 *       k = 0  the row copied.
 *       k = 1  rotate the triangle, keeping its orientation, so that the marked edge is ab: (a, m, c), (m, b, c).
 *       k = 3  (a, m0, m2), (m0, b, m1), (m2, m1, c), (m0, m1, m2).
 *       k = 2  rotate so that the unmarked edge is ca: (m0, b, m1) first; the quad a m0 m1 c is cut along m0-c iff q(m0, c) < q(a, m1)
 *              and along a-m1 otherwise (a tie and a NaN included), q step 3's expression on the float32 output positions of step 4;
 *              along a-m1: (a, m0, m1), (a, m1, c); along m0-c: (a, m0, c), (m0, m1, c).
 *     Every child inherits its parent's selection byte.  Orientation is kept everywhere; a mark belongs to an edge and not to a triangle,
 *     so no T-junction arises.
 *  6. n_v + M > 2^31 or n_t + E > 2^29 is refused after the count.
 * Not in the contract: Loop or butterfly subdivision (positions stay on the input's edges); edge flips or any other quality measure;
 * the removal of the degenerate triangles.
 */
#ifndef RGBID_REFINE_H_
#define RGBID_REFINE_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_REFINE_MAX_VERTICES 2147483648ull    /* 2^31 */
#define RGBID_REFINE_MAX_TRIANGLES 536870912ull    /* 2^29 */

typedef struct rgbid_refine rgbid_refine;

/* a handle for meshes of up to max_vertices vertices and max_triangles triangles (each 1 .. the limit above, RGBID_E_INVALID otherwise);
 * it works on the context's stream.  It owns 0 bytes per vertex of capacity and 116 bytes per triangle of capacity: 72 for the corner
 * sort's workspace (two key and two index buffers of three items per triangle; after the sort they hold every corner's edge and the
 * ends of the marked edges), 36 for the ends and the rank of up to three edges, 3 for the flags of those edges, 5 for k and base; and
 * for the sort 1 KiB per 4 096 items and 4 bytes per 2 048 items for the tiles' tables. */
int rgbid_refine_create(rgbid_refine** h, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles);
int rgbid_refine_destroy(rgbid_refine* h);
/* steps 2 and 3 for the triangles triangles_dev (device memory, uint32 [n_triangles][3], contiguous and 4-byte aligned) over the
 * positions vertices_dev (float32 [n_vertices][3], 4-byte aligned) with the selection selection_or_null (uint8 [n_triangles], NULL: all).
 *  -> counts[9] (may be NULL) = the distinct edges, the eligible edges, the marked edges M, the triangles with k = 0, 1, 2, 3 (the
 *     degenerate ones are among k = 0), the degenerate triangles, the new triangles E.
 * RGBID_E_INVALID before any launch, the handle usable and the former plan KEPT, for: a count above the capacity; a NULL or misaligned
 * triangle buffer with a non-zero count; triangles with n_vertices = 0; a NULL or misaligned vertex buffer with n_vertices > 0; a
 * max_edge that is not finite or is negative.  The first launch only counts the triangles with an index >= n_vertices; with such a
 * triangle the call returns RGBID_E_INVALID and no other kernel is launched; the former plan is GONE and the handle is usable.  Every
 * kernel still tests an index before it uses it as an address.  RGBID_E_INVALID after the count, the plan gone, when n_vertices + M >
 * 2^31 or n_triangles + E > 2^29.  n_triangles = 0 is a valid plan without edges.  Synchronises for the first count and for the nine.
 * The plan holds until the next plan; rgbid_refine_emit reads its own arguments, not the plan's buffers. */
int rgbid_refine_plan(rgbid_refine* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                      const float* vertices_dev, const uint8_t* selection_or_null, double max_edge, unsigned long long counts[9]);
/* steps 4 and 5 over the last plan: vertices_in float32 [n_vertices][3] and triangles_in uint32 [n_triangles][3], the planned mesh ->
 * vertices_out of vertex_capacity rows and triangles_out of triangle_capacity rows; colours (uint8 [.][3]), normals (float32 [.][3]) and
 * selection (uint8 [.], one byte per triangle) are each given as a pair of in and out or as two NULLs.  RGBID_E_INVALID, nothing
 * written, for: no plan; one of an attribute pair NULL and the other not; vertex_capacity below n_vertices + M or triangle_capacity
 * below n_triangles + E; a NULL vertices or triangles buffer of a non-empty side; a misaligned (4 bytes) vertices, normals or triangles
 * buffer; an in buffer that overlaps its out buffer.  Nothing is written past n_vertices + M and n_triangles + E rows.  Asynchronous:
 * all buffers must stay valid until it has run. */
int rgbid_refine_emit(rgbid_refine* h, const float* vertices_in, const uint8_t* colours_in, const float* normals_in, const uint32_t* triangles_in,
                      const uint8_t* selection_in, float* vertices_out, uint8_t* colours_out, float* normals_out, uint32_t* triangles_out,
                      uint8_t* selection_out, unsigned long long vertex_capacity, unsigned long long triangle_capacity);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last plan (the host's wait for the first count is not in it) and the last emit.  Call it for ms after the calls have completed. */
int rgbid_refine_timing(rgbid_refine* h, int enable, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
