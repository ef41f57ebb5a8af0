/*
 * rgbid_smooth.h -- C-ABI of the fairing stage of the surface chain: the vertices of an indexed triangle mesh in device memory are moved
 * by Taubin's lambda | mu filter (Taubin, SIGGRAPH 1995: an umbrella-Laplacian step with a positive factor followed by one with a negative
 * factor, which removes high-frequency noise without the shrinkage of plain Laplacian smoothing), and area-weighted vertex normals are
 * computed from the triangles.  It takes any mesh of this form, not only the one rgbid_tsdf_extract_emit writes.  The reference has no
 * mesh and no program text for it.
 *
 * Contract (byte-identical to tests/smooth_mirror.py).  Only integers decide the topology; float32 and double are
 * used without contraction; all sums are doubles added in a stated order; nothing depends on execution order.
 *  1. Mesh.  n_v vertices float32 [n_v][3], n_t triangles uint32 [n_t][3]; both counts between 0 and the handle's capacities, the
 *     capacities at most RGBID_SMOOTH_MAX_VERTICES = 2^31 and RGBID_SMOOTH_MAX_TRIANGLES = 2^29, so that the 6 n_t corner pairs and the
 *     3 n_t corners are numbered in 32 bits; products of t are formed in 64 bits.  A mesh with an index >= n_v is refused.  Repeated
 *     indices inside a triangle, duplicate triangles and vertices that no triangle names are legal.
 *  2. Adjacency (topology only; no position is read).  Every triangle gives the six ordered corner pairs (i0,i1) (i1,i0) (i1,i2) (i2,i1)
 *     (i2,i0) (i0,i2); a pair with equal ends is DROPPED.  N(v) is the set of distinct u with a pair (v, u), ordered by ascending u.
 *     inc(v, u) is the number of pairs (v, u): 2 on a closed manifold, 1 on a rim, >= 3 on a non-manifold edge, 2 for the one triangle
 *     (a, b, a).  The result is a CSR: offsets uint32 [n_v + 1], neighbours uint32 [P], incidences uint32 [P], P = sum |N(v)|.  (v, u) is
 *     a BOUNDARY PAIR iff inc(v, u) = 1; a vertex is a BOUNDARY VERTEX iff it has one.
 *  3. Corner table, only for a plan with RGBID_SMOOTH_PLAN_NORMALS.  For every vertex v the corners 3 t + c with i_c(t) = v, ascending:
 *     corner_offsets uint32 [n_v + 1], corners uint32 [3 n_t].
 *  4. One pass with factor f (a double) from a position buffer `in` to a different buffer `out`; every vertex reads `in` only (Jacobi).
 *     A position is FINITE iff x, y and z are.  v MOVES iff in[v] is finite, v has at least one neighbour whose `in` position is finite
 *     and, with RGBID_SMOOTH_PIN_BOUNDARY, v is no boundary vertex.  For a vertex that moves s_a is the sum in double of (double)in[u]_a
 *     over the finite neighbours in ascending u, every add a separate rounding, k their count; m_a = s_a / (double)k and
 *     out[v]_a = (float)((double)in[v]_a + f (m_a - (double)in[v]_a)): one difference, one product, one sum, one rounding to float.  A
 *     vertex that does not move copies its three 32-bit words: a NaN keeps its payload.  A result may round to +-inf; from then on that
 *     vertex is not finite.
 *  5. Run.  iterations in 0 .. RGBID_SMOOTH_MAX_ITERATIONS = 4096, lambda finite with 0 < lambda <= 1, mu finite with -2 <= mu <= 0.
 *     Each iteration is a pass with lambda and, when mu != 0, a pass with mu.  iterations = 0 copies the words.
 *  6. Normals, for any position buffer over the plan's triangles.  A triangle is MEASURABLE iff its three positions are finite; its area
 *     vector is e1 x e2 with e1 = (double)p1 - (double)p0, e2 = (double)p2 - (double)p0, every component (a b) - (c d): two products and
 *     one difference.  s(v) is the double sum of the area vectors of the measurable triangles over v's corners in ascending 3 t + c (a
 *     triangle that names v twice adds twice; its vector is zero).  q = (s0 s0 + s1 s1) + s2 s2; the normal is (float)(s_a / sqrt(q)),
 *     0 0 0 when q is 0 or not finite.
 */
#ifndef RGBID_SMOOTH_H_
#define RGBID_SMOOTH_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_SMOOTH_MAX_VERTICES 2147483648ull   /* 2^31 */
#define RGBID_SMOOTH_MAX_TRIANGLES 536870912ull   /* 2^29 */
#define RGBID_SMOOTH_MAX_ITERATIONS 4096u
#define RGBID_SMOOTH_PLAN_NORMALS 1u              /* flag of rgbid_smooth_plan: step 3 is performed, rgbid_smooth_normals may follow */
#define RGBID_SMOOTH_PIN_BOUNDARY 1u              /* flag of rgbid_smooth_run: a boundary vertex does not move */

typedef struct rgbid_smooth rgbid_smooth;

/* a handle for meshes of up to max_vertices vertices and max_triangles triangles (each 1 .. the limit above, RGBID_E_INVALID otherwise);
 * it works on the context's stream.  It owns 21 bytes per vertex of capacity (offsets, corner offsets, the boundary byte and one position
 * buffer for the ping-pong of the passes) and 204 bytes per triangle of capacity: 144 for the pair sort's workspace (two key and two
 * index buffers of six items per triangle, which the corner sort uses again), 48 for neighbours and incidences (six rows per triangle at
 * most) and 12 for the corners; and for the sort 1 KiB per 4 096 items and 4 bytes per 2 048 items for the tiles' tables. */
int rgbid_smooth_create(rgbid_smooth** h, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles);
int rgbid_smooth_destroy(rgbid_smooth* h);
/* steps 2 and 3 for the triangles triangles_dev (device memory, uint32 [n_triangles][3], contiguous and 4-byte aligned) over n_vertices
 * vertices; flags: RGBID_SMOOTH_PLAN_NORMALS or 0.
 *  -> counts[8] (may be NULL) = P, the undirected edges P / 2, the boundary pairs, the boundary vertices, the vertices of degree 0, the
 *     largest degree, the dropped pairs with equal ends, the non-manifold pairs (inc >= 3).
 * RGBID_E_INVALID before any launch, the handle usable and the former plan KEPT, for: a count above the capacity; a NULL or misaligned
 * buffer with a non-zero count; triangles with n_vertices = 0; an unknown flag bit.  The first launch only counts the triangles with an
 * index >= n_vertices (and the pairs with equal ends); with such a triangle the call returns RGBID_E_INVALID and no other kernel is
 * launched; the former plan is GONE and the handle is usable.  Every kernel of plan, run and normals still tests an index before it uses
 * it as an address.  n_triangles = 0 is a valid plan with P = 0.  Synchronises twice: after that count, and for the counts.  The plan
 * holds until the next plan; triangles_dev must stay valid and unchanged for rgbid_smooth_normals. */
int rgbid_smooth_plan(rgbid_smooth* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev, uint32_t flags,
                      unsigned long long counts[8]);
/* the last plan's CSR copied out (device memory, each may be NULL): offsets_out uint32 [n_vertices + 1], neighbours_out and
 * incidences_out uint32 of at least pair_capacity entries, boundary_out uint8 [n_vertices] (1: a boundary vertex).  RGBID_E_INVALID,
 * nothing written, for: no plan; pair_capacity below P; a misaligned (4 bytes) offsets, neighbours or incidences buffer.  Nothing is
 * written past n_vertices + 1 offsets, P neighbours and incidences and n_vertices bytes.  Asynchronous. */
int rgbid_smooth_adjacency(rgbid_smooth* h, uint32_t* offsets_out, uint32_t* neighbours_out, uint32_t* incidences_out, uint8_t* boundary_out,
                           unsigned long long pair_capacity);
/* step 5 over the last plan: vertices_in -> vertices_out (device memory, float32 [n_vertices][3], 4-byte aligned, not overlapping);
 * flags: RGBID_SMOOTH_PIN_BOUNDARY or 0.  The handle's own buffer is the third of the ping-pong; the result lands in vertices_out
 * whatever the number of passes, vertices_in is only read.  RGBID_E_INVALID, nothing written, for: no plan; with n_vertices > 0 a NULL or
 * misaligned buffer or overlapping buffers; iterations above RGBID_SMOOTH_MAX_ITERATIONS; lambda or mu outside step 5; an unknown flag
 * bit.  Asynchronous: all passes are enqueued on the context's stream without a host wait; both buffers must stay valid until it has
 * run.  It may be called again on the same plan. */
int rgbid_smooth_run(rgbid_smooth* h, const float* vertices_in, float* vertices_out, unsigned iterations, double lambda, double mu, uint32_t flags);
/* step 6 over the last plan, which must have been made with RGBID_SMOOTH_PLAN_NORMALS (RGBID_E_INVALID otherwise, and for a NULL or
 * misaligned buffer with n_vertices > 0): vertices_dev float32 [n_vertices][3] -> normals_out float32 [n_vertices][3].  Asynchronous. */
int rgbid_smooth_normals(rgbid_smooth* h, const float* vertices_dev, float* normals_out);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last plan (the host's wait for the first count is not in it), the last run and the last normals call.  Call it for ms after the calls
 * have completed. */
int rgbid_smooth_timing(rgbid_smooth* h, int enable, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
