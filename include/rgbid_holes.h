/*
 * rgbid_holes.h -- C-ABI of the hole-filling stage of the surface chain: the small openings of an indexed triangle mesh in device memory
 * are found as closed loops of boundary half-edges and each is closed by a fan of triangles around one new vertex at the loop's centre.
 * It takes any mesh of this form, not only the one rgbid_tsdf_extract_emit writes.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/holes_mirror.py).  Only integers decide the topology; float32 and double are
 * used without contraction; all sums are doubles added in a stated order, every add a separate rounding; nothing depends on execution
 * order.
 *  1. Mesh.  n_v vertices float32 [n_v][3], n_t triangles uint32 [n_t][3]; both counts between 0 and the handle's capacities, the
 *     capacities at most RGBID_HOLES_MAX_VERTICES = 2^31 and RGBID_HOLES_MAX_TRIANGLES = 2^29 (those of rgbid_smooth.h), so that the
 *     corners 3 t + c are numbered in 32 bits.  Optional attributes: colours uint8 [n_v][3], normals float32 [n_v][3].  A mesh with an
 *     index >= n_v is refused.  Repeated indices inside a triangle, duplicate triangles and vertices that no triangle names are legal.
 *  2. Half-edges (topology only; no position is read).  A triangle with three distinct indices (a, b, c) gives the directed edges a->b
 *     from corner 0, b->c from corner 1 and c->a from corner 2; a triangle with a repeated index gives none.  n(a, b) is the number of
 *     directed edges a->b.  a->b is a BOUNDARY HALF-EDGE iff n(a, b) + n(b, a) = 1: exactly one corner names the undirected edge, and
 *     that corner 3 t + c is the half-edge's OWNER.  An edge named twice in the same direction, or three times or more, is not boundary.
 *  3. Simple vertices and loops.  out(v) and in(v) count the boundary half-edges that leave and enter v.  v is a BOUNDARY VERTEX iff
 *     out + in > 0 and SIMPLE iff out = in = 1; succ(v) of a simple v is the head of the half-edge that leaves it.  A LOOP is a cycle
 *     v_0 -> v_1 -> ... -> v_(k-1) -> v_0 of succ all of whose vertices are simple, v_0 its smallest index; k >= 3 by step 2.  The chain
 *     from a simple vertex either closes on itself or runs into a vertex that is not simple; then its half-edges are BLOCKED, and so are
 *     the half-edges that leave a vertex that is not simple: every boundary half-edge is in a loop or blocked.  Loops are numbered by
 *     ascending v_0.  The loop table: loop_offsets uint32 [L + 1], loop_vertices uint32 [S] with v_i at offset + i, loop_owners uint32
 *     [S] with the owner corner of v_i -> v_(i+1).
 *  4. Select, from the positions, max_edges in 3 .. 2^31 - 1 and flags.  Every loop gets one status, the first that applies:
 *     RGBID_HOLES_TOO_LONG k > max_edges; RGBID_HOLES_NOT_FINITE some v_i has a component that is not finite; RGBID_HOLES_OUTLINE as
 *     below, skipped under RGBID_HOLES_ANY_FACING; RGBID_HOLES_FILLED otherwise.  With p_i = (double)pos[v_i]: the centre is
 *     s_a = sum over i = 0 .. k - 1 of p_i,a in that order, m_a = (float)(s_a / (double)k), c = (double)m.  The cap's area vector is
 *     A = sum over i of (p_i - p_(i+1)) x (c - p_(i+1)), indices mod k; the rim's is N = sum over i of (q1 - q0) x (q2 - q0) with q0 q1
 *     q2 the positions of the owner triangle of v_i -> v_(i+1) in the triangle's own order.  Every cross-product component is
 *     (a b) - (c d): two products, one difference; the components are summed one by one in loop order.  The loop is an OUTLINE iff
 *     (A0 N0 + A1 N1) + A2 N2 > 0 is false (a NaN is an outline): the cap of a hole faces the way its rim's triangles face, the cap of
 *     a fragment's outer edge does not.  n_v + F > 2^31 or n_t + E > 2^29 (below) is refused.
 *  5. Emit.  The filled loops in loop order have the ranks r = 0 .. F - 1 and the bases b_r, the exclusive sum of their k; E is the sum.
 *     Output vertices: the n_v input rows copied as words, then m of loop r at n_v + r.  Output triangles: the n_t input rows copied,
 *     then for loop r the row (v_(i+1), v_i, n_v + r) at n_t + b_r + i: against the half-edge, so the orientation is consistent.
 *     Colours: per channel (2 sum + k) / (2 k) in 64-bit integers, the sum over the loop's vertices.  Normals: the double sum of
 *     (double)normal[v_i] in loop order, s; q = (s0 s0 + s1 s1) + s2 s2; (float)(s_a / sqrt(q)), 0 0 0 when q is 0 or not finite.
 *     Nothing is written past n_v + F and n_t + E rows.
 * Not in the contract: holes that touch at a vertex stay open (a vertex that is not simple needs an angular order to pair its
 * half-edges); no ear clipping; the new triangles are not refined -- rgbid_smooth_run afterwards is the intended fairing.
 */
#ifndef RGBID_HOLES_H_
#define RGBID_HOLES_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_HOLES_MAX_VERTICES 2147483648ull    /* 2^31 */
#define RGBID_HOLES_MAX_TRIANGLES 536870912ull    /* 2^29 */
#define RGBID_HOLES_MIN_EDGES 3u
#define RGBID_HOLES_MAX_EDGES 2147483647u         /* 2^31 - 1 */
#define RGBID_HOLES_ANY_FACING 1u                 /* flag of rgbid_holes_select: no loop is an outline */
/* the status of a loop */
#define RGBID_HOLES_FILLED 0u
#define RGBID_HOLES_TOO_LONG 1u
#define RGBID_HOLES_NOT_FINITE 2u
#define RGBID_HOLES_OUTLINE 3u

typedef struct rgbid_holes rgbid_holes;

/* a handle for meshes of up to max_vertices vertices and max_triangles triangles (each 1 .. the limit above, RGBID_E_INVALID otherwise);
 * it works on the context's stream.  With c = min(max_vertices, 3 max_triangles), the most simple vertices a mesh can have, it owns
 * 16 bytes per vertex of capacity (the two degrees, the leaving owner, the rank among the simple vertices), 16 bytes per c (the simple
 * vertices, their loops, the two columns of the loop table), 29 bytes per c / 3 + 1 loops (offset, base, rank, head, status, centre) and
 * 72 bytes per triangle of capacity for the corner sort's workspace (two key and two index buffers of three items per triangle, which
 * the pointer doubling uses again); and for the sort 1 KiB per 4 096 items and 4 bytes per 2 048 items for the tiles' tables. */
int rgbid_holes_create(rgbid_holes** h, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles);
int rgbid_holes_destroy(rgbid_holes* h);
/* steps 2 and 3 for the triangles triangles_dev (device memory, uint32 [n_triangles][3], contiguous and 4-byte aligned) over n_vertices
 * vertices.
 *  -> counts[8] (may be NULL) = the directed edges, the boundary half-edges, the boundary vertices, those of them that are not simple,
 *     the loops L, the half-edges in loops S, the blocked half-edges, the longest loop.
 * RGBID_E_INVALID before any launch, the handle usable and the former plan KEPT, for: a count above the capacity; a NULL or misaligned
 * buffer with a non-zero count; triangles with n_vertices = 0.  The first launch only counts the triangles with an index >= n_vertices;
 * with such a triangle the call returns RGBID_E_INVALID and no other kernel is launched; the former plan is GONE and the handle is
 * usable.  Every kernel of plan, select and emit still tests an index before it uses it as an address.  n_triangles = 0 is a valid plan
 * without loops.  Synchronises after that count and for the counts, as rgbid_smooth_plan does, and once between them when the mesh has
 * triangles: the number of simple vertices sets the number of doubling rounds.  The plan holds until the next plan; triangles_dev must
 * stay valid and unchanged for rgbid_holes_select. */
int rgbid_holes_plan(rgbid_holes* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                     unsigned long long counts[8]);
/* the last plan's loop table copied out (device memory, each may be NULL): offsets_out uint32 [L + 1], vertices_out and owners_out
 * uint32 of at least `capacity` entries, status_out uint8 [L], which needs a select since the plan.  RGBID_E_INVALID, nothing written,
 * for: no plan; capacity below S; a misaligned (4 bytes) offsets, vertices or owners buffer; status_out without a select.  Nothing is
 * written past L + 1 offsets, S vertices and owners and L bytes.  Asynchronous. */
int rgbid_holes_loops(rgbid_holes* h, uint32_t* offsets_out, uint32_t* vertices_out, uint32_t* owners_out, uint8_t* status_out,
                      unsigned long long capacity);
/* step 4 over the last plan with the positions vertices_dev (device memory, float32 [n_vertices][3], 4-byte aligned); flags:
 * RGBID_HOLES_ANY_FACING or 0.
 *  -> counts[5] (may be NULL) = the loops that are too long, not finite, outlines, the filled loops F, their edges E.
 * RGBID_E_INVALID before any launch, the former selection kept, for: no plan; max_edges outside 3 .. 2^31 - 1; an unknown flag bit; a
 * NULL or misaligned buffer with n_vertices > 0.  RGBID_E_INVALID after the run, the selection gone, when n_vertices + F > 2^31 or
 * n_triangles + E > 2^29.  Synchronises once.  It may be called again on the same plan with other arguments. */
int rgbid_holes_select(rgbid_holes* h, const float* vertices_dev, unsigned max_edges, uint32_t flags, unsigned long long counts[5]);
/* step 5 over the last selection: vertices_in float32 [n_vertices][3] and triangles_in uint32 [n_triangles][3] -> vertices_out of
 * vertex_capacity rows and triangles_out of triangle_capacity rows; colours (uint8 [.][3]) and normals (float32 [.][3]) are each given
 * as a pair of in and out or as two NULLs.  RGBID_E_INVALID, nothing written, for: no selection; one of an attribute pair NULL and the
 * other not; vertex_capacity below n_vertices + F or triangle_capacity below n_triangles + E; a NULL vertices or triangles buffer of a
 * non-empty side; a misaligned (4 bytes) vertices, normals or triangles buffer; an in buffer that overlaps its out buffer.  Asynchronous:
 * all buffers must stay valid until it has run. */
int rgbid_holes_emit(rgbid_holes* h, const float* vertices_in, const uint8_t* colours_in, const float* normals_in, const uint32_t* triangles_in,
                     float* vertices_out, uint8_t* colours_out, float* normals_out, uint32_t* triangles_out, unsigned long long vertex_capacity,
                     unsigned long long triangle_capacity);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last plan (the host's wait for the first count is not in it), the last select and the last emit.  Call it for ms after the calls have
 * completed. */
int rgbid_holes_timing(rgbid_holes* h, int enable, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
