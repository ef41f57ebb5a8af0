/*
 * rgbid_denoise.h -- C-ABI of the feature-preserving denoising stage of the surface chain: the face normals of an indexed triangle mesh
 * in device memory are filtered over the faces that share a vertex with them, with a weight that is zero across a crease, and the vertices
 * are then moved along the filtered normals of their faces until those faces fit them (Sun, Rosin, Martin and Langbein, "Fast and effective
 * feature-preserving mesh denoising", TVCG 2007).  Unlike Taubin's filter (rgbid_smooth.h) it keeps the edge between two planes.  It takes
 * any mesh of this form.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/denoise_mirror.py).  Only integers decide the topology; float32 and double are
 * used without contraction; all sums are doubles added in a stated order, one rounding per operation; nothing depends on execution order.
 *  1. Mesh.  As rgbid_smooth.h step 1: n_v vertices float32 [n_v][3], n_t triangles uint32 [n_t][3]; both counts between 0 and the handle's
 *     capacities, the capacities at most RGBID_DENOISE_MAX_VERTICES = 2^31 and RGBID_DENOISE_MAX_TRIANGLES = 2^29.  A mesh with an index
 *     >= n_v is refused.  Repeated indices inside a triangle, duplicate triangles and vertices that no triangle names are legal.
 *  2. Face table (topology only; made by the plan).  For every vertex v the row of the triangles t with a corner at v, in ascending corner
 *     number 3 t + c: a triangle that names v twice stands twice in the row, adjacent.  A CSR: offsets uint32 [n_v + 1], faces uint32
 *     [3 n_t].
 *  3. Neighbourhood.  F(t) is the set of the distinct triangles in the rows of t's three vertices, in ascending order.  It contains t.
 *  4. Raw face normal.  A triangle is MEASURABLE iff its three positions are finite; its area vector a is that of rgbid_smooth.h step 6
 *     (e1 x e2 in double, every component (a b) - (c d)); q = (a0 a0 + a1 a1) + a2 a2; the normal is (float)(a_k / sqrt(q)), 0 0 0 when
 *     the triangle is not measurable or q is 0 or not finite.
 *  5. One normal pass from a buffer `in` to a different buffer `out` (Jacobi) with threshold T, a double with 0 <= T < 1.  A triangle whose
 *     `in` normal has a non-finite component, or is 0 0 0, copies its three 32-bit words.  Otherwise over j in F(t) in ascending j:
 *     d = ((double)n_t0 (double)n_j0 + n_t1 n_j1) + n_t2 n_j2; j is skipped when its normal has a non-finite component or d is not finite
 *     or not > T; otherwise w = (d - T) (d - T) and s_k = s_k + w (double)n_jk: a product, then an add.  q = (s0 s0 + s1 s1) + s2 s2;
 *     out[t]_k = (float)(s_k / sqrt(q)) when q is finite and > 0, otherwise the triangle copies its words.  t itself goes through the same
 *     arithmetic as every other member.
 *  6. One vertex pass from positions `in` to a different buffer `out` (Jacobi) with face normals N, any float32 triples (they need not be
 *     unit).  A triangle TAKES PART iff its normal has three finite components, not all zero, and its three `in` positions are finite.
 *     Vertex v MOVES iff in[v] is finite and at least one triangle of its row takes part.  Over the distinct triangles of the row in
 *     ascending t (a repeat counts once) that take part: c_k = (((double)p0_k + (double)p1_k) + (double)p2_k) / 3.0; e_k = c_k -
 *     (double)in[v]_k; dd = (N0 e0 + N1 e1) + N2 e2 with N in double; s_k = s_k + (double)N_k dd; m counts them.
 *     out[v]_k = (float)((double)in[v]_k + s_k / (double)m).  A vertex that does not move copies its three words: a NaN keeps its payload.
 *     A result may round to +-inf; from then on that vertex is not finite.  Nothing is pinned at a boundary.
 *  7. Runs.  Normal and vertex iterations each in 0 .. RGBID_DENOISE_MAX_ITERATIONS = 256.  rgbid_denoise_normals performs step 4 and then
 *     `iterations` passes of step 5; rgbid_denoise_vertices performs `iterations` passes of step 6 with the normals it is handed.  Zero
 *     iterations give the raw normals, or copy the position words.
 */
#ifndef RGBID_DENOISE_H_
#define RGBID_DENOISE_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_DENOISE_MAX_VERTICES 2147483648ull   /* 2^31 */
#define RGBID_DENOISE_MAX_TRIANGLES 536870912ull   /* 2^29 */
#define RGBID_DENOISE_MAX_ITERATIONS 256u

typedef struct rgbid_denoise rgbid_denoise;

/* a handle for meshes of up to max_vertices vertices and max_triangles triangles (each 1 .. the limit above, RGBID_E_INVALID otherwise);
 * it works on the context's stream.  It owns 16 bytes per vertex of capacity (the offsets and one position buffer for the ping-pong of the
 * vertex passes) and 96 bytes per triangle of capacity: 72 for the corner sort's workspace (two key and two index buffers of three items
 * per triangle), 12 for the face table and 12 for one normal buffer for the ping-pong of the normal passes; and for the sort 1 KiB per
 * 4 096 items and 4 bytes per 2 048 items for the tiles' tables. */
int rgbid_denoise_create(rgbid_denoise** h, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles);
int rgbid_denoise_destroy(rgbid_denoise* h);
/* step 2 for the triangles triangles_dev (device memory, uint32 [n_triangles][3], contiguous and 4-byte aligned) over n_vertices vertices.
 *  -> counts[4] (may be NULL) = the vertices with an empty row, the longest row, the triangles that name a vertex more than once, and the
 *     sum over the triangles of the lengths of their three rows: the work of one normal pass.
 * RGBID_E_INVALID before any launch, the handle usable and the former plan KEPT, for: a count above the capacity; a NULL or misaligned
 * buffer with a non-zero count; triangles with n_vertices = 0.  The first launch only counts the triangles with an index >= n_vertices;
 * with such a triangle the call returns RGBID_E_INVALID and no other kernel is launched; the former plan is GONE and the handle is usable.
 * Every kernel of plan, normals and vertices still tests an index before it uses it as an address.  n_triangles = 0 is a valid plan.
 * Synchronises twice: after that count, and for the counts.  The plan holds until the next plan; triangles_dev must stay valid and
 * unchanged until then: the passes read it. */
int rgbid_denoise_plan(rgbid_denoise* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                       unsigned long long counts[4]);
/* the last plan's CSR copied out (device memory, each may be NULL): offsets_out uint32 [n_vertices + 1], faces_out uint32 [3 n_triangles].
 * RGBID_E_INVALID, nothing written, for: no plan; a misaligned (4 bytes) buffer.  Asynchronous. */
int rgbid_denoise_faces(rgbid_denoise* h, uint32_t* offsets_out, uint32_t* faces_out);
/* steps 4 and 5 over the last plan: vertices_dev float32 [n_vertices][3] -> normals_out float32 [n_triangles][3] (device memory, 4-byte
 * aligned, not overlapping).  The handle's own buffer is the other of the ping-pong; the result lands in normals_out whatever the number
 * of passes, vertices_dev is only read.  RGBID_E_INVALID, nothing written, for: no plan; with n_triangles > 0 a NULL or misaligned buffer
 * or overlapping buffers; iterations above RGBID_DENOISE_MAX_ITERATIONS; a threshold that is not finite or outside 0 <= T < 1.
 * Asynchronous: all passes are enqueued on the context's stream without a host wait; both buffers must stay valid until it has run.  It
 * may be called again on the same plan. */
int rgbid_denoise_normals(rgbid_denoise* h, const float* vertices_dev, float* normals_out, unsigned iterations, double threshold);
/* `iterations` passes of step 6 over the last plan: vertices_in float32 [n_vertices][3], face_normals_dev float32 [n_triangles][3] ->
 * vertices_out float32 [n_vertices][3] (device memory, 4-byte aligned; vertices_out overlaps neither input).  The handle's own buffer is
 * the other of the ping-pong; the result lands in vertices_out whatever the number of passes, the inputs are only read.  RGBID_E_INVALID,
 * nothing written, for: no plan; with n_vertices > 0 a NULL or misaligned position buffer, with n_triangles > 0 a NULL or misaligned
 * normal buffer, or overlapping buffers; iterations above RGBID_DENOISE_MAX_ITERATIONS.  Asynchronous, as rgbid_denoise_normals. */
int rgbid_denoise_vertices(rgbid_denoise* h, const float* vertices_in, const float* face_normals_dev, float* vertices_out, unsigned iterations);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last plan (the host's wait for the first count is not in it), the last normals call and the last vertices call.  Call it for ms after the
 * calls have completed. */
int rgbid_denoise_timing(rgbid_denoise* h, int enable, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
