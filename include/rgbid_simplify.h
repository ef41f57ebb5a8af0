/*
 * rgbid_simplify.h -- C-ABI of the decimation stage of the surface chain: an indexed triangle mesh in device memory is simplified by
 * vertex clustering (Rossignac and Borrel 1993).  The vertices of one cell of a grid become one vertex, the triangles are rewritten
 * over the cells and those that collapse or repeat are dropped.  It takes any mesh of this form, not only the one
 * rgbid_tsdf_extract_emit writes.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/simplify_mirror.py).  Only integers decide; float32 is used without
 * contraction, double where stated; nothing depends on execution order.
 *  1. Mesh.  n_v vertices float32 [n_v][3], optionally colours uint8 [n_v][3] and normals float32 [n_v][3], n_t triangles uint32
 *     [n_t][3]; both counts between 0 and the handle's capacities, the capacities at most RGBID_SIMPLIFY_MAX_VERTICES =
 *     RGBID_SIMPLIFY_MAX_TRIANGLES = 2^31; 3 t is formed in 64 bits.  A mesh with an index >= n_v is refused.  Repeated indices inside a
 *     triangle, duplicate triangles and vertices that no triangle names are legal.
 *  2. Participation.  A vertex TAKES PART iff x, y and z are finite.
 *  3. Grid and clusters.  The grid is the voxel filter's (rgbid_voxel.h) with leaf = cell[3] over the vertices
 *     that take part: inv_a = 1.f / cell_a, min_b_a = (int)floorf(lo_a inv_a), div_b_a = (int)floorf(hi_a inv_a) - min_b_a + 1,
 *     ijk_a = (int)(floorf(p_a inv_a) - (float)min_b_a), key = ijk_0 + ijk_1 div_b_0 + ijk_2 div_b_0 div_b_1 in 64 bits.  A CLUSTER is an
 *     occupied cell; clusters are numbered 0 .. C - 1 by ascending key; the members of a cluster are ordered by ascending vertex index.
 *     cluster_of[v] is the cluster number of v, RGBID_SIMPLIFY_NO_CLUSTER for a vertex that does not take part.
 *  4. Representative of a cluster.  Position: three sums in double, in member order, every add a separate rounding, divided by the
 *     member count and rounded to float once.  Colour: per channel (2 sum + n) / (2 n) in 64-bit integers, the rounded mean.  Normal:
 *     the double sums s over the members whose three normal components are finite, q = (s0 s0 + s1 s1) + s2 s2 in double, the normal
 *     (float)(s_a / sqrt(q)); 0 0 0 when there is no such member, when q is 0 or when q is not finite.  Members: the count, uint32.
 *  5. Triangles.  t' = (cluster_of[i0], cluster_of[i1], cluster_of[i2]).  Every triangle gets exactly one class, tested in this order:
 *     LOST, an entry is RGBID_SIMPLIFY_NO_CLUSTER; COLLAPSED, two entries are equal; DUPLICATE, a triangle of smaller input index that
 *     is neither lost nor collapsed has the same set of three clusters, whatever its orientation; KEPT, every other one.  With the flag
 *     RGBID_SIMPLIFY_KEEP_DUPLICATES nothing is a duplicate.  Kept triangles are written as t' in input order, their index order as it
 *     was: the orientation is preserved.
 *  6. Emit.  All C representatives in cluster order, the kept triangles, optionally cluster_of.  Clusters that no kept triangle names
 *     are written too; rgbid_mesh_select with min_triangles = 1 removes them.
 * Consequences: a cell smaller than every vertex distance on a mesh without duplicates returns the triangles under the permutation
 * cluster_of, every representative with the bits of its one member; a cell larger than the mesh gives C = 1 and no triangle.
 */
#ifndef RGBID_SIMPLIFY_H_
#define RGBID_SIMPLIFY_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_SIMPLIFY_MAX_VERTICES 2147483648ull    /* 2^31 */
#define RGBID_SIMPLIFY_MAX_TRIANGLES 2147483648ull   /* 2^31 */
#define RGBID_SIMPLIFY_NO_CLUSTER 0xFFFFFFFFu        /* cluster_of of a vertex that does not take part */
#define RGBID_SIMPLIFY_KEEP_DUPLICATES 1u            /* flag of rgbid_simplify_plan: step 5 has no DUPLICATE class */

typedef struct rgbid_simplify rgbid_simplify;

/* a handle for meshes of up to max_vertices vertices and max_triangles triangles (each 1 .. the limit above, RGBID_E_INVALID otherwise);
 * it works on the context's stream.  It owns 28 bytes per vertex of capacity (the two key and the two index buffers of the sort, which
 * afterwards hold the members in cluster order and the clusters' first members, and cluster_of) and 25 bytes per triangle of capacity
 * (the same four buffers for the duplicate search and one byte that says whether the triangle is kept), and per sort 1 KiB per 4 096
 * items and 4 bytes per 2 048 items for the tiles' tables. */
int rgbid_simplify_create(rgbid_simplify** h, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles);
int rgbid_simplify_destroy(rgbid_simplify* h);
/* steps 1 - 5 for the mesh vertices_dev (device memory, float32 [n_vertices][3]) and triangles_dev (device memory, uint32
 * [n_triangles][3]), both contiguous and 4-byte aligned, with the cell edges cell[3] in metres.
 *  -> grid[6] = min_b[3], div_b[3] as rgbid_voxel_plan gives them (zeros when no vertex takes part);
 *     counts[6] = the vertices that take part, C, and the lost, collapsed, duplicate and kept triangles (the last four sum to
 *     n_triangles).  Either may be NULL.
 * RGBID_E_INVALID before any launch, the handle usable and the former plan KEPT, for: a count above the capacity; a NULL or misaligned
 * buffer with a non-zero count; triangles with n_vertices = 0; a NULL cell or a component of it that is not finite or is <= 0; a flag
 * bit other than RGBID_SIMPLIFY_KEEP_DUPLICATES.  The first launches only count the triangles with an index >= n_vertices and take the
 * box of the vertices; both are read back together.  With such a triangle the call returns RGBID_E_INVALID and no other kernel is
 * launched; with a box form_grid refuses (a bound outside int32, or 2^62 cells or more) likewise.  After these two refusals the former
 * plan is GONE and the handle is usable.  Every kernel of plan and emit still tests an index before it uses it as an address.
 * Synchronises (three times: the box, C, the counts).  The plan holds until the next plan; both buffers must stay valid and unchanged
 * until the emit has run. */
int rgbid_simplify_plan(rgbid_simplify* h, unsigned long long n_vertices, const float* vertices_dev, unsigned long long n_triangles,
                        const uint32_t* triangles_dev, const float cell[3], uint32_t flags, long long grid[6], unsigned long long counts[6]);
/* step 6 for the last plan.  Inputs (device memory, n_vertices rows, or NULL): colours uint8 [.][3], normals float32 [.][3]; positions
 * and triangles are the plan's.  Outputs (device memory): vertices_out float32 [.][3], colours_out uint8 [.][3] or NULL, normals_out
 * float32 [.][3] or NULL, members_out uint32 [.] or NULL, each of at least vertex_capacity rows; cluster_of_out uint32 [n_vertices]
 * or NULL; triangles_out uint32 [.][3] of at least triangle_capacity rows.  RGBID_E_INVALID, nothing written, for: no plan;
 * vertex_capacity below C or triangle_capacity below the kept triangles; with C > 0 a NULL or misaligned (4 bytes) vertices_out; with
 * kept triangles a NULL or misaligned triangles_out; a misaligned normals, members or cluster_of buffer; with n_vertices > 0,
 * colours_out without colours_dev or normals_out without normals_dev.  Nothing is written past C rows, the kept triangles and
 * n_vertices entries of cluster_of_out.  No output may overlap an input or another output.  Asynchronous: inputs and outputs must
 * stay valid until it has run.  It may be called again on the same plan. */
int rgbid_simplify_emit(rgbid_simplify* h, const uint8_t* colours_dev, const float* normals_dev, float* vertices_out, uint8_t* colours_out,
                        float* normals_out, uint32_t* members_out, uint32_t* cluster_of_out, uint32_t* triangles_out,
                        unsigned long long vertex_capacity, unsigned long long triangle_capacity);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last plan's vertex stage (box, keys, sort, runs, cluster map; the host's wait for the box is not in it), its triangle stage
 * (classes, sort, heads, count) and the last emit.  Call it for ms after the calls have completed. */
int rgbid_simplify_timing(rgbid_simplify* h, int enable, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
