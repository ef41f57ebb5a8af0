/*
 * rgbid_mesh.h -- C-ABI of the clean-up stage of the surface chain: the connected components of an indexed triangle mesh in device
 * memory are labelled, counted and the small ones removed.  It takes any mesh of this form, not only the one rgbid_tsdf_extract_emit
 * writes.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/mesh_mirror.py).  Only integers decide; attribute bytes are copied, never
 * recomputed; nothing depends on execution order.
 *  1. Mesh.  n_v vertices and n_t triangles uint32 [n_t][3], both counts between 0 and the handle's capacities, the capacities at most
 *     RGBID_MESH_MAX_VERTICES = RGBID_MESH_MAX_TRIANGLES = 2^31; the index 3 t and everything derived from it is formed in 64 bits.  A
 *     triangle is WELL FORMED iff all three indices are < n_v; a mesh with a triangle that is not is refused.  Repeated indices inside a
 *     triangle, duplicate triangles and vertices that no triangle names are all legal.
 *  2. Components.  Two vertices are adjacent iff one triangle names both; a component is a class of the transitive closure; a vertex in
 *     no triangle is a component of its own.  The ROOT of a component is its smallest vertex index; components are numbered 0 .. C - 1 by
 *     ascending root.  A triangle belongs to the component of its first index.
 *  3. Table and labels.  table uint32 [C][3] = (root, vertices, triangles) per component; labels uint32 [n_v] = the component number of
 *     every vertex.
 *  4. Selection.  A component is KEPT iff triangles >= min_triangles and, when a mask uint8 [C] is given, its mask byte is not 0.
 *     min_triangles is any uint32; with 0 the components without a triangle stay as well.  Kept vertices are numbered by ascending old
 *     index; kept triangles keep their order and their indices are renumbered.
 *  5. Emit.  The kept vertices' positions float32 [.][3], optionally their colours uint8 [.][3], their normals float32 [.][3] and their
 *     old indices uint32 [.], and the kept triangles uint32 [.][3].  Positions and normals are moved as 32-bit words: a NaN keeps its
 *     payload.
 * Consequences: min_triangles = 0 without a mask returns the input's bytes; min_triangles = 1 removes exactly the unreferenced vertices.
 */
#ifndef RGBID_MESH_H_
#define RGBID_MESH_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_MESH_MAX_VERTICES 2147483648ull    /* 2^31 */
#define RGBID_MESH_MAX_TRIANGLES 2147483648ull   /* 2^31 */

typedef struct rgbid_mesh rgbid_mesh;

/* a handle for meshes of up to max_vertices vertices and max_triangles triangles (each 1 .. the limit above, RGBID_E_INVALID otherwise);
 * it works on the context's stream.  It owns 20 bytes per vertex of capacity (parent, the vertex and triangle counts per root, the
 * component number per root, the renumbering) and 4 bytes per 2 048 vertices (twice) and per 2 048 triangles for the compactions' tiles. */
int rgbid_mesh_create(rgbid_mesh** m, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles);
int rgbid_mesh_destroy(rgbid_mesh* m);
/* steps 1 - 3 for the mesh triangles_dev (device memory, uint32 [n_triangles][3], contiguous, 4-byte aligned) over n_vertices vertices;
 * -> the number of components C.  RGBID_E_INVALID before any launch, the handle usable afterwards, for a count above the capacity and,
 * with n_triangles > 0, for a NULL or misaligned buffer or n_vertices = 0.  The first launch only counts the triangles that are not well
 * formed; if there is one the call returns RGBID_E_INVALID, no other kernel has touched the handle's state beyond its first instruction,
 * the former labelling and selection are gone and the handle is usable.  Synchronises once.  The labelling holds until the next label;
 * triangles_dev must stay valid and unchanged as long as select or emit are called on it.  n_vertices = 0 gives C = 0 without a launch. */
int rgbid_mesh_label(rgbid_mesh* m, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                     unsigned long long* n_components);
/* step 3 into caller buffers (device memory, 4-byte aligned, RGBID_E_INVALID otherwise): table uint32 [C][3], labels uint32 [n_vertices];
 * either may be NULL to skip it.  RGBID_E_INVALID without a labelling.  Asynchronous. */
int rgbid_mesh_components(rgbid_mesh* m, uint32_t* table_dev, uint32_t* labels_dev);
/* step 4 on the last labelling: keep_mask_dev (device memory, uint8 [C]) or NULL; -> the numbers of kept components, vertices and
 * triangles (each pointer may be NULL).  RGBID_E_INVALID without a labelling.  Synchronises: the mask has been read when it returns.  It
 * may be called again with other arguments on the same labelling; the selection holds until the next select or label. */
int rgbid_mesh_select(rgbid_mesh* m, uint32_t min_triangles, const uint8_t* keep_mask_dev, unsigned long long* kept_components,
                      unsigned long long* kept_vertices, unsigned long long* kept_triangles);
/* step 5 for the last selection.  Inputs (device memory, n_vertices rows): vertices float32 [.][3], colours uint8 [.][3] or NULL, normals
 * float32 [.][3] or NULL; the triangles are the label call's.  Outputs (device memory): vertices_out, colours_out or NULL, normals_out or
 * NULL, old_index_out uint32 [.] or NULL, each of at least vertex_capacity rows, triangles_out uint32 [.][3] of at least
 * triangle_capacity rows.  RGBID_E_INVALID, nothing written, for: no selection; with kept vertices, a NULL or misaligned (4 bytes)
 * vertices_dev or vertices_out or vertex_capacity below the kept vertices; with kept triangles, a NULL or misaligned triangles_out or
 * triangle_capacity below the kept triangles; a misaligned normals or old-index buffer; colours_out without colours_dev or normals_out
 * without normals_dev.  Nothing is written past the kept counts.  No output may overlap an input, the label call's triangles or another
 * output.  Asynchronous: inputs and outputs must stay valid until it has run. */
int rgbid_mesh_emit(rgbid_mesh* m, const float* vertices_dev, const uint8_t* colours_dev, const float* normals_dev, float* vertices_out,
                    uint8_t* colours_out, float* normals_out, uint32_t* old_index_out, uint32_t* triangles_out,
                    unsigned long long vertex_capacity, unsigned long long triangle_capacity);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last label, select and emit.  Call it for ms after the calls have completed. */
int rgbid_mesh_timing(rgbid_mesh* m, int enable, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
