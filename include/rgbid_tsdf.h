/*
 * rgbid_tsdf.h -- C-ABI of the surface at the end of the map chain: the keyframes' inverse-depth planes are averaged into a dense
 * truncated signed distance volume and the volume's zero crossing is extracted as one triangle mesh.  The reference has no volumetric
 * fusion and no program text for it; only the pose, intrinsics and export-block conventions are the ones the project mirrors already.
 *
 * Contract (byte-identical to tests/tsdf_mirror.py).  Integers decide; float32 without contraction throughout.
 *
 * Volume.  nx, ny, nz >= 2 voxels with nx ny nz <= the handle's capacity <= RGBID_TSDF_MAX_VOXELS; origin (float32 x 3) is the world
 * position of the centre of voxel (0, 0, 0); voxel and trunc are float32, finite and > 0.  Voxel (i, j, k) has the linear index
 * (k ny + j) nx + i and the centre x = ox + (float)i voxel, y and z likewise: one product and one sum each.  Per voxel: D (float32 metres,
 * initially 0), the counts W and Cn (0 .. 65 535, initially 0) and three integer colour sums.  The state is exchanged as the planes
 * D float32 [nz][ny][nx], counts uint32 [nz][ny][nx] = W | Cn << 16, rgb_sum uint32 [3][nz][ny][nx].
 * rgbid_tsdf_set_state checks no value, so every step below is defined for any bits: W and Cn up to 65 535 in any combination, any sums,
 * and a D that is NaN, infinite, a signed zero, denormal or huge.  Denormals are not flushed, -0.0 is not < 0 and a NaN fails every
 * comparison.
 *
 * Integrate.  V views (pose, inverse-depth plane float32 [rows][cols], optionally the colour area uint8 [rows][cols][3] of the keyframe's
 * export block: r g b per pixel, as rgbid_cloud reads it), one K = fx, fy, cx, cy, one depth gate 0 < z_min <= z_max.  Every voxel
 * visits the views in call order, so integrating a then b in two calls is integrating a + b in one, bit for bit:
 *  1. The pose goes to twelve floats r00 .. r22, tx, ty, tz through rgbid_render_pose_cw (step 1 of rgbid_render.h).
 *  2. Camera point: X = ((r00 x + r01 y) + r02 z) + tx, Y and Z likewise with rows 1 and 2 (step 3 of rgbid_render.h).
 *  3. Depth gate: z_min <= Z <= z_max (NaN and infinity fail); otherwise the view is skipped.
 *  4. Projection: u = fx (X / Z) + cx, v = fy (Y / Z) + cy with IEEE division, one product and one sum each; pu = floorf(u + 0.5f),
 *     pv = floorf(v + 0.5f).  In float: the view is skipped unless 0 <= pu <= cols - 1 and 0 <= pv <= rows - 1; only then are pu, pv
 *     converted to int.
 *  5. m = iD[pv][pu] is MEASURED iff it is finite and > 0 and z_m = 1.f / m (IEEE division) is finite; otherwise the view is skipped.
 *  6. s = z_m - Z.  If s < -trunc the voxel is hidden behind the surface and the view is skipped.
 *  7. A voxel whose W is 65 535 skips the view.  Otherwise d = fminf(s, trunc), D = (D (float)W + d) / (float)(W + 1) -- one product,
 *     one sum, one IEEE division -- and W += 1.  Cn and the sums of a voxel with a full W stay as well.  A D that is NaN stays NaN: the
 *     stored bits are the operand's, sign and payload, with the quiet bit set, as the IEEE operations of the device and of the mirror's
 *     host both return them (measured); an operation that has no NaN operand and is invalid (D infinite with W = 0) gives 0xFFC00000 on
 *     both.  Nothing is canonicalised in the state.
 *  8. If the view has colours, |s| <= trunc and Cn < 65 535: the pixel's r, g, b are added to the sums and Cn += 1.  The sums are
 *     uint32 and the additions are modulo 2^32.  A full Cn does not stop W (step 7), and W never carries into Cn.
 *
 * Extract: marching tetrahedra on the Kuhn split of every cell.  Corner code c (0 .. 7) has the offset (c & 1, (c >> 1) & 1, (c >> 2) & 1).
 * The six tetrahedra of a cell are the monotone paths 0 -> e_a -> e_a + e_b -> 7 for the axis orders xyz, xzy, yxz, yzx, zxy, zyx, in
 * that order: the corners 0 1 3 7, 0 1 5 7, 0 2 3 7, 0 2 6 7, 0 4 5 7, 0 4 6 7 are their vertices 0 .. 3.
 * A voxel is VALID iff W >= min_weight (1 .. 65 535) and INSIDE iff it is valid and D < 0.
 *  9. A lattice edge is (voxel p, offset code c in 1 .. 7) with q = p + offset(c) inside the volume; it is ACTIVE iff p and q are valid
 *     and exactly one of them is inside.  Active edges are numbered by ascending linear(p) 7 + (c - 1): that rank is the vertex index.
 * 10. With a the inside end and b the other: t = D_a / (D_a - D_b) (IEEE division) and the position per component is
 *     p_a + t (p_b - p_a): one difference, one product, one sum of the ends' centres.  A component that comes out NaN (D_a and D_b
 *     infinite, or D_b NaN) is written with the bits RGBID_RENDER_NAN_BITS, as the render and the ray cast write theirs: the
 *     arithmetic's own NaN differs between device and host (a - b turns the sign of a NaN b on the device).  D_b = +-0 gives t = 1.
 * 11. Colour: the mean of an end per channel is min((2 sum + Cn) / (2 Cn), 255) in 64-bit integers, absent when Cn = 0 (or when the handle
 *     holds no colour).  Both ends have one: fminf(fmaxf(floorf((c_a + t (c_b - c_a)) + 0.5f), 0.f), 255.f) with the means as float32
 *     (a NaN gives 0); one end has one: that mean; neither: 0.
 * 12. Triangles come from every cell (i < nx - 1, j < ny - 1, k < nz - 1) whose 8 corners are all valid, cells in raster order of their
 *     corner 0, tetrahedra 0 .. 5, triangles in row order; a triangle is three vertex indices, each the index of a tetrahedron edge (u v),
 *     u < v, which is the lattice edge (cell + offset(corner_u), corner_v - corner_u).  Rows per tetrahedron:
 *       one vertex inside, a, the others o1 < o2 < o3:       (a o1, a o2, a o3)
 *       three inside, i1 < i2 < i3, o outside:               (i1 o, i2 o, i3 o)
 *       two inside, a < b, c < d outside:                    (a c, a d, b d) then (a c, b d, b c)
 *     A row has its last two entries swapped iff, with every cut at its edge's midpoint, ((M1 - M0) x (M2 - M0)) . (P_out - P_in) < 0 for
 *     the row's first edge: the normal points from inside to outside.  The swap depends on (tetrahedron, case) only; it is one constant
 *     table of 6 x 16 entries (case = sum of 1 << u over the inside vertices u).  Zero-area triangles (D_b = 0) are kept.
 *
 * Steps 13 - 23 (the volume ray-cast into camera views, a normal per vertex) and their calls are in rgbid_tsdf_raycast.h, steps 24 - 33
 * (depth frames aligned to the volume) in rgbid_tsdf_align.h, both included below.
 */
#ifndef RGBID_TSDF_H_
#define RGBID_TSDF_H_

#include <stdint.h>
#include "rgbid_cloud.h"
#include "rgbid_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_TSDF_MAX_VOXELS 536870912ull      /* 2^29: 7 edges per voxel are numbered in 32 bits */
#define RGBID_TSDF_MAX_VIEWS 65535              /* views per integrate call at most */
#define RGBID_TSDF_MAX_DIM 1048576              /* 2^20: rows and cols at most, as RGBID_RENDER_MAX_DIM */
#define RGBID_TSDF_MAX_WEIGHT 65535             /* W and Cn at most */
#define RGBID_TSDF_VIEW_CHUNK 16                /* views one integrate launch walks; further views go in further launches, in order */

/* one view: the keyframe's world pose, its inverse-depth plane (device memory, float32 [rows][cols], contiguous, 4-byte aligned) and its
 * colours (device memory, uint8 [rows][cols][3], or NULL: the view adds no colour) */
typedef struct rgbid_tsdf_view {
  rgbid_render_pose pose;
  const float* depthinv_dev;
  const uint8_t* colour_dev;
} rgbid_tsdf_view;

typedef struct rgbid_tsdf rgbid_tsdf;

/* a volume of up to max_voxels (8 .. RGBID_TSDF_MAX_VOXELS) voxels that takes up to max_views (1 .. RGBID_TSDF_MAX_VIEWS) views per
 * integrate call; it works on the context's stream.  with_colour == 0: it holds no colour sums (8 instead of 20 bytes of state per voxel),
 * every view is taken as one without colours and rgb_sum reads as zeros.  Beside the state it holds 6 bytes per voxel for the extraction. */
int rgbid_tsdf_create(rgbid_tsdf** v, rgbid_ctx* ctx, unsigned long long max_voxels, int max_views, int with_colour);
int rgbid_tsdf_destroy(rgbid_tsdf* v);
/* the volume's shape, and a reset.  RGBID_E_INVALID (the former shape stays) for: a dimension < 2; nx ny nz above the capacity; voxel,
 * trunc or an origin component that is not finite; voxel or trunc <= 0.  A new handle is configured as 2 x 2 x 2 voxels of 1 m. */
int rgbid_tsdf_configure(rgbid_tsdf* v, int nx, int ny, int nz, const float origin[3], float voxel, float trunc);
/* D = 0, W = Cn = 0, sums = 0.  Asynchronous. */
int rgbid_tsdf_reset(rgbid_tsdf* v);
/* steps 1 - 8 for V views.  RGBID_E_INVALID before any launch, the handle usable afterwards and the state unchanged, for: V < 1 or above
 * the handle's capacity; rows or cols < 1 or > RGBID_TSDF_MAX_DIM; z_min or z_max not finite, <= 0 or z_min > z_max; a pose or intrinsic
 * that is not finite (as double or once rounded to float32), fx or fy equal to 0; a NULL or misaligned plane.  Asynchronous on the
 * context's stream: planes and colours must stay valid and unchanged until it has run. */
int rgbid_tsdf_integrate(rgbid_tsdf* v, int V, const rgbid_tsdf_view* views, const float K[4], int rows, int cols, float z_min, float z_max);
/* the exact state to / from caller device buffers (4-byte aligned, RGBID_E_INVALID otherwise), each of nx ny nz elements (rgb_sum: three
 * times that).  get: any buffer may be NULL to skip it.  set: a NULL buffer zeroes that part of the state; nothing about the values is
 * checked (a W or Cn above 65 535 cannot be expressed); rgb_sum must be NULL for a handle without colour.  Asynchronous. */
int rgbid_tsdf_get_state(rgbid_tsdf* v, float* D_dev, uint32_t* counts_dev, uint32_t* rgb_sum_dev);
int rgbid_tsdf_set_state(rgbid_tsdf* v, const float* D_dev, const uint32_t* counts_dev, const uint32_t* rgb_sum_dev);
/* steps 9 and 12 counted: the active edges and the triangles of the state as it is, for min_weight in 1 .. RGBID_TSDF_MAX_WEIGHT
 * (RGBID_E_INVALID otherwise, and when the triangles cannot be counted in 32 bits).  Synchronises.  The plan holds until the next
 * configure, reset, integrate or set_state. */
int rgbid_tsdf_extract_plan(rgbid_tsdf* v, unsigned min_weight, unsigned long long* n_vertices, unsigned long long* n_triangles);
/* write the last plan's mesh: vertices float32 [n_vertices][3], colours uint8 [n_vertices][3] (or NULL), triangles uint32 [n_triangles][3]
 * (device memory; vertices and triangles 4-byte aligned).  RGBID_E_INVALID without a plan, for a NULL or misaligned vertex or triangle
 * buffer and when vertex_capacity < n_vertices or triangle_capacity < n_triangles (in vertices and triangles); nothing is written past
 * the counts.  A plan of 0 vertices writes nothing and takes any pointers.  Asynchronous. */
int rgbid_tsdf_extract_emit(rgbid_tsdf* v, float* vertices_dev, uint8_t* colours_dev, uint32_t* triangles_dev,
                            unsigned long long vertex_capacity, unsigned long long triangle_capacity);
/* stage timing: enable != 0 records HIP events around the stages of the following calls; ms (optional, host) receives the device
 * milliseconds of the last ones: integrate (the view table's upload and the launches of one integrate call), scan (the flags and counts
 * of a plan and their scans), emit (the vertex and index writes).  Call it for ms after the calls have completed. */
int rgbid_tsdf_timing(rgbid_tsdf* v, int enable, float ms[3]);

#ifdef __cplusplus
}
#endif

/* steps 13 - 23 and their calls: the volume ray-cast into camera views, and a normal per mesh vertex */
#include "rgbid_tsdf_raycast.h"
/* steps 24 - 33 and their calls: depth frames aligned to the volume */
#include "rgbid_tsdf_align.h"
#endif
