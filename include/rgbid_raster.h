/*
 * rgbid_raster.h -- C-ABI of the view of the mesh the surface chain ends in: an indexed triangle mesh in device memory is projected into
 * V pinhole cameras and every pixel keeps the nearest triangle, with perspective-correct depth, colour and camera-frame normal.  It takes
 * any mesh of this form, not only the one rgbid_tsdf_extract_emit writes.  The reference has no mesh and no program text for it.
 *
 * Contract (byte-identical to tests/raster_mirror.py).  Integers decide coverage and the winner; float32 and double
 * are used without contraction, division and square root are IEEE; nothing depends on execution order or on which kernel drew a triangle.
 *  1. Input.  n_v vertices float32 [n_v][3], n_t triangles uint32 [n_t][3] with n_t <= RGBID_RASTER_MAX_TRIANGLES = 2^31 - 1, optional
 *     colours uint8 [n_v][3], optional normals float32 [n_v][3]; V >= 1 poses as rgbid_render_pose, which rgbid_render_pose_cw turns
 *     into the twelve floats r00 .. r22, tx, ty, tz; K = fx, fy, cx, cy; rows, cols; float32 0 < z_min <= z_max.  A mesh with an index
 *     >= n_v is refused.  Repeated indices, duplicate triangles and vertices that no triangle names are legal.
 *  2. rows and cols lie in 1 .. RGBID_RASTER_MAX_DIM = 16384.
 *  3. Vertex, per view.  Camera point X = ((r00 x + r01 y) + r02 z) + tx, Y and Z likewise (rgbid_render.h step 3).  The vertex is
 *     USABLE iff x, y, z are finite and z_min <= Z <= z_max.  u = fx (X / Z) + cx, v = fy (Y / Z) + cy; pixel p's centre is at u = p.
 *     xs = floorf(u * 256.0f + 0.5f), ys likewise (RGBID_RASTER_SUB = 256; the product is exact); the vertex is usable only if
 *     |xs| <= 2^23 and |ys| <= 2^23 (NaN and infinity fail); only then are xs, ys converted to int32.
 *  4. Triangle, per view, exactly one class in this order.  GATED: a corner is not usable (no near-plane clipping: a triangle that
 *     crosses a gate is not drawn).  DEGENERATE: with the snapped corners a, b, c, A = (xb - xa)(yc - ya) - (yb - ya)(xc - xa) in int64
 *     is 0.  EMPTY BOX: x0 = max(0, ceil(min x / 256)), x1 = min(cols - 1, floor(max x / 256)), y likewise, in integers with floor and
 *     ceiling towards -inf / +inf; the box holds no pixel.  DRAWN: everything else.  s = sign(A); both windings are drawn.
 *  5. Coverage at pixel (px, py) of the box, P = (256 px, 256 py): Ea = s ((xc - xb)(Py - yb) - (yc - yb)(Px - xb)), Eb over (c, a),
 *     Ec over (a, b), all int64 (every product below 2^48; Ea + Eb + Ec = |A|).  Covered iff Ea >= 0, Eb >= 0 and Ec >= 0.  There is
 *     no fill rule: a centre on a shared edge is covered by both triangles and step 7 decides.
 *  6. Depth in double: wa = 1.0 / (double)Za, wb, wc likewise; pa = (double)Ea wa, pb, pc likewise; q = (pa + pb) + pc;
 *     Zp = (float)((double)|A| / q).  q > 0 and Zp > 0.
 *  7. Winner: key = (uint64(bits of Zp) << 32) | triangle index; every pixel of every view keeps the minimum key.
 *  8. Resolve.  An empty pixel has index RGBID_RASTER_EMPTY, depth and normal NaN with the bits RGBID_RASTER_NAN_BITS, colour 0 0 0.
 *     Another one the winner's index and Zp; colour channel k = floor(((pa ca_k + pb cb_k) + pc cc_k) / q + 0.5) clamped to 0 .. 255,
 *     in double; normal m_k = (pa na_k + pb nb_k) + pc nc_k in double, c = R_CW m with the float entries widened, each row
 *     ((r0 m0 + r1 m1) + r2 m2), g = (c0 c0 + c1 c1) + c2 c2, output (float)(c_k / sqrt(g)), 0 0 0 when g is 0 or not finite.
 *     Planes (device memory, each may be NULL): index uint32 [V][rows][cols], depth float32 [V][rows][cols], colour uint8
 *     [V][rows][cols][3], normal float32 [V][3][rows][cols].
 *  9. Counts, six uint64 per view: gated, degenerate, empty-box and drawn triangles, covered pixel tests that passed (fragments), pixels
 *     that are not empty.
 */
#ifndef RGBID_RASTER_H_
#define RGBID_RASTER_H_

#include <stdint.h>
#include "rgbid_render.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_RASTER_MAX_TRIANGLES 2147483647ull  /* 2^31 - 1: an index fits a key and RGBID_RASTER_EMPTY is nobody's */
#define RGBID_RASTER_MAX_VERTICES 2147483648ull   /* 2^31 */
#define RGBID_RASTER_MAX_DIM 16384                /* rows and cols at most: 256 (dim - 1) < 2^22 */
#define RGBID_RASTER_MAX_VIEWS 4096               /* views of one call at most: the handle holds their counts */
#define RGBID_RASTER_SUB 256                      /* sub-pixel positions per pixel */
#define RGBID_RASTER_VIEW_CHUNK 16                /* views one launch handles; further views go in further launches */
#define RGBID_RASTER_SMALL_BOX 16                 /* a drawn triangle whose box holds at most this many pixels is walked by one thread */
#define RGBID_RASTER_TILE 8                       /* larger boxes: tiles of TILE x TILE pixels aligned to the image, one wave per tile */
#define RGBID_RASTER_TIMED_CHUNKS 8               /* rgbid_raster_timing covers calls of up to this many chunks of views */
#define RGBID_RASTER_EMPTY 0xFFFFFFFFu            /* index of a pixel no triangle covers */
#define RGBID_RASTER_NAN_BITS 0x7FFFFFFFu         /* bits of every NaN in the depth and normal planes */

typedef struct rgbid_raster rgbid_raster;

/* a rasteriser for meshes of up to max_vertices (1 .. 2^31) vertices and max_triangles (1 .. 2^31 - 1) triangles and
 * rows * cols * V <= max_pixels_times_views per call (RGBID_E_INVALID otherwise); it works on the context's stream.  It holds 8 bytes per
 * pixel and view, 16 bytes per vertex and chunk view (256 per vertex) and 5 bytes per triangle and chunk view (80 per triangle: the flag
 * of the large path and the list of the flagged pairs), and 4 MiB for the counts of RGBID_RASTER_MAX_VIEWS views. */
int rgbid_raster_create(rgbid_raster** r, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles,
                        unsigned long long max_pixels_times_views);
int rgbid_raster_destroy(rgbid_raster* r);
/* steps 3 - 9: the mesh (device memory; vertices, normals and triangles 4-byte aligned; colours_dev and normals_dev may be NULL) into V
 * views of rows x cols pixels.  RGBID_E_INVALID before any launch, the handle usable afterwards and the outputs untouched, for: a NULL
 * handle, poses or K, V < 1 or V > RGBID_RASTER_MAX_VIEWS; rows or cols < 1 or > RGBID_RASTER_MAX_DIM; rows * cols * V above the handle's
 * capacity; z_min or z_max not finite, <= 0 or z_min > z_max; a pose or intrinsic that is not finite (as double or once rounded to
 * float32), fx or fy equal to 0; n_vertices or n_triangles above the capacities; triangles with n_vertices = 0; a NULL or misaligned
 * vertex or triangle buffer with a non-zero count; a misaligned normals buffer or index, depth or normal plane; with n_vertices > 0 a
 * colour plane without colours_dev or a normal plane without normals_dev.  The first kernel counts the triangles with an index >=
 * n_vertices and the host reads that count (the call's one synchronisation); with such a triangle RGBID_E_INVALID is returned, nothing
 * else is launched and the outputs are untouched.  Every kernel still tests an index before it uses it as an address.  n_triangles = 0
 * or n_vertices = 0 gives all-empty views.  Everything else is asynchronous on the context's stream: mesh and outputs must stay valid
 * until it ran. */
int rgbid_raster_views(rgbid_raster* r, const float* vertices_dev, unsigned long long n_vertices, const uint32_t* triangles_dev,
                       unsigned long long n_triangles, const uint8_t* colours_dev, const float* normals_dev, int V,
                       const rgbid_render_pose* poses, const float K[4], int rows, int cols, float z_min, float z_max, uint32_t* index_dev,
                       float* depth_dev, uint8_t* colour_dev, float* normal_dev);
/* step 9 of the last successful call, which must have had V views (RGBID_E_INVALID otherwise): out (host) uint64 [V][6].  Synchronises. */
int rgbid_raster_counts(rgbid_raster* r, int V, unsigned long long* out);
/* stage timing: enable != 0 records HIP events around the stages of the following calls; ms (optional, host) receives the device
 * milliseconds of the last one, summed over its chunks of views: project (with the clear), setup + small, large (with the list's
 * compaction), resolve; zeros for a call of more than RGBID_RASTER_TIMED_CHUNKS chunks.  Call it for ms after the call has completed. */
int rgbid_raster_timing(rgbid_raster* r, int enable, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif
