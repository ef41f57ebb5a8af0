/*
 * rgbid_texture.h -- C-ABI of the texturing stage of the surface chain: every triangle of an indexed triangle mesh in device memory gets
 * a right-angled patch of an image (the atlas), every texel of a patch is a point of the triangle's plane, and that point is projected
 * into the keyframes, gated, sampled and accumulated exactly as rgbid_recolour.h does it for a vertex.  A mesh of few triangles then keeps
 * the keyframes' resolution in an image.  No unwrapping: two triangles share a square tile.  The reference has no mesh and no program text
 * for it.
 *
 * Contract (byte-identical to tests/texture_mirror.py).  Integers decide everything that is accumulated; float32 and
 * double are used without contraction; nothing depends on execution order or on how the views are split over calls.  The views, the
 * parameters, the two modes and the constants are rgbid_recolour.h's, unchanged.
 *  1. Layout.  n_t triangles, a patch size n (texels along a leg, 2 .. 30), tiles_x >= 1.  T = n + 2, tiles = ceil(n_t / 2),
 *     tile_rows = max(1, ceil(tiles / tiles_x)), W = tiles_x T, H = tile_rows T, both <= RGBID_RASTER_MAX_DIM.  Triangle t lives in tile
 *     t >> 1, which sits at column (t >> 1) % tiles_x and row (t >> 1) / tiles_x of the tiles; its half is t & 1.
 *     P = n (n + 1) / 2 + (n - 1) texels per triangle.
 *  2. Texels of a half, tile-local (i, j) = (column, row).  The lower half (t & 1 = 0) uses the texels with i + j <= n - 1 and the gutter
 *     i + j = n with 1 <= i <= n - 1.  The upper half uses the same set at (T - 1 - i, T - 1 - j).  Every other texel of the atlas is
 *     unused: the rest of a tile, tiles beyond `tiles`, the upper half of the last tile when n_t is odd.  A bilinear look-up anywhere in
 *     a triangle's uv triangle (step 7) touches with non-zero weight only texels of its own set.
 *  3. Corners and weights.  Corner a sits on the texel centre (0, 0), b on (n - 1, 0), c on (0, n - 1) of the lower half; the upper half
 *     mirrors this.  Texel (i, j) has the signed integer weights wa = (n - 1) - i - j, wb = i, wc = j over D = n - 1; wa = -1 on the
 *     gutter, whose texels are extrapolated one step past the hypotenuse in the triangle's plane.
 *  4. Texel point, per component k, from the float32 corners A, B, C widened to double:
 *     p_k = (float)((((double)wa A_k + (double)wb B_k) + (double)wc C_k) / (double)D).  With normals, nrm_k is formed the same way from
 *     the three vertex normals.  A non-finite corner makes the point non-finite through the arithmetic (0 * inf is NaN).
 *  5. Pair (texel, view).  p and nrm go through steps 3 - 6 of rgbid_recolour.h word for word: the projection and its gates, the six
 *     classes GATED, OUTSIDE, HIDDEN, UNMEASURED, AVERTED, TAKEN in their order, the four-texel gates, the weight, the integer sample, and
 *     the MEAN or BEST accumulation in uint64.
 *  6. rgbid_texture_finish.  A used texel that some view took: the colour of rgbid_recolour.h's step 7.  A used texel no view took: with
 *     colours_in (vertex colours uint8 [n_v][3]) per channel q = (wa ca + wb cb) + wc cc in int64 and the byte
 *     clamp(floor((2 q + D) / (2 D)), 0, 255) (round half up; q may be negative on the gutter); without colours_in 0 0 0.  An unused
 *     texel: 0 0 0, views_used 0, best_view RGBID_RECOLOUR_NO_VIEW.  Outputs (device memory, each may be NULL): atlas uint8 [H][W][3],
 *     views_used uint32 [H][W], for BEST best_view uint32 [H][W].  The image origin is top-left.  finish only reads the state: it may
 *     be repeated and views may follow it.
 *  7. rgbid_texture_uv.  float32 [n_t][3][2], per corner from the corner's atlas texel (col, row):
 *     u = (float)((double)(2 col + 1) / (double)(2 W)), v = (float)((double)(2 (H - 1 - row) + 1) / (double)(2 H)): the uv origin is
 *     bottom-left, as OBJ has it.
 *  8. Counts.  Six uint64 per view since begin, the (used texel, view) pairs per class in the order of step 5; they sum to n_t P.
 */
#ifndef RGBID_TEXTURE_H_
#define RGBID_TEXTURE_H_

#include <stdint.h>
#include "rgbid_recolour.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_TEXTURE_MIN_PATCH 2
#define RGBID_TEXTURE_MAX_PATCH 30                  /* T = 32 at most: a tile is at most 1024 slots */
#define RGBID_TEXTURE_MAX_TRIANGLES 2147483647ull   /* 2^31 - 1 */
#define RGBID_TEXTURE_MAX_TEXELS 268435456ull       /* 2^28 = RGBID_RASTER_MAX_DIM squared: slots of a handle at most */

typedef struct rgbid_texture_layout_t {
  int T;                                   /* side of a tile: patch + 2 */
  int W, H;                                /* the atlas */
  unsigned long long tiles;                /* tiles that hold a triangle: ceil(n_t / 2) */
  int tile_rows;
  int texels_per_triangle;                 /* P */
} rgbid_texture_layout_t;

typedef struct rgbid_texture rgbid_texture;

/* step 1 on the host, without a device.  RGBID_E_INVALID, *out untouched, for: a NULL out, patch outside 2 .. 30, tiles_x < 1, W or H above
 * RGBID_RASTER_MAX_DIM, n_triangles > 2^31 - 1. */
int rgbid_texture_layout(unsigned long long n_triangles, int patch, int tiles_x, rgbid_texture_layout_t* out);
/* a handle for meshes of up to max_triangles (1 .. 2^31 - 1) triangles whose layouts have at most max_texels (1 .. 2^28) slots, a slot
 * being a texel of a tile that holds a triangle: tiles T^2 of them (RGBID_E_INVALID otherwise).  It holds 36 bytes per slot (four 64-bit
 * sums and the count of views) and 4 MiB for the counts of RGBID_RECOLOUR_MAX_VIEWS views, and works on the context's stream. */
int rgbid_texture_create(rgbid_texture** h, rgbid_ctx* ctx, unsigned long long max_triangles, unsigned long long max_texels);
int rgbid_texture_destroy(rgbid_texture* h);
/* step 1: clears the state and numbers the following views from 0.  RGBID_E_INVALID, the handle usable afterwards and its state as it
 * was, for: a NULL handle, what rgbid_texture_layout refuses, n_triangles above the capacity, tiles T^2 above max_texels, a mode that is
 * neither RGBID_RECOLOUR_MEAN nor RGBID_RECOLOUR_BEST.  n_triangles = 0 is legal.  Asynchronous. */
int rgbid_texture_begin(rgbid_texture* h, unsigned long long n_triangles, int patch, int tiles_x, int mode);
/* steps 2 - 5 for V further views.  RGBID_E_INVALID before any launch, the handle usable afterwards, state and counts untouched, for:
 * everything rgbid_recolour_add refuses (with n_triangles other than begin's in the place of n_vertices); and the mesh as
 * rgbid_raster_views refuses it: n_triangles > 0 with NULL or misaligned triangles or with n_vertices = 0, n_vertices above 2^31, a
 * triangle that names a vertex >= n_vertices (the call waits once for that count).  With n_triangles = 0 the views are numbered and
 * counted (all zeros) and nothing else happens.  Otherwise asynchronous on the context's stream: mesh and planes must stay valid. */
int rgbid_texture_add(rgbid_texture* h, const float* vertices_dev, const float* normals_dev, unsigned long long n_vertices,
                      const uint32_t* triangles_dev, unsigned long long n_triangles, int V, const rgbid_recolour_view* views, const float K[4],
                      int rows, int cols, const rgbid_recolour_params* params);
/* step 6 for begin's layout.  triangles_dev, colours_in_dev and n_vertices are read only for the texels no view took; colours_in_dev may
 * be NULL.  RGBID_E_INVALID before any launch, the outputs untouched, for: a NULL handle, no begin, a misaligned views_used or best_view,
 * a best_view after a begin with RGBID_RECOLOUR_MEAN, colours_in with n_triangles > 0 and NULL or misaligned triangles or n_vertices = 0 or
 * above 2^31.  The kernel tests every index before it is an address: a triangle that names a vertex >= n_vertices falls back to 0 0 0.
 * The state is not changed.  Asynchronous. */
int rgbid_texture_finish(rgbid_texture* h, const uint32_t* triangles_dev, const uint8_t* colours_in_dev, unsigned long long n_vertices,
                         uint8_t* atlas_dev, uint32_t* views_used_dev, uint32_t* best_view_dev);
/* step 7 for begin's layout: uv_dev float32 [n_t][3][2].  RGBID_E_INVALID for a NULL handle, no begin, a NULL (with n_t > 0) or misaligned
 * uv_dev.  Asynchronous. */
int rgbid_texture_uv(rgbid_texture* h, float* uv_dev);
/* step 8 of the views first_view .. first_view + V - 1 since begin, which must have been added (RGBID_E_INVALID otherwise, and for a NULL
 * handle or out, first_view < 0 or V < 1): out (host) uint64 [V][6].  Synchronises. */
int rgbid_texture_counts(rgbid_texture* h, int first_view, int V, unsigned long long* out);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the
 * last add (accumulate, all its launches) and of the last finish (resolve).  Call it for ms after the calls have completed. */
int rgbid_texture_timing(rgbid_texture* h, int enable, float ms[2]);

#ifdef __cplusplus
}
#endif
#endif
