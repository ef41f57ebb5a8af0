// kernels_texture.hip -- a per-triangle texture atlas baked from the keyframes that see the mesh (include/rgbid_texture.h).
//
// The judge is tests/texture_mirror.py; atlas, views_used, best_view, uv and the six counts per view are byte-identical to it.
//   k_mesh_check            mesh_device.h: counts the triangles with an index >= n_v into one slot, copied to the host: a bad index ends add there
//   k_texture_add<BEST>     one thread per texel slot, tile-major (g = tile T^2 + j T + i), per chunk of up to RGBID_RECOLOUR_VIEW_CHUNK views in
//                           the kernel arguments: triangle, half and weights are decoded by integer arithmetic, the three corners are read (a
//                           wave's lanes share a few tiles: broadcasts), the point and the normal are formed once, the state is read once, the
//                           views are walked in order with the state in registers, the state is written once.  The classes of the used texels are
//                           counted as kernels_recolour.hip counts them (view_device.h): ballot per wave, LDS, one 64-bit atomic per block, view and non-zero
//                           class.  An unused slot takes part in the ballots with no class and touches no memory
//   k_texture_finish<BEST>  one thread per slot of the whole atlas (tiles beyond the last triangle's included): state -> the row-major planes
//   k_texture_uv            one thread per triangle
// State, [slots] each (slots = tiles T^2 of begin's layout): four uint64 planes -- MEAN S_0 S_1 S_2 W, BEST s_0 s_1 s_2 key -- and one
// uint32 plane `used`.  The pair's arithmetic is rgbid_recolour.h's steps 3 - 6, written out as in kernels_recolour.hip
// around view_device.h's rot_row, texel tests and accumulation.
//
// Exact arithmetic: every function that forms a product followed by a sum opens with RGBID_FP_STRICT (common.h), so the compiler forms no
// FMA from them; division and square root are hipcc's default correctly rounded ones.
#include "../../include/rgbid_texture.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"
#include "view_device.h"    // the view entry, rot_row, the texel tests, the accumulation, the class tally, step 7's byte; the host's checks

#include <cmath>

using namespace rgbid;

namespace {

constexpr int CHUNK = VIEWS_PER_CHUNK;
static_assert(VT == VIEW_BLOCK, "view_device.h's tally");

struct TextureGeom {                                        // begin's layout
  unsigned n_t, slots;                                      // slots = tiles T^2 <= 2^28
  int n, T, TT, tiles_x, W, H;
};

// steps 1 - 3: slot g -> its triangle and signed weights over n - 1; false for an unused texel (t may then name no triangle)
__device__ __forceinline__ bool texel_of(const TextureGeom& L, unsigned g, unsigned& tile, int& i_abs, int& j_abs, unsigned& t, int& wa, int& wb,
                                         int& wc) {
  tile = g / (unsigned)L.TT;
  const int r = (int)(g - tile * (unsigned)L.TT);
  j_abs = r / L.T;
  i_abs = r - j_abs * L.T;
  const bool upper = i_abs + j_abs > L.n;                   // the lower half lies in i + j <= n, the upper in i + j >= n + 2
  const int i = upper ? L.T - 1 - i_abs : i_abs, j = upper ? L.T - 1 - j_abs : j_abs;
  const int s = i + j;
  t = 2u * tile + (upper ? 1u : 0u);                        // tile < 2^28
  wa = (L.n - 1) - s; wb = i; wc = j;
  return (s <= L.n - 1 || (s == L.n && i >= 1 && i <= L.n - 1)) && t < L.n_t;
}

// step 4 for one component
__device__ __forceinline__ float texel_mix(int wa, int wb, int wc, int D, float a, float b, float c) {
  RGBID_FP_STRICT
  return (float)((((double)wa * (double)a + (double)wb * (double)b) + (double)wc * (double)c) / (double)D);
}

// steps 2 - 5 of one chunk of views.  counts: the count lines of the launch's first view
template <bool BEST>
__global__ __launch_bounds__(VT) void k_texture_add(const float* __restrict__ pos, const float* __restrict__ normals, unsigned n_v,
                                                    const unsigned* __restrict__ tri, TextureGeom L, ViewChunk vw, ViewCam cam, int nv,
                                                    unsigned first_view, unsigned long long* __restrict__ state, unsigned* __restrict__ used_plane,
                                                    unsigned long long* __restrict__ counts) {
  RGBID_FP_STRICT
  __shared__ unsigned tally[VIEW_WAVES][CHUNK * VIEW_N_COUNTS];
  const unsigned g = blockIdx.x * VT + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
  bool live = false, fin = false, facing = false;
  unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;       // MEAN: S_0 S_1 S_2 W; BEST: s_0 s_1 s_2 key
  unsigned used = 0;
  if (g < L.slots) {
    unsigned tile, t;
    int ia_, ja_, wa, wb, wc;
    live = texel_of(L, g, tile, ia_, ja_, t, wa, wb, wc);
    if (live) {                                             // t < n_t: the three indices are in the buffer
      const unsigned ia = tri[3 * (size_t)t], ib = tri[3 * (size_t)t + 1], ic = tri[3 * (size_t)t + 2];
      if (ia < n_v && ib < n_v && ic < n_v) {               // add refused such a mesh on the host; no index is an address untested
        const int D = L.n - 1;
        const float* A = pos + 3 * (size_t)ia; const float* B = pos + 3 * (size_t)ib; const float* Cc = pos + 3 * (size_t)ic;
        x = texel_mix(wa, wb, wc, D, A[0], B[0], Cc[0]);
        y = texel_mix(wa, wb, wc, D, A[1], B[1], Cc[1]);
        z = texel_mix(wa, wb, wc, D, A[2], B[2], Cc[2]);
        fin = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
        if (normals) {
          A = normals + 3 * (size_t)ia; B = normals + 3 * (size_t)ib; Cc = normals + 3 * (size_t)ic;
          n0 = texel_mix(wa, wb, wc, D, A[0], B[0], Cc[0]);
          n1 = texel_mix(wa, wb, wc, D, A[1], B[1], Cc[1]);
          n2 = texel_mix(wa, wb, wc, D, A[2], B[2], Cc[2]);
          const float q = (n0 * n0 + n1 * n1) + n2 * n2;
          facing = __builtin_isfinite(q) && q != 0.f;
        }
      }
      a0 = state[g]; a1 = state[(size_t)L.slots + g]; a2 = state[2 * (size_t)L.slots + g]; a3 = state[3 * (size_t)L.slots + g];
      used = used_plane[g];
    }
  }
  const int last_x = 256 * (cam.cols - 1), last_y = 256 * (cam.rows - 1);   // dims <= 16384: below 2^22
  for (int v = 0; v < nv; ++v) {
    const ViewEntry& view = vw.v[v];                        // wave-uniform: scalar registers
    const float* m = view.m;
    int cls = -1;                                           // an unused slot has no class
    if (live) {
      cls = VIEW_GATED;
      if (fin) {
        const float Z = rot_row(m + 6, x, y, z) + m[11];
        if (Z >= cam.z_min && Z <= cam.z_max) {             // NaN fails; z_max is finite, so infinity does too
          const float X = rot_row(m, x, y, z) + m[9];
          const float Y = rot_row(m + 3, x, y, z) + m[10];
          const float u = cam.fx * (X / Z) + cam.cx;
          const float w_ = cam.fy * (Y / Z) + cam.cy;
          const float xf = floorf(u * 256.0f + 0.5f);
          const float yf = floorf(w_ * 256.0f + 0.5f);
          if (fabsf(xf) <= 8388608.f && fabsf(yf) <= 8388608.f) {   // in float: nothing out of range reaches the cast
            const int xs = (int)xf, ys = (int)yf;
            cls = VIEW_OUTSIDE;
            if (xs >= 0 && xs <= last_x && ys >= 0 && ys <= last_y) {
              const int x0 = xs >> 8, y0 = ys >> 8, x1 = min(x0 + 1, cam.cols - 1), y1 = min(y0 + 1, cam.rows - 1);
              const unsigned ax = (unsigned)(xs & 255), ay = (unsigned)(ys & 255);
              // every texel index lies in the plane: 0 <= x0 <= x1 <= cols - 1, 0 <= y0 <= y1 <= rows - 1
              const size_t r0 = (size_t)y0 * (size_t)cam.cols, r1 = (size_t)y1 * (size_t)cam.cols;
              const size_t t00 = r0 + (size_t)x0, t10 = r0 + (size_t)x1, t01 = r1 + (size_t)x0, t11 = r1 + (size_t)x1;
              cls = VIEW_TAKEN;
              if (view.surface) {
                const float* d = view.surface;
                const float d00 = d[t00], d10 = d[t10], d01 = d[t01], d11 = d[t11];
                if (!(surface_ok(d00, Z, cam.tol_surface) && surface_ok(d10, Z, cam.tol_surface) && surface_ok(d01, Z, cam.tol_surface) &&
                      surface_ok(d11, Z, cam.tol_surface)))
                  cls = VIEW_HIDDEN;
              }
              if (cls == VIEW_TAKEN && view.measured) {
                const float* d = view.measured;
                const float m00 = d[t00], m10 = d[t10], m01 = d[t01], m11 = d[t11];
                if (!(measured_ok(m00, Z, cam.tol_measured) && measured_ok(m10, Z, cam.tol_measured) && measured_ok(m01, Z, cam.tol_measured) &&
                      measured_ok(m11, Z, cam.tol_measured)))
                  cls = VIEW_UNMEASURED;
              }
              unsigned w = RGBID_RECOLOUR_UNIT_WEIGHT;
              if (cls == VIEW_TAKEN && facing) {
                const double c0 = (double)rot_row(m, n0, n1, n2), c1 = (double)rot_row(m + 3, n0, n1, n2), c2 = (double)rot_row(m + 6, n0, n1, n2);
                const double Xd = (double)X, Yd = (double)Y, Zd = (double)Z;
                const double dot = -((c0 * Xd + c1 * Yd) + c2 * Zd);
                const double gg = (c0 * c0 + c1 * c1) + c2 * c2;
                const double rr = (Xd * Xd + Yd * Yd) + Zd * Zd;
                double cs = dot / sqrt(gg * rr);
                if (cam.two_sided) cs = fabs(cs);
                if (cs > 0.0 && cs >= cam.min_cos) {        // a NaN fails; cs <= 1 up to rounding, so the cast is in range
                  const unsigned f = (unsigned)floor(cs * 1024.0 + 0.5);
                  w = f < 1u ? 1u : f;
                } else {
                  cls = VIEW_AVERTED;
                }
              }
              if (cls == VIEW_TAKEN)
                view_accumulate<BEST>(view.colour, ViewSample{X, Y, Z, w, ax, ay, t00, t10, t01, t11}, first_view + (unsigned)v, a0, a1, a2, a3, used);
            }
          }
        }
      }
    }
    view_tally(tally, v, cls);
  }
  if (live) {
    state[g] = a0; state[(size_t)L.slots + g] = a1; state[2 * (size_t)L.slots + g] = a2; state[3 * (size_t)L.slots + g] = a3;
    used_plane[g] = used;
  }
  view_tally_add(tally, nv, counts);
}

// step 6's byte of a texel no view took: floor((2 q + D) / (2 D)) clamped, q = (wa ca + wb cb) + wc cc
__device__ __forceinline__ unsigned char fallback_byte(int wa, int wb, int wc, int D, unsigned ca, unsigned cb, unsigned cc) {
  const long long q = ((long long)wa * (long long)ca + (long long)wb * (long long)cb) + (long long)wc * (long long)cc;
  const long long num = 2 * q + D, den = 2 * (long long)D;
  const long long f = num >= 0 ? num / den : -((-num + den - 1) / den);
  return (unsigned char)(f < 0 ? 0 : f > 255 ? 255 : f);
}

// step 6 over every slot of the atlas, tile-major: `all` = tiles_x tile_rows T^2 >= L.slots; a tile beyond the last triangle's has no state
template <bool BEST>
__global__ __launch_bounds__(VT) void k_texture_finish(const unsigned long long* __restrict__ state, const unsigned* __restrict__ used_plane, TextureGeom L,
                                                       unsigned all, const unsigned* __restrict__ tri, const unsigned char* __restrict__ colours_in,
                                                       unsigned n_v, unsigned char* __restrict__ atlas, unsigned* __restrict__ views_used,
                                                       unsigned* __restrict__ best_view) {
  const unsigned g = blockIdx.x * VT + threadIdx.x;
  if (g >= all) return;
  unsigned tile, t;
  int i, j, wa, wb, wc;
  const bool live = texel_of(L, g, tile, i, j, t, wa, wb, wc);    // a tile without a triangle: t >= n_t
  const unsigned tx = tile % (unsigned)L.tiles_x, ty = tile / (unsigned)L.tiles_x;
  const size_t px = ((size_t)ty * L.T + j) * (size_t)L.W + ((size_t)tx * L.T + i);     // < W H <= 2^28
  unsigned used = 0;
  unsigned long long a3 = 0;
  if (live) { used = used_plane[g]; a3 = state[3 * (size_t)L.slots + g]; }
  if (views_used) views_used[px] = used;
  if (BEST && best_view) best_view[px] = used ? 0xFFFFFFFFu - (unsigned)a3 : RGBID_RECOLOUR_NO_VIEW;
  if (!atlas) return;
  unsigned char rgb[3] = {0, 0, 0};
  if (used) {
    for (int k = 0; k < 3; ++k) rgb[k] = view_state_byte<BEST>(state[(size_t)k * L.slots + g], a3);
  } else if (live && colours_in) {
    const unsigned ia = tri[3 * (size_t)t], ib = tri[3 * (size_t)t + 1], ic = tri[3 * (size_t)t + 2];
    if (ia < n_v && ib < n_v && ic < n_v)
      for (int k = 0; k < 3; ++k)
        rgb[k] = fallback_byte(wa, wb, wc, L.n - 1, colours_in[3 * (size_t)ia + k], colours_in[3 * (size_t)ib + k], colours_in[3 * (size_t)ic + k]);
  }
  for (int k = 0; k < 3; ++k) atlas[3 * px + k] = rgb[k];
}

// step 7: uv [n_t][3][2]
__global__ __launch_bounds__(VT) void k_texture_uv(TextureGeom L, float* __restrict__ uv) {
  const unsigned t = blockIdx.x * VT + threadIdx.x;
  if (t >= L.n_t) return;
  const unsigned tile = t >> 1;
  const int tx = (int)(tile % (unsigned)L.tiles_x), ty = (int)(tile / (unsigned)L.tiles_x);
  const int ci[3] = {0, L.n - 1, 0}, cj[3] = {0, 0, L.n - 1};
  for (int c = 0; c < 3; ++c) {
    const int i = (t & 1u) ? L.T - 1 - ci[c] : ci[c], j = (t & 1u) ? L.T - 1 - cj[c] : cj[c];
    const int col = tx * L.T + i, row = ty * L.T + j;
    uv[6 * (size_t)t + 2 * c] = (float)((double)(2 * col + 1) / (double)(2 * L.W));
    uv[6 * (size_t)t + 2 * c + 1] = (float)((double)(2 * (L.H - 1 - row) + 1) / (double)(2 * L.H));
  }
}

// step 1 on the host; tiles_x T and tile_rows T are held to the limit before they are ints
bool layout_of(unsigned long long n_t, int patch, int tiles_x, rgbid_texture_layout_t* out) {
  if (patch < RGBID_TEXTURE_MIN_PATCH || patch > RGBID_TEXTURE_MAX_PATCH || tiles_x < 1 || n_t > RGBID_TEXTURE_MAX_TRIANGLES) return false;
  const unsigned long long T = (unsigned long long)patch + 2, tiles = (n_t + 1) / 2;
  unsigned long long tile_rows = (tiles + (unsigned long long)tiles_x - 1) / (unsigned long long)tiles_x;
  if (tile_rows < 1) tile_rows = 1;
  if ((unsigned long long)tiles_x * T > RGBID_RASTER_MAX_DIM || tile_rows * T > RGBID_RASTER_MAX_DIM) return false;
  out->T = (int)T; out->W = (int)((unsigned long long)tiles_x * T); out->H = (int)(tile_rows * T);
  out->tiles = tiles; out->tile_rows = (int)tile_rows;
  out->texels_per_triangle = patch * (patch + 1) / 2 + (patch - 1);
  return true;
}

enum { M_ADD0 = 0, M_ADD1, M_FIN0, M_FIN1, MARKS };

}  // namespace

struct rgbid_texture {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0, cap_slots = 0;
  unsigned long long* state = nullptr;         // 36 bytes per slot of capacity: [4][slots] uint64, then [slots] uint32
  unsigned long long* counts = nullptr;        // [MAX_VIEWS][VIEW_COUNT_LINE]
  unsigned* bad = nullptr;                     // the count of k_mesh_check
  unsigned* bad_host = nullptr;                // pinned
  bool begun = false;
  TextureGeom geom = {};                       // begin's
  int tile_rows = 1;
  int mode = RGBID_RECOLOUR_MEAN, views = 0;   // views since begin
  bool timed[2] = {false, false};              // whether the last add / the last finish was recorded
  Buffers buf;
  StageTimer<MARKS> timer;
  unsigned* used_plane() const { return reinterpret_cast<unsigned*>(state + 4 * (size_t)geom.slots); }
};

extern "C" {

int rgbid_texture_layout(unsigned long long n_triangles, int patch, int tiles_x, rgbid_texture_layout_t* out) {
  rgbid_texture_layout_t l;
  if (!out || !layout_of(n_triangles, patch, tiles_x, &l)) return RGBID_E_INVALID;
  *out = l;
  return RGBID_OK;
}

int rgbid_texture_create(rgbid_texture** out, rgbid_ctx* ctx, unsigned long long max_triangles, unsigned long long max_texels) {
  if (out) *out = nullptr;                     // also when the texel capacity is refused
  if (max_texels < 1 || max_texels > RGBID_TEXTURE_MAX_TEXELS) return RGBID_E_INVALID;
  return mesh_create(out, ctx, RGBID_RECOLOUR_MAX_VERTICES, max_triangles, RGBID_RECOLOUR_MAX_VERTICES, RGBID_TEXTURE_MAX_TRIANGLES, [&](rgbid_texture* h) {
    h->cap_slots = max_texels;
    int e = h->buf.alloc(&h->state, (size_t)max_texels * 36 + 4);   // the uint32 plane ends on a whole 8 bytes
    if (!e) e = h->buf.alloc(&h->counts, sizeof(unsigned long long) * VIEW_COUNT_LINE * RGBID_RECOLOUR_MAX_VIEWS);
    if (!e) e = h->buf.alloc(&h->bad, sizeof(unsigned));
    if (!e) e = h->buf.alloc_host(&h->bad_host, sizeof(unsigned));
    return e;
  });
}

int rgbid_texture_destroy(rgbid_texture* h) { return destroy_handle(h); }   // a launch may still read the state

int rgbid_texture_begin(rgbid_texture* h, unsigned long long n_triangles, int patch, int tiles_x, int mode) {
  rgbid_texture_layout_t l;
  if (!h || (mode != RGBID_RECOLOUR_MEAN && mode != RGBID_RECOLOUR_BEST) || !layout_of(n_triangles, patch, tiles_x, &l)) return RGBID_E_INVALID;
  const unsigned long long slots = l.tiles * (unsigned long long)(l.T * l.T);   // <= W H <= 2^28
  if (n_triangles > h->cap_t || slots > h->cap_slots) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  if (slots) RGBID_HIP(hipMemsetAsync(h->state, 0, (size_t)slots * 36, h->ctx->stream));
  TextureGeom& g = h->geom;
  g.n_t = (unsigned)n_triangles; g.slots = (unsigned)slots; g.n = patch; g.T = l.T; g.TT = l.T * l.T; g.tiles_x = tiles_x; g.W = l.W; g.H = l.H;
  h->tile_rows = l.tile_rows;
  h->begun = true; h->mode = mode; h->views = 0;            // a view's count line is cleared when the view is added
  return RGBID_OK;
}

int rgbid_texture_add(rgbid_texture* h, const float* vertices_dev, const float* normals_dev, unsigned long long n_vertices,
                      const uint32_t* triangles_dev, unsigned long long n_triangles, int V, const rgbid_recolour_view* views, const float K[4],
                      int rows, int cols, const rgbid_recolour_params* params) {
  if (!h || !views || !K || !params || V < 1 || !h->begun || V > RGBID_RECOLOUR_MAX_VIEWS - h->views) return RGBID_E_INVALID;
  if (n_triangles != h->geom.n_t) return RGBID_E_INVALID;
  if (!view_camera_ok(K, rows, cols, *params)) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  if (n_vertices && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  if (!aligned4(normals_dev)) return RGBID_E_INVALID;
  for (int v = 0; v < V; ++v) if (!view_ok(views[v])) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t st = h->ctx->stream;
  const TextureGeom& L = h->geom;
  const unsigned n_v = (unsigned)n_vertices;                // 2^31 at most
  if (L.n_t) {
    RGBID_HIP(hipMemsetAsync(h->bad, 0, sizeof(unsigned), st));
    check_triangles(st, triangles_dev, L.n_t, n_v, h->bad);
    RGBID_HIP(hipGetLastError());
    RGBID_HIP(hipMemcpyAsync(h->bad_host, h->bad, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    RGBID_HIP(hipStreamSynchronize(st));
    if (*h->bad_host) return RGBID_E_INVALID;               // a triangle names a vertex that does not exist
  }
  unsigned long long* lines = h->counts + (size_t)h->views * VIEW_COUNT_LINE;
  RGBID_HIP(hipMemsetAsync(lines, 0, sizeof(unsigned long long) * VIEW_COUNT_LINE * (size_t)V, st));
  const ViewCam cam = view_cam(K, rows, cols, *params);
  h->timed[0] = false;
  h->timer.mark(M_ADD0, st);
  ViewChunk vw;
  for (int v0 = 0; L.slots && v0 < V; v0 += CHUNK) {
    const int nv = V - v0 < CHUNK ? V - v0 : CHUNK;
    view_pack(views + v0, nv, vw);
    const unsigned first_view = (unsigned)(h->views + v0);  // global index of the launch's first view
    const dim3 grid((L.slots + VT - 1) / VT), block(VT);
    if (h->mode == RGBID_RECOLOUR_BEST)
      hipLaunchKernelGGL(k_texture_add<true>, grid, block, 0, st, vertices_dev, normals_dev, n_v, triangles_dev, L, vw, cam, nv, first_view, h->state,
                         h->used_plane(), lines + (size_t)v0 * VIEW_COUNT_LINE);
    else
      hipLaunchKernelGGL(k_texture_add<false>, grid, block, 0, st, vertices_dev, normals_dev, n_v, triangles_dev, L, vw, cam, nv, first_view, h->state,
                         h->used_plane(), lines + (size_t)v0 * VIEW_COUNT_LINE);
  }
  h->timer.mark(M_ADD1, st);
  h->timed[0] = h->timer.on;
  RGBID_HIP(hipGetLastError());
  h->views += V;
  return RGBID_OK;
}

int rgbid_texture_finish(rgbid_texture* h, const uint32_t* triangles_dev, const uint8_t* colours_in_dev, unsigned long long n_vertices,
                         uint8_t* atlas_dev, uint32_t* views_used_dev, uint32_t* best_view_dev) {
  if (!h || !h->begun || !aligned4(views_used_dev) || !aligned4(best_view_dev)) return RGBID_E_INVALID;
  if (best_view_dev && h->mode != RGBID_RECOLOUR_BEST) return RGBID_E_INVALID;
  const TextureGeom& L = h->geom;
  if (colours_in_dev && !mesh_in_ok(n_vertices, L.n_t, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t st = h->ctx->stream;
  h->timed[1] = false;
  h->timer.mark(M_FIN0, st);
  if (atlas_dev || views_used_dev || best_view_dev) {
    const unsigned all = (unsigned)L.W * (unsigned)L.H;     // <= 2^28
    const dim3 grid((all + VT - 1) / VT), block(VT);
    if (h->mode == RGBID_RECOLOUR_BEST)
      hipLaunchKernelGGL(k_texture_finish<true>, grid, block, 0, st, h->state, h->used_plane(), L, all, triangles_dev, colours_in_dev, (unsigned)n_vertices,
                         atlas_dev, views_used_dev, best_view_dev);
    else
      hipLaunchKernelGGL(k_texture_finish<false>, grid, block, 0, st, h->state, h->used_plane(), L, all, triangles_dev, colours_in_dev, (unsigned)n_vertices,
                         atlas_dev, views_used_dev, best_view_dev);
  }
  h->timer.mark(M_FIN1, st);
  h->timed[1] = h->timer.on;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_texture_uv(rgbid_texture* h, float* uv_dev) {
  if (!h || !h->begun || !aligned4(uv_dev) || (h->geom.n_t && !uv_dev)) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  if (h->geom.n_t) {
    hipLaunchKernelGGL(k_texture_uv, dim3((h->geom.n_t + VT - 1) / VT), dim3(VT), 0, h->ctx->stream, h->geom, uv_dev);
    RGBID_HIP(hipGetLastError());
  }
  return RGBID_OK;
}

int rgbid_texture_counts(rgbid_texture* h, int first_view, int V, unsigned long long* out) {
  if (!h || !out || !h->begun || first_view < 0 || V < 1 || first_view > h->views || V > h->views - first_view) return RGBID_E_INVALID;
  return view_counts_read(h->ctx, h->counts + (size_t)first_view * VIEW_COUNT_LINE, V, out);
}

int rgbid_texture_timing(rgbid_texture* h, int enable, float ms[2]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  if (ms) {
    static const int pairs[2][4] = {{M_ADD0, M_ADD1, 0, 0}, {M_FIN0, M_FIN1, 0, 0}};
    if (int e = stage_times(h->timer, h->timed, pairs, ms)) return e;
  }
  return h->timer.enable(enable != 0);
}

}  // extern "C"
