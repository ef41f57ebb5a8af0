// kernels_raster.hip -- an indexed triangle mesh seen from camera poses (include/rgbid_raster.h).
//
// The judge is tests/raster_mirror.py; every plane and the six counts per view are byte-identical to it.
//   k_mesh_check    mesh_device.h: counts the triangles with an index >= n_v into one slot, copied to the host: a bad index ends the call here
//   k_rast_clear    the key buffer [V][rows][cols] of uint64 is set to all ones, 16 bytes per store
// then per chunk of up to RGBID_RASTER_VIEW_CHUNK views, their twelve floats each in the kernel arguments:
//   k_rast_project  one thread per vertex, the chunk's views in an inner loop: the 16-byte record xs, ys, Z, usable per (view, vertex)
//   k_rast_setup    one thread per (triangle, view): class and class counts; a drawn triangle whose box holds at most SMALL_BOX pixels is
//                   walked here, a larger one sets its flag byte
//   flag compaction voxel_device.h, stable: the flagged (view, triangle) pairs in ascending order, their number in a device slot
//   k_rast_large    one block per listed pair: its waves take the 8 x 8 tiles of the box in turn, one lane per pixel; a tile is skipped when
//                   one edge function is negative at all four of its corners
//   k_rast_resolve  one thread per pixel and view: key -> the winner's triangle, its three records and attributes -> the planes
//   k_rast_sum      once per call: the per-view counts from their COUNT_SLOTS copies
// Both raster paths evaluate a pixel through raster_pixel: coverage in int64, depth in double, one 64-bit integer atomic minimum on
// global memory.  No float atomics, no wait on another thread, every loop has its bound when it starts.
//
// Exact arithmetic: every function that forms a product followed by a sum opens with RGBID_FP_STRICT (common.h), so the compiler forms no
// FMA from them; division and square root are hipcc's default correctly rounded ones.
#include "../../include/rgbid_raster.h"
#include "common.h"
#include "hip_host.h"
#include "view_device.h"    // rot_row
#include "mesh_device.h"    // the index check, the argument test, the create; voxel_device.h's VT, grid_of, the stable flag compaction

#include <cmath>

using namespace rgbid;

namespace {

enum { SLOT_BAD = 9 };                                      // beside the workspace's own 0 .. 8; SLOT_RUNS holds the listed pairs
static_assert(SLOT_VOXELS < SLOT_BAD && SLOT_BAD < SLOTS, "the slot of this file lies behind the workspace's");

constexpr unsigned long long EMPTY_KEY = ~0ull;
constexpr unsigned long long MAX_PIXEL_VIEWS = 1ull << 38;  // 2 TiB of keys: keeps every grid below 2^31 blocks
constexpr unsigned LARGE_GRID = 8192;                       // blocks of k_rast_large at most; they stride over the list
constexpr int SMALL_BOX = RGBID_RASTER_SMALL_BOX, TILE = RGBID_RASTER_TILE, SUB = RGBID_RASTER_SUB;
constexpr int N_COUNTS = 6;
// Every wave adds to its view's counts.  One address per view and count would serialise those atomics (about 11 ns each on one line: the
// 18 470 waves of a 1.18 M triangle mesh spent 0.6 ms there), so a view has COUNT_SLOTS copies of its counts, one 64-byte line each, a block
// adds to the copy blockIdx.x mod COUNT_SLOTS and k_rast_sum adds the copies up at the end of the call: integer sums, the same whatever the order.
constexpr int COUNT_SLOTS = 16, COUNT_LINE = 8;
enum { C_GATED = 0, C_DEGENERATE, C_EMPTY_BOX, C_DRAWN, C_FRAGMENTS, C_PIXELS };
static_assert(TILE * TILE == 64, "one wave per tile, one lane per pixel");
static_assert(SMALL_BOX >= 1 && SMALL_BOX <= 64, "a thread's walk stays short");

struct RasterViews {                                        // kernel argument: 16 x 12 floats = 768 bytes
  float m[RGBID_RASTER_VIEW_CHUNK][12];                     // r00 r01 r02 r10 r11 r12 r20 r21 r22 tx ty tz
};

struct RasterCam {
  float fx, fy, cx, cy, z_min, z_max;
  int rows, cols, nv;                                       // nv: views of this launch
};

struct RasterVertex {                                       // the record of step 3
  int xs, ys;
  float Z;
  unsigned usable;
};
static_assert(sizeof(RasterVertex) == 16, "one 16-byte load");

__global__ __launch_bounds__(VT) void k_rast_clear(uint4* __restrict__ keys, size_t n16) {
  const size_t i = (size_t)blockIdx.x * VT + threadIdx.x;
  if (i < n16) keys[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// step 3: rec[view][vertex]; the position is read once for all views of the chunk
__global__ __launch_bounds__(VT) void k_rast_project(const float* __restrict__ pos, unsigned n_v, RasterViews vw, RasterCam cam,
                                                     RasterVertex* __restrict__ rec) {
  RGBID_FP_STRICT
  const unsigned i = blockIdx.x * VT + threadIdx.x;
  if (i >= n_v) return;
  const float x = pos[3 * (size_t)i], y = pos[3 * (size_t)i + 1], z = pos[3 * (size_t)i + 2];
  const bool fin = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
  for (int v = 0; v < cam.nv; ++v) {
    const float* m = vw.m[v];                               // wave-uniform: scalar registers
    RasterVertex o{0, 0, 0.f, 0u};
    if (fin) {
      const float Z = rot_row(m + 6, x, y, z) + m[11];
      if (Z >= cam.z_min && Z <= cam.z_max) {               // NaN fails; z_max is finite, so infinity does too
        const float X = rot_row(m, x, y, z) + m[9];
        const float Y = rot_row(m + 3, x, y, z) + m[10];
        const float u = cam.fx * (X / Z) + cam.cx;
        const float w = cam.fy * (Y / Z) + cam.cy;
        const float xs = floorf(u * 256.0f + 0.5f);
        const float ys = floorf(w * 256.0f + 0.5f);
        if (fabsf(xs) <= 8388608.f && fabsf(ys) <= 8388608.f) {   // in float: nothing out of range reaches the cast
          o.xs = (int)xs; o.ys = (int)ys; o.Z = Z; o.usable = 1u;
        }
      }
    }
    rec[(size_t)v * n_v + i] = o;
  }
}

// a triangle of one view after step 4: the snapped corners, s, |A| and the inverse depths of step 6
struct RasterTri {
  long long xa, ya, xb, yb, xc, yc, s, absA;
  double wa, wb, wc;
};

// steps 4: -> the class (C_GATED .. C_DRAWN); for a drawn triangle `tr` and the pixel box
__device__ __forceinline__ int raster_classify(const RasterVertex& a, const RasterVertex& b, const RasterVertex& c, int rows, int cols, RasterTri& tr,
                                               int& x0, int& x1, int& y0, int& y1) {
  if (!(a.usable && b.usable && c.usable)) return C_GATED;
  tr.xa = a.xs; tr.ya = a.ys; tr.xb = b.xs; tr.yb = b.ys; tr.xc = c.xs; tr.yc = c.ys;
  const long long A = (tr.xb - tr.xa) * (tr.yc - tr.ya) - (tr.yb - tr.ya) * (tr.xc - tr.xa);
  if (A == 0) return C_DEGENERATE;
  tr.s = A > 0 ? 1 : -1;
  tr.absA = A > 0 ? A : -A;
  const int lo_x = min(a.xs, min(b.xs, c.xs)), hi_x = max(a.xs, max(b.xs, c.xs));
  const int lo_y = min(a.ys, min(b.ys, c.ys)), hi_y = max(a.ys, max(b.ys, c.ys));
  x0 = max(0, (lo_x + (SUB - 1)) >> 8);                     // an arithmetic shift floors towards -inf; |xs| <= 2^23, no overflow
  x1 = min(cols - 1, hi_x >> 8);
  y0 = max(0, (lo_y + (SUB - 1)) >> 8);
  y1 = min(rows - 1, hi_y >> 8);
  if (x0 > x1 || y0 > y1) return C_EMPTY_BOX;
  tr.wa = 1.0 / (double)a.Z; tr.wb = 1.0 / (double)b.Z; tr.wc = 1.0 / (double)c.Z;
  return C_DRAWN;
}

// step 5: the three edge functions at pixel (px, py)
__device__ __forceinline__ void raster_edges(const RasterTri& tr, int px, int py, long long& Ea, long long& Eb, long long& Ec) {
  const long long Px = (long long)SUB * px, Py = (long long)SUB * py;
  Ea = tr.s * ((tr.xc - tr.xb) * (Py - tr.yb) - (tr.yc - tr.yb) * (Px - tr.xb));
  Eb = tr.s * ((tr.xa - tr.xc) * (Py - tr.yc) - (tr.ya - tr.yc) * (Px - tr.xc));
  Ec = tr.s * ((tr.xb - tr.xa) * (Py - tr.ya) - (tr.yb - tr.ya) * (Px - tr.xa));
}

// step 6's weights of a covered pixel
__device__ __forceinline__ void raster_weights(const RasterTri& tr, long long Ea, long long Eb, long long Ec, double& pa, double& pb, double& pc,
                                               double& q) {
  RGBID_FP_STRICT
  pa = (double)Ea * tr.wa; pb = (double)Eb * tr.wb; pc = (double)Ec * tr.wc;
  q = (pa + pb) + pc;
}

// steps 5 - 7 for one pixel of one triangle, the one function both paths draw through -> whether the pixel is covered
__device__ __forceinline__ bool raster_pixel(const RasterTri& tr, unsigned t, int px, int py, unsigned long long* __restrict__ view, int cols) {
  RGBID_FP_STRICT
  long long Ea, Eb, Ec;
  raster_edges(tr, px, py, Ea, Eb, Ec);
  if (!(Ea >= 0 && Eb >= 0 && Ec >= 0)) return false;
  double pa, pb, pc, q;
  raster_weights(tr, Ea, Eb, Ec, pa, pb, pc, q);
  const float Zp = (float)((double)tr.absA / q);
  const unsigned long long key = ((unsigned long long)__float_as_uint(Zp) << 32) | t;   // Zp > 0: its bits order like its value
  unsigned long long* at = view + (size_t)py * (size_t)cols + (size_t)px;
  // A plain load first: a key only ever decreases, so a stale value is never smaller than the current one and a pixel that already holds
  // a key that is not larger cannot be won: the atomic is skipped (rgbid_render.h's argument).
  if (*at > key) (void)__hip_atomic_fetch_min(at, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// the three records of triangle t in one view; false (nothing read through a bad index) when an index names no vertex
__device__ __forceinline__ bool raster_corners(const unsigned* __restrict__ tri, unsigned t, unsigned n_v, const RasterVertex* __restrict__ rec,
                                               unsigned& ia, unsigned& ib, unsigned& ic, RasterVertex& a, RasterVertex& b, RasterVertex& c) {
  ia = tri[3 * (size_t)t]; ib = tri[3 * (size_t)t + 1]; ic = tri[3 * (size_t)t + 2];
  if (!(ia < n_v && ib < n_v && ic < n_v)) return false;
  a = rec[ia]; b = rec[ib]; c = rec[ic];
  return true;
}

// the counts of view v (of the launch) that this block adds to
__device__ __forceinline__ unsigned long long* count_line(unsigned long long* parts, unsigned v) {
  return parts + ((size_t)v * COUNT_SLOTS + (blockIdx.x & (COUNT_SLOTS - 1))) * COUNT_LINE;
}

// view = blockIdx.y of this launch.  counts: the count lines of the launch's first view; flags: [view][n_t] bytes
__global__ __launch_bounds__(VT) void k_rast_setup(const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v, const RasterVertex* __restrict__ rec,
                                                   RasterCam cam, unsigned long long* __restrict__ keys, unsigned char* __restrict__ flags,
                                                   unsigned long long* __restrict__ counts) {
  const unsigned t = blockIdx.x * VT + threadIdx.x;
  const int v = blockIdx.y;
  const size_t npix = (size_t)cam.rows * (size_t)cam.cols;
  int cls = -1;                                             // a thread behind the last triangle has no class
  unsigned frags = 0;
  if (t < n_t) {
    unsigned ia, ib, ic;
    RasterVertex a, b, c;
    RasterTri tr;
    int x0 = 0, x1 = -1, y0 = 0, y1 = -1;
    cls = raster_corners(tri, t, n_v, rec + (size_t)v * n_v, ia, ib, ic, a, b, c) ? raster_classify(a, b, c, cam.rows, cam.cols, tr, x0, x1, y0, y1)
                                                                                   : (int)C_GATED;
    bool large = false;
    if (cls == C_DRAWN) {
      const long long box = (long long)(x1 - x0 + 1) * (long long)(y1 - y0 + 1);
      large = box > SMALL_BOX;
      if (!large) {
        unsigned long long* view = keys + (size_t)v * npix;
        for (int y = y0; y <= y1; ++y)                      // at most SMALL_BOX pixels
          for (int x = x0; x <= x1; ++x) frags += raster_pixel(tr, t, x, y, view, cam.cols) ? 1u : 0u;
      }
    }
    flags[(size_t)v * n_t + t] = large ? 1 : 0;
  }
  // wave sums, one integer atomic per wave and count
  const unsigned n_gated = (unsigned)__popcll(__ballot(cls == C_GATED)), n_deg = (unsigned)__popcll(__ballot(cls == C_DEGENERATE));
  const unsigned n_box = (unsigned)__popcll(__ballot(cls == C_EMPTY_BOX)), n_drawn = (unsigned)__popcll(__ballot(cls == C_DRAWN));
  frags = wave_sum(frags);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* c = count_line(counts, v);
    if (n_gated) atomicAdd(c + C_GATED, (unsigned long long)n_gated);
    if (n_deg) atomicAdd(c + C_DEGENERATE, (unsigned long long)n_deg);
    if (n_box) atomicAdd(c + C_EMPTY_BOX, (unsigned long long)n_box);
    if (n_drawn) atomicAdd(c + C_DRAWN, (unsigned long long)n_drawn);
    if (frags) atomicAdd(c + C_FRAGMENTS, (unsigned long long)frags);
  }
}

// the flagged pairs: item v n_t + t -> list[rank]
struct LargeSrc {
  const unsigned char* flags;
  unsigned items;
  unsigned* list;
  __device__ __forceinline__ unsigned size() const { return items; }
  __device__ __forceinline__ bool flag(unsigned i) const { return flags[i] != 0; }
  __device__ __forceinline__ void write(unsigned pos, unsigned i) const { list[pos] = i; }
};

// one block per listed pair (the blocks stride over the list, whose length is in a device slot): wave w takes the tiles w, w + 4, ...
// of the box's tile rectangle in row-major order; lane l is pixel (l & 7, l >> 3) of the tile
__global__ __launch_bounds__(VT) void k_rast_large(const unsigned* __restrict__ list, const unsigned* __restrict__ n_list, unsigned items,
                                                   const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v, const RasterVertex* __restrict__ rec,
                                                   RasterCam cam, unsigned long long* __restrict__ keys, unsigned long long* __restrict__ counts) {
  const unsigned n = min(*n_list, items);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t npix = (size_t)cam.rows * (size_t)cam.cols;
  for (unsigned p = blockIdx.x; p < n; p += gridDim.x) {
    const unsigned item = list[p];
    const unsigned v = item / n_t, t = item - v * n_t;
    if (v >= (unsigned)cam.nv) continue;
    unsigned ia, ib, ic;
    RasterVertex a, b, c;
    RasterTri tr;
    int x0, x1, y0, y1;
    if (!raster_corners(tri, t, n_v, rec + (size_t)v * n_v, ia, ib, ic, a, b, c)) continue;
    if (raster_classify(a, b, c, cam.rows, cam.cols, tr, x0, x1, y0, y1) != C_DRAWN) continue;
    const int tx0 = x0 / TILE, ty0 = y0 / TILE;
    const unsigned ntx = (unsigned)(x1 / TILE - tx0 + 1), nty = (unsigned)(y1 / TILE - ty0 + 1);
    const unsigned ntiles = ntx * nty;                      // at most 2048 x 2048
    unsigned long long* view = keys + (size_t)v * npix;
    unsigned frags = 0;
    for (unsigned k = wave; k < ntiles; k += VT / 64) {
      const int ty = ty0 + (int)(k / ntx), tx = tx0 + (int)(k % ntx);
      const int cx0 = tx * TILE, cy0 = ty * TILE, cx1 = cx0 + TILE - 1, cy1 = cy0 + TILE - 1;
      // an edge function is affine: negative at the four corner pixels of the tile, it is negative at every pixel of it
      long long e00[3], e10[3], e01[3], e11[3];
      raster_edges(tr, cx0, cy0, e00[0], e00[1], e00[2]);
      raster_edges(tr, cx1, cy0, e10[0], e10[1], e10[2]);
      raster_edges(tr, cx0, cy1, e01[0], e01[1], e01[2]);
      raster_edges(tr, cx1, cy1, e11[0], e11[1], e11[2]);
      bool skip = false;
      for (int e = 0; e < 3; ++e) skip = skip || (e00[e] < 0 && e10[e] < 0 && e01[e] < 0 && e11[e] < 0);
      if (skip) continue;                                   // uniform over the wave
      const int px = cx0 + (lane & (TILE - 1)), py = cy0 + (lane >> 3);
      if (px >= x0 && px <= x1 && py >= y0 && py <= y1) frags += raster_pixel(tr, t, px, py, view, cam.cols) ? 1u : 0u;
    }
    wave_add_to(count_line(counts, v) + C_FRAGMENTS, frags);
  }
}

// view = blockIdx.y of this launch; keys, counts and planes start at the launch's first view
__global__ __launch_bounds__(VT) void k_rast_resolve(const unsigned long long* __restrict__ keys, const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v,
                                                     const RasterVertex* __restrict__ rec, const unsigned char* __restrict__ colours,
                                                     const float* __restrict__ normals, RasterViews vw, RasterCam cam, unsigned* __restrict__ index,
                                                     float* __restrict__ depth, unsigned char* __restrict__ colour, float* __restrict__ normal,
                                                     unsigned long long* __restrict__ counts) {
  RGBID_FP_STRICT
  const size_t npix = (size_t)cam.rows * (size_t)cam.cols;
  const size_t pix = (size_t)blockIdx.x * VT + threadIdx.x;
  const int v = blockIdx.y;
  bool won = false;
  if (pix < npix) {
    const size_t at = (size_t)v * npix + pix;
    const unsigned long long key = keys[at];
    unsigned idx = RGBID_RASTER_EMPTY;
    float Z = __uint_as_float(RGBID_RASTER_NAN_BITS), nrm[3] = {Z, Z, Z};
    unsigned char rgb[3] = {0, 0, 0};
    if (key != EMPTY_KEY && (unsigned)key < n_t) {
      won = true;
      idx = (unsigned)key;
      Z = __uint_as_float((unsigned)(key >> 32));
      if (colour || normal) {
        unsigned ia, ib, ic;
        RasterVertex a, b, c;
        RasterTri tr;
        int x0, x1, y0, y1;
        nrm[0] = nrm[1] = nrm[2] = 0.f;
        if (raster_corners(tri, idx, n_v, rec + (size_t)v * n_v, ia, ib, ic, a, b, c) &&
            raster_classify(a, b, c, cam.rows, cam.cols, tr, x0, x1, y0, y1) == C_DRAWN) {
          const int py = (int)(pix / (size_t)cam.cols), px = (int)(pix - (size_t)py * (size_t)cam.cols);
          long long Ea, Eb, Ec;
          double pa, pb, pc, q;
          raster_edges(tr, px, py, Ea, Eb, Ec);
          raster_weights(tr, Ea, Eb, Ec, pa, pb, pc, q);
          if (colour) {
            for (int k = 0; k < 3; ++k) {
              const double ca = (double)colours[3 * (size_t)ia + k], cb = (double)colours[3 * (size_t)ib + k], cc = (double)colours[3 * (size_t)ic + k];
              double f = floor(((pa * ca + pb * cb) + pc * cc) / q + 0.5);
              f = f < 0.0 ? 0.0 : (f > 255.0 ? 255.0 : f);
              rgb[k] = (unsigned char)(int)f;
            }
          }
          if (normal) {
            double m[3];
            for (int k = 0; k < 3; ++k)
              m[k] = (pa * (double)normals[3 * (size_t)ia + k] + pb * (double)normals[3 * (size_t)ib + k]) + pc * (double)normals[3 * (size_t)ic + k];
            const float* r = vw.m[v];
            double cw[3];
            for (int k = 0; k < 3; ++k) cw[k] = ((double)r[3 * k] * m[0] + (double)r[3 * k + 1] * m[1]) + (double)r[3 * k + 2] * m[2];
            const double g = (cw[0] * cw[0] + cw[1] * cw[1]) + cw[2] * cw[2];
            if (g != 0.0 && isfinite(g)) {
              const double l = sqrt(g);
              for (int k = 0; k < 3; ++k) nrm[k] = (float)(cw[k] / l);
            }
          }
        }
      }
    }
    if (index) index[at] = idx;
    if (depth) depth[at] = Z;
    if (colour) {
      unsigned char* c = colour + 3 * at;
      c[0] = rgb[0]; c[1] = rgb[1]; c[2] = rgb[2];
    }
    if (normal) {
      float* p = normal + 3 * (at - pix) + pix;             // [view][3][rows][cols]
      p[0] = nrm[0]; p[npix] = nrm[1]; p[2 * npix] = nrm[2];
    }
  }
  const int n_won = __syncthreads_count(won);              // every thread of the block is here
  if (threadIdx.x == 0 && n_won) atomicAdd(count_line(counts, v) + C_PIXELS, (unsigned long long)n_won);
}

// the COUNT_SLOTS copies of every view's counts added up: one thread per (view, count)
__global__ __launch_bounds__(VT) void k_rast_sum(const unsigned long long* __restrict__ parts, unsigned n, unsigned long long* __restrict__ counts) {
  const unsigned i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  const unsigned v = i / N_COUNTS, k = i - v * N_COUNTS;
  unsigned long long sum = 0;
  for (int s = 0; s < COUNT_SLOTS; ++s) sum += parts[((size_t)v * COUNT_SLOTS + s) * COUNT_LINE + k];
  counts[i] = sum;
}

constexpr int MARKS = 5;                                    // per chunk: project [0, 1], setup + small [1, 2], large [2, 3], resolve [3, 4]

}  // namespace

struct rgbid_raster {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0, cap_pix = 0;
  SortWorkspace w;                             // the compaction's tile counts and the slots; nothing is sorted
  unsigned long long* keys = nullptr;          // [cap_pix rounded up to even]
  RasterVertex* rec = nullptr;                 // [VIEW_CHUNK][cap_v]
  unsigned char* flags = nullptr;              // [VIEW_CHUNK][cap_t]
  unsigned* list = nullptr;                    // [VIEW_CHUNK][cap_t]
  unsigned long long* counts = nullptr;        // [MAX_VIEWS][6]
  unsigned long long* parts = nullptr;         // [MAX_VIEWS][COUNT_SLOTS][COUNT_LINE]
  int last_views = 0, timed_chunks = 0;        // of the last successful call
  Buffers buf;
  StageTimer<MARKS * RGBID_RASTER_TIMED_CHUNKS> timer;
};

extern "C" {

int rgbid_raster_create(rgbid_raster** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles,
                        unsigned long long max_pixels_times_views) {
  if (out) *out = nullptr;                     // also when the pixel capacity is refused
  if (max_pixels_times_views == 0 || max_pixels_times_views > MAX_PIXEL_VIEWS) return RGBID_E_INVALID;
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_RASTER_MAX_VERTICES, RGBID_RASTER_MAX_TRIANGLES, [&](rgbid_raster* r) {
    r->cap_pix = max_pixels_times_views;
    const size_t cv = (size_t)max_vertices, ct = (size_t)max_triangles;
    const unsigned long long pairs = (unsigned long long)RGBID_RASTER_VIEW_CHUNK * max_triangles;   // a chunk is shortened to 2^32 - 1 pairs
    int e = r->w.alloc_compaction(r->buf, pairs < 0xFFFFFFFFull ? pairs : 0xFFFFFFFFull);
    if (!e) e = r->buf.alloc(&r->keys, sizeof(unsigned long long) * (size_t)((max_pixels_times_views + 1) & ~1ull));   // whole 16-byte stores
    if (!e) e = r->buf.alloc(&r->rec, sizeof(RasterVertex) * RGBID_RASTER_VIEW_CHUNK * cv);
    if (!e) e = r->buf.alloc(&r->flags, (size_t)RGBID_RASTER_VIEW_CHUNK * ct);
    if (!e) e = r->buf.alloc(&r->list, sizeof(unsigned) * RGBID_RASTER_VIEW_CHUNK * ct);
    if (!e) e = r->buf.alloc(&r->counts, sizeof(unsigned long long) * N_COUNTS * RGBID_RASTER_MAX_VIEWS);
    if (!e) e = r->buf.alloc(&r->parts, sizeof(unsigned long long) * COUNT_LINE * COUNT_SLOTS * RGBID_RASTER_MAX_VIEWS);
    return e;
  });
}

int rgbid_raster_destroy(rgbid_raster* r) { return destroy_handle(r); }   // a resolve may still read the tables

int rgbid_raster_views(rgbid_raster* r, const float* vertices_dev, unsigned long long n_vertices, const uint32_t* triangles_dev,
                       unsigned long long n_triangles, const uint8_t* colours_dev, const float* normals_dev, int V,
                       const rgbid_render_pose* poses, const float K[4], int rows, int cols, float z_min, float z_max, uint32_t* index_dev,
                       float* depth_dev, uint8_t* colour_dev, float* normal_dev) {
  if (!r || !poses || !K || V < 1 || V > RGBID_RASTER_MAX_VIEWS) return RGBID_E_INVALID;
  if (rows < 1 || cols < 1 || rows > RGBID_RASTER_MAX_DIM || cols > RGBID_RASTER_MAX_DIM) return RGBID_E_INVALID;
  const unsigned long long npix = (unsigned long long)rows * (unsigned long long)cols;
  if (npix > r->cap_pix || (unsigned long long)V > r->cap_pix / npix) return RGBID_E_INVALID;
  if (!(std::isfinite(z_min) && std::isfinite(z_max) && z_min > 0.f && z_min <= z_max)) return RGBID_E_INVALID;
  for (int k = 0; k < 4; ++k) if (!std::isfinite(K[k])) return RGBID_E_INVALID;
  if (K[0] == 0.f || K[1] == 0.f) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, r->cap_v, r->cap_t)) return RGBID_E_INVALID;
  if (n_vertices && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  if (!aligned4(normals_dev) || !aligned4(index_dev) || !aligned4(depth_dev) || !aligned4(normal_dev)) return RGBID_E_INVALID;
  if (n_vertices && ((colour_dev && !colours_dev) || (normal_dev && !normals_dev))) return RGBID_E_INVALID;
  for (int v = 0; v < V; ++v) {
    if (!finite_all(poses[v].R, 9) || !finite_all(poses[v].t, 3)) return RGBID_E_INVALID;
    float cw[12];
    rgbid_render_pose_cw(&poses[v], cw);
    for (int k = 0; k < 12; ++k) if (!std::isfinite(cw[k])) return RGBID_E_INVALID;
  }
  (void)hipSetDevice(r->ctx->device);
  hipStream_t st = r->ctx->stream;
  SortWorkspace& w = r->w;
  r->last_views = 0; r->timed_chunks = 0;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, st));
  if (n_t) {
    check_triangles(st, triangles_dev, n_t, n_v, w.slots + SLOT_BAD);
    RGBID_HIP(hipGetLastError());
    if (int e = w.read_slots(st)) return e;
    if (w.slots_host[SLOT_BAD]) return RGBID_E_INVALID;    // a triangle names a vertex that does not exist
  }
  // a chunk's (view, triangle) pairs are numbered in 32 bits
  int chunk_views = RGBID_RASTER_VIEW_CHUNK;
  if (n_t && (unsigned long long)chunk_views * n_t > 0xFFFFFFFFull) chunk_views = (int)(0xFFFFFFFFull / n_t);
  const int chunks = (V + chunk_views - 1) / chunk_views;
  const bool timing = r->timer.on && chunks <= RGBID_RASTER_TIMED_CHUNKS;
  auto mark = [&](int chunk, int i) { if (timing) r->timer.mark(MARKS * chunk + i, st); };
  RasterCam cam;
  cam.fx = K[0]; cam.fy = K[1]; cam.cx = K[2]; cam.cy = K[3]; cam.z_min = z_min; cam.z_max = z_max;
  cam.rows = rows; cam.cols = cols;
  RasterViews vw;
  RGBID_HIP(hipMemsetAsync(r->parts, 0, sizeof(unsigned long long) * COUNT_LINE * COUNT_SLOTS * (size_t)V, st));
  for (int ch = 0; ch < chunks; ++ch) {
    const int v0 = ch * chunk_views, nv = V - v0 < chunk_views ? V - v0 : chunk_views;
    for (int v = 0; v < RGBID_RASTER_VIEW_CHUNK; ++v) {
      if (v < nv) rgbid_render_pose_cw(&poses[v0 + v], vw.m[v]);
      else for (int k = 0; k < 12; ++k) vw.m[v][k] = 0.f;
    }
    cam.nv = nv;
    const size_t first = (size_t)v0 * (size_t)npix;
    unsigned long long* keys = r->keys + first;
    unsigned long long* counts = r->parts + (size_t)v0 * COUNT_SLOTS * COUNT_LINE;
    mark(ch, 0);
    if (ch == 0) {
      const size_t n16 = ((size_t)npix * (size_t)V + 1) / 2;
      hipLaunchKernelGGL(k_rast_clear, dim3((unsigned)((n16 + VT - 1) / VT)), dim3(VT), 0, st, reinterpret_cast<uint4*>(r->keys), n16);
    }
    if (n_v) hipLaunchKernelGGL(k_rast_project, dim3((n_v + VT - 1) / VT), dim3(VT), 0, st, vertices_dev, n_v, vw, cam, r->rec);
    mark(ch, 1);
    if (n_t) hipLaunchKernelGGL(k_rast_setup, dim3((n_t + VT - 1) / VT, (unsigned)nv), dim3(VT), 0, st, triangles_dev, n_t, n_v, r->rec, cam, keys, r->flags, counts);
    mark(ch, 2);
    if (n_t) {
      const unsigned items = (unsigned)((unsigned long long)nv * n_t);
      const LargeSrc src{r->flags, items, r->list};
      w.count_scan(st, src, items, SLOT_RUNS);
      w.write(st, src, items);
      hipLaunchKernelGGL(k_rast_large, dim3(items < LARGE_GRID ? items : LARGE_GRID), dim3(VT), 0, st, r->list, w.slots + SLOT_RUNS, items, triangles_dev, n_t,
                         n_v, r->rec, cam, keys, counts);
    }
    mark(ch, 3);
    hipLaunchKernelGGL(k_rast_resolve, dim3((unsigned)((npix + VT - 1) / VT), (unsigned)nv), dim3(VT), 0, st, keys, triangles_dev, n_t, n_v, r->rec, colours_dev,
                       normals_dev, vw, cam, index_dev ? index_dev + first : nullptr, depth_dev ? depth_dev + first : nullptr,
                       colour_dev ? colour_dev + 3 * first : nullptr, normal_dev ? normal_dev + 3 * first : nullptr, counts);
    if (ch == chunks - 1)
      hipLaunchKernelGGL(k_rast_sum, dim3(((unsigned)V * N_COUNTS + VT - 1) / VT), dim3(VT), 0, st, r->parts, (unsigned)V * N_COUNTS, r->counts);
    mark(ch, 4);
  }
  RGBID_HIP(hipGetLastError());
  r->last_views = V;
  r->timed_chunks = timing ? chunks : 0;
  return RGBID_OK;
}

int rgbid_raster_counts(rgbid_raster* r, int V, unsigned long long* out) {
  if (!r || !out || V < 1 || V != r->last_views) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  RGBID_HIP(hipMemcpyAsync(out, r->counts, sizeof(unsigned long long) * N_COUNTS * (size_t)V, hipMemcpyDeviceToHost, r->ctx->stream));
  RGBID_HIP(hipStreamSynchronize(r->ctx->stream));
  return RGBID_OK;
}

int rgbid_raster_timing(rgbid_raster* r, int enable, float ms[4]) {
  if (!r) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  if (ms) {
    for (int k = 0; k < 4; ++k) ms[k] = 0.f;
    for (int ch = 0; ch < r->timed_chunks; ++ch)
      for (int k = 0; k < 4; ++k) {
        float one = 0.f;
        RGBID_HIP(r->timer.elapsed(MARKS * ch + k, MARKS * ch + k + 1, &one));
        ms[k] += one;
      }
  }
  return r->timer.enable(enable != 0);
}

}  // extern "C"
