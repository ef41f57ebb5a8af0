// kernels_tsdf.hip -- keyframes fused into a truncated signed distance volume, the volume's surface as a triangle mesh with a normal per
// vertex, the volume ray-cast into camera views, and depth frames aligned to the volume (include/rgbid_tsdf.h, rgbid_tsdf_raycast.h and
// rgbid_tsdf_align.h, DESIGN.md sections 19 - 21).
//
// The judges are tests/tsdf_mirror.py, tests/raycast_mirror.py and tests/align_mirror.py; state, counts, mesh, normals, views and
// alignment results are byte-identical to them.
//   integrate  view table       per view 64 bytes in device memory: the twelve floats of rgbid_render_pose_cw, the plane and the colour
//                               pointer; written on the host into pinned memory and copied on the stream
//              k_tsdf_integrate one thread per voxel, x fastest, grid-strided; up to RGBID_TSDF_VIEW_CHUNK views per launch in an inner
//                               loop whose index is wave-uniform (the table row is read with scalar loads).  D and the counts are read
//                               once, walked through the views in registers and written once, and only if a view touched the voxel;
//                               the colour sums are added once.  Depth gate first (three products), then the two divisions, the range
//                               test in float, one gather.  The running mean of step 7 does not commute, so further chunks of views go
//                               in further launches, in order, on the same stream
//   plan       k_tsdf_classify  per voxel the 7-bit mask of its active edges and the triangle count (0 .. 12) of the cell it is corner 0 of
//              vertices         flag count + scan over the 7 n edge flags (voxel_device.h)
//              triangles        k_tsdf_tri_count per tile of cells, the same one-block scan of the tile counts
//   emit       flag write       an active edge writes its vertex and colour at its rank; the lowest one of a voxel also the voxel's base,
//                               so that an edge's vertex index is base + popcount(mask below it)
//              k_tsdf_tri_write a cell writes its index triples from the block scan of the counts
//   normals    flag write       a second source over the same flags and tile offsets: an active edge writes the interpolated voxel gradient
//   ray cast   pose table       per view twelve floats of rgbid_tsdf_pose_wc, through the view table's pinned buffer
//              k_tsdf_raycast   one thread per pixel, a wave per 8 x 8 pixel tile, blockIdx.y the view; two bisections per axis give the
//                               ray its n range, the march tests the 8 counts of a sample first and loads the 8 D of a defined one
//   align      view table       per view 104 bytes: the 12 pose doubles and the plane; k_tsdf_align_init makes the result records and the
//                               float32 pose rows of them
//              k_tsdf_align_system  per Gauss-Newton iteration: one thread per lattice pixel, a wave per 8 x 8 tile, blockIdx.y the view; the
//                               ray cast's sampler, 28 doubles per pixel, summed over the wave by xor butterflies; one row per tile
//              k_tsdf_align_solve   one block per view: the upper levels of the sum tree, the 6 x 6 solve, the pose update and the
//                               float32 pose row of the next launch; every iteration of every level is enqueued without a host wait
// No atomic touches the state and no result depends on the order of threads or waves.
//
// Exact arithmetic: RGBID_FP_STRICT (common.h) opens every function that forms a float32 product followed by a sum, so no FMA is formed
// from them; the divisions are hipcc's default correctly rounded ones.
#include "../../include/rgbid_tsdf.h"
#include "common.h"
#include "hip_host.h"
#include "view_device.h"    // rot_row
#include "voxel_device.h"   // flag compaction, the one-block scan, grid_of

#include <cmath>
#include <new>
#include <vector>

using namespace rgbid;

namespace {

constexpr int VIEW_CHUNK = RGBID_TSDF_VIEW_CHUNK;
constexpr unsigned MAX_W = RGBID_TSDF_MAX_WEIGHT;
enum { SLOT_VERTS = SLOT_VOXELS, SLOT_TRIS = SLOT_RUNS };

struct TsdfView {                 // one row of the view table: 64 bytes
  float m[12];                    // r00 r01 r02 r10 r11 r12 r20 r21 r22 tx ty tz
  const float* plane;             // [rows][cols] inverse depth
  const unsigned char* colour;    // [rows][cols][3] or null
};
static_assert(sizeof(TsdfView) == 64, "a view is sixteen dwords");

struct TsdfGrid {                 // the volume's shape
  unsigned nx, ny, nz, n;         // n = nx ny nz
  float ox, oy, oz, voxel, trunc;
};

struct TsdfCam {
  float fx, fy, cx, cy, z_min, z_max;
  float hi_u, hi_v;               // cols - 1, rows - 1: exact in float32 (RGBID_TSDF_MAX_DIM)
  int cols;
};

struct TsdfState {                // the contract's planes are the storage
  float* D;                       // [n]
  unsigned* counts;               // [n] W | Cn << 16
  unsigned* rgb;                  // [3][capacity] or null; channel stride = the handle's capacity
  size_t stride;
};

// the six tetrahedra of a cell as corner codes of their vertices 0 .. 3, and per tetrahedron the cases (bit = case) whose rows have
// their last two entries swapped (tests/test_cpu_tsdf.py re-derives the bits from the orientation rule)
__constant__ const unsigned char TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__constant__ const unsigned short TET_SWAP[6] = {0x4d24, 0x32da, 0x32da, 0x4d24, 0x4d24, 0x32da};

__device__ __forceinline__ float centre(float o, unsigned i, float voxel) {
  RGBID_FP_STRICT
  return o + (float)i * voxel;
}

// views v0 .. v1 - 1 over every voxel
__global__ __launch_bounds__(VT) void k_tsdf_integrate(TsdfGrid g, TsdfCam cam, const TsdfView* __restrict__ views, int v0, int v1, TsdfState st) {
  RGBID_FP_STRICT
  for (unsigned i = blockIdx.x * VT + threadIdx.x; i < g.n; i += gridDim.x * VT) {
    const unsigned ix = i % g.nx, r = i / g.nx, iy = r % g.ny, iz = r / g.ny;
    const float x = centre(g.ox, ix, g.voxel), y = centre(g.oy, iy, g.voxel), z = centre(g.oz, iz, g.voxel);
    float D = st.D[i];
    unsigned c = st.counts[i];                                  // W | Cn << 16
    unsigned dr = 0, dg = 0, db = 0;                            // what the launch adds to the colour sums
    const unsigned c_in = c;
    for (int v = v0; v < v1; ++v) {
      const TsdfView& vw = views[v];                            // wave-uniform: scalar loads
      const float Z = rot_row(vw.m + 6, x, y, z) + vw.m[11];
      if (!(Z >= cam.z_min && Z <= cam.z_max)) continue;        // NaN fails; z_max is finite, so infinity does too
      const float X = rot_row(vw.m, x, y, z) + vw.m[9];
      const float Y = rot_row(vw.m + 3, x, y, z) + vw.m[10];
      const float pu = floorf((cam.fx * (X / Z) + cam.cx) + 0.5f);
      const float pv = floorf((cam.fy * (Y / Z) + cam.cy) + 0.5f);
      if (!(pu >= 0.f && pu <= cam.hi_u && pv >= 0.f && pv <= cam.hi_v)) continue;   // in float: nothing out of range reaches the cast
      const size_t pix = (size_t)(int)pv * (size_t)cam.cols + (size_t)(int)pu;
      const float m = vw.plane[pix];
      if (!(m > 0.f && m < INFINITY)) continue;                 // NaN, 0, negative, infinity: a hole
      const float zm = 1.f / m;
      if (!(zm < INFINITY)) continue;                           // a denormal whose reciprocal overflows
      const float s = zm - Z;
      const unsigned W = c & 0xFFFFu;
      if (s < -g.trunc || W == MAX_W) continue;                 // hidden behind the surface, or the weight is full
      const float d = fminf(s, g.trunc);
      D = (D * (float)W + d) / (float)(W + 1u);
      c += 1u;
      if (vw.colour && st.rgb && fabsf(s) <= g.trunc && (c >> 16) < MAX_W) {
        const unsigned char* cp = vw.colour + 3 * pix;
        dr += cp[0]; dg += cp[1]; db += cp[2];
        c += 1u << 16;
      }
    }
    if (c != c_in) {                                            // a view touched the voxel: W grew
      st.D[i] = D;
      st.counts[i] = c;
      if (st.rgb && ((c ^ c_in) >> 16)) {                       // Cn grows only with sums; the pointer is tested all the same
        st.rgb[i] += dr; st.rgb[st.stride + i] += dg; st.rgb[2 * st.stride + i] += db;
      }
    }
  }
}

// ---- extraction ----------------------------------------------------------------------------------------------------------------------
struct TsdfRule {
  unsigned min_weight;
};

// bit 0: valid, bit 1: inside
__device__ __forceinline__ unsigned voxel_class(const TsdfState& st, unsigned i, unsigned min_weight) {
  const bool valid = (st.counts[i] & 0xFFFFu) >= min_weight;
  return valid ? (st.D[i] < 0.f ? 3u : 1u) : 0u;
}

// number of rows of a tetrahedron's case: 0 1 1 2 1 2 2 1 1 2 2 1 2 1 1 0
__device__ __forceinline__ unsigned case_rows(unsigned m) {
  const unsigned pc = __popc(m);
  return pc == 2 ? 2u : (pc == 1 || pc == 3 ? 1u : 0u);
}

// per voxel p: the mask of its active edges (bit c - 1 for the offset code c) and the triangles of the cell whose corner 0 it is
__global__ __launch_bounds__(VT) void k_tsdf_classify(TsdfGrid g, TsdfState st, TsdfRule rule, unsigned char* __restrict__ mask,
                                                      unsigned char* __restrict__ ntri) {
  for (unsigned i = blockIdx.x * VT + threadIdx.x; i < g.n; i += gridDim.x * VT) {
    const unsigned ix = i % g.nx, r = i / g.nx, iy = r % g.ny, iz = r / g.ny;
    unsigned valid = 0, inside = 0;                             // bit c: corner c
    for (unsigned c = 0; c < 8; ++c) {
      const unsigned dx = c & 1u, dy = (c >> 1) & 1u, dz = c >> 2;
      if (ix + dx >= g.nx || iy + dy >= g.ny || iz + dz >= g.nz) continue;
      const unsigned k = voxel_class(st, i + dx + dy * g.nx + dz * g.nx * g.ny, rule.min_weight);
      valid |= (k & 1u) << c;
      inside |= (k >> 1) << c;
    }
    unsigned mk = 0;
    if (valid & 1u) {
      const unsigned differs = (inside & 1u) ? ~inside : inside;   // bit c: corner c is on the other side than corner 0
      mk = ((valid & differs) >> 1) & 0x7Fu;
    }
    unsigned nt = 0;
    if (valid == 0xFFu) {
      for (int t = 0; t < 6; ++t) {
        unsigned m = 0;
        for (int u = 0; u < 4; ++u) m |= ((inside >> TET_CORNER[t][u]) & 1u) << u;
        nt += case_rows(m);
      }
    }
    mask[i] = (unsigned char)mk;
    ntri[i] = (unsigned char)nt;
  }
}

__device__ __forceinline__ float lerp_strict(float a, float b, float t) {
  RGBID_FP_STRICT
  return a + t * (b - a);
}

// every NaN that a vertex or a view receives has the bits of the render's
__device__ __forceinline__ float canonical_nan(float x) { return x != x ? __uint_as_float(RGBID_RENDER_NAN_BITS) : x; }

// step 11's mean of one voxel and channel; false when the voxel has none
__device__ __forceinline__ bool voxel_mean(const TsdfState& st, unsigned i, unsigned cn, int ch, float& out) {
  if (!st.rgb || cn == 0) return false;
  const unsigned long long s = st.rgb[ch * st.stride + i];
  const unsigned long long q = (2ull * s + cn) / (2ull * cn);
  out = (float)(q < 255ull ? q : 255ull);
  return true;
}

// stable compaction of the active edges: item e = linear(p) 7 + (c - 1)
struct EdgeSrc {
  TsdfGrid g;
  TsdfState st;
  const unsigned char* mask;
  unsigned* base;                 // [n] vertex index of a voxel's lowest active edge
  float* verts;                   // [nv][3]
  unsigned char* cols;            // [nv][3] or null
  __device__ __forceinline__ unsigned size() const { return 7u * g.n; }
  __device__ __forceinline__ bool flag(unsigned e) const { return (mask[e / 7u] >> (e % 7u)) & 1u; }
  __device__ __forceinline__ bool mean(unsigned i, unsigned cn, int ch, float& out) const { return voxel_mean(st, i, cn, ch, out); }
  __device__ __forceinline__ void write(unsigned pos, unsigned e) const {
    RGBID_FP_STRICT
    const unsigned p = e / 7u, b7 = e % 7u, c = b7 + 1u;
    if ((mask[p] & ((1u << b7) - 1u)) == 0) base[p] = pos;
    const unsigned dx = c & 1u, dy = (c >> 1) & 1u, dz = c >> 2;
    const unsigned q = p + dx + dy * g.nx + dz * g.nx * g.ny;
    const float Dp = st.D[p], Dq = st.D[q];
    const bool p_in = Dp < 0.f;                                  // both ends are valid and exactly one is inside
    const unsigned ix = p % g.nx, r = p / g.nx, iy = r % g.ny, iz = r / g.ny;
    const unsigned ax = p_in ? ix : ix + dx, ay = p_in ? iy : iy + dy, az = p_in ? iz : iz + dz;
    const unsigned bx = p_in ? ix + dx : ix, by = p_in ? iy + dy : iy, bz = p_in ? iz + dz : iz;
    const float Da = p_in ? Dp : Dq, Db = p_in ? Dq : Dp;
    const float t = Da / (Da - Db);
    float* o = verts + 3 * (size_t)pos;                         // step 10: a NaN component has the one bit pattern
    o[0] = canonical_nan(lerp_strict(centre(g.ox, ax, g.voxel), centre(g.ox, bx, g.voxel), t));
    o[1] = canonical_nan(lerp_strict(centre(g.oy, ay, g.voxel), centre(g.oy, by, g.voxel), t));
    o[2] = canonical_nan(lerp_strict(centre(g.oz, az, g.voxel), centre(g.oz, bz, g.voxel), t));
    if (cols) {
      const unsigned a = p_in ? p : q, b = p_in ? q : p;
      const unsigned cna = st.counts[a] >> 16, cnb = st.counts[b] >> 16;
      unsigned char* oc = cols + 3 * (size_t)pos;
      for (int ch = 0; ch < 3; ++ch) {
        float ca = 0.f, cb = 0.f;
        const bool ha = mean(a, cna, ch, ca), hb = mean(b, cnb, ch, cb);
        float v = ha ? ca : cb;                                  // neither: 0
        if (ha && hb) v = fminf(fmaxf(floorf(lerp_strict(ca, cb, t) + 0.5f), 0.f), 255.f);   // fmaxf(NaN, 0) = 0
        oc[ch] = (unsigned char)v;
      }
    }
  }
};

// L of steps 19 and 23; false when it is zero or not finite
__device__ __forceinline__ bool grad_length(float gx, float gy, float gz, float& L) {
  RGBID_FP_STRICT
  L = sqrtf((gx * gx + gy * gy) + gz * gz);
  return L > 0.f && L < INFINITY;                               // NaN fails both
}

// a second source over the flags of EdgeSrc: an active edge writes its vertex normal (steps 22 and 23) at its rank
struct NormalSrc {
  TsdfGrid g;
  TsdfState st;
  const unsigned char* mask;
  unsigned min_weight;
  float* normals;                 // [nv][3]
  __device__ __forceinline__ unsigned size() const { return 7u * g.n; }
  __device__ __forceinline__ bool flag(unsigned e) const { return (mask[e / 7u] >> (e % 7u)) & 1u; }
  __device__ __forceinline__ bool valid(unsigned i) const { return (st.counts[i] & 0xFFFFu) >= min_weight; }
  // step 22 along one axis: voxel i at coordinate c of an axis of n voxels with the linear stride s
  __device__ __forceinline__ float grad(unsigned i, unsigned c, unsigned n, unsigned s) const {
    RGBID_FP_STRICT
    const bool lo = c > 0u && valid(i - s), hi = c + 1u < n && valid(i + s);
    if (lo && hi) return st.D[i + s] - st.D[i - s];
    if (hi) return 2.f * (st.D[i + s] - st.D[i]);
    if (lo) return 2.f * (st.D[i] - st.D[i - s]);
    return 0.f;
  }
  __device__ __forceinline__ void write(unsigned pos, unsigned e) const {
    RGBID_FP_STRICT
    const unsigned p = e / 7u, c = e % 7u + 1u;
    const unsigned dx = c & 1u, dy = (c >> 1) & 1u, dz = c >> 2;
    const unsigned sy = g.nx, sz = g.nx * g.ny;
    const unsigned q = p + dx + dy * sy + dz * sz;
    const float Dp = st.D[p], Dq = st.D[q];
    const bool p_in = Dp < 0.f;
    const unsigned ix = p % g.nx, r = p / g.nx, iy = r % g.ny, iz = r / g.ny;
    const unsigned a = p_in ? p : q, b = p_in ? q : p;
    const unsigned ax = p_in ? ix : ix + dx, ay = p_in ? iy : iy + dy, az = p_in ? iz : iz + dz;
    const unsigned bx = p_in ? ix + dx : ix, by = p_in ? iy + dy : iy, bz = p_in ? iz + dz : iz;
    const float Da = p_in ? Dp : Dq, Db = p_in ? Dq : Dp;
    const float t = Da / (Da - Db);
    const float gx = lerp_strict(grad(a, ax, g.nx, 1u), grad(b, bx, g.nx, 1u), t);
    const float gy = lerp_strict(grad(a, ay, g.ny, sy), grad(b, by, g.ny, sy), t);
    const float gz = lerp_strict(grad(a, az, g.nz, sz), grad(b, bz, g.nz, sz), t);
    float L;
    const bool ok = grad_length(gx, gy, gz, L);
    float* o = normals + 3 * (size_t)pos;
    o[0] = ok ? gx / L : 0.f;
    o[1] = ok ? gy / L : 0.f;
    o[2] = ok ? gz / L : 0.f;
  }
};

// ---- ray casting (include/rgbid_tsdf_raycast.h) --------------------------------------------------------------
struct RayCam {
  float fx, fy, cx, cy, z_min, step;
  float hi_i, hi_j, hi_k;         // nx - 2, ny - 2, nz - 2 as the largest float32 not above them: against a floorf result the exact test
  unsigned n_last;                // the last n of step 15
  unsigned min_weight;
  int rows, cols;
  unsigned tiles_x, tiles;        // 8 x 8 pixel tiles per tile row and per view
};

struct RayOut {
  float* depth;                   // [V][rows][cols] or null
  float* normal;                  // [V][3][rows][cols] or null
  unsigned char* colour;          // [V][rows][cols][3] or null
};

__device__ __forceinline__ float ray_depth(const RayCam& cam, unsigned n) {
  RGBID_FP_STRICT
  return cam.z_min + (float)n * cam.step;
}

__device__ __forceinline__ float ray_pos(float a, float b, float Z) {
  RGBID_FP_STRICT
  return a + Z * b;
}

// The n whose sample passes the range test of step 15 along one axis are an interval, and two bisections find it exactly.  Proof:
// (float)n is exact (n <= 65 536), and a correctly rounded product or sum is monotone in each operand, so Z_n = z_min + (float)n step
// does not decrease with n (step > 0); Z_n >= 0, so Z_n b does not decrease for b >= 0 and does not increase for b < 0, and neither do
// a + Z_n b and its floorf.  With b >= 0 the tests "floorf(g_n) >= 0" and "not floorf(g_n) <= hi" are therefore false up to some n
// and true from it on: the samples in range are those from the first n of the former up to, not including, the first n of the latter;
// with b < 0 the two tests change roles.  The bisections evaluate the very expression the march evaluates, so no error bound is
// involved and no margin is needed.  A non-finite a or b makes every g_n infinite or NaN: no sample is defined and any interval is
// right.  n0 and n1 (exclusive) are narrowed to the axis' interval.
__device__ __forceinline__ void ray_axis_range(const RayCam& cam, float a, float b, float hi, unsigned& n0, unsigned& n1) {
  const bool up = b >= 0.f;
  unsigned lo = 0, end = cam.n_last + 1u;
  while (lo < end) {
    const unsigned mid = (lo + end) >> 1;
    const float fl = floorf(ray_pos(a, b, ray_depth(cam, mid)));
    if (up ? fl >= 0.f : fl <= hi) end = mid; else lo = mid + 1u;
  }
  n0 = max(n0, lo);
  lo = 0; end = cam.n_last + 1u;
  while (lo < end) {
    const unsigned mid = (lo + end) >> 1;
    const float fl = floorf(ray_pos(a, b, ray_depth(cam, mid)));
    if (up ? !(fl <= hi) : !(fl >= 0.f)) end = mid; else lo = mid + 1u;
  }
  n1 = min(n1, lo);
}

// step 15 for one position: the linear index of the cell's corner 000 and the fractions; false when the sample is undefined.  The
// counts come first: a sample in unobserved space loads no D
__device__ __forceinline__ bool ray_cell(const TsdfGrid& g, const TsdfState& st, const RayCam& cam, float gx, float gy, float gz, unsigned& base,
                                         float& fx_, float& fy_, float& fz_) {
  const float i0 = floorf(gx), j0 = floorf(gy), k0 = floorf(gz);
  if (!(i0 >= 0.f && i0 <= cam.hi_i && j0 >= 0.f && j0 <= cam.hi_j && k0 >= 0.f && k0 <= cam.hi_k)) return false;   // NaN fails
  base = ((unsigned)(int)k0 * g.ny + (unsigned)(int)j0) * g.nx + (unsigned)(int)i0;
  fx_ = gx - i0; fy_ = gy - j0; fz_ = gz - k0;
  const unsigned sy = g.nx, sz = g.nx * g.ny;
  unsigned w = 0xFFFFu;
#pragma unroll
  for (unsigned c = 0; c < 8; ++c) w = min(w, st.counts[base + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz] & 0xFFFFu);
  return w >= cam.min_weight;
}

// step 16's value of 8 corner values d[i + 2 j + 4 k]
__device__ __forceinline__ float tri_value(const float d[8], float fx_, float fy_, float fz_) {
  const float ly0 = lerp_strict(lerp_strict(d[0], d[1], fx_), lerp_strict(d[2], d[3], fx_), fy_);
  const float ly1 = lerp_strict(lerp_strict(d[4], d[5], fx_), lerp_strict(d[6], d[7], fx_), fy_);
  return lerp_strict(ly0, ly1, fz_);
}

// One thread per pixel; a wave is an 8 x 8 pixel tile, so that the corner gathers of neighbouring rays fall on neighbouring voxels; a
// block holds four tiles of the view blockIdx.y, whose pose row is read with scalar loads.  No LDS, no atomic.
__global__ __launch_bounds__(VT) void k_tsdf_raycast(TsdfGrid g, TsdfState st, RayCam cam, const float* __restrict__ poses, RayOut out) {
  RGBID_FP_STRICT
  const unsigned tile = blockIdx.x * (VT / 64) + (threadIdx.x >> 6);
  if (tile >= cam.tiles) return;
  const unsigned lane = threadIdx.x & 63u;
  const int pu = (int)((tile % cam.tiles_x) * 8u + (lane & 7u)), pv = (int)((tile / cam.tiles_x) * 8u + (lane >> 3));
  if (pu >= cam.cols || pv >= cam.rows) return;                 // ragged tiles
  const float* __restrict__ m = poses + 12u * blockIdx.y;       // R00 .. R22 tx ty tz of R_WC | t_WC
  // step 14
  const float dx = ((float)pu - cam.cx) / cam.fx, dy = ((float)pv - cam.cy) / cam.fy;
  const float ax = (m[9] - g.ox) / g.voxel, ay = (m[10] - g.oy) / g.voxel, az = (m[11] - g.oz) / g.voxel;
  const float bx = ((m[0] * dx + m[1] * dy) + m[2]) / g.voxel;
  const float by = ((m[3] * dx + m[4] * dy) + m[5]) / g.voxel;
  const float bz = ((m[6] * dx + m[7] * dy) + m[8]) / g.voxel;
  // the n outside [n0, n1) are proved undefined
  unsigned n0 = 0, n1 = cam.n_last + 1u;
  ray_axis_range(cam, ax, bx, cam.hi_i, n0, n1);
  ray_axis_range(cam, ay, by, cam.hi_j, n0, n1);
  ray_axis_range(cam, az, bz, cam.hi_k, n0, n1);
  const unsigned sy = g.nx, sz = g.nx * g.ny;
  // step 17
  bool prev = false, hit = false;
  float f_prev = 0.f, Z_prev = 0.f, Zs = 0.f;
  for (unsigned n = n0; n < n1; ++n) {
    const float Z = ray_depth(cam, n);
    unsigned base;
    float fx_, fy_, fz_, f = 0.f;
    const bool def = ray_cell(g, st, cam, ray_pos(ax, bx, Z), ray_pos(ay, by, Z), ray_pos(az, bz, Z), base, fx_, fy_, fz_);
    if (def) {
      float d[8];
#pragma unroll
      for (unsigned c = 0; c < 8; ++c) d[c] = st.D[base + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz];
      f = tri_value(d, fx_, fy_, fz_);
      if (prev) {
        if (f_prev > 0.f && f <= 0.f) {                         // step 18
          const float t = f_prev / (f_prev - f);
          Zs = Z_prev + t * (Z - Z_prev);
          hit = true;
          break;
        }
        if (!(f_prev > 0.f) && f > 0.f) break;                  // out of a surface from behind
      }
    }
    prev = def; f_prev = f; Z_prev = Z;
  }
  const float qnan = __uint_as_float(RGBID_RENDER_NAN_BITS);
  float depth = qnan, nc0 = qnan, nc1 = qnan, nc2 = qnan;
  unsigned char rgb[3] = {0, 0, 0};
  if (hit) {
    depth = canonical_nan(Zs);
    unsigned base;
    float fx_, fy_, fz_;
    if (ray_cell(g, st, cam, ray_pos(ax, bx, Zs), ray_pos(ay, by, Zs), ray_pos(az, bz, Zs), base, fx_, fy_, fz_)) {
      if (out.normal) {                                         // step 19
        float d[8];
#pragma unroll
        for (unsigned c = 0; c < 8; ++c) d[c] = st.D[base + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz];
        const float lx00 = lerp_strict(d[0], d[1], fx_), lx10 = lerp_strict(d[2], d[3], fx_);
        const float lx01 = lerp_strict(d[4], d[5], fx_), lx11 = lerp_strict(d[6], d[7], fx_);
        const float Gx = lerp_strict(lerp_strict(d[1] - d[0], d[3] - d[2], fy_), lerp_strict(d[5] - d[4], d[7] - d[6], fy_), fz_);
        const float Gy = lerp_strict(lx10 - lx00, lx11 - lx01, fz_);
        const float Gz = lerp_strict(lx01, lx11, fy_) - lerp_strict(lx00, lx10, fy_);
        float L;
        if (grad_length(Gx, Gy, Gz, L)) {
          const float nx_ = Gx / L, ny_ = Gy / L, nz_ = Gz / L;
          nc0 = canonical_nan((m[0] * nx_ + m[3] * ny_) + m[6] * nz_);
          nc1 = canonical_nan((m[1] * nx_ + m[4] * ny_) + m[7] * nz_);
          nc2 = canonical_nan((m[2] * nx_ + m[5] * ny_) + m[8] * nz_);
        }
      }
      if (out.colour && st.rgb) {                               // step 20
        unsigned cn[8], all = 1u;
#pragma unroll
        for (unsigned c = 0; c < 8; ++c) {
          cn[c] = st.counts[base + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz] >> 16;
          all &= cn[c] != 0u;
        }
        const unsigned near = (fx_ >= 0.5f ? 1u : 0u) | (fy_ >= 0.5f ? 2u : 0u) | (fz_ >= 0.5f ? 4u : 0u);
        for (int ch = 0; ch < 3; ++ch) {
          float mean[8], v = 0.f;
#pragma unroll
          for (unsigned c = 0; c < 8; ++c) {
            mean[c] = 0.f;
            const bool has = (all || c == near) && voxel_mean(st, base + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz, cn[c], ch, mean[c]);
            if (has && c == near) v = mean[c];
          }
          if (all) v = fminf(fmaxf(floorf(tri_value(mean, fx_, fy_, fz_) + 0.5f), 0.f), 255.f);   // fmaxf(NaN, 0) = 0
          rgb[ch] = (unsigned char)v;
        }
      }
    }
  }
  const size_t plane = (size_t)cam.rows * (size_t)cam.cols;
  const size_t pix = (size_t)pv * (size_t)cam.cols + (size_t)pu, view = (size_t)blockIdx.y * plane;
  if (out.depth) out.depth[view + pix] = depth;
  if (out.normal) {
    float* o = out.normal + 3 * view + pix;
    o[0] = nc0; o[plane] = nc1; o[2 * plane] = nc2;
  }
  if (out.colour) {
    unsigned char* o = out.colour + 3 * (view + pix);
    o[0] = rgb[0]; o[1] = rgb[1]; o[2] = rgb[2];
  }
}

// ---- alignment (include/rgbid_tsdf_align.h) -------------------------------------------------------------------
constexpr int ALIGN_TERMS = RGBID_TSDF_ALIGN_TERMS;

struct AlignView {                // one row of the alignment's view table: 104 bytes
  double pose[12];                // R00 .. R22 tx ty tz of R_WC | t_WC, as given
  const float* plane;             // [rows][cols] inverse depth
};
static_assert(sizeof(AlignView) == 104, "twelve doubles and a pointer");
static_assert(sizeof(rgbid_tsdf_align_result) == 560, "step 33");

struct AlignCam {
  RayCam ray;                     // fx fy cx cy, z_min, hi_i hi_j hi_k, min_weight, rows, cols: what ray_cell and the rays of step 14 read
  float z_max, huber;
  unsigned stride, lw, lh;        // the level's lattice
  unsigned tiles_x, tiles;        // 8 x 8 lattice tiles per tile row and per view
  unsigned restart;               // the first iteration of a later level: CONVERGED views run again
};

struct AlignWork {                // the handle's workspace
  double* a;                      // [V][28][a_stride] tile sums, term-major, and the third round of the upper tree
  double* b;                      // [V][28][b_stride] the second and fourth round
  unsigned* used;                 // [V][a_stride] used pixels per tile
  size_t a_stride, b_stride;
  float* pose32;                  // [V][12] step 24's roundings: what the next system launch reads
};

struct AlignRule {
  double damping, eps;
  unsigned min_pixels, tiles;
  unsigned restart;
};

__device__ __forceinline__ int align_status(const rgbid_tsdf_align_result* res, unsigned view, unsigned restart) {
  const int s = res[view].status;
  return s == RGBID_TSDF_ALIGN_CONVERGED && restart ? RGBID_TSDF_ALIGN_RUNNING : s;
}

// step 33: a NaN among the record's doubles has the one bit pattern (a - b turns the sign of a NaN b here and not on every host)
__device__ __forceinline__ double canonical_nan64(double x) { return x != x ? __longlong_as_double((long long)RGBID_TSDF_ALIGN_NAN_BITS) : x; }

// step 28's tree64 over the wave: every lane ends with the sum
__device__ __forceinline__ double tree64(double v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = v + __shfl_xor(v, m);
  return v;
}

__global__ __launch_bounds__(VT) void k_tsdf_align_init(const AlignView* __restrict__ views, int V, rgbid_tsdf_align_result* __restrict__ res,
                                                        float* __restrict__ pose32) {
  const int v = blockIdx.x * VT + threadIdx.x;
  if (v >= V) return;
  rgbid_tsdf_align_result& r = res[v];
  for (int k = 0; k < 12; ++k) {
    r.pose[k] = views[v].pose[k];
    pose32[12 * v + k] = (float)views[v].pose[k];
  }
  r.status = RGBID_TSDF_ALIGN_RUNNING;
  r.iterations = 0;
  r.used[0] = r.used[1] = 0u;
  for (int k = 0; k < ALIGN_TERMS; ++k) r.sums[0][k] = r.sums[1][k] = 0.0;
}

// One thread per lattice pixel; a wave is an 8 x 8 lattice tile, a block four tiles of the view blockIdx.y: the ray cast's shape, so the
// corner gathers of neighbouring pixels fall on neighbouring voxels.  The pose row and the status are wave-uniform.  Lanes outside the
// lattice and pixels that are not used stay in the wave with +0.0: the butterflies need all 64.  No LDS, no atomic.
__global__ __launch_bounds__(VT) void k_tsdf_align_system(TsdfGrid g, TsdfState st, AlignCam cam, const AlignView* __restrict__ views,
                                                          const float* __restrict__ pose32, const rgbid_tsdf_align_result* __restrict__ res,
                                                          double* __restrict__ sums, unsigned* __restrict__ used, size_t a_stride) {
  RGBID_FP_STRICT
  const unsigned view = blockIdx.y;
  if (align_status(res, view, cam.restart) != RGBID_TSDF_ALIGN_RUNNING) return;   // a stopped view's blocks leave at once
  const unsigned tile = blockIdx.x * (VT / 64) + (threadIdx.x >> 6);
  if (tile >= cam.tiles) return;                                // the whole wave
  const unsigned lane = threadIdx.x & 63u;
  const unsigned lx = (tile % cam.tiles_x) * 8u + (lane & 7u), ly = (tile / cam.tiles_x) * 8u + (lane >> 3);
  double tm[ALIGN_TERMS];
#pragma unroll
  for (int k = 0; k < ALIGN_TERMS; ++k) tm[k] = 0.0;
  bool is_used = false;
  if (lx < cam.lw && ly < cam.lh) {                             // ragged tiles
    const unsigned pu = lx * cam.stride, pv = ly * cam.stride;  // step 25: inside the image, the lattice is ceil(cols / stride) wide
    const float mi = views[view].plane[(size_t)pv * (size_t)cam.ray.cols + pu];
    const float z = 1.f / mi;
    if (mi > 0.f && mi < INFINITY && z >= cam.ray.z_min && z <= cam.z_max) {   // measured (NaN fails), and the gate: z_max is finite
      const float* __restrict__ m = pose32 + 12u * view;
      const float dx = ((float)pu - cam.ray.cx) / cam.ray.fx, dy = ((float)pv - cam.ray.cy) / cam.ray.fy;
      const float xc = dx * z, yc = dy * z;
      const float px = rot_row(m, xc, yc, z) + m[9], py = rot_row(m + 3, xc, yc, z) + m[10], pz = rot_row(m + 6, xc, yc, z) + m[11];
      const float gx = (px - g.ox) / g.voxel, gy = (py - g.oy) / g.voxel, gz = (pz - g.oz) / g.voxel;
      unsigned base;
      float fx_, fy_, fz_;
      if (ray_cell(g, st, cam.ray, gx, gy, gz, base, fx_, fy_, fz_)) {   // the 8 counts first; D only for a defined sample
        const unsigned sy = g.nx, sz = g.nx * g.ny;
        float d[8];
#pragma unroll
        for (unsigned c = 0; c < 8; ++c) d[c] = st.D[base + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz];
        const float lx00 = lerp_strict(d[0], d[1], fx_), lx10 = lerp_strict(d[2], d[3], fx_);
        const float lx01 = lerp_strict(d[4], d[5], fx_), lx11 = lerp_strict(d[6], d[7], fx_);
        const float ly0 = lerp_strict(lx00, lx10, fy_), ly1 = lerp_strict(lx01, lx11, fy_);
        const float f = lerp_strict(ly0, ly1, fz_);
        if (fabsf(f) < g.trunc) {
          is_used = true;
          float J[6];
          J[0] = lerp_strict(lerp_strict(d[1] - d[0], d[3] - d[2], fy_), lerp_strict(d[5] - d[4], d[7] - d[6], fy_), fz_) / g.voxel;
          J[1] = lerp_strict(lx10 - lx00, lx11 - lx01, fz_) / g.voxel;
          J[2] = (ly1 - ly0) / g.voxel;
          J[3] = py * J[2] - pz * J[1];
          J[4] = pz * J[0] - px * J[2];
          J[5] = px * J[1] - py * J[0];
          const float af = fabsf(f);
          const float w = af <= cam.huber ? 1.f : cam.huber / af;
          double a[6], Jd[6];
#pragma unroll
          for (int i = 0; i < 6; ++i) { a[i] = (double)(w * J[i]); Jd[i] = (double)J[i]; }
          const double fd = (double)f;
          int k = 0;
#pragma unroll
          for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) tm[k++] = a[i] * Jd[j];   // exact: 24 x 24 bits
#pragma unroll
          for (int i = 0; i < 6; ++i) tm[21 + i] = a[i] * fd;
          tm[27] = (double)(w * f) * fd;
        }
      }
    }
  }
  const unsigned n_used = (unsigned)__popcll(__ballot(is_used));
#pragma unroll
  for (int k = 0; k < ALIGN_TERMS; ++k) tm[k] = tree64(tm[k]);
  if (lane == 0) {
    double* o = sums + (size_t)view * ALIGN_TERMS * a_stride + tile;
#pragma unroll
    for (int k = 0; k < ALIGN_TERMS; ++k) o[(size_t)k * a_stride] = tm[k];
    used[(size_t)view * a_stride + tile] = n_used;
  }
}

// One block per view: the upper rounds of step 28 between the two buffers, then thread 0 walks steps 29 - 32 in double.
__global__ __launch_bounds__(VT) void k_tsdf_align_solve(AlignWork w, AlignRule rule, rgbid_tsdf_align_result* res) {
  RGBID_FP_STRICT
  __shared__ unsigned lds[VT / 64];
  const unsigned view = blockIdx.x;
  if (align_status(res, view, rule.restart) != RGBID_TSDF_ALIGN_RUNNING) return;   // the whole block
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // the used pixels: an integer sum, the same in any order
  unsigned cnt = 0;
  for (unsigned i = threadIdx.x; i < rule.tiles; i += VT) cnt += w.used[(size_t)view * w.a_stride + i];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
  if (lane == 0) lds[wave] = cnt;
  double* src = w.a + (size_t)view * ALIGN_TERMS * w.a_stride;
  double* dst = w.b + (size_t)view * ALIGN_TERMS * w.b_stride;
  size_t src_stride = w.a_stride, dst_stride = w.b_stride;
  unsigned n = rule.tiles;
  while (n > 1u) {
    const unsigned groups = (n + 63u) / 64u;
    for (unsigned item = wave; item < groups * ALIGN_TERMS; item += VT / 64) {
      const unsigned term = item / groups, grp = item % groups, i = grp * 64u + lane;
      const double s = tree64(i < n ? src[(size_t)term * src_stride + i] : 0.0);
      if (lane == 0) dst[(size_t)term * dst_stride + grp] = s;
    }
    __syncthreads();                                            // the round's sums are written before the next round reads them
    double* p = src; src = dst; dst = p;
    const size_t q = src_stride; src_stride = dst_stride; dst_stride = q;
    n = groups;
  }
  __syncthreads();
  rgbid_tsdf_align_result& r = res[view];
  const bool first = r.iterations == 0;
  if (threadIdx.x < ALIGN_TERMS) {                              // step 33: the first and the last system built
    const double s = canonical_nan64(src[(size_t)threadIdx.x * src_stride]);
    r.sums[1][threadIdx.x] = s;
    if (first) r.sums[0][threadIdx.x] = s;
  }
  if (threadIdx.x != 0) return;
  static_assert(VT / 64 == 4, "four waves left their counts");
  const unsigned n_used = lds[0] + lds[1] + lds[2] + lds[3];
  r.used[1] = n_used;
  if (first) r.used[0] = n_used;
  r.iterations += 1;
  if (n_used < rule.min_pixels) { r.status = RGBID_TSDF_ALIGN_FEW; return; }          // step 29
  // step 30
  double H[6][6], L[6][6], b[6], y[6], x[6];
  {
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) { H[i][j] = H[j][i] = src[(size_t)k * src_stride]; ++k; }
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = src[(size_t)(21 + i) * src_stride];
  }
  const double damp = 1.0 + rule.damping;
#pragma unroll
  for (int j = 0; j < 6; ++j) H[j][j] = H[j][j] * damp;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double s = H[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) s = s - L[j][k] * L[j][k];
    if (!(s > 0.0 && s < (double)INFINITY)) ok = false;         // NaN fails; a later column of a failed one is never used
    L[j][j] = sqrt(s);
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double q = H[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) q = q - L[i][k] * L[j][k];
      L[i][j] = q / L[j][j];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = -b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  double biggest = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double ax = fabs(x[i]);
    if (!(ax < (double)INFINITY)) ok = false;                   // NaN and infinity
    biggest = ax > biggest ? ax : biggest;
  }
  if (!ok) { r.status = RGBID_TSDF_ALIGN_SINGULAR; return; }
  // step 31
  const double hx = x[3] / 2.0, hy = x[4] / 2.0, hz = x[5] / 2.0;
  const double nn = sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz));
  const double qw = 1.0 / nn, qx = hx / nn, qy = hy / nn, qz = hz / nn;
  const double xx = qx * qx, yy = qy * qy, zz = qz * qz, xy = qx * qy, xz = qx * qz, yz = qy * qz, wx = qw * qx, wy = qw * qy, wz = qw * qz;
  const double dR[9] = {1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy),
                        2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
                        2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)};
  double P[12], Q[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = r.pose[k];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Q[3 * i + j] = (dR[3 * i] * P[j] + dR[3 * i + 1] * P[3 + j]) + dR[3 * i + 2] * P[6 + j];
    Q[9 + i] = ((dR[3 * i] * P[9] + dR[3 * i + 1] * P[10]) + dR[3 * i + 2] * P[11]) + x[i];
  }
#pragma unroll
  for (int k = 0; k < 12; ++k) {
    r.pose[k] = canonical_nan64(Q[k]);
    w.pose32[12u * view + k] = (float)Q[k];                     // step 24, for the next launch
  }
  r.status = biggest < rule.eps ? RGBID_TSDF_ALIGN_CONVERGED : RGBID_TSDF_ALIGN_RUNNING;   // step 32
}

// triangles of one tile of RUN_TILE cells (a cell is the voxel of its corner 0) -> bc[tile]; total: all of them in 64 bits
__global__ __launch_bounds__(VT) void k_tsdf_tri_count(const unsigned char* __restrict__ ntri, unsigned n, unsigned* __restrict__ bc,
                                                       unsigned long long* __restrict__ total) {
  __shared__ unsigned lds[VT / 64];
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  unsigned c = 0;
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    if (i < n) c += ntri[i];
  }
  unsigned tot;
  block_scan_incl(c, lds, tot);
  if (threadIdx.x == 0) {
    bc[blockIdx.x] = tot;
    if (tot) atomicAdd(total, (unsigned long long)tot);        // integer: the sum is the same in any order
  }
}

__device__ __forceinline__ unsigned edge_vertex(const TsdfGrid& g, const unsigned char* __restrict__ mask, const unsigned* __restrict__ base,
                                                unsigned cell, unsigned corner_lo, unsigned corner_hi) {
  const unsigned p = cell + (corner_lo & 1u) + ((corner_lo >> 1) & 1u) * g.nx + (corner_lo >> 2) * g.nx * g.ny;
  const unsigned b7 = corner_hi - corner_lo - 1u;
  return base[p] + __popc(mask[p] & ((1u << b7) - 1u));
}

// cells of a tile in (round, wave, lane) order, as k_vox_flag_write walks its items: a cell's first triangle is at tile offset + earlier
// rounds + the exclusive block scan of the counts
__global__ __launch_bounds__(VT) void k_tsdf_tri_write(TsdfGrid g, TsdfState st, TsdfRule rule, const unsigned char* __restrict__ mask,
                                                       const unsigned char* __restrict__ ntri, const unsigned* __restrict__ base,
                                                       const unsigned* __restrict__ bc, unsigned* __restrict__ tris) {
  __shared__ unsigned lds[VT / 64];
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  unsigned carry = bc[blockIdx.x];
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    const unsigned nt = i < g.n ? ntri[i] : 0u;
    unsigned tot;
    const unsigned incl = block_scan_incl(nt, lds, tot);
    if (nt) {
      const unsigned cell = (unsigned)i;
      unsigned inside = 0;
      for (unsigned c = 0; c < 8; ++c)
        inside |= (voxel_class(st, cell + (c & 1u) + ((c >> 1) & 1u) * g.nx + (c >> 2) * g.nx * g.ny, rule.min_weight) >> 1) << c;
      unsigned* o = tris + 3 * (size_t)(carry + incl - nt);
      for (int t = 0; t < 6; ++t) {
        unsigned m = 0;
        for (int u = 0; u < 4; ++u) m |= ((inside >> TET_CORNER[t][u]) & 1u) << u;
        const unsigned rows = case_rows(m);
        if (!rows) continue;
        // the rows of step 12 as tetrahedron edges (u, v), u < v
        unsigned eu[6], ev[6];
        if (rows == 1) {
          const unsigned one = __popc(m) == 1 ? m : (~m & 15u);
          const unsigned a = __ffs(one) - 1;
          int k = 0;
          for (unsigned u = 0; u < 4; ++u) {
            if (u == a) continue;
            eu[k] = min(a, u); ev[k] = max(a, u); ++k;
          }
        } else {
          const unsigned om = ~m & 15u;
          const unsigned a = __ffs(m) - 1, b = 31 - __clz(m), c = __ffs(om) - 1, d = 31 - __clz(om);
          eu[0] = min(a, c); ev[0] = max(a, c); eu[1] = min(a, d); ev[1] = max(a, d); eu[2] = min(b, d); ev[2] = max(b, d);
          eu[3] = eu[0]; ev[3] = ev[0]; eu[4] = eu[2]; ev[4] = ev[2]; eu[5] = min(b, c); ev[5] = max(b, c);
        }
        const bool swap = (TET_SWAP[t] >> m) & 1u;
        for (unsigned rw = 0; rw < rows; ++rw) {
          unsigned idx[3];
          for (int k = 0; k < 3; ++k) idx[k] = edge_vertex(g, mask, base, cell, TET_CORNER[t][eu[3 * rw + k]], TET_CORNER[t][ev[3 * rw + k]]);
          o[0] = idx[0]; o[1] = swap ? idx[2] : idx[1]; o[2] = swap ? idx[1] : idx[2];
          o += 3;
        }
      }
    }
    carry += tot;
  }
}

// the largest float32 that is not above m: a floorf result is <= m exactly iff it is <= this
float float_below(unsigned m) {
  float f = (float)m;
  if ((double)f > (double)m) f = std::nextafterf(f, 0.f);
  return f;
}

}  // namespace

struct rgbid_tsdf {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_voxels = 0;
  int cap_views = 0;
  bool with_colour = false;
  TsdfGrid g{};
  TsdfState st{};
  SortWorkspace ws;                            // its compaction part over the 7 n edge flags: bc holds the tile offsets from the plan until the emit
  unsigned* bc_tri = nullptr;                  // [tiles of cap_voxels] the triangles' tile offsets, likewise
  unsigned long long* tri_total = nullptr;     // the triangle count in 64 bits
  unsigned long long* tri_total_host = nullptr;   // pinned
  TsdfView* views = nullptr;                   // [cap_views]
  TsdfView* views_host = nullptr;              // pinned
  unsigned char* mask = nullptr;               // [cap_voxels]
  unsigned char* ntri = nullptr;               // [cap_voxels]
  unsigned* base = nullptr;                    // [cap_voxels]
  // the last plan
  bool planned = false;
  TsdfRule rule{};
  unsigned long long nv = 0, nt = 0;
  // stage timing (rgbid_tsdf_timing): integrate [0, 1], flags and scans [2, 3], emit [4, 5]; rgbid_tsdf_raycast_timing: [6, 7]
  bool timed[3] = {false, false, false};
  bool ray_timed = false;
  Buffers buf;
  StageTimer<8> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
  // alignment (rgbid_tsdf_align): the view table on the first call, the workspace grown to the largest call.  A buffer that is outgrown
  // stays with the handle until it is destroyed (a launch may still read it), and the next one is at least twice as large
  AlignView* align_views = nullptr;            // [cap_views]
  AlignView* align_views_host = nullptr;       // pinned
  AlignWork aw{};
  size_t aw_a = 0, aw_b = 0, aw_used = 0;      // capacities in elements
  // rgbid_tsdf_align_timing: an event before the first launch and after every launch of the last call
  std::vector<hipEvent_t> align_ev;
  int align_timed = 0;                         // iterations of the last call that were recorded
  ~rgbid_tsdf() { for (hipEvent_t e : align_ev) if (e) (void)hipEventDestroy(e); }
  unsigned tiles() const { return (g.n + RUN_TILE - 1) / RUN_TILE; }
};

namespace {

int zero_state(rgbid_tsdf* v) {
  hipStream_t s = v->ctx->stream;
  RGBID_HIP(hipMemsetAsync(v->st.D, 0, sizeof(float) * (size_t)v->g.n, s));
  RGBID_HIP(hipMemsetAsync(v->st.counts, 0, sizeof(unsigned) * (size_t)v->g.n, s));
  if (v->st.rgb)
    for (int ch = 0; ch < 3; ++ch) RGBID_HIP(hipMemsetAsync(v->st.rgb + ch * v->st.stride, 0, sizeof(unsigned) * (size_t)v->g.n, s));
  return RGBID_OK;
}

// one plane of the state to or from a caller buffer; a null source zeroes the destination
int copy_plane(hipStream_t s, void* dst, const void* src, size_t bytes) {
  if (src) RGBID_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s));
  else RGBID_HIP(hipMemsetAsync(dst, 0, bytes, s));
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_tsdf_create(rgbid_tsdf** out, rgbid_ctx* ctx, unsigned long long max_voxels, int max_views, int with_colour) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_voxels < 8 || max_voxels > RGBID_TSDF_MAX_VOXELS) return RGBID_E_INVALID;
  if (max_views < 1 || max_views > RGBID_TSDF_MAX_VIEWS) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_tsdf* v = new (std::nothrow) rgbid_tsdf;
  if (!v) return RGBID_E_NOMEM;
  v->ctx = ctx;
  v->cap_voxels = max_voxels;
  v->cap_views = max_views;
  v->with_colour = with_colour != 0;
  const size_t cap = (size_t)max_voxels;
  v->st.stride = cap;
  int r = v->ws.alloc_compaction(v->buf, 7ull * max_voxels);
  if (!r) r = v->buf.alloc(&v->bc_tri, sizeof(unsigned) * ((cap + RUN_TILE - 1) / RUN_TILE));
  if (!r) r = v->buf.alloc(&v->tri_total, sizeof(unsigned long long));
  if (!r) r = v->buf.alloc_host(&v->tri_total_host, sizeof(unsigned long long));
  if (!r) r = v->buf.alloc(&v->views, sizeof(TsdfView) * (size_t)max_views);
  if (!r) r = v->buf.alloc_host(&v->views_host, sizeof(TsdfView) * (size_t)max_views);
  if (!r) r = v->buf.alloc(&v->st.D, sizeof(float) * cap);
  if (!r) r = v->buf.alloc(&v->st.counts, sizeof(unsigned) * cap);
  if (!r && v->with_colour) r = v->buf.alloc(&v->st.rgb, sizeof(unsigned) * 3 * cap);
  if (!r) r = v->buf.alloc(&v->mask, cap);
  if (!r) r = v->buf.alloc(&v->ntri, cap);
  if (!r) r = v->buf.alloc(&v->base, sizeof(unsigned) * cap);
  const float origin[3] = {0.f, 0.f, 0.f};
  if (!r) r = rgbid_tsdf_configure(v, 2, 2, 2, origin, 1.f, 1.f);
  if (r) { rgbid_tsdf_destroy(v); return r; }
  *out = v;
  return RGBID_OK;
}

int rgbid_tsdf_destroy(rgbid_tsdf* v) { return destroy_handle(v); }   // a launch may still read the tables

int rgbid_tsdf_configure(rgbid_tsdf* v, int nx, int ny, int nz, const float origin[3], float voxel, float trunc) {
  if (!v || !origin || nx < 2 || ny < 2 || nz < 2) return RGBID_E_INVALID;
  if ((unsigned long long)nx * (unsigned long long)ny > v->cap_voxels || (unsigned long long)nx * ny * (unsigned long long)nz > v->cap_voxels)
    return RGBID_E_INVALID;
  if (!(std::isfinite(voxel) && std::isfinite(trunc) && voxel > 0.f && trunc > 0.f)) return RGBID_E_INVALID;
  for (int a = 0; a < 3; ++a) if (!std::isfinite(origin[a])) return RGBID_E_INVALID;
  v->g.nx = (unsigned)nx; v->g.ny = (unsigned)ny; v->g.nz = (unsigned)nz;
  v->g.n = (unsigned)((unsigned long long)nx * ny * nz);
  v->g.ox = origin[0]; v->g.oy = origin[1]; v->g.oz = origin[2]; v->g.voxel = voxel; v->g.trunc = trunc;
  return rgbid_tsdf_reset(v);
}

int rgbid_tsdf_reset(rgbid_tsdf* v) {
  if (!v) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  v->planned = false;
  return zero_state(v);
}

int rgbid_tsdf_integrate(rgbid_tsdf* v, int V, const rgbid_tsdf_view* views, const float K[4], int rows, int cols, float z_min, float z_max) {
  if (!v || !views || !K) return RGBID_E_INVALID;
  if (V < 1 || V > v->cap_views) return RGBID_E_INVALID;
  if (rows < 1 || cols < 1 || rows > RGBID_TSDF_MAX_DIM || cols > RGBID_TSDF_MAX_DIM) return RGBID_E_INVALID;
  if (!(std::isfinite(z_min) && std::isfinite(z_max) && z_min > 0.f && z_min <= z_max)) return RGBID_E_INVALID;
  for (int k = 0; k < 4; ++k) if (!std::isfinite(K[k])) return RGBID_E_INVALID;
  if (K[0] == 0.f || K[1] == 0.f) return RGBID_E_INVALID;
  for (int i = 0; i < V; ++i) {
    if (!finite_all(views[i].pose.R, 9) || !finite_all(views[i].pose.t, 3)) return RGBID_E_INVALID;
    float cw[12];
    rgbid_render_pose_cw(&views[i].pose, cw);
    for (int k = 0; k < 12; ++k) if (!std::isfinite(cw[k])) return RGBID_E_INVALID;
    if (!views[i].depthinv_dev || !aligned4(views[i].depthinv_dev)) return RGBID_E_INVALID;
  }
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  RGBID_HIP(hipStreamSynchronize(s));   // the previous call's copy has read the pinned table
  for (int i = 0; i < V; ++i) {
    TsdfView& vw = v->views_host[i];
    rgbid_render_pose_cw(&views[i].pose, vw.m);
    vw.plane = views[i].depthinv_dev;
    vw.colour = v->with_colour ? views[i].colour_dev : nullptr;
  }
  TsdfCam cam;
  cam.fx = K[0]; cam.fy = K[1]; cam.cx = K[2]; cam.cy = K[3]; cam.z_min = z_min; cam.z_max = z_max;
  cam.hi_u = (float)(cols - 1); cam.hi_v = (float)(rows - 1); cam.cols = cols;
  v->planned = false;
  v->timed[0] = false;
  const unsigned gx = grid_of(((unsigned long long)v->g.n + VT - 1) / VT);
  v->mark(0);
  RGBID_HIP(hipMemcpyAsync(v->views, v->views_host, sizeof(TsdfView) * (size_t)V, hipMemcpyHostToDevice, s));
  for (int v0 = 0; v0 < V; v0 += VIEW_CHUNK)   // in order: the mean of step 7 does not commute
    hipLaunchKernelGGL(k_tsdf_integrate, dim3(gx), dim3(VT), 0, s, v->g, cam, v->views, v0, v0 + VIEW_CHUNK < V ? v0 + VIEW_CHUNK : V, v->st);
  v->mark(1);
  RGBID_HIP(hipGetLastError());
  v->timed[0] = v->timer.on;
  return RGBID_OK;
}

int rgbid_tsdf_get_state(rgbid_tsdf* v, float* D_dev, uint32_t* counts_dev, uint32_t* rgb_sum_dev) {
  if (!v || !aligned4(D_dev) || !aligned4(counts_dev) || !aligned4(rgb_sum_dev)) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  const size_t n = v->g.n;
  if (D_dev) RGBID_HIP(hipMemcpyAsync(D_dev, v->st.D, sizeof(float) * n, hipMemcpyDeviceToDevice, s));
  if (counts_dev) RGBID_HIP(hipMemcpyAsync(counts_dev, v->st.counts, sizeof(unsigned) * n, hipMemcpyDeviceToDevice, s));
  if (rgb_sum_dev)
    for (int ch = 0; ch < 3; ++ch)
      if (int r = copy_plane(s, rgb_sum_dev + ch * n, v->st.rgb ? v->st.rgb + ch * v->st.stride : nullptr, sizeof(unsigned) * n)) return r;
  return RGBID_OK;
}

int rgbid_tsdf_set_state(rgbid_tsdf* v, const float* D_dev, const uint32_t* counts_dev, const uint32_t* rgb_sum_dev) {
  if (!v || !aligned4(D_dev) || !aligned4(counts_dev) || !aligned4(rgb_sum_dev)) return RGBID_E_INVALID;
  if (rgb_sum_dev && !v->with_colour) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  const size_t n = v->g.n;
  v->planned = false;
  if (int r = copy_plane(s, v->st.D, D_dev, sizeof(float) * n)) return r;
  if (int r = copy_plane(s, v->st.counts, counts_dev, sizeof(unsigned) * n)) return r;
  if (v->st.rgb)
    for (int ch = 0; ch < 3; ++ch)
      if (int r = copy_plane(s, v->st.rgb + ch * v->st.stride, rgb_sum_dev ? rgb_sum_dev + ch * n : nullptr, sizeof(unsigned) * n)) return r;
  return RGBID_OK;
}

int rgbid_tsdf_extract_plan(rgbid_tsdf* v, unsigned min_weight, unsigned long long* n_vertices, unsigned long long* n_triangles) {
  if (!v || !n_vertices || !n_triangles) return RGBID_E_INVALID;
  if (min_weight < 1 || min_weight > MAX_W) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  v->planned = false;
  v->timed[1] = false;
  *n_vertices = *n_triangles = 0;
  const TsdfRule rule{min_weight};
  const unsigned n = v->g.n;
  v->mark(2);
  RGBID_HIP(hipMemsetAsync(v->tri_total, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_tsdf_classify, dim3(grid_of(((unsigned long long)n + VT - 1) / VT)), dim3(VT), 0, s, v->g, v->st, rule, v->mask, v->ntri);
  v->ws.count_scan(s, EdgeSrc{v->g, v->st, v->mask, nullptr, nullptr, nullptr}, 7u * n, SLOT_VERTS);   // the emit writes with these offsets
  hipLaunchKernelGGL(k_tsdf_tri_count, dim3(v->tiles()), dim3(VT), 0, s, v->ntri, n, v->bc_tri, v->tri_total);
  hipLaunchKernelGGL(k_vox_scan1, dim3(1), dim3(VT), 0, s, v->bc_tri, v->tiles(), v->ws.slots, (int)SLOT_TRIS, (unsigned*)nullptr, 0u);
  v->mark(3);
  RGBID_HIP(hipGetLastError());
  RGBID_HIP(hipMemcpyAsync(v->tri_total_host, v->tri_total, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  if (int r = v->ws.read_slots(s)) return r;
  v->timed[1] = v->timer.on;
  if (*v->tri_total_host != v->ws.slots_host[SLOT_TRIS]) return RGBID_E_INVALID;   // 2^32 triangles or more
  v->nv = v->ws.slots_host[SLOT_VERTS];
  v->nt = v->ws.slots_host[SLOT_TRIS];
  v->rule = rule;
  v->planned = true;
  *n_vertices = v->nv;
  *n_triangles = v->nt;
  return RGBID_OK;
}

int rgbid_tsdf_extract_emit(rgbid_tsdf* v, float* vertices_dev, uint8_t* colours_dev, uint32_t* triangles_dev,
                            unsigned long long vertex_capacity, unsigned long long triangle_capacity) {
  if (!v || !v->planned) return RGBID_E_INVALID;
  if (v->nv == 0) return RGBID_OK;             // no active edge: no triangle either
  if (!vertices_dev || !aligned4(vertices_dev) || vertex_capacity < v->nv) return RGBID_E_INVALID;
  if (v->nt && (!triangles_dev || !aligned4(triangles_dev) || triangle_capacity < v->nt)) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  v->timed[2] = false;
  v->mark(4);
  v->ws.write(s, EdgeSrc{v->g, v->st, v->mask, v->base, vertices_dev, colours_dev}, 7u * v->g.n);
  if (v->nt)
    hipLaunchKernelGGL(k_tsdf_tri_write, dim3(v->tiles()), dim3(VT), 0, s, v->g, v->st, v->rule, v->mask, v->ntri, v->base, v->bc_tri, triangles_dev);
  v->mark(5);
  RGBID_HIP(hipGetLastError());
  v->timed[2] = v->timer.on;
  return RGBID_OK;
}

int rgbid_tsdf_pose_wc(const rgbid_render_pose* pose, float wc[12]) {
  if (!pose || !wc) return RGBID_E_INVALID;
  for (int k = 0; k < 9; ++k) wc[k] = (float)pose->R[k];
  for (int k = 0; k < 3; ++k) wc[9 + k] = (float)pose->t[k];
  return RGBID_OK;
}

int rgbid_tsdf_raycast(rgbid_tsdf* v, int V, const rgbid_render_pose* poses, const float K[4], int rows, int cols, float z_min, float z_max,
                       float step, unsigned min_weight, float* depth_dev, float* normal_dev, uint8_t* colour_dev) {
  RGBID_FP_STRICT
  if (!v || !poses || !K) return RGBID_E_INVALID;
  if (V < 1 || V > v->cap_views) return RGBID_E_INVALID;
  if (rows < 1 || cols < 1 || rows > RGBID_TSDF_MAX_DIM || cols > RGBID_TSDF_MAX_DIM) return RGBID_E_INVALID;
  if ((unsigned long long)rows * (unsigned long long)cols * (unsigned long long)V >= (1ull << 31)) return RGBID_E_INVALID;
  if (!(std::isfinite(z_min) && std::isfinite(z_max) && z_min > 0.f && z_min <= z_max)) return RGBID_E_INVALID;
  if (!(std::isfinite(step) && step > 0.f)) return RGBID_E_INVALID;
  if (((double)z_max - (double)z_min) / (double)step > (double)RGBID_TSDF_MAX_STEPS) return RGBID_E_INVALID;
  if (min_weight < 1 || min_weight > MAX_W) return RGBID_E_INVALID;
  for (int k = 0; k < 4; ++k) if (!std::isfinite(K[k])) return RGBID_E_INVALID;
  if (K[0] == 0.f || K[1] == 0.f) return RGBID_E_INVALID;
  for (int i = 0; i < V; ++i) {
    if (!finite_all(poses[i].R, 9) || !finite_all(poses[i].t, 3)) return RGBID_E_INVALID;
    float wc[12];
    rgbid_tsdf_pose_wc(&poses[i], wc);
    for (int k = 0; k < 12; ++k) if (!std::isfinite(wc[k])) return RGBID_E_INVALID;
  }
  if (!aligned4(depth_dev) || !aligned4(normal_dev)) return RGBID_E_INVALID;
  if (!depth_dev && !normal_dev && !colour_dev) return RGBID_OK;
  RayCam cam;
  cam.fx = K[0]; cam.fy = K[1]; cam.cx = K[2]; cam.cy = K[3]; cam.z_min = z_min; cam.step = step;
  cam.hi_i = float_below(v->g.nx - 2u); cam.hi_j = float_below(v->g.ny - 2u); cam.hi_k = float_below(v->g.nz - 2u);
  cam.n_last = 0;                              // step 15: Z_0 = z_min <= z_max; Z_n does not decrease with n
  while (cam.n_last < RGBID_TSDF_MAX_STEPS && z_min + (float)(cam.n_last + 1u) * step <= z_max) ++cam.n_last;
  cam.min_weight = min_weight;
  cam.rows = rows; cam.cols = cols;
  cam.tiles_x = ((unsigned)cols + 7u) / 8u;
  cam.tiles = cam.tiles_x * (((unsigned)rows + 7u) / 8u);   // below 2^31 / 64 + 2^18
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  RGBID_HIP(hipStreamSynchronize(s));   // the previous call's copy has read the pinned table
  float* table_host = reinterpret_cast<float*>(v->views_host);   // 48 of a view's 64 bytes
  float* table = reinterpret_cast<float*>(v->views);
  for (int i = 0; i < V; ++i) rgbid_tsdf_pose_wc(&poses[i], table_host + 12 * i);
  v->ray_timed = false;
  v->mark(6);
  RGBID_HIP(hipMemcpyAsync(table, table_host, sizeof(float) * 12 * (size_t)V, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_tsdf_raycast, dim3((cam.tiles + VT / 64 - 1) / (VT / 64), (unsigned)V), dim3(VT), 0, s, v->g, v->st, cam, table,
                     RayOut{depth_dev, normal_dev, colour_dev});
  v->mark(7);
  RGBID_HIP(hipGetLastError());
  v->ray_timed = v->timer.on;
  return RGBID_OK;
}

int rgbid_tsdf_raycast_timing(rgbid_tsdf* v, int enable, float ms[1]) {
  if (!v) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  if (ms) {
    ms[0] = 0.f;
    if (v->ray_timed) RGBID_HIP(v->timer.elapsed(6, 7, &ms[0]));
  }
  return v->timer.enable(enable != 0);
}

int rgbid_tsdf_extract_normals(rgbid_tsdf* v, float* normals_dev, unsigned long long vertex_capacity) {
  if (!v || !v->planned) return RGBID_E_INVALID;
  if (v->nv == 0) return RGBID_OK;
  if (!normals_dev || !aligned4(normals_dev) || vertex_capacity < v->nv) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  v->ws.write(v->ctx->stream, NormalSrc{v->g, v->st, v->mask, v->rule.min_weight, normals_dev}, 7u * v->g.n);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_tsdf_timing(rgbid_tsdf* v, int enable, float ms[3]) {
  if (!v) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  if (ms)
    for (int k = 0; k < 3; ++k) {
      ms[k] = 0.f;
      if (v->timed[k]) RGBID_HIP(v->timer.elapsed(2 * k, 2 * k + 1, &ms[k]));
    }
  return v->timer.enable(enable != 0);
}

}  // extern "C"

namespace {

template <class T>
int grow(Buffers& buf, T** p, size_t& cap, size_t need) {
  if (need <= cap) return RGBID_OK;
  const size_t n = need > 2 * cap ? need : 2 * cap;
  T* q = nullptr;
  if (int r = buf.alloc(&q, sizeof(T) * n)) return r;
  *p = q;
  cap = n;
  return RGBID_OK;
}

unsigned tiles_of(int rows, int cols, int stride, unsigned* tiles_x) {
  const unsigned lw = ((unsigned)cols + stride - 1) / stride, lh = ((unsigned)rows + stride - 1) / stride;
  *tiles_x = (lw + 7u) / 8u;
  return *tiles_x * ((lh + 7u) / 8u);
}

}  // namespace

extern "C" {

int rgbid_tsdf_align(rgbid_tsdf* v, int V, const rgbid_tsdf_view* views, const float K[4], int rows, int cols, float z_min, float z_max,
                     unsigned min_weight, float huber, double damping, double eps, unsigned min_pixels, int n_levels,
                     const rgbid_tsdf_align_level* levels, rgbid_tsdf_align_result* result_dev) {
  if (!v || !views || !K || !levels) return RGBID_E_INVALID;
  if (V < 1 || V > v->cap_views) return RGBID_E_INVALID;
  if (rows < 1 || cols < 1 || rows > RGBID_TSDF_MAX_DIM || cols > RGBID_TSDF_MAX_DIM) return RGBID_E_INVALID;
  if ((unsigned long long)rows * (unsigned long long)cols * (unsigned long long)V >= (1ull << 31)) return RGBID_E_INVALID;
  if (!(std::isfinite(z_min) && std::isfinite(z_max) && z_min > 0.f && z_min <= z_max)) return RGBID_E_INVALID;
  if (min_weight < 1 || min_weight > MAX_W) return RGBID_E_INVALID;
  if (!(std::isfinite(huber) && huber > 0.f)) return RGBID_E_INVALID;
  if (!(std::isfinite(damping) && damping >= 0.0)) return RGBID_E_INVALID;
  if (!(std::isfinite(eps) && eps > 0.0)) return RGBID_E_INVALID;
  if (min_pixels < 6) return RGBID_E_INVALID;
  if (n_levels < 1 || n_levels > RGBID_TSDF_ALIGN_MAX_LEVELS) return RGBID_E_INVALID;
  int total = 0, finest = 8;
  for (int l = 0; l < n_levels; ++l) {
    const int s = levels[l].stride, it = levels[l].iterations;
    if (s != 1 && s != 2 && s != 4 && s != 8) return RGBID_E_INVALID;
    if (it < 1 || it > RGBID_TSDF_ALIGN_MAX_ITERATIONS) return RGBID_E_INVALID;
    total += it;
    finest = s < finest ? s : finest;
  }
  if (total > RGBID_TSDF_ALIGN_MAX_ITERATIONS) return RGBID_E_INVALID;
  for (int k = 0; k < 4; ++k) if (!std::isfinite(K[k])) return RGBID_E_INVALID;
  if (K[0] == 0.f || K[1] == 0.f) return RGBID_E_INVALID;
  for (int i = 0; i < V; ++i) {
    if (!finite_all(views[i].pose.R, 9) || !finite_all(views[i].pose.t, 3)) return RGBID_E_INVALID;
    float wc[12];
    rgbid_tsdf_pose_wc(&views[i].pose, wc);
    for (int k = 0; k < 12; ++k) if (!std::isfinite(wc[k])) return RGBID_E_INVALID;
    if (!views[i].depthinv_dev || !aligned4(views[i].depthinv_dev)) return RGBID_E_INVALID;
  }
  if (!result_dev || (((uintptr_t)result_dev) & 7)) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  // the workspace: the finest level has the most tiles
  unsigned tx;
  const size_t a_stride = tiles_of(rows, cols, finest, &tx), b_stride = (a_stride + 63) / 64;
  if (!v->align_views) {
    int r = v->buf.alloc(&v->align_views, sizeof(AlignView) * (size_t)v->cap_views);
    if (!r) r = v->buf.alloc_host(&v->align_views_host, sizeof(AlignView) * (size_t)v->cap_views);
    if (!r) r = v->buf.alloc(&v->aw.pose32, sizeof(float) * 12 * (size_t)v->cap_views);
    if (r) { v->align_views = nullptr; return r; }
  }
  if (int r = grow(v->buf, &v->aw.a, v->aw_a, (size_t)V * ALIGN_TERMS * a_stride)) return r;
  if (int r = grow(v->buf, &v->aw.b, v->aw_b, (size_t)V * ALIGN_TERMS * b_stride)) return r;
  if (int r = grow(v->buf, &v->aw.used, v->aw_used, (size_t)V * a_stride)) return r;
  v->aw.a_stride = a_stride; v->aw.b_stride = b_stride;
  const bool timing = v->timer.on;
  if (timing) {
    if (v->align_ev.size() < (size_t)(2 * total + 1)) v->align_ev.resize(2 * total + 1, nullptr);
    for (int k = 0; k < 2 * total + 1; ++k) if (!v->align_ev[k]) RGBID_HIP(hipEventCreate(&v->align_ev[k]));
  }
  RGBID_HIP(hipStreamSynchronize(s));   // the previous call's copy has read the pinned table
  for (int i = 0; i < V; ++i) {
    AlignView& vw = v->align_views_host[i];
    for (int k = 0; k < 9; ++k) vw.pose[k] = views[i].pose.R[k];
    for (int k = 0; k < 3; ++k) vw.pose[9 + k] = views[i].pose.t[k];
    vw.plane = views[i].depthinv_dev;
  }
  AlignCam cam{};
  cam.ray.fx = K[0]; cam.ray.fy = K[1]; cam.ray.cx = K[2]; cam.ray.cy = K[3]; cam.ray.z_min = z_min;
  cam.ray.hi_i = float_below(v->g.nx - 2u); cam.ray.hi_j = float_below(v->g.ny - 2u); cam.ray.hi_k = float_below(v->g.nz - 2u);
  cam.ray.min_weight = min_weight;
  cam.ray.rows = rows; cam.ray.cols = cols;
  cam.z_max = z_max; cam.huber = huber;
  AlignRule rule{damping, eps, min_pixels, 0u, 0u};
  v->align_timed = 0;
  int e = 0;
  RGBID_HIP(hipMemcpyAsync(v->align_views, v->align_views_host, sizeof(AlignView) * (size_t)V, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_tsdf_align_init, dim3(((unsigned)V + VT - 1) / VT), dim3(VT), 0, s, v->align_views, V, result_dev, v->aw.pose32);
  if (timing) (void)hipEventRecord(v->align_ev[e++], s);
  for (int l = 0; l < n_levels; ++l) {
    cam.stride = (unsigned)levels[l].stride;
    cam.lw = ((unsigned)cols + cam.stride - 1u) / cam.stride;
    cam.lh = ((unsigned)rows + cam.stride - 1u) / cam.stride;
    cam.tiles = tiles_of(rows, cols, levels[l].stride, &cam.tiles_x);
    rule.tiles = cam.tiles;
    for (int it = 0; it < levels[l].iterations; ++it) {          // enqueued without waiting: the device decides who still runs
      cam.restart = rule.restart = (l > 0 && it == 0) ? 1u : 0u;
      hipLaunchKernelGGL(k_tsdf_align_system, dim3((cam.tiles + VT / 64 - 1) / (VT / 64), (unsigned)V), dim3(VT), 0, s, v->g, v->st, cam,
                         v->align_views, v->aw.pose32, result_dev, v->aw.a, v->aw.used, a_stride);
      if (timing) (void)hipEventRecord(v->align_ev[e++], s);
      hipLaunchKernelGGL(k_tsdf_align_solve, dim3((unsigned)V), dim3(VT), 0, s, v->aw, rule, result_dev);
      if (timing) (void)hipEventRecord(v->align_ev[e++], s);
    }
  }
  RGBID_HIP(hipGetLastError());
  v->align_timed = timing ? total : 0;
  return RGBID_OK;
}

int rgbid_tsdf_align_timing(rgbid_tsdf* v, int enable, float ms[2]) {
  if (!v) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  if (ms) {
    ms[0] = ms[1] = 0.f;
    for (int i = 0; i < v->align_timed; ++i) {
      float a = 0.f, b = 0.f;
      RGBID_HIP(hipEventElapsedTime(&a, v->align_ev[2 * i], v->align_ev[2 * i + 1]));
      RGBID_HIP(hipEventElapsedTime(&b, v->align_ev[2 * i + 1], v->align_ev[2 * i + 2]));
      ms[0] += a; ms[1] += b;
    }
  }
  return v->timer.enable(enable != 0);
}

}  // extern "C"
