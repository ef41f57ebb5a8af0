// kernels_tsdf.hip -- keyframes fused into a truncated signed distance volume, and the volume's surface as a triangle mesh
// (include/rgbid_tsdf.h).
//
// The judge is tests/tsdf_mirror.py; state, counts and mesh are byte-identical to it.
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
// No atomic touches the state and no result depends on the order of threads or waves.
//
// Exact arithmetic: RGBID_FP_STRICT (common.h) opens every function that forms a float32 product followed by a sum, so no FMA is formed
// from them; the divisions are hipcc's default correctly rounded ones.
#include "../../include/rgbid_tsdf.h"
#include "common.h"
#include "hip_host.h"
#include "voxel_device.h"   // flag compaction, the one-block scan, grid_of

#include <cmath>
#include <new>

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

__device__ __forceinline__ float rot_row(const float* __restrict__ m, float x, float y, float z) {
  RGBID_FP_STRICT
  return (m[0] * x + m[1] * y) + m[2] * z;
}

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
      if ((c ^ c_in) >> 16) {
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
  // step 11's mean of one end and channel; false when the end has none
  __device__ __forceinline__ bool mean(unsigned i, unsigned cn, int ch, float& out) const {
    if (!st.rgb || cn == 0) return false;
    const unsigned long long s = st.rgb[ch * st.stride + i];
    const unsigned long long q = (2ull * s + cn) / (2ull * cn);
    out = (float)(q < 255ull ? q : 255ull);
    return true;
  }
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
    float* o = verts + 3 * (size_t)pos;
    o[0] = lerp_strict(centre(g.ox, ax, g.voxel), centre(g.ox, bx, g.voxel), t);
    o[1] = lerp_strict(centre(g.oy, ay, g.voxel), centre(g.oy, by, g.voxel), t);
    o[2] = lerp_strict(centre(g.oz, az, g.voxel), centre(g.oz, bz, g.voxel), t);
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

bool finite_all(const double* p, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(p[i])) return false;
  return true;
}

bool aligned4(const void* p) { return !(((uintptr_t)p) & 3); }

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
  // stage timing (rgbid_tsdf_timing): integrate [0, 1], flags and scans [2, 3], emit [4, 5]
  bool timed[3] = {false, false, false};
  Buffers buf;
  StageTimer<6> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
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
