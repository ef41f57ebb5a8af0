// kernels_meshdist.hip -- the nearest triangle of an indexed triangle mesh within d_max of every query point, the closest point on it and
// the distance (include/rgbid_meshdist.h).
//
// The judge is tests/meshdist_mirror.py, a brute force over all triangles; the grid only finds the candidates.
//   plan   k_mesh_check       mesh_device.h: counts the triangles with an index >= n_v into a slot
//          k_md_gather        one thread per triangle: its nine coordinates once, as three 16-byte rows (NaN rows for a bad index)
//          k_vox_box          twice, over the low and the high corners of the boxes of the triangles that take part (TriBox); read back
//                             with the slot of the index check: a bad index or a box outside the grid's bounds ends the call here
//          k_md_count         a triangle's cells, (hi - lo + 1) per axis multiplied in 64 bits, summed per tile of 2 048 triangles with
//          k_md_total         saturating adds; the total is read back and held against max_pairs
//          k_vox_scan1        the tiles' offsets
//          k_md_pairs         a triangle writes (cell key, triangle) for every cell of its range at tile offset + scan inside the tile
//          LSD radix sort     voxel_device.h, stable: a cell's run in ascending triangle index
//          cell table         flag compaction of the heads key[i] != key[i - 1]: the occupied cells' keys and run starts
//          k_md_longest       the longest run, one integer atomic per wave
//   query  k_vox_keys + sort  (the handle's switch) the queries' cells over points clamped to the mesh's box: the order of the walk only
//          k_meshdist_query   one thread per query: 9 rows of 3 x-adjacent cells, each one binary search on the occupied cells and one
//                             contiguous walk; per candidate the box test, the closest point in double and a compare on (d2, index);
//                             results go to the query's input position
// No float atomics, no wait on another thread, every loop has its bound when it starts.
#include "../../include/rgbid_meshdist.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // the index check, the argument test, the create; voxel_device.h's box, grid, cell keys, radix sort, flag
                            // compaction and point sources; the sort workspace

#include <cmath>
#include <cstring>

using namespace rgbid;

static_assert(sizeof(rgbid_cloud_point) == 32, "RecordPoints reads the first 16 bytes of a 32-byte record");

namespace {

constexpr unsigned NONE = RGBID_MESHDIST_NONE;
constexpr unsigned NAN_BITS = RGBID_RENDER_NAN_BITS;
// beside the workspace's own 0 .. 8: the low corner of the box (3), the bad indices, the pairs (2 words), the longest run
enum { SLOT_CELLS = SLOT_RUNS, SLOT_OFFSETS = SLOT_VOXELS, SLOT_LO = 9, SLOT_BAD = 12, SLOT_PAIRS = 13, SLOT_LONGEST = 15 };
static_assert(SLOT_VOXELS < SLOT_LO && SLOT_LONGEST < SLOTS, "the slots of this file lie behind the workspace's");

struct MdGrid {
  VoxGrid g;
  int d[3];       // cells per axis (each <= 2^19 + 1)
};

// ---- the triangles' corners -------------------------------------------------------------------------------------------------------------
struct Corners {
  float4 a, b, c;   // x y z and a fourth float that nobody reads
  __device__ __forceinline__ bool finite() const { return finite3(a.x, a.y, a.z) && finite3(b.x, b.y, b.z) && finite3(c.x, c.y, c.z); }
  __device__ __forceinline__ void box(float lo[3], float hi[3]) const {
    lo[0] = fminf(fminf(a.x, b.x), c.x); lo[1] = fminf(fminf(a.y, b.y), c.y); lo[2] = fminf(fminf(a.z, b.z), c.z);
    hi[0] = fmaxf(fmaxf(a.x, b.x), c.x); hi[1] = fmaxf(fmaxf(a.y, b.y), c.y); hi[2] = fmaxf(fmaxf(a.z, b.z), c.z);
  }
};

__device__ __forceinline__ Corners corners_of(const float4* __restrict__ rec, size_t t) {
  return Corners{rec[3 * t], rec[3 * t + 1], rec[3 * t + 2]};
}

__global__ __launch_bounds__(VT) void k_md_gather(const float* __restrict__ verts, const unsigned* __restrict__ tri, unsigned n_v, unsigned n_t,
                                                  float4* __restrict__ rec) {
  for (size_t t = (size_t)blockIdx.x * VT + threadIdx.x; t < n_t; t += (size_t)gridDim.x * VT) {
    for (int k = 0; k < 3; ++k) {
      const unsigned i = tri[3 * t + k];
      float4 p = make_float4(NAN, NAN, NAN, 0.f);              // an index that names no vertex reads nothing; the plan refuses the mesh
      if (i < n_v) p = VertexPoints{verts}.at(i);
      rec[3 * t + k] = p;
    }
  }
}

// k_vox_box's point source over the triangles: the low or the high corner of the box of a triangle that takes part, NaN for the others
template <bool HI>
struct TriBox {
  const float4* rec;
  __device__ __forceinline__ float4 at(unsigned t) const {
    const Corners c = corners_of(rec, t);
    if (!c.finite()) return make_float4(NAN, NAN, NAN, 0.f);
    float lo[3], hi[3];
    c.box(lo, hi);
    return HI ? make_float4(hi[0], hi[1], hi[2], 0.f) : make_float4(lo[0], lo[1], lo[2], 0.f);
  }
};

// cell_key's index on one axis
__device__ __forceinline__ int cell_axis(float p, float inv, float minb) {
  RGBID_FP_STRICT
  return (int)(floorf(p * inv) - minb);
}

// the cell range of triangle t; false when it does not take part
__device__ __forceinline__ bool tri_cells(const float4* __restrict__ rec, size_t t, const VoxGrid& g, int lo[3], int hi[3]) {
  const Corners c = corners_of(rec, t);
  if (!c.finite()) return false;
  float flo[3], fhi[3];
  c.box(flo, fhi);
  for (int a = 0; a < 3; ++a) {
    lo[a] = cell_axis(flo[a], g.inv[a], g.minb[a]);
    hi[a] = cell_axis(fhi[a], g.inv[a], g.minb[a]);
  }
  return true;
}

__device__ __forceinline__ unsigned long long sat_add(unsigned long long a, unsigned long long b) {
  const unsigned long long s = a + b;
  return s < a ? ~0ull : s;
}

// the cells of the tile's triangles: the 64-bit sum, saturating, and its 32-bit clamp for the scan (used only when the total fits)
__global__ __launch_bounds__(VT) void k_md_count(const float4* __restrict__ rec, unsigned n_t, VoxGrid g, unsigned long long* __restrict__ tile64,
                                                 unsigned* __restrict__ bc) {
  __shared__ unsigned long long lds[VT / 64];
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  unsigned long long c = 0;
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t t = t0 + j * VT + threadIdx.x;
    int lo[3], hi[3];
    if (t < n_t && tri_cells(rec, t, g, lo, hi))   // each factor <= 2^19 + 1: the product is below 2^58
      c = sat_add(c, (unsigned long long)(hi[0] - lo[0] + 1) * (unsigned long long)(hi[1] - lo[1] + 1) * (unsigned long long)(hi[2] - lo[2] + 1));
  }
  for (int o = 32; o > 0; o >>= 1) c = sat_add(c, __shfl_xor(c, o, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long s = sat_add(sat_add(lds[0], lds[1]), sat_add(lds[2], lds[3]));
    tile64[blockIdx.x] = s;
    bc[blockIdx.x] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)s;
  }
}

// one wave: the tiles' sums -> the pair count in two slots
__global__ __launch_bounds__(64) void k_md_total(const unsigned long long* __restrict__ tile64, unsigned tiles, unsigned* __restrict__ slots) {
  unsigned long long c = 0;
  for (unsigned b = threadIdx.x; b < tiles; b += 64) c = sat_add(c, tile64[b]);
  for (int o = 32; o > 0; o >>= 1) c = sat_add(c, __shfl_xor(c, o, 64));
  if (threadIdx.x == 0) {
    slots[SLOT_PAIRS] = (unsigned)c;
    slots[SLOT_PAIRS + 1] = (unsigned)(c >> 32);
  }
}

// the pairs of a tile's triangles, triangle after triangle, a triangle's cells in ascending key: items of a tile in (round, thread)
// order, position = tile offset + earlier rounds + the scan over the round.  n_pairs bounds every store
template <typename K>
__global__ __launch_bounds__(VT) void k_md_pairs(const float4* __restrict__ rec, unsigned n_t, MdGrid og, const unsigned* __restrict__ bc, unsigned n_pairs,
                                                 K* __restrict__ keys, unsigned* __restrict__ idx) {
  __shared__ unsigned lds[VT / 64];
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  unsigned carry = bc[blockIdx.x];
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t t = t0 + j * VT + threadIdx.x;
    int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};
    unsigned c = 0;
    if (t < n_t && tri_cells(rec, t, og.g, lo, hi)) c = (unsigned)(hi[0] - lo[0] + 1) * (unsigned)(hi[1] - lo[1] + 1) * (unsigned)(hi[2] - lo[2] + 1);
    unsigned tot;
    const unsigned incl = block_scan_incl(c, lds, tot);
    unsigned pos = carry + incl - c;
    if (c)
      for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y) {
          const unsigned long long base = (unsigned long long)y * og.g.d0 + (unsigned long long)z * og.g.d01;
          for (int x = lo[0]; x <= hi[0]; ++x, ++pos)
            if (pos < n_pairs) {
              keys[pos] = (K)(base + (unsigned long long)x);
              idx[pos] = (unsigned)t;
            }
        }
    carry += tot;
  }
}

// the cell table, as the radius outlier filter builds its own: head i -> (start, key) of cell `rank`
template <typename K>
struct RunSrc {
  const K* keys;
  unsigned n;
  unsigned* starts;
  K* ukeys;
  __device__ __forceinline__ unsigned size() const { return n; }
  __device__ __forceinline__ bool flag(unsigned i) const { return i == 0 || keys[i] != keys[i - 1]; }
  __device__ __forceinline__ void write(unsigned pos, unsigned i) const { starts[pos] = i; ukeys[pos] = keys[i]; }
};

// first cell whose key is >= k, in [0, cells]
template <typename K>
__device__ __forceinline__ unsigned lower_run(const K* __restrict__ ukeys, unsigned cells, K k) {
  unsigned lo = 0, hi = cells;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (ukeys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(VT) void k_md_longest(const unsigned* __restrict__ starts, unsigned* __restrict__ slots) {
  const unsigned cells = slots[SLOT_CELLS];
  unsigned m = 0;
  for (size_t c = (size_t)blockIdx.x * VT + threadIdx.x; c < cells; c += (size_t)gridDim.x * VT) m = max(m, starts[c + 1] - starts[c]);
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(slots + SLOT_LONGEST, m);
}

// ---- the query -----------------------------------------------------------------------------------------------------------------------------
// a point source clamped to the mesh's box: the cell of such a point lies in the grid, so k_vox_keys can key queries that lie anywhere.
// The keys only order the walk
template <class P>
struct ClampedPoints {
  P in;
  float lo[3], hi[3];
  __device__ __forceinline__ float4 at(unsigned i) const {
    float4 a = in.at(i);
    if (finite3(a.x, a.y, a.z)) {
      a.x = fminf(fmaxf(a.x, lo[0]), hi[0]);
      a.y = fminf(fmaxf(a.y, lo[1]), hi[1]);
      a.z = fminf(fmaxf(a.z, lo[2]), hi[2]);
    }
    return a;
  }
};

__device__ __forceinline__ double dot3(const double x[3], const double y[3]) {
  RGBID_FP_STRICT
  return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2];
}

// step 4 of the header: the closest point r of triangle a b c to p -> the region
__device__ __forceinline__ int closest_point(const double p[3], const double a[3], const double b[3], const double c[3], double r[3]) {
  RGBID_FP_STRICT
  double ab[3], ac[3], ap[3], bp[3], cp[3];
  for (int k = 0; k < 3; ++k) {
    ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k];
    ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k];
  }
  const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
  if (d1 <= 0.0 && d2 <= 0.0) { for (int k = 0; k < 3; ++k) r[k] = a[k]; return 0; }
  const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
  if (d3 >= 0.0 && d4 <= d3) { for (int k = 0; k < 3; ++k) r[k] = b[k]; return 1; }
  const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
  if (d6 >= 0.0 && d5 <= d6) { for (int k = 0; k < 3; ++k) r[k] = c[k]; return 2; }
  const double vc = d1 * d4 - d3 * d2;
  if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) {
    const double v = d1 / (d1 - d3);
    for (int k = 0; k < 3; ++k) r[k] = a[k] + v * ab[k];
    return 3;
  }
  const double vb = d5 * d2 - d1 * d6;
  if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) {
    const double w = d2 / (d2 - d6);
    for (int k = 0; k < 3; ++k) r[k] = a[k] + w * ac[k];
    return 4;
  }
  const double va = d3 * d6 - d5 * d4;
  const double s = d4 - d3, u = d5 - d6;
  if (va <= 0.0 && s >= 0.0 && u >= 0.0) {
    const double w = s / (s + u);
    for (int k = 0; k < 3; ++k) r[k] = b[k] + w * (c[k] - b[k]);
    return 5;
  }
  const double den = 1.0 / ((va + vb) + vc);
  const double v = vb * den, w = vc * den;
  for (int k = 0; k < 3; ++k) r[k] = (a[k] + v * ab[k]) + w * ac[k];
  return 6;
}

// One thread per query, in the order `order` gives (null: input order).  cells = 0: no triangle takes part, every query is without a
// winner.
template <typename K, class P>
__global__ __launch_bounds__(VT) void k_meshdist_query(P pts, unsigned n, const unsigned* __restrict__ order, MdGrid og, unsigned cells,
                                                       const K* __restrict__ ukeys, const unsigned* __restrict__ starts,
                                                       const unsigned* __restrict__ ptri, const float4* __restrict__ rec, double dmax, double dmax2,
                                                       unsigned* __restrict__ tri_out, float* __restrict__ dist_out, float* __restrict__ closest_out,
                                                       unsigned char* __restrict__ region_out, unsigned* __restrict__ cand_out) {
  RGBID_FP_STRICT
  const unsigned i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  const unsigned id = order ? order[i] : i;
  if (id >= n) return;
  const float4 q4 = pts.at(id);
  const double q[3] = {(double)q4.x, (double)q4.y, (double)q4.z};
  double best = INFINITY, br[3] = {0.0, 0.0, 0.0};
  unsigned best_t = NONE, cand = 0;
  int best_region = RGBID_MESHDIST_NO_REGION;
  // the query's cell relative to the grid, as floats: integers, exact within one cell of the grid and beyond it only compared
  const float rx = floorf(q4.x * og.g.inv[0]) - og.g.minb[0], ry = floorf(q4.y * og.g.inv[1]) - og.g.minb[1],
              rz = floorf(q4.z * og.g.inv[2]) - og.g.minb[2];
  const bool walk = cells != 0 && finite3(q4.x, q4.y, q4.z) && rx >= -1.f && rx <= (float)og.d[0] && ry >= -1.f && ry <= (float)og.d[1] &&
                    rz >= -1.f && rz <= (float)og.d[2];
  if (walk) {
    const int ci = (int)rx, cj = (int)ry, ck = (int)rz;
    const unsigned long long x0 = (unsigned long long)(ci > 0 ? ci - 1 : 0);                 // a key of i - 1 at i = 0 belongs to another row
    const unsigned long long x1 = (unsigned long long)(ci + 1 < og.d[0] ? ci + 1 : og.d[0] - 1);
    for (int row = 0; row < 9; ++row) {
      const int j = cj + row % 3 - 1, k = ck + row / 3 - 1;
      if (j < 0 || j >= og.d[1] || k < 0 || k >= og.d[2]) continue;
      const unsigned long long base = (unsigned long long)j * og.g.d0 + (unsigned long long)k * og.g.d01;
      const K klo = (K)(base + x0), khi = (K)(base + x1);
      const unsigned a = lower_run(ukeys, cells, klo);
      unsigned b = a;
      while (b < cells && b < a + 3 && ukeys[b] <= khi) ++b;      // at most the three x-adjacent cells of the row
      if (b == a) continue;
      const unsigned m0 = starts[a], m1 = starts[b];
      cand += m1 - m0;
      for (unsigned m = m0; m < m1; ++m) {
        const unsigned t = ptri[m];
        const Corners c = corners_of(rec, t);
        float lo[3], hi[3];
        c.box(lo, hi);
        bool pass = true;
        for (int ax = 0; ax < 3; ++ax) {
          const double cl = fmin(fmax(q[ax], (double)lo[ax]), (double)hi[ax]);
          pass = pass && fabs(q[ax] - cl) <= dmax;
        }
        if (!pass) continue;
        const double A[3] = {(double)c.a.x, (double)c.a.y, (double)c.a.z}, B[3] = {(double)c.b.x, (double)c.b.y, (double)c.b.z},
                     C[3] = {(double)c.c.x, (double)c.c.y, (double)c.c.z};
        double r[3];
        const int region = closest_point(q, A, B, C, r);
        const double ex = q[0] - r[0], ey = q[1] - r[1], ez = q[2] - r[2];
        const double d2 = (ex * ex + ey * ey) + ez * ez;
        if (d2 <= dmax2 && (d2 < best || (d2 == best && t < best_t))) {   // a NaN fails the first comparison
          best = d2; best_t = t; best_region = region;
          br[0] = r[0]; br[1] = r[1]; br[2] = r[2];
        }
      }
    }
  }
  const bool won = best_t != NONE;
  if (tri_out) tri_out[id] = best_t;
  if (dist_out) dist_out[id] = won ? (float)sqrt(best) : __uint_as_float(NAN_BITS);
  if (closest_out)
    for (int k = 0; k < 3; ++k) closest_out[3 * (size_t)id + k] = won ? (float)br[k] : __uint_as_float(NAN_BITS);
  if (region_out) region_out[id] = (unsigned char)best_region;
  if (cand_out) cand_out[id] = cand;
}

}  // namespace

struct rgbid_meshdist {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0, cap_p = 0, cap_q = 0;
  SortWorkspace wp;                        // the pairs' sort: afterwards the runs (idx), the occupied cells' keys and their starts; its box
                                           // partials and its slots serve the whole plan
  SortWorkspace wt;                        // the triangles' tile offsets (compaction part only); it shares wp's slots
  SortWorkspace wq;                        // the queries' sort
  float4* rec = nullptr;                   // [cap_t][3] the corners
  unsigned long long* tile64 = nullptr;    // [tiles of cap_t]
  // the last plan
  bool planned = false, sort_queries = true;
  unsigned cells = 0;                      // 0: no triangle takes part
  MdGrid og = {};
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  double dmax = 0.0;
  const void* ukeys = nullptr;
  const unsigned* starts = nullptr;
  const unsigned* ptri = nullptr;
  // stage timing: box [0, 1], pairs [2, 3] + [4, 5], sort [5, 6], cells [6, 7], query [8, 9]
  bool timed[5] = {false, false, false, false, false};
  Buffers buf;
  StageTimer<10> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

// offsets, pairs, sort, cell table and the longest run for keys of type K
template <typename K>
int pair_stage(rgbid_meshdist* h, unsigned n_t, unsigned n_pairs) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->wp;
  const unsigned tiles = (n_t + RUN_TILE - 1) / RUN_TILE;
  h->mark(4);
  hipLaunchKernelGGL(k_vox_scan1, dim3(1), dim3(VT), 0, s, h->wt.bc, tiles, w.slots, (int)SLOT_OFFSETS, (unsigned*)nullptr, 0u);
  hipLaunchKernelGGL(k_md_pairs<K>, dim3(tiles), dim3(VT), 0, s, h->rec, n_t, h->og, h->wt.bc, n_pairs, w.keys_as<K>(0), w.idx[0]);
  h->mark(5);
  const SortedPairs<K> sp = w.sort<K>(s, n_pairs, h->og.g);
  h->mark(6);
  const RunSrc<K> rs{sp.keys, n_pairs, sp.starts, sp.scratch};
  w.count_scan(s, rs, n_pairs, SLOT_CELLS, sp.starts, n_pairs);
  w.write(s, rs, n_pairs);
  hipLaunchKernelGGL(k_md_longest, dim3(grid_of(((unsigned long long)n_pairs + VT - 1) / VT)), dim3(VT), 0, s, sp.starts, w.slots);
  h->mark(7);
  h->ukeys = sp.scratch;
  h->starts = sp.starts;
  h->ptri = sp.idx;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

template <typename K, class P>
int query_stage(rgbid_meshdist* h, const P& pts, unsigned n, unsigned* tri_out, float* dist_out, float* closest_out, unsigned char* region_out,
                unsigned* cand_out) {
  hipStream_t s = h->ctx->stream;
  const unsigned* order = nullptr;
  if (h->cells && h->sort_queries) {
    ClampedPoints<P> cp{pts, {h->lo[0], h->lo[1], h->lo[2]}, {h->hi[0], h->hi[1], h->hi[2]}};
    h->wq.make_keys<K>(s, cp, n, h->og.g);
    order = h->wq.sort<K>(s, n, h->og.g).idx;
  }
  hipLaunchKernelGGL((k_meshdist_query<K, P>), dim3((n + VT - 1) / VT), dim3(VT), 0, s, pts, n, order, h->og, h->cells, (const K*)h->ukeys, h->starts,
                     h->ptri, h->rec, h->dmax, h->dmax * h->dmax, tri_out, dist_out, closest_out, region_out, cand_out);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

template <class P>
int query_call(rgbid_meshdist* h, const P& pts, unsigned long long n, uint32_t* tri_out, float* dist_out, float* closest_out, uint8_t* region_out,
               uint32_t* cand_out) {
  if (!aligned4(tri_out) || !aligned4(dist_out) || !aligned4(closest_out) || !aligned4(cand_out)) return RGBID_E_INVALID;
  if (n == 0 || !(tri_out || dist_out || closest_out || region_out || cand_out)) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  h->timed[4] = false;
  h->mark(8);
  const unsigned nu = (unsigned)n;
  int r;
  if (h->cells == 0) r = query_stage<unsigned>(h, pts, nu, tri_out, dist_out, closest_out, region_out, cand_out);
  else r = with_key_type(h->og.g, [&](auto k) { return query_stage<decltype(k)>(h, pts, nu, tri_out, dist_out, closest_out, region_out, cand_out); });
  if (r) return r;
  h->mark(9);
  h->timed[4] = h->timer.on;
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_meshdist_create(rgbid_meshdist** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles,
                          unsigned long long max_pairs, unsigned long long max_queries) {
  if (out) *out = nullptr;
  if (max_pairs < 1 || max_pairs > RGBID_MESHDIST_MAX_PAIRS || max_queries < 1 || max_queries > RGBID_MESHDIST_MAX_QUERIES) return RGBID_E_INVALID;
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_MESHDIST_MAX_VERTICES, RGBID_MESHDIST_MAX_TRIANGLES, [&](rgbid_meshdist* h) {
    h->cap_p = max_pairs;
    h->cap_q = max_queries;
    int r = h->wp.alloc(h->buf, max_pairs);
    if (!r) r = h->wt.alloc_compaction(h->buf, max_triangles);
    if (!r) r = h->wq.alloc(h->buf, max_queries);
    if (!r) r = h->buf.alloc(&h->rec, sizeof(float4) * 3 * (size_t)max_triangles);
    if (!r) r = h->buf.alloc(&h->tile64, sizeof(unsigned long long) * (size_t)h->wt.run_tiles);
    h->wt.slots = h->wp.slots;         // one slot area, one read-back
    h->wt.slots_host = h->wp.slots_host;
    return r;
  });
}

int rgbid_meshdist_destroy(rgbid_meshdist* h) { return destroy_handle(h); }   // a query may still read the tables

int rgbid_meshdist_plan(rgbid_meshdist* h, unsigned long long n_vertices, const float* vertices_dev, unsigned long long n_triangles,
                        const uint32_t* triangles_dev, float d_max, float cell, long long grid[6], unsigned long long stats[4]) {
  RGBID_FP_STRICT
  if (!h) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  if (n_vertices && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  if (!(std::isfinite(d_max) && d_max >= RGBID_MESHDIST_MIN_DISTANCE && d_max <= RGBID_MESHDIST_MAX_DISTANCE)) return RGBID_E_INVALID;
  const float least = d_max * RGBID_MESHDIST_CELL_FACTOR;
  if (!(std::isfinite(cell) && cell >= 0.f && cell <= RGBID_MESHDIST_MAX_DISTANCE * RGBID_MESHDIST_CELL_FACTOR)) return RGBID_E_INVALID;
  if (cell != 0.f && cell < least) return RGBID_E_INVALID;
  if (grid) for (int i = 0; i < 6; ++i) grid[i] = 0;
  if (stats) for (int i = 0; i < 4; ++i) stats[i] = 0;
  h->planned = false;
  h->cells = 0;
  h->og = MdGrid{};
  h->dmax = (double)d_max;
  for (int k = 0; k < 4; ++k) h->timed[k] = false;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  if (n_t == 0) { h->planned = true; return RGBID_OK; }   // no triangle: every query is without a winner
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->wp;
  const unsigned gt = grid_of(((unsigned long long)n_t + VT - 1) / VT);
  h->mark(0);
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, s));
  check_triangles(s, triangles_dev, n_t, n_v, w.slots + SLOT_BAD);
  hipLaunchKernelGGL(k_md_gather, dim3(gt), dim3(VT), 0, s, vertices_dev, triangles_dev, n_v, n_t, h->rec);
  w.box(s, TriBox<false>{h->rec}, n_t);
  RGBID_HIP(hipMemcpyAsync(w.slots + SLOT_LO, w.slots + SLOT_BOX, 3 * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
  w.box(s, TriBox<true>{h->rec}, n_t);
  h->mark(1);
  unsigned part;
  float lo_of_hi[3], hi[3], lo[3];
  if (int r = w.read_box(s, part, lo_of_hi, hi)) return r;
  if (w.slots_host[SLOT_BAD]) return RGBID_E_INVALID;      // a triangle names a vertex that does not exist
  memcpy(lo, w.slots_host + SLOT_LO, sizeof lo);
  if (stats) stats[0] = part;
  if (part == 0) { h->planned = true; return RGBID_OK; }
  const float c = cell != 0.f ? cell : least;
  const float leaf[3] = {c, c, c};
  long long gr[6];
  if (int r = form_grid(lo, hi, leaf, h->og.g, gr)) return r;
  for (int a = 0; a < 3; ++a) {   // the bound of the 3 x 3 x 3 walk: |floorf(p * inv)| <= 2^18 at both ends of the box
    if (gr[a] < -(long long)RGBID_MESHDIST_MAX_CELL || gr[a] + gr[3 + a] - 1 > (long long)RGBID_MESHDIST_MAX_CELL) return RGBID_E_INVALID;
    h->og.d[a] = (int)gr[3 + a];
    h->lo[a] = lo[a];
    h->hi[a] = hi[a];
  }
  const unsigned tiles = (n_t + RUN_TILE - 1) / RUN_TILE;
  h->mark(2);
  hipLaunchKernelGGL(k_md_count, dim3(tiles), dim3(VT), 0, s, h->rec, n_t, h->og.g, h->tile64, h->wt.bc);
  hipLaunchKernelGGL(k_md_total, dim3(1), dim3(64), 0, s, h->tile64, tiles, w.slots);
  h->mark(3);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  const unsigned long long pairs = (unsigned long long)w.slots_host[SLOT_PAIRS] | ((unsigned long long)w.slots_host[SLOT_PAIRS + 1] << 32);
  if (stats) stats[1] = pairs;
  if (pairs > h->cap_p) return RGBID_E_INVALID;            // the needed count is reported
  if (int r = with_key_type(h->og.g, [&](auto k) { return pair_stage<decltype(k)>(h, n_t, (unsigned)pairs); })) return r;
  if (int r = w.read_slots(s)) return r;
  h->cells = w.slots_host[SLOT_CELLS];
  if (grid) memcpy(grid, gr, sizeof gr);
  if (stats) { stats[2] = h->cells; stats[3] = w.slots_host[SLOT_LONGEST]; }
  for (int k = 0; k < 4; ++k) h->timed[k] = h->timer.on;
  h->planned = true;
  return RGBID_OK;
}

int rgbid_meshdist_query(rgbid_meshdist* h, unsigned long long n, const float* points_dev, uint32_t* triangle_out, float* distance_out,
                         float* closest_out, uint8_t* region_out, uint32_t* candidates_out) {
  if (!h || !h->planned || n > h->cap_q) return RGBID_E_INVALID;
  if (n && (!points_dev || !aligned4(points_dev))) return RGBID_E_INVALID;
  return query_call(h, VertexPoints{points_dev}, n, triangle_out, distance_out, closest_out, region_out, candidates_out);
}

int rgbid_meshdist_query_records(rgbid_meshdist* h, unsigned long long n, const rgbid_cloud_point* records_dev, uint32_t* triangle_out,
                                 float* distance_out, float* closest_out, uint8_t* region_out, uint32_t* candidates_out) {
  if (!h || !h->planned || !records_in_ok(records_dev, n, h->cap_q)) return RGBID_E_INVALID;
  return query_call(h, RecordPoints{reinterpret_cast<const float4*>(records_dev)}, n, triangle_out, distance_out, closest_out, region_out,
                    candidates_out);
}

int rgbid_meshdist_set_query_sort(rgbid_meshdist* h, int enable) {
  if (!h) return RGBID_E_INVALID;
  h->sort_queries = enable != 0;
  return RGBID_OK;
}

int rgbid_meshdist_timing(rgbid_meshdist* h, int enable, float ms[5]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  static const int pairs[5][4] = {{0, 1}, {2, 3, 4, 5}, {5, 6}, {6, 7}, {8, 9}};   // the pairs stage: the count and, after the read-back, the rest
  if (ms)
    if (int r = stage_times(h->timer, h->timed, pairs, ms)) return r;
  return h->timer.enable(enable != 0);
}

}  // extern "C"
