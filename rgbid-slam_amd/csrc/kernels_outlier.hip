// kernels_outlier.hip -- radius outlier filter over keyframe point clouds (include/rgbid_outlier.h).
//
// The judge is the brute-force definition of the header (d2 <= r2 in float32 over every pair); the grid only finds the candidates:
//   plan  k_vox_box / k_vox_box_final   box and count of the finite points -> host: the grid with cell = r * 1.0625f, refused when
//                                       |floorf(p * inv)| > 2^18 anywhere (the 3 x 3 x 3 walk is proved inside that bound only)
//         k_vox_keys + radix sort       (cell key, index) pairs, stable, non-finite records last (voxel_device.h)
//         k_outlier_gather              sorted copy of the positions as float4 (x, y, z, bits of the input index)
//         cell table                    flag compaction of the heads key[i] != key[i - 1]: unique keys and run starts
//         k_outlier_count               one thread per point in sorted order: 9 rows of 3 x-adjacent cells, each one binary search on
//                                       the unique keys and one contiguous walk; centre row first; leaves at cap; count and keep flag
//                                       go to the point's input position
//         keep                          flag count + scan of the keep flags -> kept
//   emit  flag write                    kept records, input order, 2 x 16 B stores each
// Keys are 32-bit when the largest key + 1 < 2^32, 64-bit otherwise.
#include "../../include/rgbid_outlier.h"
#include "common.h"
#include "hip_host.h"
#include "voxel_device.h"   // box, grid, keys, radix sort, flag compaction; the sort workspace

#include <cmath>
#include <cstring>
#include <new>

using namespace rgbid;

static_assert(sizeof(rgbid_cloud_point) == 32, "rgbid_cloud_point is two 16-byte stores");

namespace {

enum { SLOT_CELLS = SLOT_RUNS, SLOT_KEPT = SLOT_VOXELS };

struct OutGrid {
  VoxGrid g;
  int d[3];       // cells per axis (each <= 2^19 + 1)
  float r2;       // r * r in float32
};

__device__ __forceinline__ int cell_axis(float p, float inv, float minb) {
  RGBID_FP_STRICT
  return (int)(floorf(p * inv) - minb);
}

// sorted copy of the finite points: spos[i] = (x, y, z, bits of the input index) of the i-th record in key order
__global__ __launch_bounds__(VT) void k_outlier_gather(const float4* __restrict__ in, const unsigned* __restrict__ sidx, unsigned finite,
                                                       float4* __restrict__ spos) {
  const unsigned i = blockIdx.x * VT + threadIdx.x;
  if (i >= finite) return;
  const unsigned id = sidx[i];
  const float4 a = in[2 * (size_t)id];
  spos[i] = make_float4(a.x, a.y, a.z, __uint_as_float(id));
}

// cell table: head i -> (start, key) of cell `rank`
template <typename K>
struct CellSrc {
  const K* keys;
  unsigned finite;
  unsigned* starts;
  K* ukeys;
  __device__ __forceinline__ unsigned size() const { return finite; }
  __device__ __forceinline__ bool flag(unsigned i) const { return i == 0 || keys[i] != keys[i - 1]; }
  __device__ __forceinline__ void write(unsigned pos, unsigned i) const { starts[pos] = i; ukeys[pos] = keys[i]; }
};

// first cell whose key is >= k, in [0, cells]
template <typename K>
__device__ __forceinline__ unsigned lower_cell(const K* __restrict__ ukeys, unsigned cells, K k) {
  unsigned lo = 0, hi = cells;
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    if (ukeys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One thread per record in sorted order (a wave's lanes share cells, so their look-ups and walks read the same lines).  Records past
// `finite` are the non-finite ones: count 0, never kept.
template <typename K>
__global__ __launch_bounds__(VT) void k_outlier_count(const float4* __restrict__ spos, const unsigned* __restrict__ sidx, unsigned n, unsigned finite,
                                                      OutGrid og, const K* __restrict__ ukeys, const unsigned* __restrict__ starts,
                                                      const unsigned* __restrict__ slots, unsigned cap, unsigned min_neighbours,
                                                      unsigned* __restrict__ counts, unsigned char* __restrict__ keep) {
  RGBID_FP_STRICT
  const unsigned i = blockIdx.x * VT + threadIdx.x;
  if (i >= n) return;
  if (i >= finite) {
    const unsigned id = sidx[i];
    counts[id] = 0;
    keep[id] = 0;
    return;
  }
  const unsigned cells = slots[SLOT_CELLS];
  const float4 p = spos[i];
  const int ci = cell_axis(p.x, og.g.inv[0], og.g.minb[0]);
  const int cj = cell_axis(p.y, og.g.inv[1], og.g.minb[1]);
  const int ck = cell_axis(p.z, og.g.inv[2], og.g.minb[2]);
  const unsigned long long x0 = (unsigned long long)(ci > 0 ? ci - 1 : 0);                 // a key of i - 1 at i = 0 belongs to another row
  const unsigned long long x1 = (unsigned long long)(ci + 1 < og.d[0] ? ci + 1 : og.d[0] - 1);
  unsigned c = 0;
  // rows in the order centre, then by distance: (dj, dk) packed two bits each, value + 1
  constexpr unsigned ROWS[9] = {0x5, 0x4, 0x6, 0x1, 0x9, 0x0, 0x2, 0x8, 0xa};
  for (int row = 0; row < 9 && c < cap; ++row) {
    const int j = cj + (int)(ROWS[row] & 3u) - 1, k = ck + (int)(ROWS[row] >> 2) - 1;
    if (j < 0 || j >= og.d[1] || k < 0 || k >= og.d[2]) continue;
    const unsigned long long base = (unsigned long long)j * og.g.d0 + (unsigned long long)k * og.g.d01;
    const K klo = (K)(base + x0), khi = (K)(base + x1);
    const unsigned a = lower_cell(ukeys, cells, klo);
    unsigned b = a;
    while (b < cells && b < a + 3 && ukeys[b] <= khi) ++b;      // at most the three x-adjacent cells of the row
    if (b == a) continue;
    const unsigned m1 = starts[b];
    for (unsigned m = starts[a]; m < m1; ++m) {
      const float4 q = spos[m];
      const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
      const float d2 = (dx * dx + dy * dy) + dz * dz;
      if (d2 <= og.r2 && m != i) {
        if (++c >= cap) break;
      }
    }
  }
  const unsigned id = __float_as_uint(p.w);
  counts[id] = c;
  keep[id] = c >= min_neighbours ? 1 : 0;
}

// stable compaction of the kept records
struct KeepRec {
  const unsigned char* keep;
  unsigned n;
  const uint4* in;
  uint4* out;
  __device__ __forceinline__ unsigned size() const { return n; }
  __device__ __forceinline__ bool flag(unsigned i) const { return keep[i] != 0; }
  __device__ __forceinline__ void write(unsigned pos, unsigned i) const {
    const uint4 a = in[2 * (size_t)i], b = in[2 * (size_t)i + 1];
    out[2 * (size_t)pos] = a;
    out[2 * (size_t)pos + 1] = b;
  }
};

}  // namespace

struct rgbid_outlier {
  rgbid_ctx* ctx = nullptr;
  SortWorkspace ws;                            // after the sort the free index buffer holds the cell starts, the free key buffer the unique keys;
                                               // its bc holds the keep compaction's tile offsets from the plan until the emit
  float4* spos = nullptr;                      // [cap] sorted positions
  unsigned* counts = nullptr;                  // [cap] input order
  unsigned char* keep = nullptr;               // [cap] input order
  // the last plan
  const rgbid_cloud_point* in = nullptr;
  unsigned long long n = 0, kept = 0;
  bool counted = false;                        // false: no finite point, every count is 0
  // stage timing (rgbid_outlier_timing): box [0, 1], keys + sort [2, 3], cells [3, 4], count [4, 5], keep count + scan [5, 6], emit [7, 8]
  bool plan_timed = false, emit_timed = false;
  Buffers buf;
  StageTimer<9> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

template <typename K>
int sort_and_count(rgbid_outlier* o, const float4* in, unsigned n, unsigned finite, const OutGrid& og, unsigned cap, unsigned min_neighbours) {
  hipStream_t s = o->ctx->stream;
  SortWorkspace& w = o->ws;
  o->mark(2);
  w.make_keys<K>(s, RecordPoints{in}, n, og.g);
  const SortedPairs<K> sp = w.sort<K>(s, n, og.g);
  o->mark(3);
  hipLaunchKernelGGL(k_outlier_gather, dim3((finite + VT - 1) / VT), dim3(VT), 0, s, in, sp.idx, finite, o->spos);
  const CellSrc<K> cs{sp.keys, finite, sp.starts, sp.scratch};
  w.count_scan(s, cs, finite, SLOT_CELLS, sp.starts, finite);
  w.write(s, cs, finite);
  o->mark(4);
  hipLaunchKernelGGL(k_outlier_count<K>, dim3((n + VT - 1) / VT), dim3(VT), 0, s, o->spos, sp.idx, n, finite, og, sp.scratch, sp.starts, w.slots, cap,
                     min_neighbours, o->counts, o->keep);
  o->mark(5);
  w.count_scan(s, KeepRec{o->keep, n, nullptr, nullptr}, n, SLOT_KEPT);   // the emit writes with these offsets
  o->mark(6);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_outlier_create(rgbid_outlier** out, rgbid_ctx* ctx, unsigned long long max_points) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_points == 0 || max_points > RGBID_OUTLIER_MAX_POINTS) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_outlier* o = new (std::nothrow) rgbid_outlier;
  if (!o) return RGBID_E_NOMEM;
  o->ctx = ctx;
  const size_t cap = (size_t)max_points;
  int r = o->ws.alloc(o->buf, max_points);
  if (!r) r = o->buf.alloc(&o->spos, sizeof(float4) * cap);
  if (!r) r = o->buf.alloc(&o->counts, sizeof(unsigned) * cap);
  if (!r) r = o->buf.alloc(&o->keep, cap);
  if (r) { rgbid_outlier_destroy(o); return r; }
  *out = o;
  return RGBID_OK;
}

int rgbid_outlier_destroy(rgbid_outlier* o) { return destroy_handle(o); }   // an emit may still read the tables

int rgbid_outlier_plan(rgbid_outlier* o, const rgbid_cloud_point* in_dev, unsigned long long n, float radius, unsigned cap,
                       unsigned min_neighbours, unsigned long long stats[3], unsigned long long* kept) {
  RGBID_FP_STRICT
  if (!o || !kept || !records_in_ok(in_dev, n, o->ws.cap)) return RGBID_E_INVALID;
  if (!(std::isfinite(radius) && radius >= RGBID_OUTLIER_MIN_RADIUS && radius <= RGBID_OUTLIER_MAX_RADIUS)) return RGBID_E_INVALID;
  if (cap == 0 || min_neighbours > cap) return RGBID_E_INVALID;
  o->kept = 0; o->n = 0; o->in = nullptr; o->counted = false;
  *kept = 0;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (n == 0) return RGBID_OK;
  (void)hipSetDevice(o->ctx->device);
  hipStream_t s = o->ctx->stream;
  RGBID_HIP(hipStreamSynchronize(s));   // the previous emit has read the tables
  const float4* in = reinterpret_cast<const float4*>(in_dev);
  const unsigned nu = (unsigned)n;
  o->plan_timed = false; o->emit_timed = false;
  o->mark(0);
  o->ws.box(s, RecordPoints{in}, nu);
  o->mark(1);
  unsigned finite;
  float lo[3], hi[3];
  if (int r = o->ws.read_box(s, finite, lo, hi)) return r;
  if (stats) stats[0] = finite;
  if (finite == 0) { o->n = n; return RGBID_OK; }   // every count is 0, nothing is kept
  const float cell = radius * RGBID_OUTLIER_CELL_FACTOR;
  const float leaf[3] = {cell, cell, cell};
  OutGrid og;
  long long gr[6];
  if (int r = form_grid(lo, hi, leaf, og.g, gr)) return r;
  for (int a = 0; a < 3; ++a) {   // the bound of the 3 x 3 x 3 walk: |floorf(p * inv)| <= 2^18 at both ends of the box
    if (gr[a] < -(long long)RGBID_OUTLIER_MAX_CELL || gr[a] + gr[3 + a] - 1 > (long long)RGBID_OUTLIER_MAX_CELL) return RGBID_E_INVALID;
    og.d[a] = (int)gr[3 + a];
  }
  og.r2 = radius * radius;
  if (int r = with_key_type(og.g, [&](auto k) { return sort_and_count<decltype(k)>(o, in, nu, finite, og, cap, min_neighbours); })) return r;
  if (int r = o->ws.read_slots(s)) return r;
  const unsigned k = o->ws.slots_host[SLOT_KEPT];
  if (stats) { stats[1] = o->ws.slots_host[SLOT_CELLS]; stats[2] = k; }
  *kept = k;
  o->kept = k; o->n = n; o->in = in_dev; o->counted = true;
  o->plan_timed = o->timer.on;
  return RGBID_OK;
}

int rgbid_outlier_counts(rgbid_outlier* o, uint32_t* counts_dev) {
  if (!o) return RGBID_E_INVALID;
  if (o->n == 0) return RGBID_OK;
  if (!counts_dev) return RGBID_E_INVALID;
  (void)hipSetDevice(o->ctx->device);
  if (o->counted) RGBID_HIP(hipMemcpyAsync(counts_dev, o->counts, sizeof(unsigned) * (size_t)o->n, hipMemcpyDeviceToDevice, o->ctx->stream));
  else RGBID_HIP(hipMemsetAsync(counts_dev, 0, sizeof(unsigned) * (size_t)o->n, o->ctx->stream));
  return RGBID_OK;
}

int rgbid_outlier_emit(rgbid_outlier* o, rgbid_cloud_point* out_dev, unsigned long long capacity) {
  if (!o) return RGBID_E_INVALID;
  if (o->kept == 0) return RGBID_OK;
  if (!records_out_ok(out_dev, capacity, o->kept)) return RGBID_E_INVALID;
  (void)hipSetDevice(o->ctx->device);
  const unsigned nu = (unsigned)o->n;
  o->mark(7);
  o->ws.write(o->ctx->stream, KeepRec{o->keep, nu, reinterpret_cast<const uint4*>(o->in), reinterpret_cast<uint4*>(out_dev)}, nu);
  o->mark(8);
  RGBID_HIP(hipGetLastError());
  o->emit_timed = o->timer.on;
  return RGBID_OK;
}

int rgbid_outlier_timing(rgbid_outlier* o, int enable, float ms[5]) {
  if (!o) return RGBID_E_INVALID;
  (void)hipSetDevice(o->ctx->device);
  if (ms) {
    static const int pair[5][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}, {5, 6}};
    for (int k = 0; k < 5; ++k) {
      ms[k] = 0.f;
      if (o->plan_timed) RGBID_HIP(o->timer.elapsed(pair[k][0], pair[k][1], &ms[k]));
    }
    if (o->emit_timed) {
      float w = 0.f;
      RGBID_HIP(o->timer.elapsed(7, 8, &w));
      ms[4] += w;
    }
  }
  return o->timer.enable(enable != 0);
}

}  // extern "C"
