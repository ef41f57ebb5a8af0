// kernels_smooth.hip -- an indexed triangle mesh in device memory smoothed by Taubin's lambda | mu filter over the umbrella neighbourhood
// of its vertices, and area-weighted vertex normals from its triangles (include/rgbid_smooth.h).
//
// The judge is tests/smooth_mirror.py; counts, CSR, boundary bytes, positions and normals are byte-identical to it.
//   plan  k_mesh_check<true> mesh_device.h: counts the triangles with an index >= n_v and the corner pairs with equal ends into two slots,
//                            copied to the host: a bad index ends the call here, the other count gives the number M of pairs that stay
//         sort_rounds        voxel_device.h: k_vox_round_keys over PairKey, one (key, item) pair per ordered corner pair 6 t + c (a pair
//                            with equal ends gets the sentinel n_v), and the stable LSD radix sort, two rounds: by u, then by v with the
//                            keys recomputed in the order the first round left.  Equal (v, u) are adjacent, the dropped pairs last
//         k_smooth_ends      the u of the sorted items beside their v
//         flag compaction    over the heads (v, u)[m] != (v, u)[m - 1]: heads[rank] = m, heads[P] = M
//         k_smooth_rows      neighbours[r] = u, incidences[r] = heads[r + 1] - heads[r]
//         k_mesh_offsets<true>  mesh_device.h: offsets[w] = the rows of the vertices below w: a bounded binary search per vertex
//         k_smooth_rowstats  one thread per vertex over its own row: the boundary byte, the counts (integer atomics, one per wave)
//         corner table       mesh_device.h's k_mesh_corner_keys, one stable sort of (vertex, corner) by bitlen(n_v) bits, k_mesh_offsets<false>,
//                            a copy
//   run   k_smooth_pass      one thread per vertex: gathers its row's positions, sums in order in double
//   normals k_smooth_normals one thread per vertex: gathers its corners' triangles, sums the area vectors in order in double
// No float atomics, no wait on another thread, every loop has its bound when it starts.
#include "../../include/rgbid_smooth.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // the index check, the corner table, tri_load, area_vector, the argument test, the create; voxel_device.h's
                            // sort_rounds, flag compaction and ordered gather; the sort workspace

#include <cmath>
#include <cstring>

using namespace rgbid;

namespace {

// beside the workspace's own 0 .. 8; SLOT_RUNS holds P
enum { SLOT_BAD = 9, SLOT_DROPPED = 10, SLOT_BPAIRS = 11, SLOT_BVERTS = 12, SLOT_DEG0 = 13, SLOT_MAXDEG = 14, SLOT_NONMANIFOLD = 15 };
static_assert(SLOT_VOXELS < SLOT_BAD && SLOT_NONMANIFOLD < SLOTS, "the slots of this file lie behind the workspace's");

// ---- adjacency --------------------------------------------------------------------------------------------------------------------
// the mesh as the pair kernels see it: item 6 t + c is the c-th of (i0,i1) (i1,i0) (i1,i2) (i2,i1) (i2,i0) (i0,i2)
struct PairView {
  const unsigned* tri;
  unsigned n_t, n_v;
  unsigned long long items;          // 6 n_t
  // -> whether the item is a pair that stays; an item or an index that names nothing reads nothing
  __device__ __forceinline__ bool ends(unsigned item, unsigned& v, unsigned& u) const {
    if (item >= items) return false;
    const unsigned t = item / 6u, c = item - 6u * t;
    const unsigned from = ((c + 1u) >> 1) % 3u, to = (c & 1u) ? (c >> 1) : ((c >> 1) + 1u) % 3u;
    v = tri[3 * (size_t)t + from];
    u = tri[3 * (size_t)t + to];
    return v < n_v && u < n_v && v != u;
  }
};

// sort_rounds' key of round r (0: u, 1: v) for an item; the sentinel n_v for a pair that is dropped
struct PairKey {
  PairView view;
  __device__ __forceinline__ unsigned long long size() const { return view.items; }
  __device__ __forceinline__ unsigned operator()(unsigned item, int r) const {
    unsigned v, u;
    const bool ok = view.ends(item, v, u);
    return ok ? (r ? v : u) : view.n_v;
  }
};

// after the two rounds: the u of the first n_pairs sorted items
__global__ __launch_bounds__(VT) void k_smooth_ends(PairView view, const unsigned* __restrict__ order, unsigned n_pairs, unsigned* __restrict__ us) {
  for (size_t m = (size_t)blockIdx.x * VT + threadIdx.x; m < n_pairs; m += (size_t)gridDim.x * VT) {
    unsigned v, u;
    us[m] = view.ends(order[m], v, u) ? u : view.n_v;
  }
}

// HeadSrc over two keys: item m < n_pairs is a head iff (v, u)[m] != (v, u)[m - 1] -> heads[rank] = m
struct PairHeadSrc {
  const unsigned* vs;
  const unsigned* us;
  unsigned n_pairs;
  unsigned* heads;
  __device__ __forceinline__ unsigned size() const { return n_pairs; }
  __device__ __forceinline__ bool flag(unsigned m) const { return m == 0 || vs[m] != vs[m - 1] || us[m] != us[m - 1]; }
  __device__ __forceinline__ void write(unsigned pos, unsigned m) const { heads[pos] = m; }
};

// row r < P (the device slot): its neighbour and the length of its run of equal pairs
__global__ __launch_bounds__(VT) void k_smooth_rows(const unsigned* __restrict__ us, const unsigned* __restrict__ heads, const unsigned* __restrict__ n_rows,
                                                    unsigned* __restrict__ nbr, unsigned* __restrict__ inc) {
  const unsigned p = *n_rows;
  for (size_t r = (size_t)blockIdx.x * VT + threadIdx.x; r < p; r += (size_t)gridDim.x * VT) {
    const unsigned m = heads[r];
    nbr[r] = us[m];
    inc[r] = heads[r + 1] - m;
  }
}

// one thread per vertex over its own row: the boundary byte and what the row adds to the counts
__global__ __launch_bounds__(VT) void k_smooth_rowstats(const unsigned* __restrict__ offsets, const unsigned* __restrict__ inc, unsigned n_v,
                                                        unsigned char* __restrict__ boundary, unsigned* __restrict__ slots) {
  const size_t v = (size_t)blockIdx.x * VT + threadIdx.x;
  unsigned bpairs = 0, nonmanifold = 0, deg = 0, deg0 = 0;
  if (v < n_v) {
    const unsigned b = offsets[v], e = offsets[v + 1];
    deg = e - b;
    deg0 = deg == 0;
    for (unsigned j = b; j < e; ++j) {
      const unsigned i = inc[j];
      bpairs += i == 1;
      nonmanifold += i >= 3;
    }
    boundary[v] = bpairs != 0;
  }
  unsigned bverts = bpairs != 0;
  bpairs = wave_sum(bpairs);
  bverts = wave_sum(bverts);
  nonmanifold = wave_sum(nonmanifold);
  deg0 = wave_sum(deg0);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) deg = max(deg, (unsigned)__shfl_xor(deg, o, 64));
  if ((threadIdx.x & 63) == 0) {     // five counts behind one branch: four wave_add_to would make four
    if (bpairs) atomicAdd(slots + SLOT_BPAIRS, bpairs);
    if (bverts) atomicAdd(slots + SLOT_BVERTS, bverts);
    if (nonmanifold) atomicAdd(slots + SLOT_NONMANIFOLD, nonmanifold);
    if (deg0) atomicAdd(slots + SLOT_DEG0, deg0);
    if (deg) atomicMax(slots + SLOT_MAXDEG, deg);
  }
}

// ---- the pass -----------------------------------------------------------------------------------------------------------------------
struct Pos {
  float p[3];
};

// the position of vertex id; an index that names no vertex reads nothing and counts as not finite
__device__ __forceinline__ Pos pos_load(const float* __restrict__ in, unsigned id, unsigned n_v) {
  Pos q = {{NAN, NAN, NAN}};
  if (id < n_v) {
    const size_t o = 3 * (size_t)id;
    q.p[0] = in[o]; q.p[1] = in[o + 1]; q.p[2] = in[o + 2];
  }
  return q;
}

struct PosSum {
  double s[3] = {0, 0, 0};
  unsigned k = 0;                    // the finite neighbours
};

// one neighbour, in order; the pragma keeps every add a separate rounding
__device__ __forceinline__ void pos_add(PosSum& sum, const Pos& q) {
  RGBID_FP_STRICT
  if (finite3(q.p[0], q.p[1], q.p[2])) {
    for (int a = 0; a < 3; ++a) sum.s[a] += (double)q.p[a];
    ++sum.k;
  }
}

__global__ __launch_bounds__(VT) void k_smooth_pass(const float* __restrict__ in, float* __restrict__ out, const unsigned* __restrict__ offsets,
                                                    const unsigned* __restrict__ nbr, const unsigned char* __restrict__ pinned, unsigned n_v, double f) {
  RGBID_FP_STRICT
  const size_t v = (size_t)blockIdx.x * VT + threadIdx.x;
  if (v >= n_v) return;
  const size_t o = 3 * v;
  const unsigned* words = reinterpret_cast<const unsigned*>(in);
  const unsigned w[3] = {words[o], words[o + 1], words[o + 2]};
  const float x[3] = {__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
  PosSum sum;
  if (finite3(x[0], x[1], x[2]) && !(pinned && pinned[v]))
    gather_in_order(nbr, offsets[v], offsets[v + 1], sum, [&](unsigned id) { return pos_load(in, id, n_v); }, pos_add);
  unsigned* wout = reinterpret_cast<unsigned*>(out);
  if (sum.k) {
    const double dk = (double)sum.k;
    for (int a = 0; a < 3; ++a) {
      const double xa = (double)x[a];
      const double mean = sum.s[a] / dk;
      const double d = mean - xa;
      const double step = f * d;
      out[o + a] = (float)(xa + step);
    }
  } else {
    for (int a = 0; a < 3; ++a) wout[o + a] = w[a];   // the words: a NaN keeps its payload
  }
}

// ---- normals ------------------------------------------------------------------------------------------------------------------------
// one measurable triangle's area vector, in order
__device__ __forceinline__ void tri_add(double s[3], const TriPos& q) {
  RGBID_FP_STRICT
  if (!q.ok) return;
  double n[3];
  area_vector(q, n);
  s[0] += n[0]; s[1] += n[1]; s[2] += n[2];
}

__global__ __launch_bounds__(VT) void k_smooth_normals(const float* __restrict__ pos, const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v,
                                                       const unsigned* __restrict__ corner_offsets, const unsigned* __restrict__ corners,
                                                       float* __restrict__ out) {
  RGBID_FP_STRICT
  const size_t v = (size_t)blockIdx.x * VT + threadIdx.x;
  if (v >= n_v) return;
  double s[3] = {0, 0, 0};
  gather_in_order(corners, corner_offsets[v], corner_offsets[v + 1], s, [&](unsigned c) { return tri_load(pos, tri, c / 3u, n_t, n_v); }, tri_add);
  float n[3];
  unit_of(s, n);
  for (int a = 0; a < 3; ++a) out[3 * v + a] = n[a];
}

}  // namespace

struct rgbid_smooth {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0;
  SortWorkspace w;                   // 6 cap_t items: the pair sort, then the corner sort
  unsigned* offsets = nullptr;       // [cap_v + 1]
  unsigned* nbr = nullptr;           // [6 cap_t]
  unsigned* inc = nullptr;           // [6 cap_t]
  unsigned char* boundary = nullptr; // [cap_v]
  unsigned* corner_offsets = nullptr;// [cap_v + 1]
  unsigned* corners = nullptr;       // [3 cap_t]
  float* spare = nullptr;            // [cap_v][3] the third position buffer of the ping-pong
  // the last plan
  bool planned = false, has_corners = false;
  unsigned n_v = 0, n_t = 0, n_rows = 0;
  const unsigned* tri = nullptr;
  // stage timing: check [0, 1], the rest of the plan [2, 3], run [4, 5], normals [6, 7]
  bool timed[3] = {false, false, false};
  Buffers buf;
  StageTimer<8> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

// the CSR of step 2 from the n_pairs corner pairs that stay
int adjacency_stage(rgbid_smooth* h, unsigned n_pairs) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  const unsigned n_v = h->n_v;
  const unsigned* vs = nullptr;
  const unsigned* us = nullptr;
  const unsigned* heads = nullptr;
  if (n_pairs) {
    const PairView view{h->tri, h->n_t, n_v, 6ull * h->n_t};
    const int p = w.sort_rounds(s, PairKey{view}, n_v, (unsigned)view.items, {0, 1});   // by u, then by v
    unsigned* u_out = w.keys_as<unsigned>(p ^ 1);
    hipLaunchKernelGGL(k_smooth_ends, dim3(grid_of(((unsigned long long)n_pairs + VT - 1) / VT)), dim3(VT), 0, s, view, w.idx[p], n_pairs, u_out);
    vs = w.keys_as<unsigned>(p);
    us = u_out;
    const PairHeadSrc src{vs, us, n_pairs, w.idx[p ^ 1]};
    w.count_scan(s, src, n_pairs, SLOT_RUNS, w.idx[p ^ 1], n_pairs);
    w.write(s, src, n_pairs);
    heads = w.idx[p ^ 1];
    hipLaunchKernelGGL(k_smooth_rows, dim3(grid_of(((unsigned long long)n_pairs + VT - 1) / VT)), dim3(VT), 0, s, us, heads, w.slots + SLOT_RUNS, h->nbr,
                       h->inc);
  }
  // without a pair the slot holds 0 and nothing is read through the null tables
  hipLaunchKernelGGL(k_mesh_offsets<true>, dim3(grid_of(((unsigned long long)n_v + 1 + VT - 1) / VT)), dim3(VT), 0, s, vs, heads, w.slots + SLOT_RUNS, 0u, n_v,
                     h->offsets);
  hipLaunchKernelGGL(k_smooth_rowstats, dim3((n_v + VT - 1) / VT), dim3(VT), 0, s, h->offsets, h->inc, n_v, h->boundary, w.slots);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

// step 3: the corners of every vertex, ascending
int corner_stage(rgbid_smooth* h) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  const unsigned n_v = h->n_v;
  const unsigned long long corners = 3ull * h->n_t;
  const unsigned* keys = nullptr;
  if (corners) {
    // <unsigned> is no choice: the kernel is a template only so that a file that does not launch it does not compile it
    hipLaunchKernelGGL(k_mesh_corner_keys<unsigned>, dim3(grid_of((corners + VT - 1) / VT)), dim3(VT), 0, s, h->tri, corners, n_v, w.keys_as<unsigned>(0), w.idx[0]);
    const int p = w.sort_bits<unsigned>(s, (unsigned)corners, bitlen(n_v), 0);
    keys = w.keys_as<unsigned>(p);
    RGBID_HIP(hipMemcpyAsync(h->corners, w.idx[p], sizeof(unsigned) * (size_t)corners, hipMemcpyDeviceToDevice, s));
  }
  hipLaunchKernelGGL(k_mesh_offsets<false>, dim3(grid_of(((unsigned long long)n_v + 1 + VT - 1) / VT)), dim3(VT), 0, s, keys, (const unsigned*)nullptr,
                     (const unsigned*)nullptr, (unsigned)corners, n_v, h->corner_offsets);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_smooth_create(rgbid_smooth** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles) {
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_SMOOTH_MAX_VERTICES, RGBID_SMOOTH_MAX_TRIANGLES, [&](rgbid_smooth* h) {
    const size_t cv = (size_t)max_vertices, ct = (size_t)max_triangles;
    int r = h->w.alloc(h->buf, 6ull * max_triangles);
    if (!r) r = h->buf.alloc(&h->offsets, sizeof(unsigned) * (cv + 1));
    if (!r) r = h->buf.alloc(&h->nbr, sizeof(unsigned) * 6 * ct);
    if (!r) r = h->buf.alloc(&h->inc, sizeof(unsigned) * 6 * ct);
    if (!r) r = h->buf.alloc(&h->boundary, cv);
    if (!r) r = h->buf.alloc(&h->corner_offsets, sizeof(unsigned) * (cv + 1));
    if (!r) r = h->buf.alloc(&h->corners, sizeof(unsigned) * 3 * ct);
    if (!r) r = h->buf.alloc(&h->spare, sizeof(float) * 3 * cv);
    return r;
  });
}

int rgbid_smooth_destroy(rgbid_smooth* h) { return destroy_handle(h); }   // a pass may still read the tables

int rgbid_smooth_plan(rgbid_smooth* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev, uint32_t flags,
                      unsigned long long counts[8]) {
  if (!h || (flags & ~RGBID_SMOOTH_PLAN_NORMALS)) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  if (counts) for (int i = 0; i < 8; ++i) counts[i] = 0;
  h->planned = h->has_corners = false;
  h->timed[0] = false;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  h->n_v = n_v; h->n_t = n_t; h->n_rows = 0;
  h->tri = triangles_dev;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  if (n_v == 0) {                                          // no vertex, no triangle: two tables of one zero
    RGBID_HIP(hipMemsetAsync(h->offsets, 0, sizeof(unsigned), s));
    RGBID_HIP(hipMemsetAsync(h->corner_offsets, 0, sizeof(unsigned), s));
    h->has_corners = (flags & RGBID_SMOOTH_PLAN_NORMALS) != 0;
    h->planned = true;
    return RGBID_OK;
  }
  h->mark(0);
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, s));
  if (n_t) check_triangles<true>(s, triangles_dev, n_t, n_v, w.slots + SLOT_BAD, w.slots + SLOT_DROPPED);
  h->mark(1);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  if (w.slots_host[SLOT_BAD]) return RGBID_E_INVALID;      // a triangle names a vertex that does not exist
  const unsigned long long dropped = w.slots_host[SLOT_DROPPED];
  const unsigned n_pairs = (unsigned)(6ull * n_t - dropped);
  h->mark(2);
  if (int r = adjacency_stage(h, n_pairs)) return r;
  if (flags & RGBID_SMOOTH_PLAN_NORMALS)
    if (int r = corner_stage(h)) return r;
  h->mark(3);
  if (int r = w.read_slots(s)) return r;
  h->timed[0] = h->timer.on;
  h->n_rows = w.slots_host[SLOT_RUNS];
  if (counts) {
    counts[0] = h->n_rows;
    counts[1] = h->n_rows / 2;
    counts[2] = w.slots_host[SLOT_BPAIRS];
    counts[3] = w.slots_host[SLOT_BVERTS];
    counts[4] = w.slots_host[SLOT_DEG0];
    counts[5] = w.slots_host[SLOT_MAXDEG];
    counts[6] = dropped;
    counts[7] = w.slots_host[SLOT_NONMANIFOLD];
  }
  h->has_corners = (flags & RGBID_SMOOTH_PLAN_NORMALS) != 0;
  h->planned = true;
  return RGBID_OK;
}

int rgbid_smooth_adjacency(rgbid_smooth* h, uint32_t* offsets_out, uint32_t* neighbours_out, uint32_t* incidences_out, uint8_t* boundary_out,
                           unsigned long long pair_capacity) {
  if (!h || !h->planned || pair_capacity < h->n_rows) return RGBID_E_INVALID;
  if (!aligned4(offsets_out) || !aligned4(neighbours_out) || !aligned4(incidences_out)) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const size_t rows = sizeof(unsigned) * (size_t)h->n_rows;
  if (offsets_out) RGBID_HIP(hipMemcpyAsync(offsets_out, h->offsets, sizeof(unsigned) * ((size_t)h->n_v + 1), hipMemcpyDeviceToDevice, s));
  if (neighbours_out && rows) RGBID_HIP(hipMemcpyAsync(neighbours_out, h->nbr, rows, hipMemcpyDeviceToDevice, s));
  if (incidences_out && rows) RGBID_HIP(hipMemcpyAsync(incidences_out, h->inc, rows, hipMemcpyDeviceToDevice, s));
  if (boundary_out && h->n_v) RGBID_HIP(hipMemcpyAsync(boundary_out, h->boundary, (size_t)h->n_v, hipMemcpyDeviceToDevice, s));
  return RGBID_OK;
}

int rgbid_smooth_run(rgbid_smooth* h, const float* vertices_in, float* vertices_out, unsigned iterations, double lambda, double mu, uint32_t flags) {
  if (!h || !h->planned || (flags & ~RGBID_SMOOTH_PIN_BOUNDARY)) return RGBID_E_INVALID;
  if (iterations > RGBID_SMOOTH_MAX_ITERATIONS) return RGBID_E_INVALID;
  if (!(std::isfinite(lambda) && lambda > 0.0 && lambda <= 1.0) || !(std::isfinite(mu) && mu >= -2.0 && mu <= 0.0)) return RGBID_E_INVALID;
  const size_t bytes = sizeof(float) * 3 * (size_t)h->n_v;
  if (h->n_v) {
    if (!vertices_in || !vertices_out || !aligned4(vertices_in) || !aligned4(vertices_out)) return RGBID_E_INVALID;
    const uintptr_t a = (uintptr_t)vertices_in, b = (uintptr_t)vertices_out;
    if (a < b + bytes && b < a + bytes) return RGBID_E_INVALID;   // the passes are Jacobi: never in place
  }
  h->timed[1] = false;
  if (h->n_v == 0) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  h->mark(4);
  const unsigned passes = iterations * (mu != 0.0 ? 2u : 1u);
  if (passes == 0) RGBID_HIP(hipMemcpyAsync(vertices_out, vertices_in, bytes, hipMemcpyDeviceToDevice, s));
  const unsigned char* pinned = (flags & RGBID_SMOOTH_PIN_BOUNDARY) ? h->boundary : nullptr;
  const float* src = vertices_in;
  for (unsigned i = 0; i < passes; ++i) {
    float* dst = ((passes - 1 - i) & 1u) ? h->spare : vertices_out;   // the last pass writes vertices_out
    const double f = (mu != 0.0 && (i & 1u)) ? mu : lambda;
    hipLaunchKernelGGL(k_smooth_pass, dim3((h->n_v + VT - 1) / VT), dim3(VT), 0, s, src, dst, h->offsets, h->nbr, pinned, h->n_v, f);
    src = dst;
  }
  h->mark(5);
  RGBID_HIP(hipGetLastError());
  h->timed[1] = h->timer.on;
  return RGBID_OK;
}

int rgbid_smooth_normals(rgbid_smooth* h, const float* vertices_dev, float* normals_out) {
  if (!h || !h->planned || !h->has_corners) return RGBID_E_INVALID;
  if (h->n_v && (!vertices_dev || !normals_out || !aligned4(vertices_dev) || !aligned4(normals_out))) return RGBID_E_INVALID;
  h->timed[2] = false;
  if (h->n_v == 0) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  h->mark(6);
  hipLaunchKernelGGL(k_smooth_normals, dim3((h->n_v + VT - 1) / VT), dim3(VT), 0, s, vertices_dev, h->tri, h->n_t, h->n_v, h->corner_offsets, h->corners,
                     normals_out);
  h->mark(7);
  RGBID_HIP(hipGetLastError());
  h->timed[2] = h->timer.on;
  return RGBID_OK;
}

int rgbid_smooth_timing(rgbid_smooth* h, int enable, float ms[3]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  static const int pairs[3][4] = {{0, 1, 2, 3}, {4, 5}, {6, 7}};   // the plan: the check and the rest
  if (ms)
    if (int r = stage_times(h->timer, h->timed, pairs, ms)) return r;
  return h->timer.enable(enable != 0);
}

}  // extern "C"
