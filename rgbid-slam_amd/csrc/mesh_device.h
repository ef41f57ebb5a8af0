// mesh_device.h -- what the operators over an indexed triangle mesh share and the point-cloud filters do not (kernels_mesh.hip,
// kernels_simplify.hip, kernels_smooth.hip, kernels_raster.hip, kernels_meshdist.hip, kernels_meshreg.hip, kernels_texture.hip,
// kernels_holes.hip, kernels_denoise.hip, kernels_refine.hip).  Device half: the check of the triangles' indices; the corners of a mesh as
// directed edges, their sort key and their larger ends (holes, refine); the (vertex, corner) keys and the row offsets of a table sorted by
// vertex (smooth, denoise); the loads of a vertex in double and of a triangle's three positions, and the area vector.  Host half: the test
// every call makes of its mesh arguments, the prologue of a create, the overlap test of an emit and the blocks of a launch.  What they share
// with the filters is voxel_device.h's (point sources, sort_rounds, gather_in_order, unit_of, the flag compaction, the value scan),
// wave_device.h's (wave_add_to) and hip_host.h's (aligned4, stage_times).
// Everything has internal linkage, and every kernel is a template: an including file compiles its own copy of the kernels it launches and
// of no other.
#pragma once
#include "voxel_device.h"

#include <new>

namespace rgbid {
namespace {

// counts the triangles with an index >= n_v into *bad; with PAIRS also the ordered corner pairs with equal ends (two per equal pair of
// corners) into *dropped.  One atomic per wave and count
template <bool PAIRS>
__global__ __launch_bounds__(VT) void k_mesh_check(const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v, unsigned* __restrict__ bad,
                                                   unsigned* __restrict__ dropped) {
  unsigned n_bad = 0, n_dropped = 0;
  for (size_t t = (size_t)blockIdx.x * VT + threadIdx.x; t < n_t; t += (size_t)gridDim.x * VT) {
    const unsigned a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    if (!(a < n_v && b < n_v && c < n_v)) ++n_bad;
    if (PAIRS) n_dropped += 2u * ((a == b) + (b == c) + (c == a));
  }
  wave_add_to(bad, n_bad);
  if (PAIRS) wave_add_to(dropped, n_dropped);
}

// n_t > 0 triangles checked on stream s
template <bool PAIRS = false>
void check_triangles(hipStream_t s, const unsigned* tri, unsigned n_t, unsigned n_v, unsigned* bad, unsigned* dropped = nullptr) {
  hipLaunchKernelGGL(k_mesh_check<PAIRS>, dim3(grid_of(((unsigned long long)n_t + VT - 1) / VT)), dim3(VT), 0, s, tri, n_t, n_v, bad, dropped);
}

// ---- corners as edges ----------------------------------------------------------------------------------------------------------------
// the mesh as the corner kernels see it: item 3 t + c is the directed edge from corner c to corner c + 1 of triangle t
struct CornerView {
  const unsigned* tri;
  unsigned n_t, n_v;
  unsigned long long items;          // 3 n_t
  // -> whether the item is a directed edge; an item or an index that names nothing reads nothing
  __device__ __forceinline__ bool ends(unsigned item, unsigned& from, unsigned& to) const {
    if (item >= items) return false;
    const unsigned t = item / 3u, c = item - 3u * t;
    const unsigned i0 = tri[3 * (size_t)t], i1 = tri[3 * (size_t)t + 1], i2 = tri[3 * (size_t)t + 2];
    from = c == 0 ? i0 : c == 1 ? i1 : i2;
    to = c == 0 ? i1 : c == 1 ? i2 : i0;
    return i0 < n_v && i1 < n_v && i2 < n_v && i0 != i1 && i1 != i2 && i2 != i0;
  }
};

// sort_rounds' key of round r (0: the larger end, 1: the smaller) for a corner; the sentinel n_v for a corner that gives no edge
struct CornerKey {
  CornerView view;
  __device__ __forceinline__ unsigned long long size() const { return view.items; }
  __device__ __forceinline__ unsigned operator()(unsigned item, int r) const {
    unsigned a, b;
    const bool ok = view.ends(item, a, b);
    return ok ? (r ? min(a, b) : max(a, b)) : view.n_v;
  }
};

// after the two rounds: the larger end of every sorted corner; with COUNT the corners that give an edge are counted into *directed
template <bool COUNT>
__global__ __launch_bounds__(VT) void k_mesh_corner_ends(CornerView view, const unsigned* __restrict__ order, unsigned* __restrict__ his,
                                                         unsigned* __restrict__ directed) {
  unsigned c = 0;
  for (size_t m = (size_t)blockIdx.x * VT + threadIdx.x; m < view.items; m += (size_t)gridDim.x * VT) {
    unsigned a, b;
    const bool ok = view.ends(order[m], a, b);
    his[m] = ok ? max(a, b) : view.n_v;
    if (COUNT) c += ok;
  }
  if (COUNT) wave_add_to(directed, c);
}

// ---- corners by vertex ----------------------------------------------------------------------------------------------------------------
// one (vertex, corner) pair per corner for one stable sort_bits by bitlen(n_v) bits.  One round, so not sort_rounds': k_vox_round_keys'
// test of the order and its round argument would make this stream half as long again.  I is always unsigned: the parameter is there
// only because a kernel that is no template would be compiled into every file that includes this header
template <typename I>
__global__ __launch_bounds__(VT) void k_mesh_corner_keys(const I* __restrict__ tri, unsigned long long corners, unsigned n_v,
                                                         unsigned* __restrict__ keys, unsigned* __restrict__ idx) {
  for (size_t i = (size_t)blockIdx.x * VT + threadIdx.x; i < corners; i += (size_t)gridDim.x * VT) {
    const unsigned v = tri[i];
    keys[i] = v < n_v ? v : n_v;
    idx[i] = (unsigned)i;
  }
}

// offsets[w], w = 0 .. n_v: how many of the ascending keys are below w; nothing is read without a key.  Without HEADS the key of entry r
// is keys[r] and the entries are `count`; with HEADS it is keys[heads[r]] and the entries are *n_slot.  32 halvings at most
template <bool HEADS>
__global__ __launch_bounds__(VT) void k_mesh_offsets(const unsigned* __restrict__ keys, const unsigned* __restrict__ heads, const unsigned* __restrict__ n_slot,
                                                     unsigned count, unsigned n_v, unsigned* __restrict__ offsets) {
  const unsigned n = HEADS ? *n_slot : count;
  for (size_t w = (size_t)blockIdx.x * VT + threadIdx.x; w <= n_v; w += (size_t)gridDim.x * VT) {
    unsigned lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      const unsigned k = keys[HEADS ? heads[mid] : mid];
      if (k < w) lo = mid + 1; else hi = mid;
    }
    offsets[w] = lo;
  }
}

// ---- positions ------------------------------------------------------------------------------------------------------------------------
struct P3 {
  double p[3];
  bool finite;
};

// the position of vertex id in double; an index that names no vertex reads nothing and is not finite
__device__ __forceinline__ P3 p3_load(const float* __restrict__ pos, unsigned id, unsigned n_v) {
  P3 q = {{NAN, NAN, NAN}, false};
  if (id < n_v) {
    const size_t o = 3 * (size_t)id;
    const float x = pos[o], y = pos[o + 1], z = pos[o + 2];
    q.p[0] = (double)x; q.p[1] = (double)y; q.p[2] = (double)z;
    q.finite = finite3(x, y, z);
  }
  return q;
}

struct TriPos {
  float p[3][3];
  bool ok;                            // the triangle and its indices exist and the three positions are finite
};

// the three positions of triangle t; a triangle or an index that names nothing reads nothing
__device__ __forceinline__ TriPos tri_load(const float* __restrict__ pos, const unsigned* __restrict__ tri, unsigned t, unsigned n_t, unsigned n_v) {
  TriPos q;
  q.ok = false;
  for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) q.p[k][a] = 0.f;
  if (t >= n_t) return q;
  const unsigned i[3] = {tri[3 * (size_t)t], tri[3 * (size_t)t + 1], tri[3 * (size_t)t + 2]};
  if (!(i[0] < n_v && i[1] < n_v && i[2] < n_v)) return q;
  for (int k = 0; k < 3; ++k)
    for (int a = 0; a < 3; ++a) q.p[k][a] = pos[3 * (size_t)i[k] + a];
  q.ok = finite3(q.p[0][0], q.p[0][1], q.p[0][2]) && finite3(q.p[1][0], q.p[1][1], q.p[1][2]) && finite3(q.p[2][0], q.p[2][1], q.p[2][2]);
  return q;
}

// c = u x w: every component two products and one difference, each a separate rounding
__device__ __forceinline__ void cross3(const double u[3], const double w[3], double c[3]) {
  RGBID_FP_STRICT
  c[0] = (u[1] * w[2]) - (u[2] * w[1]);
  c[1] = (u[2] * w[0]) - (u[0] * w[2]);
  c[2] = (u[0] * w[1]) - (u[1] * w[0]);
}

// the area vector (p1 - p0) x (p2 - p0) of a measurable triangle, in double
__device__ __forceinline__ void area_vector(const TriPos& q, double n[3]) {
  RGBID_FP_STRICT
  double e1[3], e2[3];
  for (int a = 0; a < 3; ++a) {
    e1[a] = (double)q.p[1][a] - (double)q.p[0][a];
    e2[a] = (double)q.p[2][a] - (double)q.p[0][a];
  }
  cross3(e1, e2, n);
}

// ---- host side --------------------------------------------------------------------------------------------------------------------------
unsigned blocks_of(unsigned long long items) { return (unsigned)((items + VT - 1) / VT); }

// whether the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte; a null or empty range shares none
bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// what every call checks about the mesh it is given: the counts against the handle's capacities, triangles that are there and 4-byte
// aligned, and none of them without a vertex
bool mesh_in_ok(unsigned long long n_v, unsigned long long n_t, const void* tri, unsigned long long cap_v, unsigned long long cap_t) {
  return n_v <= cap_v && n_t <= cap_t && (n_t == 0 || (tri && aligned4(tri) && n_v != 0));
}

// The create of a mesh operator's handle H (ctx, cap_v, cap_t, its Buffers and StageTimer): the capacities lie in 1 .. the header's limits,
// alloc(h) makes the operator's own allocations; a failed one destroys the handle
template <class H, class A>
int mesh_create(H** out, rgbid_ctx* ctx, unsigned long long max_v, unsigned long long max_t, unsigned long long limit_v, unsigned long long limit_t,
                A&& alloc) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_v < 1 || max_v > limit_v || max_t < 1 || max_t > limit_t) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  H* h = new (std::nothrow) H;
  if (!h) return RGBID_E_NOMEM;
  h->ctx = ctx;
  h->cap_v = max_v;
  h->cap_t = max_t;
  if (int r = alloc(h)) { destroy_handle(h); return r; }
  *out = h;
  return RGBID_OK;
}

}  // namespace
}  // namespace rgbid
