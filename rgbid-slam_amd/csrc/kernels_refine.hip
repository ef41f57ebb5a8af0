// kernels_refine.hip -- one round of the conforming edge split of an indexed triangle mesh in device memory: the edges above a length get
// a vertex at their midpoint, every triangle is cut by the pattern of its split edges (include/rgbid_refine.h).
//
// The judge is tests/refine_mirror.py; the nine counts and the emitted mesh are byte-identical to it.
//   plan   k_mesh_check<false> mesh_device.h: counts the triangles with an index >= n_v, copied to the host: a bad index ends the call here
//          sort_rounds         voxel_device.h: one (key, item) pair per corner 3 t + c, keyed by the ends of its edge (a triangle with a
//                              repeated index gets the sentinel n_v), two stable rounds: by the larger end, then by the smaller.  Equal
//                              undirected edges are adjacent and in ascending (lo, hi) order, the sentinels last
//          k_mesh_corner_ends  mesh_device.h: the larger end of the sorted corners beside their smaller end
//          value scan          over the run heads: item m of run e writes corner_edge[corner] = e, the head the ends of e, a member of a
//                              selected triangle the eligibility flag (every writer writes the same byte)
//          k_refine_mark       one thread per edge, two position gathers: the mark beside the flag; counts the eligible edges
//          flag compaction     over the marks: rank[e], and the ends of the marked edges by rank
//          k_refine_k          one thread per triangle: k(t) from its corners' ranks; counts k = 1, 2, 3 and the degenerate triangles
//          value scan          over k: base(t), E
//   emit   k_refine_vertices   one thread per marked edge: position, colour, normal of vertex n_v + r
//          k_refine_triangles  one thread per triangle: one to four rows and selection bytes; for k = 2 the midpoints in registers
//          the input's vertex rows are copied as words
// No float atomics, no wait on another thread, every loop has its bound when it starts.
#include "../../include/rgbid_refine.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // the index check, the corners as edges, p3_load, the argument and overlap tests, the create;
                            // voxel_device.h's sort_rounds, flag compaction, value scan and unit_of; the sort workspace

#include <cmath>
#include <cstring>

using namespace rgbid;

namespace {

// the plan's slots: this file forms no box, so the workspace's own slots 0 .. 6 stay zero; SLOT_RUNS holds n_e, SLOT_VOXELS M
enum { SLOT_BAD = 9, SLOT_ELIGIBLE = 10, SLOT_K1 = 11, SLOT_K2 = 12, SLOT_K3 = 13, SLOT_DEGENERATE = 14, SLOT_NEW = 15 };
static_assert(SLOT_VOXELS < SLOT_BAD && SLOT_NEW < SLOTS, "the slots of this file lie behind the workspace's");

constexpr unsigned NONE = 0xFFFFFFFFu;
constexpr unsigned char ELIGIBLE = 1, MARKED = 2;

// ---- the edge table ---------------------------------------------------------------------------------------------------------------------
// sorted corner m: 1 for the first of its edge's run.  The sum before it, plus its own value, less one is its edge: the edges are ranked
// in the order of the sort.  Every member tells its corner the edge; the head writes the ends; a member of a selected triangle the flag
struct EdgeSrc {
  const unsigned* los;
  const unsigned* his;
  const unsigned* order;
  const unsigned char* selection;    // null: every triangle is selected
  unsigned n, n_v;                   // n = 3 n_t items
  unsigned* corner_edge;             // [n]
  unsigned* edge_lo;                 // [n]
  unsigned* edge_hi;                 // [n]
  unsigned char* flags;              // [n], zeroed
  __device__ __forceinline__ unsigned size() const { return n; }
  __device__ __forceinline__ unsigned value(unsigned m) const {
    const unsigned lo = los[m];
    if (lo >= n_v) return 0u;
    return m == 0 || los[m - 1] != lo || his[m - 1] != his[m];
  }
  __device__ __forceinline__ void write(unsigned m, unsigned before, unsigned head) const {
    const unsigned lo = los[m], corner = order[m];
    if (lo >= n_v || corner >= n || before + head == 0) return;
    const unsigned e = before + head - 1u;
    if (e >= n) return;
    corner_edge[corner] = e;
    if (head) { edge_lo[e] = lo; edge_hi[e] = his[m]; }
    if (!selection || selection[corner / 3u]) flags[e] = ELIGIBLE;
  }
};

// ---- the marks --------------------------------------------------------------------------------------------------------------------------
// step 3's q between two positions in double
__device__ __forceinline__ double q_of(const double a[3], const double b[3]) {
  RGBID_FP_STRICT
  const double d0 = b[0] - a[0], d1 = b[1] - a[1], d2 = b[2] - a[2];
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// step 4's midpoint, one component
__device__ __forceinline__ float mid_of(double lo, double hi) {
  RGBID_FP_STRICT
  return (float)((lo + hi) / 2.0);
}

// one thread per edge e < *n_e: the mark beside the flag, NONE for the rank (the compaction overwrites the marked edges')
__global__ __launch_bounds__(VT) void k_refine_mark(const float* __restrict__ pos, const unsigned* __restrict__ edge_lo, const unsigned* __restrict__ edge_hi,
                                                    const unsigned* __restrict__ n_e, unsigned cap_e, unsigned n_v, double l2,
                                                    unsigned char* __restrict__ flags, unsigned* __restrict__ edge_rank, unsigned* __restrict__ eligible) {
  const unsigned n = min(*n_e, cap_e);
  unsigned c = 0;
  for (size_t e = (size_t)blockIdx.x * VT + threadIdx.x; e < n; e += (size_t)gridDim.x * VT) {
    unsigned char f = flags[e] & ELIGIBLE;
    if (f) {
      ++c;
      const P3 a = p3_load(pos, edge_lo[e], n_v), b = p3_load(pos, edge_hi[e], n_v);
      if (a.finite && b.finite && q_of(a.p, b.p) > l2) f |= MARKED;
    }
    flags[e] = f;
    edge_rank[e] = NONE;
  }
  wave_add_to(eligible, c);
}

// the marked edges: rank[e], and their ends by rank
struct MarkedSrc {
  const unsigned char* flags;
  const unsigned* edge_lo;
  const unsigned* edge_hi;
  const unsigned* n_e;               // device slot
  unsigned cap_e;
  unsigned* edge_rank;
  unsigned* mlo;                     // [cap_e]
  unsigned* mhi;
  __device__ __forceinline__ unsigned size() const { return min(*n_e, cap_e); }
  __device__ __forceinline__ bool flag(unsigned e) const { return (flags[e] & MARKED) != 0; }
  __device__ __forceinline__ void write(unsigned pos, unsigned e) const {
    if (pos >= cap_e) return;
    edge_rank[e] = pos;
    mlo[pos] = edge_lo[e];
    mhi[pos] = edge_hi[e];
  }
};

// ---- the triangles' patterns ------------------------------------------------------------------------------------------------------------
// what the triangle kernels know of the plan
struct Pattern {
  const unsigned* tri;
  const unsigned* corner_edge;       // [3 n_t], written for the corners that name an edge only
  const unsigned* edge_rank;         // [cap_e]
  unsigned n_t, n_v, cap_e;
  // the corners of triangle t < n_t and the ranks of its three edges (NONE: not marked) -> k(t); a degenerate triangle has no edge
  __device__ __forceinline__ unsigned load(unsigned t, unsigned v[3], unsigned r[3], bool& degenerate) const {
    const size_t o = 3 * (size_t)t;
    v[0] = tri[o]; v[1] = tri[o + 1]; v[2] = tri[o + 2];
    r[0] = r[1] = r[2] = NONE;
    const bool in = v[0] < n_v && v[1] < n_v && v[2] < n_v;
    degenerate = in && (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]);
    if (!in || degenerate) return 0u;
    unsigned k = 0;
    for (int c = 0; c < 3; ++c) {
      const unsigned e = corner_edge[o + c];
      if (e < cap_e) r[c] = edge_rank[e];
      k += r[c] != NONE;
    }
    return k;
  }
};

__global__ __launch_bounds__(VT) void k_refine_k(Pattern pt, unsigned char* __restrict__ kk, unsigned* __restrict__ slots) {
  unsigned k1 = 0, k2 = 0, k3 = 0, deg = 0;
  for (size_t t = (size_t)blockIdx.x * VT + threadIdx.x; t < pt.n_t; t += (size_t)gridDim.x * VT) {
    unsigned v[3], r[3];
    bool degenerate;
    const unsigned k = pt.load((unsigned)t, v, r, degenerate);
    kk[t] = (unsigned char)k;
    k1 += k == 1; k2 += k == 2; k3 += k == 3; deg += degenerate;
  }
  wave_add_to(slots + SLOT_K1, k1);
  wave_add_to(slots + SLOT_K2, k2);
  wave_add_to(slots + SLOT_K3, k3);
  wave_add_to(slots + SLOT_DEGENERATE, deg);
}

struct BaseSrc {
  const unsigned char* kk;
  unsigned n_t;
  unsigned* base;
  __device__ __forceinline__ unsigned size() const { return n_t; }
  __device__ __forceinline__ unsigned value(unsigned t) const { return kk[t]; }
  __device__ __forceinline__ void write(unsigned t, unsigned before, unsigned) const { base[t] = before; }
};

// ---- emit -------------------------------------------------------------------------------------------------------------------------------
// one thread per marked edge r < n_m: vertex n_v + r
__global__ __launch_bounds__(VT) void k_refine_vertices(const unsigned* __restrict__ mlo, const unsigned* __restrict__ mhi, unsigned n_m, unsigned n_v,
                                                        const float* __restrict__ pos_in, const unsigned char* __restrict__ col_in,
                                                        const float* __restrict__ nrm_in, float* __restrict__ pos_out,
                                                        unsigned char* __restrict__ col_out, float* __restrict__ nrm_out) {
  RGBID_FP_STRICT
  const size_t r = (size_t)blockIdx.x * VT + threadIdx.x;
  if (r >= n_m) return;
  const unsigned lo = mlo[r], hi = mhi[r];
  if (lo >= n_v || hi >= n_v) return;
  const size_t o = 3 * ((size_t)n_v + r), a = 3 * (size_t)lo, b = 3 * (size_t)hi;
  for (int c = 0; c < 3; ++c) pos_out[o + c] = mid_of((double)pos_in[a + c], (double)pos_in[b + c]);
  if (col_out)
    for (int c = 0; c < 3; ++c) {
      col_out[o + c] = (unsigned char)(((unsigned)col_in[a + c] + (unsigned)col_in[b + c] + 1u) >> 1);
    }
  if (nrm_out) {
    double s[3];
    for (int c = 0; c < 3; ++c) s[c] = (double)nrm_in[a + c] + (double)nrm_in[b + c];
    float n[3];
    unit_of(s, n);
    for (int c = 0; c < 3; ++c) nrm_out[o + c] = n[c];
  }
}

__device__ __forceinline__ void put_row(unsigned* __restrict__ tri_out, unsigned char* __restrict__ sel_out, size_t row, unsigned a, unsigned b, unsigned c,
                                        unsigned char s) {
  tri_out[3 * row] = a; tri_out[3 * row + 1] = b; tri_out[3 * row + 2] = c;
  if (sel_out) sel_out[row] = s;
}

// one thread per triangle: row t and the k(t) rows at n_t + base(t); rows_t = n_t + E bounds every row that is written
__global__ __launch_bounds__(VT) void k_refine_triangles(Pattern pt, const unsigned* __restrict__ base, const float* __restrict__ pos,
                                                         const unsigned char* __restrict__ sel_in, unsigned rows_t, unsigned* __restrict__ tri_out,
                                                         unsigned char* __restrict__ sel_out) {
  for (size_t ti = (size_t)blockIdx.x * VT + threadIdx.x; ti < pt.n_t; ti += (size_t)gridDim.x * VT) {
    const unsigned t = (unsigned)ti;
    unsigned v[3], r[3];
    bool degenerate;
    const unsigned k = pt.load(t, v, r, degenerate);
    const unsigned char s = sel_in ? sel_in[t] : (unsigned char)0;
    const size_t more = (size_t)pt.n_t + base[t];
    if (k == 0 || more + k > rows_t) {       // the second never with a base that is right
      put_row(tri_out, sel_out, t, v[0], v[1], v[2], s);
      continue;
    }
    if (k == 3) {
      const unsigned m0 = pt.n_v + r[0], m1 = pt.n_v + r[1], m2 = pt.n_v + r[2];
      put_row(tri_out, sel_out, t, v[0], m0, m2, s);
      put_row(tri_out, sel_out, more, m0, v[1], m1, s);
      put_row(tri_out, sel_out, more + 1, m2, m1, v[2], s);
      put_row(tri_out, sel_out, more + 2, m0, m1, m2, s);
      continue;
    }
    // the rotation: k = 1 brings the marked edge to ab, k = 2 the unmarked edge to ca, that is, the corner behind it to the front
    const int j = k == 1 ? (r[0] != NONE ? 0 : r[1] != NONE ? 1 : 2) : (r[0] == NONE ? 1 : r[1] == NONE ? 2 : 0);
    const unsigned a = v[j], b = v[(j + 1) % 3], c = v[(j + 2) % 3];
    const unsigned m0 = pt.n_v + r[j];
    if (k == 1) {
      put_row(tri_out, sel_out, t, a, m0, c, s);
      put_row(tri_out, sel_out, more, m0, b, c, s);
      continue;
    }
    const unsigned m1 = pt.n_v + r[(j + 1) % 3];
    const P3 pa = p3_load(pos, a, pt.n_v), pb = p3_load(pos, b, pt.n_v), pc = p3_load(pos, c, pt.n_v);
    double p0[3], p1[3];               // the midpoints as the float32 rows that k_refine_vertices writes
    for (int x = 0; x < 3; ++x) {
      p0[x] = (double)mid_of(pa.p[x], pb.p[x]);
      p1[x] = (double)mid_of(pb.p[x], pc.p[x]);
    }
    put_row(tri_out, sel_out, t, m0, b, m1, s);
    if (q_of(p0, pc.p) < q_of(pa.p, p1)) {
      put_row(tri_out, sel_out, more, a, m0, c, s);
      put_row(tri_out, sel_out, more + 1, m0, m1, c, s);
    } else {
      put_row(tri_out, sel_out, more, a, m0, m1, s);
      put_row(tri_out, sel_out, more + 1, a, m1, c, s);
    }
  }
}

}  // namespace

struct rgbid_refine {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0;
  SortWorkspace w;                   // 3 cap_t items: the corner sort; afterwards corner_edge and the marked edges' ends lie in its buffers
  unsigned* edge_lo = nullptr;       // [3 cap_t]
  unsigned* edge_hi = nullptr;       // [3 cap_t]
  unsigned* edge_rank = nullptr;     // [3 cap_t]
  unsigned char* flags = nullptr;    // [3 cap_t] ELIGIBLE | MARKED
  unsigned char* kk = nullptr;       // [cap_t]
  unsigned* base = nullptr;          // [cap_t]
  // the last plan
  bool planned = false;
  unsigned n_v = 0, n_t = 0, n_m = 0, n_new = 0;
  const unsigned* corner_edge = nullptr;   // in the workspace
  const unsigned* mlo = nullptr;
  const unsigned* mhi = nullptr;
  // stage timing: check [0, 1], the rest of the plan [2, 3], emit [4, 5]
  bool timed[2] = {false, false};
  Buffers buf;
  StageTimer<6> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

// steps 2 and 3 behind the index check, n_t > 0
int plan_stage(rgbid_refine* h, const unsigned* tri, const float* pos, const unsigned char* selection, double l2) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  const unsigned n_v = h->n_v, n_t = h->n_t;
  const CornerView view{tri, n_t, n_v, 3ull * n_t};
  const unsigned items = (unsigned)view.items;
  const int p = w.sort_rounds(s, CornerKey{view}, n_v, items, {0, 1});   // by the larger end, then by the smaller
  unsigned* his = w.keys_as<unsigned>(p ^ 1);
  hipLaunchKernelGGL(k_mesh_corner_ends<false>, dim3(grid_of(blocks_of(items))), dim3(VT), 0, s, view, w.idx[p], his, (unsigned*)nullptr);
  unsigned* corner_edge = w.idx[p ^ 1];
  RGBID_HIP(hipMemsetAsync(h->flags, 0, (size_t)items, s));
  const EdgeSrc edges{w.keys_as<unsigned>(p), his, w.idx[p], selection, items, n_v, corner_edge, h->edge_lo, h->edge_hi, h->flags};
  w.value_scan(s, edges, items, SLOT_RUNS);
  hipLaunchKernelGGL(k_refine_mark, dim3(grid_of(blocks_of(items))), dim3(VT), 0, s, pos, h->edge_lo, h->edge_hi, w.slots + SLOT_RUNS, items, n_v, l2,
                     h->flags, h->edge_rank, w.slots + SLOT_ELIGIBLE);
  // the sorted keys are read no more: the second halves of the key buffers take the marked edges' ends
  unsigned* mlo = w.keys_as<unsigned>(0) + (size_t)w.cap;
  unsigned* mhi = w.keys_as<unsigned>(1) + (size_t)w.cap;
  const MarkedSrc marked{h->flags, h->edge_lo, h->edge_hi, w.slots + SLOT_RUNS, items, h->edge_rank, mlo, mhi};
  w.count_scan(s, marked, items, SLOT_VOXELS);
  w.write(s, marked, items);
  const Pattern pt{tri, corner_edge, h->edge_rank, n_t, n_v, items};
  hipLaunchKernelGGL(k_refine_k, dim3(grid_of(blocks_of(n_t))), dim3(VT), 0, s, pt, h->kk, w.slots);
  const BaseSrc base{h->kk, n_t, h->base};
  w.value_scan(s, base, n_t, SLOT_NEW);
  h->corner_edge = corner_edge;
  h->mlo = mlo;
  h->mhi = mhi;
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_refine_create(rgbid_refine** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles) {
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_REFINE_MAX_VERTICES, RGBID_REFINE_MAX_TRIANGLES, [&](rgbid_refine* h) {
    const unsigned long long corners = 3ull * max_triangles;
    const size_t ce = (size_t)corners, ct = (size_t)max_triangles;
    int r = h->w.alloc(h->buf, corners);
    if (!r) r = h->buf.alloc(&h->edge_lo, sizeof(unsigned) * ce);
    if (!r) r = h->buf.alloc(&h->edge_hi, sizeof(unsigned) * ce);
    if (!r) r = h->buf.alloc(&h->edge_rank, sizeof(unsigned) * ce);
    if (!r) r = h->buf.alloc(&h->flags, ce);
    if (!r) r = h->buf.alloc(&h->kk, ct);
    if (!r) r = h->buf.alloc(&h->base, sizeof(unsigned) * ct);
    return r;
  });
}

int rgbid_refine_destroy(rgbid_refine* h) { return destroy_handle(h); }   // an emit may still read the tables

int rgbid_refine_plan(rgbid_refine* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                      const float* vertices_dev, const uint8_t* selection_or_null, double max_edge, unsigned long long counts[9]) {
  if (!h) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  if (n_vertices && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  if (!std::isfinite(max_edge) || max_edge < 0.0) return RGBID_E_INVALID;
  if (counts) for (int i = 0; i < 9; ++i) counts[i] = 0;
  h->planned = false;
  h->timed[0] = false;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  h->n_v = n_v; h->n_t = n_t; h->n_m = h->n_new = 0;
  if (n_t == 0) {                                                    // no triangle: no edge
    h->planned = true;
    return RGBID_OK;
  }
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  h->mark(0);
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, s));
  check_triangles<false>(s, triangles_dev, n_t, n_v, w.slots + SLOT_BAD);
  h->mark(1);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  if (w.slots_host[SLOT_BAD]) return RGBID_E_INVALID;                // a triangle names a vertex that does not exist
  h->mark(2);
  if (int r = plan_stage(h, triangles_dev, vertices_dev, selection_or_null, max_edge * max_edge)) return r;
  h->mark(3);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  h->timed[0] = h->timer.on;
  const unsigned long long n_e = w.slots_host[SLOT_RUNS], n_m = w.slots_host[SLOT_VOXELS], n_new = w.slots_host[SLOT_NEW];
  const unsigned long long k1 = w.slots_host[SLOT_K1], k2 = w.slots_host[SLOT_K2], k3 = w.slots_host[SLOT_K3];
  if (n_e > 3ull * n_t || n_m > n_e || k1 + k2 + k3 > n_t || n_new != k1 + 2 * k2 + 3 * k3) return RGBID_E_INVALID;   // never with tables that are right
  if (counts) {
    counts[0] = n_e;
    counts[1] = w.slots_host[SLOT_ELIGIBLE];
    counts[2] = n_m;
    counts[3] = n_t - (k1 + k2 + k3);
    counts[4] = k1;
    counts[5] = k2;
    counts[6] = k3;
    counts[7] = w.slots_host[SLOT_DEGENERATE];
    counts[8] = n_new;
  }
  if (n_v + n_m > RGBID_REFINE_MAX_VERTICES || n_t + n_new > RGBID_REFINE_MAX_TRIANGLES) return RGBID_E_INVALID;
  h->n_m = (unsigned)n_m;
  h->n_new = (unsigned)n_new;
  h->planned = true;
  return RGBID_OK;
}

int rgbid_refine_emit(rgbid_refine* h, const float* vertices_in, const uint8_t* colours_in, const float* normals_in, const uint32_t* triangles_in,
                      const uint8_t* selection_in, float* vertices_out, uint8_t* colours_out, float* normals_out, uint32_t* triangles_out,
                      uint8_t* selection_out, unsigned long long vertex_capacity, unsigned long long triangle_capacity) {
  if (!h || !h->planned) return RGBID_E_INVALID;
  if (!colours_in != !colours_out || !normals_in != !normals_out || !selection_in != !selection_out) return RGBID_E_INVALID;
  const unsigned long long rows_v = (unsigned long long)h->n_v + h->n_m, rows_t = (unsigned long long)h->n_t + h->n_new;
  if (vertex_capacity < rows_v || triangle_capacity < rows_t) return RGBID_E_INVALID;
  if (h->n_v && !vertices_in) return RGBID_E_INVALID;
  if (h->n_t && !triangles_in) return RGBID_E_INVALID;
  if (rows_v && !vertices_out) return RGBID_E_INVALID;
  if (rows_t && !triangles_out) return RGBID_E_INVALID;
  if (!aligned4(vertices_in) || !aligned4(vertices_out) || !aligned4(normals_in) || !aligned4(normals_out) || !aligned4(triangles_in) ||
      !aligned4(triangles_out))
    return RGBID_E_INVALID;
  const size_t in_v = (size_t)h->n_v, in_t = (size_t)h->n_t;
  if (overlap(vertices_in, 12 * in_v, vertices_out, 12 * (size_t)rows_v) || overlap(normals_in, 12 * in_v, normals_out, 12 * (size_t)rows_v) ||
      overlap(colours_in, 3 * in_v, colours_out, 3 * (size_t)rows_v) || overlap(triangles_in, 12 * in_t, triangles_out, 12 * (size_t)rows_t) ||
      overlap(selection_in, in_t, selection_out, (size_t)rows_t))
    return RGBID_E_INVALID;
  h->timed[1] = false;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  h->mark(4);
  if (in_v) {
    RGBID_HIP(hipMemcpyAsync(vertices_out, vertices_in, 12 * in_v, hipMemcpyDeviceToDevice, s));
    if (colours_out) RGBID_HIP(hipMemcpyAsync(colours_out, colours_in, 3 * in_v, hipMemcpyDeviceToDevice, s));
    if (normals_out) RGBID_HIP(hipMemcpyAsync(normals_out, normals_in, 12 * in_v, hipMemcpyDeviceToDevice, s));
  }
  if (h->n_m)
    hipLaunchKernelGGL(k_refine_vertices, dim3(blocks_of(h->n_m)), dim3(VT), 0, s, h->mlo, h->mhi, h->n_m, h->n_v, vertices_in, colours_in, normals_in,
                       vertices_out, colours_out, normals_out);
  if (in_t) {
    const Pattern pt{triangles_in, h->corner_edge, h->edge_rank, h->n_t, h->n_v, 3u * h->n_t};
    hipLaunchKernelGGL(k_refine_triangles, dim3(grid_of(blocks_of(in_t))), dim3(VT), 0, s, pt, h->base, vertices_in, selection_in, (unsigned)rows_t,
                       triangles_out, selection_out);
  }
  h->mark(5);
  RGBID_HIP(hipGetLastError());
  h->timed[1] = h->timer.on;
  return RGBID_OK;
}

int rgbid_refine_timing(rgbid_refine* h, int enable, float ms[2]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  static const int pairs[2][4] = {{0, 1, 2, 3}, {4, 5}};   // the plan: the check and the rest
  if (ms)
    if (int r = stage_times(h->timer, h->timed, pairs, ms)) return r;
  return h->timer.enable(enable != 0);
}

}  // extern "C"
