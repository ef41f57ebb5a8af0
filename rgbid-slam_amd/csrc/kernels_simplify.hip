// kernels_simplify.hip -- an indexed triangle mesh in device memory simplified by vertex clustering: the vertices of one grid cell become
// one vertex, the triangles are rewritten over the cells, those that collapse or repeat are dropped (include/rgbid_simplify.h, DESIGN.md
// section 23).
//
// The judge is tests/simplify_mirror.py; grid, counts and every emitted buffer are byte-identical to it.
//   plan  k_mesh_check       mesh_device.h: counts the triangles with an index >= n_v into a slot
//         k_vox_box          per-axis min / max and the count of the finite vertices (voxel_device.h, over VertexPoints), copied to the
//                            host with that slot: a bad index ends the call here
//         (host)             form_grid, the key width
//         k_vox_keys         one (key, vertex) pair per vertex; a vertex that does not take part gets the sentinel (largest key + 1)
//         LSD radix sort     voxel_device.h, stable: the members of a cluster in ascending vertex order
//         k_simp_runs        the flag compaction's write pass over the heads key[i] != key[i - 1] with one more store per item: a head
//                            writes its position as the start of cluster `rank`, EVERY item writes cluster_of[vertex] = the heads up to
//                            and including it - 1.  A scatter to distinct addresses
//         k_simp_classes     one thread per triangle: lost / collapsed / candidate; the first two counted (one atomic per wave and
//                            class), the third flagged as kept
//         duplicate search   sort_rounds: three stable sorts of (key, triangle) by s2, s1, s0, the sorted cluster numbers of a candidate
//                            (k_vox_round_keys over TriKey recomputes the key of the next round in the order the last round left;
//                            lost and collapsed triangles carry the sentinel C and sort behind the candidates); k_simp_heads clears the
//                            flag of a candidate whose predecessor has the same triple: equal triples are adjacent and in input order
//         kept               flag count + scan over the flags
//   emit  k_simp_emit        one thread per cluster: gathers its members through the sorted indices, sums in order in double
//         cluster_of         a copy
//         flag write         a kept triangle writes cluster_of of its three indices at its rank
// No float atomics, no wait on another thread, every loop has its bound when it starts.
#include "../../include/rgbid_simplify.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // the index check, the argument test, the create; voxel_device.h's box, grid, cell keys, radix sort, flag
                            // compaction and unit vector; the sort workspace

#include <cmath>
#include <cstring>

using namespace rgbid;

namespace {

constexpr unsigned NO_CLUSTER = RGBID_SIMPLIFY_NO_CLUSTER;
enum { SLOT_BAD = 9, SLOT_LOST = 10, SLOT_COLLAPSED = 11, SLOT_DUPLICATE = 12, SLOT_KEPT = 13 };   // beside the workspace's own 0 .. 8
static_assert(SLOT_VOXELS < SLOT_BAD && SLOT_KEPT < SLOTS, "the slots of this file lie behind the workspace's");

// ---- vertices ---------------------------------------------------------------------------------------------------------------------
// k_vox_flag_write over HeadSrc's flags, and the cluster number of every item: items of a tile in (round, wave, lane) order, the heads
// before an item = tile offset + earlier rounds + lower waves + mbcnt
template <typename K>
__global__ __launch_bounds__(VT) void k_simp_runs(const K* __restrict__ keys, const unsigned* __restrict__ sidx, unsigned finite, unsigned n_v,
                                                  const unsigned* __restrict__ bc, unsigned* __restrict__ starts, unsigned* __restrict__ cluster_of) {
  __shared__ unsigned lds[VT / 64];
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  if (t0 >= finite) return;              // uniform over the block
  unsigned carry = bc[blockIdx.x];
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    const bool in = i < finite;
    const bool head = in && (i == 0 || keys[i] != keys[i - 1]);
    unsigned tot;
    const unsigned before = carry + block_rank(head, lds, tot);
    if (in) {
      const unsigned run = head ? before : before - 1;     // item 0 is a head: before >= 1 for every other item
      if (head) starts[run] = (unsigned)i;
      const unsigned v = sidx[i];
      if (v < n_v) cluster_of[v] = run;
    }
    carry += tot;
  }
}

// ---- representatives --------------------------------------------------------------------------------------------------------------
struct Member {
  float p[3], n[3];
  unsigned c[3];
};

struct ClusterSum {
  double p[3] = {0, 0, 0}, n[3] = {0, 0, 0};
  unsigned long long c[3] = {0, 0, 0};
  bool normal = false;
};

__device__ __forceinline__ Member member_load(const float* __restrict__ verts, const unsigned char* __restrict__ cols, const float* __restrict__ nrm,
                                              unsigned id) {
  const size_t o = 3 * (size_t)id;
  Member m;
  for (int a = 0; a < 3; ++a) {
    m.p[a] = verts[o + a];
    m.c[a] = cols ? cols[o + a] : 0u;
    m.n[a] = nrm ? nrm[o + a] : 0.f;
  }
  return m;
}

// one member, in order; the pragma keeps every add a separate rounding
__device__ __forceinline__ void member_add(ClusterSum& s, const Member& m, bool normals) {
  RGBID_FP_STRICT
  for (int a = 0; a < 3; ++a) { s.p[a] += (double)m.p[a]; s.c[a] += m.c[a]; }
  if (normals && finite3(m.n[0], m.n[1], m.n[2])) {
    for (int a = 0; a < 3; ++a) s.n[a] += (double)m.n[a];
    s.normal = true;
  }
}

__global__ __launch_bounds__(VT) void k_simp_emit(const float* __restrict__ verts, const unsigned char* __restrict__ cols, const float* __restrict__ nrm,
                                                  const unsigned* __restrict__ sidx, const unsigned* __restrict__ starts, unsigned n_c,
                                                  float* __restrict__ verts_out, unsigned char* __restrict__ cols_out, float* __restrict__ nrm_out,
                                                  unsigned* __restrict__ members_out) {
  RGBID_FP_STRICT
  const size_t c = (size_t)blockIdx.x * VT + threadIdx.x;
  if (c >= n_c) return;
  const unsigned b = starts[c], e = starts[c + 1];
  ClusterSum s;
  unsigned m = b;
  for (; e - m >= 4; m += 4) {                   // gather_in_order's loop, kept here: through it this kernel measured 1 % slower at 192 members
    unsigned id[4];
    Member mem[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) id[u] = sidx[m + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) mem[u] = member_load(verts, cols, nrm, id[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) member_add(s, mem[u], nrm != nullptr);
  }
  for (; m < e; ++m) member_add(s, member_load(verts, cols, nrm, sidx[m]), nrm != nullptr);
  const unsigned cnt = e - b;
  const double dc = (double)cnt;
  const size_t o = 3 * c;
  for (int a = 0; a < 3; ++a) verts_out[o + a] = (float)(s.p[a] / dc);
  if (cols_out)
    for (int a = 0; a < 3; ++a) cols_out[o + a] = (unsigned char)((2 * s.c[a] + cnt) / (2 * (unsigned long long)cnt));   // the rounded mean
  if (nrm_out) {
    float n[3] = {0.f, 0.f, 0.f};
    if (s.normal) unit_of(s.n, n);
    for (int a = 0; a < 3; ++a) nrm_out[o + a] = n[a];
  }
  if (members_out) members_out[c] = cnt;
}

// ---- triangles --------------------------------------------------------------------------------------------------------------------
enum TriClass { TRI_LOST, TRI_COLLAPSED, TRI_CANDIDATE };

struct TriView {
  const unsigned* tri;
  const unsigned* cluster_of;
  unsigned n_v;
  // t' of triangle t; an index that names no vertex reads nothing
  __device__ __forceinline__ void clusters(size_t t, unsigned c[3]) const {
    for (int k = 0; k < 3; ++k) {
      const unsigned i = tri[3 * t + k];
      c[k] = i < n_v ? cluster_of[i] : NO_CLUSTER;
    }
  }
};

// step 5's first two classes, in its order
__device__ __forceinline__ TriClass tri_class(const unsigned c[3]) {
  if (c[0] == NO_CLUSTER || c[1] == NO_CLUSTER || c[2] == NO_CLUSTER) return TRI_LOST;
  if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return TRI_COLLAPSED;
  return TRI_CANDIDATE;
}

__device__ __forceinline__ void sort3(unsigned c[3]) {
  const unsigned lo = min(c[0], c[1]), hi = max(c[0], c[1]), z = c[2];
  c[0] = min(lo, z);
  c[1] = max(lo, min(hi, z));
  c[2] = max(hi, z);
}

__global__ __launch_bounds__(VT) void k_simp_classes(TriView view, unsigned n_t, unsigned char* __restrict__ kept, unsigned* __restrict__ slots) {
  unsigned lost = 0, collapsed = 0;
  for (size_t t = (size_t)blockIdx.x * VT + threadIdx.x; t < n_t; t += (size_t)gridDim.x * VT) {
    unsigned c[3];
    view.clusters(t, c);
    const TriClass k = tri_class(c);
    lost += k == TRI_LOST;
    collapsed += k == TRI_COLLAPSED;
    kept[t] = k == TRI_CANDIDATE;
  }
  wave_add_to(slots + SLOT_LOST, lost);
  wave_add_to(slots + SLOT_COLLAPSED, collapsed);
}

// sort_rounds' key of round r (2, 1, 0) for triangle t: s_r of a candidate, the sentinel n_c of every other triangle
struct TriKey {
  TriView view;
  unsigned n_t, n_c;
  __device__ __forceinline__ unsigned size() const { return n_t; }
  __device__ __forceinline__ unsigned operator()(unsigned t, int r) const {
    unsigned c[3], key = n_c;
    if (t < n_t) {
      view.clusters(t, c);
      if (tri_class(c) == TRI_CANDIDATE) { sort3(c); key = c[r]; }
    }
    return key;
  }
};

// after the three rounds the candidates come first, equal triples are adjacent and in input order: a candidate whose predecessor has
// its triple is a duplicate and loses its flag (a store to its own input index)
__global__ __launch_bounds__(VT) void k_simp_heads(TriView view, unsigned n_t, const unsigned* __restrict__ order, unsigned char* __restrict__ kept,
                                                   unsigned* __restrict__ slots) {
  unsigned dup = 0;
  for (size_t m = (size_t)blockIdx.x * VT + threadIdx.x; m < n_t; m += (size_t)gridDim.x * VT) {
    if (m == 0) continue;
    const unsigned t = order[m], u = order[m - 1];
    if (t >= n_t || u >= n_t) continue;
    unsigned c[3], d[3];
    view.clusters(t, c);
    view.clusters(u, d);
    if (tri_class(c) != TRI_CANDIDATE || tri_class(d) != TRI_CANDIDATE) continue;
    sort3(c);
    sort3(d);
    if (c[0] == d[0] && c[1] == d[1] && c[2] == d[2]) { kept[t] = 0; ++dup; }
  }
  wave_add_to(slots + SLOT_DUPLICATE, dup);
}

// stable compaction of the kept triangles: t' at the rank; out == null only counts
struct KeptTriSrc {
  unsigned n_t;
  TriView view;
  const unsigned char* kept;
  unsigned* out;                     // [kept][3]
  __device__ __forceinline__ unsigned size() const { return n_t; }
  __device__ __forceinline__ bool flag(unsigned t) const { return kept[t] != 0; }
  __device__ __forceinline__ void write(unsigned pos, unsigned t) const {
    unsigned c[3];
    view.clusters(t, c);
    unsigned* o = out + 3 * (size_t)pos;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
  }
};

}  // namespace

struct rgbid_simplify {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0;
  SortWorkspace wv;                  // the vertices' sort: afterwards the members in cluster order (sidx) and the clusters' starts
  SortWorkspace wt;                  // the triangles': the duplicate search and the tile offsets of the kept ones; it shares wv's slots
  unsigned* cluster_of = nullptr;    // [cap_v]
  unsigned char* kept = nullptr;     // [cap_t] 1: the triangle is kept
  // the last plan
  bool planned = false;
  unsigned n_v = 0, n_t = 0, n_c = 0, n_kept = 0;
  const float* verts = nullptr;
  const unsigned* tri = nullptr;
  const unsigned* sidx = nullptr;
  const unsigned* starts = nullptr;
  // stage timing: box [0, 1], the rest of the vertex stage [2, 3], triangles [4, 5], emit [6, 7]
  bool timed[3] = {false, false, false};
  Buffers buf;
  StageTimer<8> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

// keys, sort, runs and the cluster map for keys of type K
template <typename K>
int vertex_stage(rgbid_simplify* h, unsigned finite, const VoxGrid& g) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->wv;
  const unsigned n_v = h->n_v;
  w.make_keys<K>(s, VertexPoints{h->verts}, n_v, g);
  const SortedPairs<K> sp = w.sort<K>(s, n_v, g);
  w.count_scan(s, HeadSrc<K>{sp.keys, finite, sp.starts}, finite, SLOT_RUNS, sp.starts, finite);
  hipLaunchKernelGGL(k_simp_runs<K>, dim3((finite + RUN_TILE - 1) / RUN_TILE), dim3(VT), 0, s, sp.keys, sp.idx, finite, n_v, w.bc, sp.starts,
                     h->cluster_of);
  h->sidx = sp.idx;
  h->starts = sp.starts;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int triangle_stage(rgbid_simplify* h, bool keep_duplicates) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->wt;
  const unsigned n_t = h->n_t, gt = grid_of(((unsigned long long)n_t + VT - 1) / VT);
  const TriView view{h->tri, h->cluster_of, h->n_v};
  hipLaunchKernelGGL(k_simp_classes, dim3(gt), dim3(VT), 0, s, view, n_t, h->kept, w.slots);
  if (!keep_duplicates) {
    const int p = w.sort_rounds(s, TriKey{view, n_t, h->n_c}, h->n_c, n_t, {2, 1, 0});
    hipLaunchKernelGGL(k_simp_heads, dim3(gt), dim3(VT), 0, s, view, n_t, w.idx[p], h->kept, w.slots);
  }
  w.count_scan(s, KeptTriSrc{n_t, view, h->kept, nullptr}, n_t, SLOT_KEPT);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_simplify_create(rgbid_simplify** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles) {
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_SIMPLIFY_MAX_VERTICES, RGBID_SIMPLIFY_MAX_TRIANGLES, [&](rgbid_simplify* h) {
    int r = h->wv.alloc(h->buf, max_vertices);
    if (!r) r = h->wt.alloc(h->buf, max_triangles);
    if (!r) r = h->buf.alloc(&h->cluster_of, sizeof(unsigned) * (size_t)max_vertices);
    if (!r) r = h->buf.alloc(&h->kept, (size_t)max_triangles);
    h->wt.slots = h->wv.slots;         // one slot area, one read-back
    h->wt.slots_host = h->wv.slots_host;
    return r;
  });
}

int rgbid_simplify_destroy(rgbid_simplify* h) { return destroy_handle(h); }   // an emit may still read the tables

int rgbid_simplify_plan(rgbid_simplify* h, unsigned long long n_vertices, const float* vertices_dev, unsigned long long n_triangles,
                        const uint32_t* triangles_dev, const float cell[3], uint32_t flags, long long grid[6], unsigned long long counts[6]) {
  if (!h || !cell || (flags & ~RGBID_SIMPLIFY_KEEP_DUPLICATES)) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  if (n_vertices && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  for (int a = 0; a < 3; ++a) if (!(std::isfinite(cell[a]) && cell[a] > 0.f)) return RGBID_E_INVALID;
  if (grid) for (int i = 0; i < 6; ++i) grid[i] = 0;
  if (counts) for (int i = 0; i < 6; ++i) counts[i] = 0;
  h->planned = false;
  h->timed[0] = h->timed[1] = false;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  h->n_v = n_v; h->n_t = n_t; h->n_c = 0; h->n_kept = 0;
  h->verts = vertices_dev; h->tri = triangles_dev;
  if (n_v == 0) { h->planned = true; return RGBID_OK; }   // no vertex, no triangle, no cluster
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->wv;
  h->mark(0);
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, s));
  if (n_t) check_triangles(s, triangles_dev, n_t, n_v, w.slots + SLOT_BAD);
  w.box(s, VertexPoints{vertices_dev}, n_v);
  h->mark(1);
  unsigned finite;
  float lo[3], hi[3];
  if (int r = w.read_box(s, finite, lo, hi)) return r;
  if (w.slots_host[SLOT_BAD]) return RGBID_E_INVALID;      // a triangle names a vertex that does not exist
  unsigned long long cnt[6] = {finite, 0, 0, 0, 0, 0};
  long long gr[6] = {0, 0, 0, 0, 0, 0};
  h->mark(2);
  RGBID_HIP(hipMemsetAsync(h->cluster_of, 0xFF, sizeof(unsigned) * (size_t)n_v, s));   // NO_CLUSTER; k_simp_runs writes the others
  if (finite == 0) {
    cnt[2] = n_t;                                          // every triangle is lost
  } else {
    VoxGrid g;
    if (int r = form_grid(lo, hi, cell, g, gr)) return r;
    if (int r = with_key_type(g, [&](auto k) { return vertex_stage<decltype(k)>(h, finite, g); })) return r;
    h->mark(3);
    if (int r = w.read_slots(s)) return r;
    h->n_c = w.slots_host[SLOT_RUNS];
    h->timed[0] = h->timer.on;
    cnt[1] = h->n_c;
    if (n_t) {
      h->mark(4);
      if (int r = triangle_stage(h, (flags & RGBID_SIMPLIFY_KEEP_DUPLICATES) != 0)) return r;
      h->mark(5);
      if (int r = w.read_slots(s)) return r;
      h->timed[1] = h->timer.on;
      h->n_kept = w.slots_host[SLOT_KEPT];
      cnt[2] = w.slots_host[SLOT_LOST];
      cnt[3] = w.slots_host[SLOT_COLLAPSED];
      cnt[4] = w.slots_host[SLOT_DUPLICATE];
      cnt[5] = h->n_kept;
    }
  }
  if (grid) memcpy(grid, gr, sizeof gr);
  if (counts) memcpy(counts, cnt, sizeof cnt);
  h->planned = true;
  return RGBID_OK;
}

int rgbid_simplify_emit(rgbid_simplify* h, const uint8_t* colours_dev, const float* normals_dev, float* vertices_out, uint8_t* colours_out,
                        float* normals_out, uint32_t* members_out, uint32_t* cluster_of_out, uint32_t* triangles_out,
                        unsigned long long vertex_capacity, unsigned long long triangle_capacity) {
  if (!h || !h->planned) return RGBID_E_INVALID;
  if (h->n_v && ((colours_out && !colours_dev) || (normals_out && !normals_dev))) return RGBID_E_INVALID;   // no vertex: no input to miss
  if (!aligned4(normals_dev) || !aligned4(normals_out) || !aligned4(members_out) || !aligned4(cluster_of_out)) return RGBID_E_INVALID;
  if (vertex_capacity < h->n_c || triangle_capacity < h->n_kept) return RGBID_E_INVALID;
  if (h->n_c && (!vertices_out || !aligned4(vertices_out))) return RGBID_E_INVALID;
  if (h->n_kept && (!triangles_out || !aligned4(triangles_out))) return RGBID_E_INVALID;
  h->timed[2] = false;
  if (h->n_v == 0) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  h->mark(6);
  if (h->n_c)
    hipLaunchKernelGGL(k_simp_emit, dim3((h->n_c + VT - 1) / VT), dim3(VT), 0, s, h->verts, colours_out ? colours_dev : nullptr,
                       normals_out ? normals_dev : nullptr, h->sidx, h->starts, h->n_c, vertices_out, colours_out, normals_out, members_out);
  if (cluster_of_out) RGBID_HIP(hipMemcpyAsync(cluster_of_out, h->cluster_of, sizeof(unsigned) * (size_t)h->n_v, hipMemcpyDeviceToDevice, s));
  if (h->n_kept) h->wt.write(s, KeptTriSrc{h->n_t, TriView{h->tri, h->cluster_of, h->n_v}, h->kept, triangles_out}, h->n_t);
  h->mark(7);
  RGBID_HIP(hipGetLastError());
  h->timed[2] = h->timer.on;
  return RGBID_OK;
}

int rgbid_simplify_timing(rgbid_simplify* h, int enable, float ms[3]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  static const int pairs[3][4] = {{0, 1, 2, 3}, {4, 5}, {6, 7}};   // the vertex stage: the box and the rest
  if (ms)
    if (int r = stage_times(h->timer, h->timed, pairs, ms)) return r;
  return h->timer.enable(enable != 0);
}

}  // extern "C"
