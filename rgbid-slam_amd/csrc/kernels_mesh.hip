// kernels_mesh.hip -- the connected components of an indexed triangle mesh in device memory: labelled, counted, selected by size or by a
// mask, and the kept part written out with renumbered indices (include/rgbid_mesh.h).
//
// The judge is tests/mesh_mirror.py; table, labels, counts and every emitted buffer are byte-identical to it.
//   label   k_mesh_check      mesh_device.h: counts the triangles with an index >= n_v into a slot; every later kernel of the call reads
//                             that slot first and does nothing when it is not 0
//           k_mesh_init       parent[v] = v, the counts per root = 0
//           k_mesh_unite      one thread per triangle: unite(i0, i1), unite(i1, i2).  A lock-free union-find: find walks parent down to a
//                             root (path splitting on the way), the larger of two roots is hooked under the smaller with one atomicCAS,
//                             a failed CAS continues from the value it returned
//           k_mesh_compress   every vertex walks to its root once more, splitting the path
//           k_mesh_flatten    parent[v] = the root of v, written by v's own thread after a walk that stores nothing; the vertices per
//                             root, one atomicAdd per distinct root of a wave
//           k_mesh_tri_count  the triangles per root (of the first index), likewise
//           roots             flag count + scan + write over parent[v] == v (voxel_device.h): number[root] = its rank
//   table   flag write        a second source over the same flags and tile offsets: (root, vertices, triangles) at the rank
//           k_mesh_labels     labels[v] = number[parent[v]]
//   select  k_mesh_mark       remap[v] = 0 where the component of v is kept, 0xFFFFFFFF elsewhere; the kept roots are counted
//           vertices          flag count + scan + write over remap[v] != 0xFFFFFFFF: remap[v] = its rank
//           triangles         flag count + scan over remap[first index] != 0xFFFFFFFF
//   emit    flag write        a kept vertex copies its attributes to its rank; a kept triangle writes remap of its three indices
//
// The invariant of the union-find: every value ever stored into parent[x] is <= x and a vertex of x's class.
//  - A find descends strictly, so it ends, whatever it reads: a value read from a cache that another compute unit's store has not reached
//    (a CU's L1 is never refreshed, the XCDs' L2s are not coherent) is an older value of parent[x], hence still x itself or an ancestor.
//  - Only the atomicCAS(&parent[hi], hi, lo), decided at device scope, turns a root into a child, and it does so at most once per vertex:
//    parent[hi] == hi holds until the one CAS that succeeds.  Path splitting stores to parent[x] only after it has read parent[x] != x,
//    so it never touches a root.
//  - A failed CAS returns parent[hi] < hi; the unite continues from there, so the sum of its two vertices falls with every round.  No
//    thread waits for another one.
//  - When every unite has returned the two ends of every edge are in one tree, and the root of a tree is its smallest vertex: the result
//    does not depend on the schedule.
// The counts are integer atomicAdds: exact in any order.  No LDS beyond the scans', no scratch.
#include "../../include/rgbid_mesh.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // the index check, the argument test, the create; voxel_device.h's flag compaction, one-block scan, grid_of

using namespace rgbid;

namespace {

constexpr unsigned DROPPED = 0xFFFFFFFFu;      // remap of a vertex that is not kept (a kept one has a rank < 2^31)
enum { SLOT_BAD = 0, SLOT_COMPONENTS = 1, SLOT_KEPT_C = 2, SLOT_KEPT_V = 3, SLOT_KEPT_T = 4 };

// parent is read with relaxed device-scope loads (never held in a register across a round, not served by the CU's L1) and written by
// path splitting with relaxed stores that need no scope: any value that satisfies the invariant will do
__device__ __forceinline__ unsigned parent_load(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void parent_store(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT); }

// the root of x as far as this thread can see it; every vertex on the way gets its grandparent as parent (g <= p < x)
__device__ __forceinline__ unsigned mesh_find(unsigned* parent, unsigned x) {
  unsigned p = parent_load(parent + x);
  while (p != x) {
    const unsigned g = parent_load(parent + p);
    if (g != p) parent_store(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void mesh_unite(unsigned* parent, unsigned a, unsigned b) {
  for (;;) {
    a = mesh_find(parent, a);
    b = mesh_find(parent, b);
    if (a == b) return;
    const unsigned hi = a > b ? a : b, lo = a > b ? b : a;
    const unsigned old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;             // hi was a root and is now a child of lo
    a = old;                           // somebody hooked hi first: old < hi is its parent
    b = lo;
  }
}

// 0: one atomicAdd per lane, for the A/B of DESIGN.md section 22 (an alternative build of the library)
#ifndef RGBID_MESH_WAVE_ADD
#define RGBID_MESH_WAVE_ADD 1
#endif

// counts[key] += 1 for every valid lane, with one atomic per distinct key of the wave.  Called by all lanes of the wave together
__device__ __forceinline__ void wave_add_by_key(unsigned* __restrict__ counts, bool valid, unsigned key) {
  if (!RGBID_MESH_WAVE_ADD) {
    if (valid) atomicAdd(counts + key, 1u);
    return;
  }
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(valid);
  while (todo) {
    const int leader = __builtin_amdgcn_readfirstlane(__builtin_ctzll(todo));
    const unsigned k = (unsigned)__builtin_amdgcn_readlane((int)key, leader);
    const unsigned long long same = __ballot(valid && key == k);
    if (lane == leader) atomicAdd(counts + k, (unsigned)__popcll(same));
    todo &= ~same;
  }
}

__device__ __forceinline__ bool well_formed(const unsigned* __restrict__ tri, size_t t, unsigned n_v, unsigned& i0, unsigned& i1, unsigned& i2) {
  i0 = tri[3 * t]; i1 = tri[3 * t + 1]; i2 = tri[3 * t + 2];
  return i0 < n_v && i1 < n_v && i2 < n_v;
}

__global__ __launch_bounds__(VT) void k_mesh_init(unsigned n_v, unsigned* __restrict__ parent, unsigned* __restrict__ vcount, unsigned* __restrict__ tcount,
                                                  const unsigned* __restrict__ bad) {
  if (*bad) return;
  for (size_t v = (size_t)blockIdx.x * VT + threadIdx.x; v < n_v; v += (size_t)gridDim.x * VT) {
    parent[v] = (unsigned)v;
    vcount[v] = 0;
    tcount[v] = 0;
  }
}

__global__ __launch_bounds__(VT) void k_mesh_unite(const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v, unsigned* parent,
                                                   const unsigned* __restrict__ bad) {
  if (*bad) return;
  for (size_t t = (size_t)blockIdx.x * VT + threadIdx.x; t < n_t; t += (size_t)gridDim.x * VT) {
    unsigned i0, i1, i2;
    if (!well_formed(tri, t, n_v, i0, i1, i2)) continue;
    mesh_unite(parent, i0, i1);
    mesh_unite(parent, i1, i2);
  }
}

// every vertex walks to its root once with path splitting: what the unites left deep becomes shallow.  Nothing is returned
__global__ __launch_bounds__(VT) void k_mesh_compress(unsigned n_v, unsigned* parent, const unsigned* __restrict__ bad) {
  if (*bad) return;
  for (size_t v = (size_t)blockIdx.x * VT + threadIdx.x; v < n_v; v += (size_t)gridDim.x * VT) (void)mesh_find(parent, (unsigned)v);
}

// parent[v] = the root of v.  The walk stores nothing and only the owner writes parent[v]: a splitting store of another thread that lands
// after the owner's would put an inner vertex back.  A walker that meets a flattened entry is at the root in one step
__global__ __launch_bounds__(VT) void k_mesh_flatten(unsigned n_v, unsigned* parent, unsigned* __restrict__ vcount, const unsigned* __restrict__ bad) {
  if (*bad) return;
  for (size_t base = (size_t)blockIdx.x * VT; base < n_v; base += (size_t)gridDim.x * VT) {   // wave-uniform trips: the ballots need every lane
    const size_t v = base + threadIdx.x;
    const bool valid = v < n_v;
    unsigned r = 0;
    if (valid) {
      r = (unsigned)v;
      for (unsigned p = parent_load(parent + r); p != r; p = parent_load(parent + r)) r = p;
      if (r != (unsigned)v) parent_store(parent + v, r);
    }
    wave_add_by_key(vcount, valid, r);
  }
}

__global__ __launch_bounds__(VT) void k_mesh_tri_count(const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v, const unsigned* __restrict__ parent,
                                                       unsigned* __restrict__ tcount, const unsigned* __restrict__ bad) {
  if (*bad) return;
  for (size_t base = (size_t)blockIdx.x * VT; base < n_t; base += (size_t)gridDim.x * VT) {
    const size_t t = base + threadIdx.x;
    bool valid = t < n_t;
    unsigned r = 0;
    if (valid) {
      const unsigned i0 = tri[3 * t];
      valid = i0 < n_v;
      if (valid) r = parent[i0];
    }
    wave_add_by_key(tcount, valid, r);
  }
}

// stable compaction of the roots: item v < n_v (none when the check has failed), number[root] = its rank
struct RootSrc {
  unsigned n_v;
  const unsigned* parent;
  const unsigned* bad;
  unsigned* number;
  __device__ __forceinline__ unsigned size() const { return *bad ? 0u : n_v; }
  __device__ __forceinline__ bool flag(unsigned v) const { return parent[v] == v; }
  __device__ __forceinline__ void write(unsigned pos, unsigned v) const { number[v] = pos; }
};

// a second source over the flags of RootSrc: the table row of a root at its rank
struct TableSrc {
  unsigned n_v;
  const unsigned* parent;
  const unsigned* vcount;
  const unsigned* tcount;
  unsigned* table;                   // [C][3]
  __device__ __forceinline__ unsigned size() const { return n_v; }
  __device__ __forceinline__ bool flag(unsigned v) const { return parent[v] == v; }
  __device__ __forceinline__ void write(unsigned pos, unsigned v) const {
    unsigned* o = table + 3 * (size_t)pos;
    o[0] = v; o[1] = vcount[v]; o[2] = tcount[v];
  }
};

__global__ __launch_bounds__(VT) void k_mesh_labels(unsigned n_v, const unsigned* __restrict__ parent, const unsigned* __restrict__ number,
                                                    unsigned* __restrict__ labels) {
  for (size_t v = (size_t)blockIdx.x * VT + threadIdx.x; v < n_v; v += (size_t)gridDim.x * VT) {
    const unsigned r = parent[v];
    labels[v] = r < n_v ? number[r] : DROPPED;     // r <= v always; the test costs nothing
  }
}

// step 4 per vertex; a kept root is counted once
__global__ __launch_bounds__(VT) void k_mesh_mark(unsigned n_v, const unsigned* __restrict__ parent, const unsigned* __restrict__ tcount,
                                                  const unsigned* __restrict__ number, unsigned min_triangles, const unsigned char* __restrict__ mask,
                                                  unsigned* __restrict__ remap, unsigned* __restrict__ kept_components) {
  unsigned c = 0;
  for (size_t v = (size_t)blockIdx.x * VT + threadIdx.x; v < n_v; v += (size_t)gridDim.x * VT) {
    const unsigned r = parent[v];
    bool keep = false;
    if (r < n_v) keep = tcount[r] >= min_triangles && (!mask || mask[number[r]] != 0);
    remap[v] = keep ? 0u : DROPPED;
    if (keep && r == (unsigned)v) ++c;
  }
  wave_add_to(kept_components, c);
}

// stable compaction of the kept vertices: remap[v] = its rank, in place (a thread reads and writes its own entry only)
struct KeptVertexSrc {
  unsigned n_v;
  unsigned* remap;
  __device__ __forceinline__ unsigned size() const { return n_v; }
  __device__ __forceinline__ bool flag(unsigned v) const { return remap[v] != DROPPED; }
  __device__ __forceinline__ void write(unsigned pos, unsigned v) const { remap[v] = pos; }
};

// a second source over the same flags: a kept vertex copies its attributes to its rank, positions and normals as 32-bit words
struct VertexEmitSrc {
  unsigned n_v;
  const unsigned* remap;
  const unsigned* verts; const unsigned char* cols; const unsigned* normals;
  unsigned* verts_out; unsigned char* cols_out; unsigned* normals_out; unsigned* old_out;
  __device__ __forceinline__ unsigned size() const { return n_v; }
  __device__ __forceinline__ bool flag(unsigned v) const { return remap[v] != DROPPED; }
  __device__ __forceinline__ void write(unsigned pos, unsigned v) const {
    const size_t i = 3 * (size_t)v, o = 3 * (size_t)pos;
    verts_out[o] = verts[i]; verts_out[o + 1] = verts[i + 1]; verts_out[o + 2] = verts[i + 2];
    if (cols_out) { cols_out[o] = cols[i]; cols_out[o + 1] = cols[i + 1]; cols_out[o + 2] = cols[i + 2]; }
    if (normals_out) { normals_out[o] = normals[i]; normals_out[o + 1] = normals[i + 1]; normals_out[o + 2] = normals[i + 2]; }
    if (old_out) old_out[pos] = v;
  }
};

// stable compaction of the kept triangles: a triangle goes with its first index; out == null only counts
struct TriangleSrc {
  unsigned n_t, n_v;
  const unsigned* tri;
  const unsigned* remap;
  unsigned* out;                     // [kept][3]
  __device__ __forceinline__ unsigned at(unsigned i) const { return i < n_v ? remap[i] : DROPPED; }
  __device__ __forceinline__ unsigned size() const { return n_t; }
  __device__ __forceinline__ bool flag(unsigned t) const { return at(tri[3 * (size_t)t]) != DROPPED; }
  __device__ __forceinline__ void write(unsigned pos, unsigned t) const {
    const unsigned* in = tri + 3 * (size_t)t;
    unsigned* o = out + 3 * (size_t)pos;
    o[0] = at(in[0]); o[1] = at(in[1]); o[2] = at(in[2]);
  }
};

}  // namespace

struct rgbid_mesh {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0;
  SortWorkspace ws;                  // its compaction part; its bc is pointed at one of the three tile arrays below before a launch
  unsigned* bc_root = nullptr;       // [tiles of cap_v] the roots' tile offsets: from the label to the tables
  unsigned* bc_vert = nullptr;       // [tiles of cap_v] the kept vertices': from the select to the emits
  unsigned* bc_tri = nullptr;        // [tiles of cap_t] the kept triangles', likewise
  unsigned* parent = nullptr;        // [cap_v] after a label: the root of every vertex
  unsigned* vcount = nullptr;        // [cap_v] vertices per root
  unsigned* tcount = nullptr;        // [cap_v] triangles per root
  unsigned* number = nullptr;        // [cap_v] component number per root
  unsigned* remap = nullptr;         // [cap_v] after a select: the new index of a kept vertex, DROPPED elsewhere
  // the last labelling and selection
  bool labelled = false, selected = false;
  unsigned n_v = 0, n_t = 0, n_c = 0, kept_c = 0, kept_v = 0, kept_t = 0;
  const unsigned* tri = nullptr;
  // stage timing: label [0, 1], select [2, 3], emit [4, 5]
  bool timed[3] = {false, false, false};
  Buffers buf;
  StageTimer<6> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
  SortWorkspace& with(unsigned* bc) { ws.bc = bc; return ws; }
};

extern "C" {

int rgbid_mesh_create(rgbid_mesh** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles) {
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_MESH_MAX_VERTICES, RGBID_MESH_MAX_TRIANGLES, [&](rgbid_mesh* m) {
    const size_t cv = (size_t)max_vertices;
    int r = m->ws.alloc_compaction(m->buf, max_vertices);
    m->bc_root = m->ws.bc;
    if (!r) r = m->buf.alloc(&m->bc_vert, sizeof(unsigned) * ((cv + RUN_TILE - 1) / RUN_TILE));
    if (!r) r = m->buf.alloc(&m->bc_tri, sizeof(unsigned) * (((size_t)max_triangles + RUN_TILE - 1) / RUN_TILE));
    if (!r) r = m->buf.alloc(&m->parent, sizeof(unsigned) * cv);
    if (!r) r = m->buf.alloc(&m->vcount, sizeof(unsigned) * cv);
    if (!r) r = m->buf.alloc(&m->tcount, sizeof(unsigned) * cv);
    if (!r) r = m->buf.alloc(&m->number, sizeof(unsigned) * cv);
    if (!r) r = m->buf.alloc(&m->remap, sizeof(unsigned) * cv);
    return r;
  });
}

int rgbid_mesh_destroy(rgbid_mesh* m) { return destroy_handle(m); }   // a launch may still read the tables

int rgbid_mesh_label(rgbid_mesh* m, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                     unsigned long long* n_components) {
  if (!m || !n_components) return RGBID_E_INVALID;
  *n_components = 0;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, m->cap_v, m->cap_t)) return RGBID_E_INVALID;
  (void)hipSetDevice(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  m->labelled = m->selected = false;
  m->timed[0] = false;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  m->n_v = n_v; m->n_t = n_t; m->n_c = 0; m->tri = triangles_dev;
  if (n_v == 0) { m->labelled = true; return RGBID_OK; }   // no vertex, no triangle, no component
  const unsigned gv = grid_of(((unsigned long long)n_v + VT - 1) / VT), gt = grid_of(((unsigned long long)n_t + VT - 1) / VT);
  unsigned* bad = m->ws.slots + SLOT_BAD;
  m->mark(0);
  RGBID_HIP(hipMemsetAsync(m->ws.slots, 0, sizeof(unsigned) * SLOTS, s));
  if (n_t) check_triangles(s, triangles_dev, n_t, n_v, bad);
  hipLaunchKernelGGL(k_mesh_init, dim3(gv), dim3(VT), 0, s, n_v, m->parent, m->vcount, m->tcount, bad);
  if (n_t) hipLaunchKernelGGL(k_mesh_unite, dim3(gt), dim3(VT), 0, s, triangles_dev, n_t, n_v, m->parent, bad);
  if (n_t) hipLaunchKernelGGL(k_mesh_compress, dim3(gv), dim3(VT), 0, s, n_v, m->parent, bad);
  hipLaunchKernelGGL(k_mesh_flatten, dim3(gv), dim3(VT), 0, s, n_v, m->parent, m->vcount, bad);
  if (n_t) hipLaunchKernelGGL(k_mesh_tri_count, dim3(gt), dim3(VT), 0, s, triangles_dev, n_t, n_v, m->parent, m->tcount, bad);
  const RootSrc roots{n_v, m->parent, bad, m->number};
  m->with(m->bc_root).count_scan(s, roots, n_v, SLOT_COMPONENTS);
  m->with(m->bc_root).write(s, roots, n_v);
  m->mark(1);
  RGBID_HIP(hipGetLastError());
  if (int r = m->ws.read_slots(s)) return r;
  m->timed[0] = m->timer.on;
  if (m->ws.slots_host[SLOT_BAD]) return RGBID_E_INVALID;   // a triangle names a vertex that does not exist
  m->n_c = m->ws.slots_host[SLOT_COMPONENTS];
  m->labelled = true;
  *n_components = m->n_c;
  return RGBID_OK;
}

int rgbid_mesh_components(rgbid_mesh* m, uint32_t* table_dev, uint32_t* labels_dev) {
  if (!m || !m->labelled || !aligned4(table_dev) || !aligned4(labels_dev)) return RGBID_E_INVALID;
  if (m->n_v == 0 || (!table_dev && !labels_dev)) return RGBID_OK;
  (void)hipSetDevice(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  if (table_dev) m->with(m->bc_root).write(s, TableSrc{m->n_v, m->parent, m->vcount, m->tcount, table_dev}, m->n_v);
  if (labels_dev)
    hipLaunchKernelGGL(k_mesh_labels, dim3(grid_of(((unsigned long long)m->n_v + VT - 1) / VT)), dim3(VT), 0, s, m->n_v, m->parent, m->number, labels_dev);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_mesh_select(rgbid_mesh* m, uint32_t min_triangles, const uint8_t* keep_mask_dev, unsigned long long* kept_components,
                      unsigned long long* kept_vertices, unsigned long long* kept_triangles) {
  if (kept_components) *kept_components = 0;
  if (kept_vertices) *kept_vertices = 0;
  if (kept_triangles) *kept_triangles = 0;
  if (!m || !m->labelled) return RGBID_E_INVALID;
  m->selected = false;
  m->timed[1] = false;
  m->kept_c = m->kept_v = m->kept_t = 0;
  if (m->n_v == 0) { m->selected = true; return RGBID_OK; }
  (void)hipSetDevice(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  const unsigned n_v = m->n_v, n_t = m->n_t;
  m->mark(2);
  RGBID_HIP(hipMemsetAsync(m->ws.slots, 0, sizeof(unsigned) * SLOTS, s));
  hipLaunchKernelGGL(k_mesh_mark, dim3(grid_of(((unsigned long long)n_v + VT - 1) / VT)), dim3(VT), 0, s, n_v, m->parent, m->tcount, m->number,
                     (unsigned)min_triangles, keep_mask_dev, m->remap, m->ws.slots + SLOT_KEPT_C);
  const KeptVertexSrc kept{n_v, m->remap};
  m->with(m->bc_vert).count_scan(s, kept, n_v, SLOT_KEPT_V);
  m->with(m->bc_vert).write(s, kept, n_v);
  if (n_t) m->with(m->bc_tri).count_scan(s, TriangleSrc{n_t, n_v, m->tri, m->remap, nullptr}, n_t, SLOT_KEPT_T);
  m->mark(3);
  RGBID_HIP(hipGetLastError());
  if (int r = m->ws.read_slots(s)) return r;
  m->timed[1] = m->timer.on;
  m->kept_c = m->ws.slots_host[SLOT_KEPT_C];
  m->kept_v = m->ws.slots_host[SLOT_KEPT_V];
  m->kept_t = m->ws.slots_host[SLOT_KEPT_T];
  m->selected = true;
  if (kept_components) *kept_components = m->kept_c;
  if (kept_vertices) *kept_vertices = m->kept_v;
  if (kept_triangles) *kept_triangles = m->kept_t;
  return RGBID_OK;
}

int rgbid_mesh_emit(rgbid_mesh* m, const float* vertices_dev, const uint8_t* colours_dev, const float* normals_dev, float* vertices_out,
                    uint8_t* colours_out, float* normals_out, uint32_t* old_index_out, uint32_t* triangles_out,
                    unsigned long long vertex_capacity, unsigned long long triangle_capacity) {
  if (!m || !m->selected) return RGBID_E_INVALID;
  if ((colours_out && !colours_dev) || (normals_out && !normals_dev)) return RGBID_E_INVALID;
  if (!aligned4(normals_dev) || !aligned4(normals_out) || !aligned4(old_index_out)) return RGBID_E_INVALID;
  if (m->kept_v && (!vertices_dev || !vertices_out || !aligned4(vertices_dev) || !aligned4(vertices_out) || vertex_capacity < m->kept_v))
    return RGBID_E_INVALID;
  if (m->kept_t && (!triangles_out || !aligned4(triangles_out) || triangle_capacity < m->kept_t)) return RGBID_E_INVALID;
  m->timed[2] = false;
  if (m->kept_v == 0) return RGBID_OK;         // no kept vertex: no kept triangle either
  (void)hipSetDevice(m->ctx->device);
  hipStream_t s = m->ctx->stream;
  m->mark(4);
  m->with(m->bc_vert).write(s, VertexEmitSrc{m->n_v, m->remap, reinterpret_cast<const unsigned*>(vertices_dev), colours_dev,
                                             reinterpret_cast<const unsigned*>(normals_dev), reinterpret_cast<unsigned*>(vertices_out), colours_out,
                                             reinterpret_cast<unsigned*>(normals_out), old_index_out}, m->n_v);
  if (m->kept_t) m->with(m->bc_tri).write(s, TriangleSrc{m->n_t, m->n_v, m->tri, m->remap, triangles_out}, m->n_t);
  m->mark(5);
  RGBID_HIP(hipGetLastError());
  m->timed[2] = m->timer.on;
  return RGBID_OK;
}

int rgbid_mesh_timing(rgbid_mesh* m, int enable, float ms[3]) {
  if (!m) return RGBID_E_INVALID;
  (void)hipSetDevice(m->ctx->device);
  static const int pairs[3][4] = {{0, 1}, {2, 3}, {4, 5}};
  if (ms)
    if (int r = stage_times(m->timer, m->timed, pairs, ms)) return r;
  return m->timer.enable(enable != 0);
}

}  // extern "C"
