// kernels_holes.hip -- the small holes of an indexed triangle mesh in device memory found as loops of boundary half-edges and closed by a
// fan around one new vertex each (include/rgbid_holes.h).
//
// The judge is tests/holes_mirror.py; counts, loop table, status and the emitted mesh are byte-identical to it.
//   plan   k_mesh_check<false> mesh_device.h: counts the triangles with an index >= n_v, copied to the host: a bad index ends the call here
//          sort_rounds         voxel_device.h: one (key, item) pair per corner 3 t + c, keyed by the ends of its edge (a triangle with a
//                              repeated index gets the sentinel n_v), two stable rounds: by the larger end, then by the smaller.  Equal
//                              undirected edges are adjacent, the sentinels last
//          k_mesh_corner_ends  mesh_device.h: the larger end of the sorted corners beside their smaller end; counts the directed edges
//          flag compaction     over the runs of length one: boundary[rank] = the owner corner
//          k_holes_degrees     out(v), in(v) and the leaving owner: integer atomics (add, add, min), a function of the mesh alone
//          k_holes_vstats      counts the boundary vertices and those that are not simple
//          flag compaction     over out = in = 1: simple[rank] = v, rank_of[v] = rank           -> the host reads n_b and n_simple
//          k_holes_link        item i of the simple vertices: label i, jump to the item of succ(v), or the block bit
//          k_holes_label       bitlen(n_simple) Jacobi rounds between two buffers: the minimum label, the OR of the block bits, the jump
//          flag compaction     over the heads (not blocked, label = own item): the loops in ascending v_0
//          k_holes_cut / k_holes_rank   the same doubling over the cycles cut before v_0: the hops to the last vertex of the loop
//          value scan          over the loops' lengths: offsets, S
//          k_holes_table       loop_vertices and loop_owners at offset + rank
//   select k_holes_select      one thread per loop walks its vertices and owners in order (the order is the contract); the flag
//                              compaction's ranks and the value scan's bases over FILLED
//   emit   k_holes_fan, k_holes_caps   one thread per new triangle, one per new vertex; the inputs are copied as words
// No float atomics, no wait on another thread, every loop has its bound when it starts.
#include "../../include/rgbid_holes.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // the index check, the corners as edges, p3_load, cross3, the argument and overlap tests, the create;
                            // voxel_device.h's sort_rounds, flag compaction, value scan and unit_of; the sort workspace

#include <cstring>

using namespace rgbid;

namespace {

// the plan's slots beside the workspace's own 0 .. 8; SLOT_RUNS holds n_b, SLOT_VOXELS n_simple
enum { SLOT_BAD = 9, SLOT_DIRECTED = 10, SLOT_BVERTS = 11, SLOT_NONSIMPLE = 12, SLOT_LOOPS = 13, SLOT_INLOOPS = 14, SLOT_LONGEST = 15 };
// select's: SLOT_RUNS holds F, SLOT_VOXELS E
enum { SLOT_TOO_LONG = 9, SLOT_NOT_FINITE = 10, SLOT_OUTLINES = 11 };
static_assert(SLOT_VOXELS < SLOT_BAD && SLOT_LONGEST < SLOTS, "the slots of this file lie behind the workspace's");

constexpr unsigned BLOCKED = 0x80000000u;   // the top bit of a jump: the chain runs into a vertex that is not simple
constexpr unsigned NONE = 0xFFFFFFFFu;

// ---- boundary half-edges ------------------------------------------------------------------------------------------------------------
// the flag compaction's source: sorted corner m is a run of length one of its undirected edge -> boundary[rank] = its corner
struct LoneSrc {
  const unsigned* los;
  const unsigned* his;
  const unsigned* order;
  unsigned n, n_v;
  unsigned* boundary;
  __device__ __forceinline__ unsigned size() const { return n; }
  __device__ __forceinline__ bool flag(unsigned m) const {
    const unsigned lo = los[m], hi = his[m];
    if (lo >= n_v) return false;
    const bool first = m == 0 || los[m - 1] != lo || his[m - 1] != hi;
    const bool last = m + 1 >= n || los[m + 1] != lo || his[m + 1] != hi;
    return first && last;
  }
  __device__ __forceinline__ void write(unsigned pos, unsigned m) const { boundary[pos] = order[m]; }
};

// ---- degrees and successors -----------------------------------------------------------------------------------------------------------
// one thread per boundary half-edge (*n_b of them): integer atomics only, so the three words of a vertex are a function of the mesh
__global__ __launch_bounds__(VT) void k_holes_degrees(CornerView view, const unsigned* __restrict__ boundary, const unsigned* __restrict__ n_b,
                                                      unsigned* __restrict__ out_cnt, unsigned* __restrict__ in_cnt, unsigned* __restrict__ out_owner) {
  const unsigned n = *n_b;
  for (size_t j = (size_t)blockIdx.x * VT + threadIdx.x; j < n; j += (size_t)gridDim.x * VT) {
    const unsigned corner = boundary[j];
    unsigned a, b;
    if (!view.ends(corner, a, b)) continue;
    atomicAdd(out_cnt + a, 1u);
    atomicAdd(in_cnt + b, 1u);
    atomicMin(out_owner + a, corner);
  }
}

__global__ __launch_bounds__(VT) void k_holes_vstats(const unsigned* __restrict__ out_cnt, const unsigned* __restrict__ in_cnt, unsigned n_v,
                                                     unsigned* __restrict__ slots) {
  unsigned bverts = 0, nonsimple = 0;
  for (size_t v = (size_t)blockIdx.x * VT + threadIdx.x; v < n_v; v += (size_t)gridDim.x * VT) {
    const unsigned o = out_cnt[v], i = in_cnt[v];
    bverts += (o | i) != 0;
    nonsimple += (o | i) != 0 && !(o == 1 && i == 1);
  }
  wave_add_to(slots + SLOT_BVERTS, bverts);
  wave_add_to(slots + SLOT_NONSIMPLE, nonsimple);
}

struct SimpleSrc {
  const unsigned* out_cnt;
  const unsigned* in_cnt;
  unsigned n_v;
  unsigned* simple;                  // [rank] = v
  unsigned* rank_of;                 // [v] = rank, written for the simple vertices only
  __device__ __forceinline__ unsigned size() const { return n_v; }
  __device__ __forceinline__ bool flag(unsigned v) const { return out_cnt[v] == 1 && in_cnt[v] == 1; }
  __device__ __forceinline__ void write(unsigned pos, unsigned v) const { simple[pos] = v; rank_of[v] = pos; }
};

// ---- loops ----------------------------------------------------------------------------------------------------------------------------
// what the doubling kernels know of the simple vertices
struct Chain {
  CornerView view;
  const unsigned* out_cnt;
  const unsigned* in_cnt;
  const unsigned* out_owner;
  const unsigned* rank_of;
  const unsigned* simple;
  unsigned n_s;
  // the item of succ(simple[i]), or NONE when that vertex is not simple
  __device__ __forceinline__ unsigned next(unsigned i) const {
    const unsigned v = simple[i];
    if (v >= view.n_v) return NONE;
    unsigned a, b;
    if (!view.ends(out_owner[v], a, b)) return NONE;
    if (!(out_cnt[b] == 1 && in_cnt[b] == 1)) return NONE;
    const unsigned j = rank_of[b];
    return j < n_s ? j : NONE;
  }
};

__global__ __launch_bounds__(VT) void k_holes_link(Chain ch, unsigned* __restrict__ lab, unsigned* __restrict__ jump) {
  const size_t i = (size_t)blockIdx.x * VT + threadIdx.x;
  if (i >= ch.n_s) return;
  const unsigned j = ch.next((unsigned)i);
  lab[i] = (unsigned)i;
  jump[i] = j == NONE ? ((unsigned)i | BLOCKED) : j;
}

// one Jacobi round: every item takes the minimum label, the OR of the block bits and the jump of the item it jumps to
__global__ __launch_bounds__(VT) void k_holes_label(const unsigned* __restrict__ lab, const unsigned* __restrict__ jump, unsigned* __restrict__ lab_out,
                                                    unsigned* __restrict__ jump_out, unsigned n_s) {
  const size_t i = (size_t)blockIdx.x * VT + threadIdx.x;
  if (i >= n_s) return;
  const unsigned j = jump[i], to = j & ~BLOCKED;
  unsigned l = lab[i], jj = j;
  if (to < n_s) {
    l = min(l, lab[to]);
    const unsigned far = jump[to];
    jj = (far & ~BLOCKED) | ((j | far) & BLOCKED);
  }
  lab_out[i] = l;
  jump_out[i] = jj;
}

// the heads of the loops: items that are not blocked and carry their own label -> heads[loop] = item, loop_of[item] = loop
struct HeadItemSrc {
  const unsigned* lab;
  const unsigned* jump;
  unsigned n_s, cap_l;               // cap_l: the loops the tables hold, n_s / 3 at most when the labels are right
  unsigned* heads;
  unsigned* loop_of;
  __device__ __forceinline__ unsigned size() const { return n_s; }
  __device__ __forceinline__ bool flag(unsigned i) const { return !(jump[i] & BLOCKED) && lab[i] == i; }
  __device__ __forceinline__ void write(unsigned pos, unsigned i) const {
    loop_of[i] = pos;
    if (pos < cap_l) heads[pos] = i;
  }
};

// the cycles cut before their heads: an item in a loop whose successor is not the head is one hop from it, every other item ends a list
__global__ __launch_bounds__(VT) void k_holes_cut(Chain ch, const unsigned* __restrict__ lab, const unsigned* __restrict__ jump, unsigned* __restrict__ hops,
                                                  unsigned* __restrict__ to) {
  const size_t i = (size_t)blockIdx.x * VT + threadIdx.x;
  if (i >= ch.n_s) return;
  unsigned h = 0, t = (unsigned)i;
  if (!(jump[i] & BLOCKED)) {
    const unsigned j = ch.next((unsigned)i);
    if (j != NONE && j != lab[i]) { h = 1; t = j; }
  }
  hops[i] = h;
  to[i] = t;
}

// one Jacobi round of the list ranking: the hops to the end of the list
__global__ __launch_bounds__(VT) void k_holes_rank(const unsigned* __restrict__ hops, const unsigned* __restrict__ to, unsigned* __restrict__ hops_out,
                                                   unsigned* __restrict__ to_out, unsigned n_s) {
  const size_t i = (size_t)blockIdx.x * VT + threadIdx.x;
  if (i >= n_s) return;
  const unsigned t = to[i];
  unsigned h = hops[i], tt = t;
  if (t < n_s) { h += hops[t]; tt = to[t]; }
  hops_out[i] = h;
  to_out[i] = tt;
}

// the loops' lengths -> offsets[loop], offsets[L] behind the last; the longest loop
struct LengthSrc {
  const unsigned* heads;
  const unsigned* hops;
  const unsigned* n_loops;           // device slot
  unsigned n_s, cap_l;
  unsigned* offsets;
  unsigned* longest;
  __device__ __forceinline__ unsigned size() const { return min(*n_loops, cap_l); }
  __device__ __forceinline__ unsigned value(unsigned l) const {
    const unsigned i = heads[l];
    return i < n_s ? hops[i] + 1u : 0u;
  }
  __device__ __forceinline__ void write(unsigned l, unsigned before, unsigned k) const {
    offsets[l] = before;
    if (l + 1 == size()) offsets[l + 1] = before + k;
    atomicMax(longest, k);
  }
};

// every item in a loop writes its vertex and its owner at offset + rank; the rank is the head's hops less its own
__global__ __launch_bounds__(VT) void k_holes_table(const unsigned* __restrict__ simple, const unsigned* __restrict__ out_owner, const unsigned* __restrict__ lab,
                                                    const unsigned* __restrict__ jump, const unsigned* __restrict__ hops, const unsigned* __restrict__ loop_of,
                                                    const unsigned* __restrict__ offsets, const unsigned* __restrict__ n_loops, unsigned n_s, unsigned n_v,
                                                    unsigned cap_l, unsigned* __restrict__ loop_vertices, unsigned* __restrict__ loop_owners) {
  const size_t i = (size_t)blockIdx.x * VT + threadIdx.x;
  if (i >= n_s || (jump[i] & BLOCKED)) return;
  const unsigned head = lab[i];
  if (head >= n_s) return;
  const unsigned l = loop_of[head];
  if (l >= min(*n_loops, cap_l)) return;
  const unsigned k = offsets[l + 1] - offsets[l], rank = hops[head] - hops[i];
  const unsigned v = simple[i];
  if (rank >= k || offsets[l] + rank >= n_s || v >= n_v) return;   // a loop table has a row per simple vertex at most
  loop_vertices[offsets[l] + rank] = v;
  loop_owners[offsets[l] + rank] = out_owner[v];
}

// ---- select ---------------------------------------------------------------------------------------------------------------------------
// acc += u x w, the three sums one add each
__device__ __forceinline__ void cross_add(double acc[3], const double u[3], const double w[3]) {
  RGBID_FP_STRICT
  double c[3];
  cross3(u, w, c);
  acc[0] += c[0]; acc[1] += c[1]; acc[2] += c[2];
}

// One thread per loop: the order of the sums is the contract, so a loop is not split across lanes.  The walk is bounded by k, which is
// at most max_edges when it begins
__global__ __launch_bounds__(VT) void k_holes_select(const float* __restrict__ pos, const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v,
                                                     const unsigned* __restrict__ offsets, const unsigned* __restrict__ loop_vertices,
                                                     const unsigned* __restrict__ loop_owners, unsigned n_loops, unsigned max_edges, unsigned any_facing,
                                                     unsigned char* __restrict__ status, float* __restrict__ centres, unsigned* __restrict__ slots) {
  RGBID_FP_STRICT
  const size_t l = (size_t)blockIdx.x * VT + threadIdx.x;
  unsigned st = NONE;
  if (l < n_loops) {
    const unsigned b = offsets[l], k = offsets[l + 1] - b;
    st = RGBID_HOLES_FILLED;
    if (k > max_edges) st = RGBID_HOLES_TOO_LONG;
    else {
      double s[3] = {0, 0, 0};
      bool finite = true;
      for (unsigned i = 0; i < k; ++i) {
        const P3 q = p3_load(pos, loop_vertices[b + i], n_v);
        finite = finite && q.finite;
        for (int a = 0; a < 3; ++a) s[a] += q.p[a];
      }
      float m[3];
      const double dk = (double)k;
      for (int a = 0; a < 3; ++a) m[a] = (float)(s[a] / dk);
      for (int a = 0; a < 3; ++a) centres[3 * l + a] = m[a];
      if (!finite) st = RGBID_HOLES_NOT_FINITE;
      else if (!any_facing) {
        const double c[3] = {(double)m[0], (double)m[1], (double)m[2]};
        double A[3] = {0, 0, 0}, N[3] = {0, 0, 0};
        P3 pi = p3_load(pos, loop_vertices[b], n_v);
        for (unsigned i = 0; i < k; ++i) {
          const P3 pn = p3_load(pos, loop_vertices[b + (i + 1 == k ? 0u : i + 1)], n_v);
          double u[3], w[3];
          for (int a = 0; a < 3; ++a) { u[a] = pi.p[a] - pn.p[a]; w[a] = c[a] - pn.p[a]; }
          cross_add(A, u, w);
          const unsigned t = loop_owners[b + i] / 3u;
          P3 q0 = {{NAN, NAN, NAN}, false}, q1 = q0, q2 = q0;
          if (t < n_t) {
            q0 = p3_load(pos, tri[3 * (size_t)t], n_v);
            q1 = p3_load(pos, tri[3 * (size_t)t + 1], n_v);
            q2 = p3_load(pos, tri[3 * (size_t)t + 2], n_v);
          }
          for (int a = 0; a < 3; ++a) { u[a] = q1.p[a] - q0.p[a]; w[a] = q2.p[a] - q0.p[a]; }
          cross_add(N, u, w);
          pi = pn;
        }
        const double dot = (A[0] * N[0] + A[1] * N[1]) + A[2] * N[2];
        if (!(dot > 0.0)) st = RGBID_HOLES_OUTLINE;
      }
    }
    status[l] = (unsigned char)st;
  }
  unsigned too_long = st == RGBID_HOLES_TOO_LONG, not_finite = st == RGBID_HOLES_NOT_FINITE, outlines = st == RGBID_HOLES_OUTLINE;
  too_long = wave_sum(too_long);
  not_finite = wave_sum(not_finite);
  outlines = wave_sum(outlines);
  if ((threadIdx.x & 63) == 0) {     // three counts behind one branch
    if (too_long) atomicAdd(slots + SLOT_TOO_LONG, too_long);
    if (not_finite) atomicAdd(slots + SLOT_NOT_FINITE, not_finite);
    if (outlines) atomicAdd(slots + SLOT_OUTLINES, outlines);
  }
}

// the filled loops: filled[rank] = loop, fill_rank[loop] = rank
struct FilledSrc {
  const unsigned char* status;
  unsigned n_loops;
  unsigned* filled;
  unsigned* fill_rank;
  __device__ __forceinline__ unsigned size() const { return n_loops; }
  __device__ __forceinline__ bool flag(unsigned l) const { return status[l] == RGBID_HOLES_FILLED; }
  __device__ __forceinline__ void write(unsigned pos, unsigned l) const { filled[pos] = l; fill_rank[l] = pos; }
};

// the filled loops' lengths -> bases[loop], the exclusive sum; bases[L] = E
struct BaseSrc {
  const unsigned char* status;
  const unsigned* offsets;
  unsigned n_loops;
  unsigned* bases;
  __device__ __forceinline__ unsigned size() const { return n_loops; }
  __device__ __forceinline__ unsigned value(unsigned l) const { return status[l] == RGBID_HOLES_FILLED ? offsets[l + 1] - offsets[l] : 0u; }
  __device__ __forceinline__ void write(unsigned l, unsigned before, unsigned k) const {
    bases[l] = before;
    if (l + 1 == n_loops) bases[l + 1] = before + k;
  }
};

// ---- emit -----------------------------------------------------------------------------------------------------------------------------
// one thread per new triangle e < n_new: its loop is the last whose base is not above e (the loops that are not filled have no width and
// lie before it), 32 halvings at most -> the row (v_(i+1), v_i, n_v + rank) at n_t + e
__global__ __launch_bounds__(VT) void k_holes_fan(const unsigned* __restrict__ bases, const unsigned* __restrict__ offsets, const unsigned* __restrict__ fill_rank,
                                                  const unsigned* __restrict__ loop_vertices, unsigned n_loops, unsigned n_new, unsigned n_v, unsigned n_t,
                                                  unsigned* __restrict__ tri_out) {
  for (size_t e = (size_t)blockIdx.x * VT + threadIdx.x; e < n_new; e += (size_t)gridDim.x * VT) {
    unsigned lo = 0, hi = n_loops;     // the first loop whose base is above e
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      if (bases[mid] <= e) lo = mid + 1; else hi = mid;
    }
    if (lo == 0) continue;
    const unsigned l = lo - 1, b = offsets[l], k = offsets[l + 1] - b, i = (unsigned)e - bases[l];
    if (i >= k) continue;
    const size_t row = 3 * ((size_t)n_t + e);
    tri_out[row] = loop_vertices[b + (i + 1 == k ? 0u : i + 1)];
    tri_out[row + 1] = loop_vertices[b + i];
    tri_out[row + 2] = n_v + fill_rank[l];
  }
}

// one thread per new vertex r < n_filled: the centre, the rounded mean colour, the unit sum of the normals in loop order
__global__ __launch_bounds__(VT) void k_holes_caps(const unsigned* __restrict__ filled, const unsigned* __restrict__ offsets, const unsigned* __restrict__ loop_vertices,
                                                   const float* __restrict__ centres, unsigned n_filled, unsigned n_loops, unsigned n_v,
                                                   const unsigned char* __restrict__ col_in, const float* __restrict__ nrm_in, float* __restrict__ pos_out,
                                                   unsigned char* __restrict__ col_out, float* __restrict__ nrm_out) {
  RGBID_FP_STRICT
  const size_t r = (size_t)blockIdx.x * VT + threadIdx.x;
  if (r >= n_filled) return;
  const unsigned l = filled[r];
  if (l >= n_loops) return;
  const unsigned b = offsets[l], k = offsets[l + 1] - b;
  const size_t o = 3 * ((size_t)n_v + r);
  for (int a = 0; a < 3; ++a) pos_out[o + a] = centres[3 * (size_t)l + a];
  if (col_out) {
    unsigned long long sum[3] = {0, 0, 0};
    for (unsigned i = 0; i < k; ++i) {
      const unsigned v = loop_vertices[b + i];
      if (v < n_v) for (int a = 0; a < 3; ++a) sum[a] += col_in[3 * (size_t)v + a];
    }
    for (int a = 0; a < 3; ++a) col_out[o + a] = k ? (unsigned char)((2ull * sum[a] + k) / (2ull * k)) : 0;
  }
  if (nrm_out) {
    double s[3] = {0, 0, 0};
    for (unsigned i = 0; i < k; ++i) {
      const unsigned v = loop_vertices[b + i];
      if (v < n_v) for (int a = 0; a < 3; ++a) s[a] += (double)nrm_in[3 * (size_t)v + a];
    }
    float n[3];
    unit_of(s, n);
    for (int a = 0; a < 3; ++a) nrm_out[o + a] = n[a];
  }
}

}  // namespace

struct rgbid_holes {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0;
  SortWorkspace w;                   // 3 cap_t items: the corner sort, then the buffers of the doubling
  unsigned* out_cnt = nullptr;       // [cap_v]
  unsigned* in_cnt = nullptr;        // [cap_v]
  unsigned* out_owner = nullptr;     // [cap_v]
  unsigned* rank_of = nullptr;       // [cap_v]
  unsigned* simple = nullptr;        // [cap_s] cap_s = min(cap_v, 3 cap_t)
  unsigned* loop_of = nullptr;       // [cap_s]
  unsigned* loop_vertices = nullptr; // [cap_s]
  unsigned* loop_owners = nullptr;   // [cap_s]
  unsigned* offsets = nullptr;       // [cap_l + 1] cap_l = cap_s / 3 + 1
  unsigned* bases = nullptr;         // [cap_l + 1]
  unsigned* heads = nullptr;         // [cap_l]; select's filled loops by rank
  unsigned* fill_rank = nullptr;     // [cap_l]
  unsigned char* status = nullptr;   // [cap_l]
  float* centres = nullptr;          // [cap_l][3]
  // the last plan and the last selection
  bool planned = false, selected = false;
  unsigned n_v = 0, n_t = 0, n_loops = 0, n_inloops = 0, n_filled = 0, n_new = 0;
  const unsigned* tri = nullptr;
  // stage timing: check [0, 1], the rest of the plan [2, 3], select [4, 5], emit [6, 7]
  bool timed[3] = {false, false, false};
  Buffers buf;
  StageTimer<8> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

// step 2 and the degrees of step 3: everything the host has to read before it knows the number of rounds
void boundary_stage(rgbid_holes* h) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  const unsigned n_v = h->n_v;
  const CornerView view{h->tri, h->n_t, n_v, 3ull * h->n_t};
  const unsigned items = (unsigned)view.items;
  const int p = w.sort_rounds(s, CornerKey{view}, n_v, items, {0, 1});   // by the larger end, then by the smaller
  unsigned* his = w.keys_as<unsigned>(p ^ 1);
  hipLaunchKernelGGL(k_mesh_corner_ends<true>, dim3(grid_of(blocks_of(items))), dim3(VT), 0, s, view, w.idx[p], his, w.slots + SLOT_DIRECTED);
  unsigned* boundary = w.idx[p ^ 1];
  const LoneSrc lone{w.keys_as<unsigned>(p), his, w.idx[p], items, n_v, boundary};
  w.count_scan(s, lone, items, SLOT_RUNS);
  w.write(s, lone, items);
  (void)hipMemsetAsync(h->out_cnt, 0, sizeof(unsigned) * (size_t)n_v, s);
  (void)hipMemsetAsync(h->in_cnt, 0, sizeof(unsigned) * (size_t)n_v, s);
  (void)hipMemsetAsync(h->out_owner, 0xFF, sizeof(unsigned) * (size_t)n_v, s);
  hipLaunchKernelGGL(k_holes_degrees, dim3(grid_of(blocks_of(items))), dim3(VT), 0, s, view, boundary, w.slots + SLOT_RUNS, h->out_cnt, h->in_cnt,
                     h->out_owner);
  hipLaunchKernelGGL(k_holes_vstats, dim3(grid_of(blocks_of(n_v))), dim3(VT), 0, s, h->out_cnt, h->in_cnt, n_v, w.slots);
  const SimpleSrc simple{h->out_cnt, h->in_cnt, n_v, h->simple, h->rank_of};
  w.count_scan(s, simple, n_v, SLOT_VOXELS);
  w.write(s, simple, n_v);
}

// the rest of step 3 over the n_s simple vertices.  The sort's four buffers are free again: two halves of each key buffer hold the labels
// and the jumps, then the jumps' halves and the index buffers hold the list ranking
void loop_stage(rgbid_holes* h, unsigned n_s) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  const CornerView view{h->tri, h->n_t, h->n_v, 3ull * h->n_t};
  const Chain ch{view, h->out_cnt, h->in_cnt, h->out_owner, h->rank_of, h->simple, n_s};
  const size_t half = (size_t)w.cap;
  unsigned* lab[2] = {w.keys_as<unsigned>(0), w.keys_as<unsigned>(0) + half};
  unsigned* jump[2] = {w.keys_as<unsigned>(1), w.keys_as<unsigned>(1) + half};
  const unsigned blocks = blocks_of(n_s);
  const int rounds = bitlen(n_s);
  int p = 0;
  hipLaunchKernelGGL(k_holes_link, dim3(blocks), dim3(VT), 0, s, ch, lab[0], jump[0]);
  for (int j = 0; j < rounds; ++j, p ^= 1)
    hipLaunchKernelGGL(k_holes_label, dim3(blocks), dim3(VT), 0, s, lab[p], jump[p], lab[p ^ 1], jump[p ^ 1], n_s);
  const unsigned cap_l = n_s / 3u + 1u;                      // within the tables: the create sized them for min(cap_v, 3 cap_t) / 3 + 1
  const HeadItemSrc head{lab[p], jump[p], n_s, cap_l, h->heads, h->loop_of};
  w.count_scan(s, head, n_s, SLOT_LOOPS);
  w.write(s, head, n_s);
  unsigned* hops[2] = {w.idx[0], w.idx[1]};
  unsigned* to[2] = {jump[p ^ 1], lab[p ^ 1]};
  int q = 0;
  hipLaunchKernelGGL(k_holes_cut, dim3(blocks), dim3(VT), 0, s, ch, lab[p], jump[p], hops[0], to[0]);
  for (int j = 0; j < rounds; ++j, q ^= 1)
    hipLaunchKernelGGL(k_holes_rank, dim3(blocks), dim3(VT), 0, s, hops[q], to[q], hops[q ^ 1], to[q ^ 1], n_s);
  const LengthSrc len{h->heads, hops[q], w.slots + SLOT_LOOPS, n_s, cap_l, h->offsets, w.slots + SLOT_LONGEST};
  w.value_scan(s, len, cap_l, SLOT_INLOOPS);
  hipLaunchKernelGGL(k_holes_table, dim3(blocks), dim3(VT), 0, s, h->simple, h->out_owner, lab[p], jump[p], hops[q], h->loop_of, h->offsets,
                     w.slots + SLOT_LOOPS, n_s, h->n_v, cap_l, h->loop_vertices, h->loop_owners);
}

}  // namespace

extern "C" {

int rgbid_holes_create(rgbid_holes** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles) {
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_HOLES_MAX_VERTICES, RGBID_HOLES_MAX_TRIANGLES, [&](rgbid_holes* h) {
    const size_t cv = (size_t)max_vertices;
    const unsigned long long corners = 3ull * max_triangles;
    const size_t cs = (size_t)(max_vertices < corners ? max_vertices : corners), cl = cs / 3 + 1;
    int r = h->w.alloc(h->buf, corners);
    if (!r && max_vertices > corners) {                      // the compaction of the simple vertices runs over the vertices
      h->w.run_tiles = (unsigned)((max_vertices + RUN_TILE - 1) / RUN_TILE);
      r = h->buf.alloc(&h->w.bc, sizeof(unsigned) * h->w.run_tiles);
    }
    if (!r) r = h->buf.alloc(&h->out_cnt, sizeof(unsigned) * cv);
    if (!r) r = h->buf.alloc(&h->in_cnt, sizeof(unsigned) * cv);
    if (!r) r = h->buf.alloc(&h->out_owner, sizeof(unsigned) * cv);
    if (!r) r = h->buf.alloc(&h->rank_of, sizeof(unsigned) * cv);
    if (!r) r = h->buf.alloc(&h->simple, sizeof(unsigned) * cs);
    if (!r) r = h->buf.alloc(&h->loop_of, sizeof(unsigned) * cs);
    if (!r) r = h->buf.alloc(&h->loop_vertices, sizeof(unsigned) * cs);
    if (!r) r = h->buf.alloc(&h->loop_owners, sizeof(unsigned) * cs);
    if (!r) r = h->buf.alloc(&h->offsets, sizeof(unsigned) * (cl + 1));
    if (!r) r = h->buf.alloc(&h->bases, sizeof(unsigned) * (cl + 1));
    if (!r) r = h->buf.alloc(&h->heads, sizeof(unsigned) * cl);
    if (!r) r = h->buf.alloc(&h->fill_rank, sizeof(unsigned) * cl);
    if (!r) r = h->buf.alloc(&h->status, cl);
    if (!r) r = h->buf.alloc(&h->centres, sizeof(float) * 3 * cl);
    return r;
  });
}

int rgbid_holes_destroy(rgbid_holes* h) { return destroy_handle(h); }   // an emit may still read the tables

int rgbid_holes_plan(rgbid_holes* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                     unsigned long long counts[8]) {
  if (!h) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  if (counts) for (int i = 0; i < 8; ++i) counts[i] = 0;
  h->planned = h->selected = false;
  h->timed[0] = false;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  h->n_v = n_v; h->n_t = n_t; h->n_loops = h->n_inloops = h->n_filled = h->n_new = 0;
  h->tri = triangles_dev;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  RGBID_HIP(hipMemsetAsync(h->offsets, 0, sizeof(unsigned), s));     // a plan without loops: a table of one zero
  if (n_t == 0) {                                                    // no triangle: no half-edge
    h->planned = true;
    return RGBID_OK;
  }
  h->mark(0);
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, s));
  check_triangles<false>(s, triangles_dev, n_t, n_v, w.slots + SLOT_BAD);
  h->mark(1);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  if (w.slots_host[SLOT_BAD]) return RGBID_E_INVALID;                // a triangle names a vertex that does not exist
  h->mark(2);
  boundary_stage(h);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  const unsigned n_b = w.slots_host[SLOT_RUNS], n_s = w.slots_host[SLOT_VOXELS];
  if (n_s) loop_stage(h, n_s);
  h->mark(3);
  RGBID_HIP(hipGetLastError());
  if (n_s)
    if (int r = w.read_slots(s)) return r;
  h->timed[0] = h->timer.on;
  h->n_loops = w.slots_host[SLOT_LOOPS];
  h->n_inloops = w.slots_host[SLOT_INLOOPS];
  if (h->n_loops > n_s / 3u || h->n_inloops > n_s) return RGBID_E_INVALID;   // never with labels that are right; the tables were not written past their rows
  if (counts) {
    counts[0] = w.slots_host[SLOT_DIRECTED];
    counts[1] = n_b;
    counts[2] = w.slots_host[SLOT_BVERTS];
    counts[3] = w.slots_host[SLOT_NONSIMPLE];
    counts[4] = h->n_loops;
    counts[5] = h->n_inloops;
    counts[6] = n_b - h->n_inloops;
    counts[7] = w.slots_host[SLOT_LONGEST];
  }
  h->planned = true;
  return RGBID_OK;
}

int rgbid_holes_loops(rgbid_holes* h, uint32_t* offsets_out, uint32_t* vertices_out, uint32_t* owners_out, uint8_t* status_out,
                      unsigned long long capacity) {
  if (!h || !h->planned || capacity < h->n_inloops || (status_out && !h->selected)) return RGBID_E_INVALID;
  if (!aligned4(offsets_out) || !aligned4(vertices_out) || !aligned4(owners_out)) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const size_t rows = sizeof(unsigned) * (size_t)h->n_inloops;
  if (offsets_out) RGBID_HIP(hipMemcpyAsync(offsets_out, h->offsets, sizeof(unsigned) * ((size_t)h->n_loops + 1), hipMemcpyDeviceToDevice, s));
  if (vertices_out && rows) RGBID_HIP(hipMemcpyAsync(vertices_out, h->loop_vertices, rows, hipMemcpyDeviceToDevice, s));
  if (owners_out && rows) RGBID_HIP(hipMemcpyAsync(owners_out, h->loop_owners, rows, hipMemcpyDeviceToDevice, s));
  if (status_out && h->n_loops) RGBID_HIP(hipMemcpyAsync(status_out, h->status, (size_t)h->n_loops, hipMemcpyDeviceToDevice, s));
  return RGBID_OK;
}

int rgbid_holes_select(rgbid_holes* h, const float* vertices_dev, unsigned max_edges, uint32_t flags, unsigned long long counts[5]) {
  if (!h || !h->planned || (flags & ~RGBID_HOLES_ANY_FACING)) return RGBID_E_INVALID;
  if (max_edges < RGBID_HOLES_MIN_EDGES || max_edges > RGBID_HOLES_MAX_EDGES) return RGBID_E_INVALID;
  if (h->n_v && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  if (counts) for (int i = 0; i < 5; ++i) counts[i] = 0;
  h->selected = false;
  h->timed[1] = false;
  h->n_filled = h->n_new = 0;
  const unsigned n_l = h->n_loops;
  if (n_l == 0) {                                                    // no loop: nothing to decide
    h->selected = true;
    return RGBID_OK;
  }
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  h->mark(4);
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, s));
  hipLaunchKernelGGL(k_holes_select, dim3(blocks_of(n_l)), dim3(VT), 0, s, vertices_dev, h->tri, h->n_t, h->n_v, h->offsets, h->loop_vertices, h->loop_owners,
                     n_l, max_edges, (unsigned)(flags & RGBID_HOLES_ANY_FACING), h->status, h->centres, w.slots);
  const FilledSrc filled{h->status, n_l, h->heads, h->fill_rank};
  w.count_scan(s, filled, n_l, SLOT_RUNS);
  w.write(s, filled, n_l);
  const BaseSrc base{h->status, h->offsets, n_l, h->bases};
  w.value_scan(s, base, n_l, SLOT_VOXELS);
  h->mark(5);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  h->timed[1] = h->timer.on;
  const unsigned long long n_filled = w.slots_host[SLOT_RUNS], n_new = w.slots_host[SLOT_VOXELS];
  if (counts) {
    counts[0] = w.slots_host[SLOT_TOO_LONG];
    counts[1] = w.slots_host[SLOT_NOT_FINITE];
    counts[2] = w.slots_host[SLOT_OUTLINES];
    counts[3] = n_filled;
    counts[4] = n_new;
  }
  if (h->n_v + n_filled > RGBID_HOLES_MAX_VERTICES || h->n_t + n_new > RGBID_HOLES_MAX_TRIANGLES) return RGBID_E_INVALID;
  h->n_filled = (unsigned)n_filled;
  h->n_new = (unsigned)n_new;
  h->selected = true;
  return RGBID_OK;
}

int rgbid_holes_emit(rgbid_holes* h, const float* vertices_in, const uint8_t* colours_in, const float* normals_in, const uint32_t* triangles_in,
                     float* vertices_out, uint8_t* colours_out, float* normals_out, uint32_t* triangles_out, unsigned long long vertex_capacity,
                     unsigned long long triangle_capacity) {
  if (!h || !h->planned || !h->selected) return RGBID_E_INVALID;
  if (!colours_in != !colours_out || !normals_in != !normals_out) return RGBID_E_INVALID;
  const unsigned long long rows_v = (unsigned long long)h->n_v + h->n_filled, rows_t = (unsigned long long)h->n_t + h->n_new;
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
      overlap(colours_in, 3 * in_v, colours_out, 3 * (size_t)rows_v) || overlap(triangles_in, 12 * in_t, triangles_out, 12 * (size_t)rows_t))
    return RGBID_E_INVALID;
  h->timed[2] = false;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  h->mark(6);
  if (in_v) {
    RGBID_HIP(hipMemcpyAsync(vertices_out, vertices_in, 12 * in_v, hipMemcpyDeviceToDevice, s));
    if (colours_out) RGBID_HIP(hipMemcpyAsync(colours_out, colours_in, 3 * in_v, hipMemcpyDeviceToDevice, s));
    if (normals_out) RGBID_HIP(hipMemcpyAsync(normals_out, normals_in, 12 * in_v, hipMemcpyDeviceToDevice, s));
  }
  if (in_t) RGBID_HIP(hipMemcpyAsync(triangles_out, triangles_in, 12 * in_t, hipMemcpyDeviceToDevice, s));
  if (h->n_filled) {
    hipLaunchKernelGGL(k_holes_fan, dim3(grid_of(blocks_of(h->n_new))), dim3(VT), 0, s, h->bases, h->offsets, h->fill_rank, h->loop_vertices, h->n_loops,
                       h->n_new, h->n_v, h->n_t, triangles_out);
    hipLaunchKernelGGL(k_holes_caps, dim3(blocks_of(h->n_filled)), dim3(VT), 0, s, h->heads, h->offsets, h->loop_vertices, h->centres, h->n_filled,
                       h->n_loops, h->n_v, colours_in, normals_in, vertices_out, colours_out, normals_out);
  }
  h->mark(7);
  RGBID_HIP(hipGetLastError());
  h->timed[2] = h->timer.on;
  return RGBID_OK;
}

int rgbid_holes_timing(rgbid_holes* h, int enable, float ms[3]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  static const int pairs[3][4] = {{0, 1, 2, 3}, {4, 5}, {6, 7}};   // the plan: the check and the rest
  if (ms)
    if (int r = stage_times(h->timer, h->timed, pairs, ms)) return r;
  return h->timer.enable(enable != 0);
}

}  // extern "C"
