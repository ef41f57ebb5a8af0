// kernels_denoise.hip -- an indexed triangle mesh in device memory denoised with its sharp edges kept: the face normals are filtered over
// the faces that share a vertex with them, with the weight (n_i . n_j - T)^2 above the threshold T and nothing below it, and the vertices
// are moved along the filtered normals of their faces (include/rgbid_denoise.h).
//
// The judge is tests/denoise_mirror.py; counts, face table, normals and positions are byte-identical to it.
//   plan     k_mesh_check<false>     mesh_device.h: counts the triangles with an index >= n_v into a slot copied to the host: a bad index ends
//                                    the call here
//            k_mesh_corner_keys      mesh_device.h: one (vertex, corner) pair per corner, one stable sort_bits by bitlen(n_v) bits
//            k_denoise_faces         faces[i] = the sorted corner / 3
//            k_mesh_offsets<false>   mesh_device.h: offsets[w] = the corners of the vertices below w: a bounded binary search per vertex
//            k_denoise_rowstats      one thread per vertex: the empty rows, the longest row (integer atomics, one per wave)
//            k_denoise_tristats      one thread per triangle: the repeats, the work of a normal pass (a 64-bit integer atomic per wave)
//   normals  k_denoise_raw           one thread per triangle: the unit normal of its area vector
//            k_denoise_normal_pass   one thread per triangle: merges the three ascending rows of its vertices with three cursors, gathers
//                                    the normals of up to four merged faces before their adds, sums in order in double
//   vertices k_denoise_vertex_pass   one thread per vertex over its row: the centroids in double in registers, sums in order in double
// The corner keys, the offsets, the load of a triangle and its area vector are kernels_smooth.hip's too: mesh_device.h has them.
// No float atomics, no wait on another thread, every loop has its bound when it starts.
#include "../../include/rgbid_denoise.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // the index check, the corner table, tri_load, area_vector, the argument and overlap tests, the create;
                            // voxel_device.h's ordered gather and sort workspace

#include <cmath>
#include <cstring>

using namespace rgbid;

namespace {

// beside the workspace's own 0 .. 8; SLOT_WORK is a 64-bit count over two slots, 8-byte aligned
enum { SLOT_BAD = 9, SLOT_WORK = 10, SLOT_EMPTY = 12, SLOT_LONGEST = 13, SLOT_REPEATS = 14 };
static_assert(SLOT_VOXELS < SLOT_BAD && SLOT_REPEATS < SLOTS && SLOT_WORK % 2 == 0, "the slots of this file lie behind the workspace's");
constexpr unsigned NO_FACE = 0xFFFFFFFFu;   // above every triangle number: the head of a row that has ended

// ---- face table -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT) void k_denoise_faces(const unsigned* __restrict__ corners_sorted, unsigned long long corners, unsigned* __restrict__ faces) {
  for (size_t i = (size_t)blockIdx.x * VT + threadIdx.x; i < corners; i += (size_t)gridDim.x * VT) faces[i] = corners_sorted[i] / 3u;
}

__global__ __launch_bounds__(VT) void k_denoise_rowstats(const unsigned* __restrict__ offsets, unsigned n_v, unsigned* __restrict__ slots) {
  const size_t v = (size_t)blockIdx.x * VT + threadIdx.x;
  unsigned len = 0, empty = 0;
  if (v < n_v) {
    len = offsets[v + 1] - offsets[v];
    empty = len == 0;
  }
  empty = wave_sum(empty);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) len = max(len, (unsigned)__shfl_xor(len, o, 64));
  if ((threadIdx.x & 63) == 0) {
    if (empty) atomicAdd(slots + SLOT_EMPTY, empty);
    if (len) atomicMax(slots + SLOT_LONGEST, len);
  }
}

__global__ __launch_bounds__(VT) void k_denoise_tristats(const unsigned* __restrict__ tri, const unsigned* __restrict__ offsets, unsigned n_t, unsigned n_v,
                                                         unsigned* __restrict__ slots) {
  const size_t t = (size_t)blockIdx.x * VT + threadIdx.x;
  unsigned long long work = 0;
  unsigned repeats = 0;
  if (t < n_t) {
    const unsigned i[3] = {tri[3 * t], tri[3 * t + 1], tri[3 * t + 2]};
    for (int k = 0; k < 3; ++k)
      if (i[k] < n_v) work += offsets[i[k] + 1] - offsets[i[k]];
    repeats = i[0] == i[1] || i[1] == i[2] || i[2] == i[0];
  }
  wave_add_to(reinterpret_cast<unsigned long long*>(slots + SLOT_WORK), work);
  wave_add_to(slots + SLOT_REPEATS, repeats);
}

// ---- raw normals ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT) void k_denoise_raw(const float* __restrict__ pos, const unsigned* __restrict__ tri, unsigned n_t, unsigned n_v,
                                                    float* __restrict__ out) {
  RGBID_FP_STRICT
  const size_t t = (size_t)blockIdx.x * VT + threadIdx.x;
  if (t >= n_t) return;
  const TriPos q = tri_load(pos, tri, (unsigned)t, n_t, n_v);
  double s[3] = {0, 0, 0};
  if (q.ok) area_vector(q, s);
  float n[3];
  unit_of(s, n);                      // zeros when |s|^2 is 0 or not finite
  for (int a = 0; a < 3; ++a) out[3 * t + a] = n[a];
}

// ---- the normal pass --------------------------------------------------------------------------------------------------------------
struct Nrm {
  float n[3];
};

// the normal of triangle id; an id that names no triangle reads nothing and counts as not finite
__device__ __forceinline__ Nrm nrm_load(const float* __restrict__ in, unsigned id, unsigned n_t) {
  Nrm q = {{NAN, NAN, NAN}};
  if (id < n_t) {
    const size_t o = 3 * (size_t)id;
    q.n[0] = in[o]; q.n[1] = in[o + 1]; q.n[2] = in[o + 2];
  }
  return q;
}

// one member of F(t), in order: the dot product, the test against T, the squared weight; every product and add a separate rounding
__device__ __forceinline__ void nrm_add(double s[3], const double nt[3], const Nrm& q, double T) {
  RGBID_FP_STRICT
  if (!finite3(q.n[0], q.n[1], q.n[2])) return;
  const double nj[3] = {(double)q.n[0], (double)q.n[1], (double)q.n[2]};
  const double d = (nt[0] * nj[0] + nt[1] * nj[1]) + nt[2] * nj[2];
  if (!(isfinite(d) && d > T)) return;
  const double dt = d - T;
  const double w = dt * dt;
  for (int a = 0; a < 3; ++a) {
    const double term = w * nj[a];
    s[a] = s[a] + term;
  }
}

// a row of the face table as the merge walks it: the cursor, the end and the face under the cursor
struct Row {
  unsigned at, end, head;
};

// the row of vertex v; a vertex that does not exist, or a row that does not lie inside the table, is an empty row
__device__ __forceinline__ Row row_open(const unsigned* __restrict__ offsets, const unsigned* __restrict__ faces, unsigned v, unsigned n_v,
                                        unsigned long long n_faces) {
  Row r = {0u, 0u, NO_FACE};
  if (v < n_v) {
    const unsigned b = offsets[v], e = offsets[v + 1];
    if (b < e && e <= n_faces) {
      r.at = b;
      r.end = e;
      r.head = faces[b];
    }
  }
  return r;
}

__device__ __forceinline__ void row_next(Row& r, const unsigned* __restrict__ faces) {
  ++r.at;
  r.head = r.at < r.end ? faces[r.at] : NO_FACE;
}

__global__ __launch_bounds__(VT) void k_denoise_normal_pass(const float* __restrict__ in, float* __restrict__ out, const unsigned* __restrict__ tri,
                                                            const unsigned* __restrict__ offsets, const unsigned* __restrict__ faces, unsigned n_t,
                                                            unsigned n_v, unsigned long long n_faces, double T) {
  RGBID_FP_STRICT
  const size_t t = (size_t)blockIdx.x * VT + threadIdx.x;
  if (t >= n_t) return;
  const size_t o = 3 * t;
  const unsigned* words = reinterpret_cast<const unsigned*>(in);
  const unsigned w[3] = {words[o], words[o + 1], words[o + 2]};
  const float x[3] = {__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
  double s[3] = {0, 0, 0};
  if (finite3(x[0], x[1], x[2]) && !(x[0] == 0.f && x[1] == 0.f && x[2] == 0.f)) {
    const double nt[3] = {(double)x[0], (double)x[1], (double)x[2]};
    Row r0 = row_open(offsets, faces, tri[o], n_v, n_faces), r1 = row_open(offsets, faces, tri[o + 1], n_v, n_faces),
        r2 = row_open(offsets, faces, tri[o + 2], n_v, n_faces);
    // the entries the three rows hold: every step of the merge takes one, so both loops end after `left` steps
    unsigned long long left = (unsigned long long)(r0.end - r0.at) + (r1.end - r1.at) + (r2.end - r2.at);
    unsigned last = NO_FACE;
    while (left) {
      unsigned id[4];
      int n = 0;
      while (n < 4 && left) {         // the smallest head; an id equal to the one taken last is a repeat inside a row or across rows
        --left;
        unsigned j;
        if (r0.head <= r1.head && r0.head <= r2.head) { j = r0.head; row_next(r0, faces); }
        else if (r1.head <= r2.head) { j = r1.head; row_next(r1, faces); }
        else { j = r2.head; row_next(r2, faces); }
        if (j != last) { id[n++] = j; last = j; }
      }
      Nrm q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = nrm_load(in, u < n ? id[u] : NO_FACE, n_t);   // the gathers before the adds
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (u < n) nrm_add(s, nt, q[u], T);
    }
  }
  const double q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
  unsigned* wout = reinterpret_cast<unsigned*>(out);
  if (isfinite(q) && q > 0.0) {
    const double l = sqrt(q);
    for (int a = 0; a < 3; ++a) out[o + a] = (float)(s[a] / l);
  } else {
    for (int a = 0; a < 3; ++a) wout[o + a] = w[a];
  }
}

// ---- the vertex pass --------------------------------------------------------------------------------------------------------------
struct Member {
  TriPos tri;
  float n[3];
  unsigned id;
};

struct VertexSum {
  double s[3] = {0, 0, 0};
  double x[3];                        // the vertex itself
  unsigned m = 0;                     // the triangles that took part
  unsigned last = NO_FACE;
};

// one entry of the row, in order; a repeat of the entry before counts once
__device__ __forceinline__ void member_add(VertexSum& sum, const Member& q) {
  RGBID_FP_STRICT
  if (q.id == sum.last) return;
  sum.last = q.id;
  if (!q.tri.ok || !finite3(q.n[0], q.n[1], q.n[2]) || (q.n[0] == 0.f && q.n[1] == 0.f && q.n[2] == 0.f)) return;
  const double N[3] = {(double)q.n[0], (double)q.n[1], (double)q.n[2]};
  double e[3];
  for (int a = 0; a < 3; ++a) {
    const double c = (((double)q.tri.p[0][a] + (double)q.tri.p[1][a]) + (double)q.tri.p[2][a]) / 3.0;
    e[a] = c - sum.x[a];
  }
  const double dd = (N[0] * e[0] + N[1] * e[1]) + N[2] * e[2];
  for (int a = 0; a < 3; ++a) {
    const double term = N[a] * dd;
    sum.s[a] = sum.s[a] + term;
  }
  ++sum.m;
}

__global__ __launch_bounds__(VT) void k_denoise_vertex_pass(const float* __restrict__ in, float* __restrict__ out, const float* __restrict__ nrm,
                                                            const unsigned* __restrict__ tri, const unsigned* __restrict__ offsets,
                                                            const unsigned* __restrict__ faces, unsigned n_t, unsigned n_v, unsigned long long n_faces) {
  RGBID_FP_STRICT
  const size_t v = (size_t)blockIdx.x * VT + threadIdx.x;
  if (v >= n_v) return;
  const size_t o = 3 * v;
  const unsigned* words = reinterpret_cast<const unsigned*>(in);
  const unsigned w[3] = {words[o], words[o + 1], words[o + 2]};
  const float x[3] = {__uint_as_float(w[0]), __uint_as_float(w[1]), __uint_as_float(w[2])};
  VertexSum sum;
  for (int a = 0; a < 3; ++a) sum.x[a] = (double)x[a];
  if (finite3(x[0], x[1], x[2])) {
    const unsigned b = offsets[v], e = offsets[v + 1];
    // three index loads, nine position loads and three normal loads per member; the centroid is formed in registers
    const auto load = [&](unsigned id) {
      Member q;
      q.id = id;
      q.tri = tri_load(in, tri, id, n_t, n_v);
      const Nrm n = nrm_load(nrm, id, n_t);
      for (int a = 0; a < 3; ++a) q.n[a] = n.n[a];
      return q;
    };
    if (b <= e && e <= n_faces) gather_in_order(faces, b, e, sum, load, member_add);
  }
  unsigned* wout = reinterpret_cast<unsigned*>(out);
  if (sum.m) {
    const double dm = (double)sum.m;
    for (int a = 0; a < 3; ++a) {
      const double step = sum.s[a] / dm;
      out[o + a] = (float)(sum.x[a] + step);
    }
  } else {
    for (int a = 0; a < 3; ++a) wout[o + a] = w[a];   // the words: a NaN keeps its payload
  }
}

}  // namespace

struct rgbid_denoise {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0;
  SortWorkspace w;                   // 3 cap_t items: the corner sort
  unsigned* offsets = nullptr;       // [cap_v + 1]
  unsigned* faces = nullptr;         // [3 cap_t]
  float* spare_n = nullptr;          // [cap_t][3] the other normal buffer of the ping-pong
  float* spare_v = nullptr;          // [cap_v][3] the other position buffer of the ping-pong
  // the last plan
  bool planned = false;
  unsigned n_v = 0, n_t = 0;
  const unsigned* tri = nullptr;
  // stage timing: check [0, 1], the rest of the plan [2, 3], normals [4, 5], vertices [6, 7]
  bool timed[3] = {false, false, false};
  Buffers buf;
  StageTimer<8> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

extern "C" {

int rgbid_denoise_create(rgbid_denoise** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles) {
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_DENOISE_MAX_VERTICES, RGBID_DENOISE_MAX_TRIANGLES, [&](rgbid_denoise* h) {
    const size_t cv = (size_t)max_vertices, ct = (size_t)max_triangles;
    int r = h->w.alloc(h->buf, 3ull * max_triangles);
    if (!r) r = h->buf.alloc(&h->offsets, sizeof(unsigned) * (cv + 1));
    if (!r) r = h->buf.alloc(&h->faces, sizeof(unsigned) * 3 * ct);
    if (!r) r = h->buf.alloc(&h->spare_n, sizeof(float) * 3 * ct);
    if (!r) r = h->buf.alloc(&h->spare_v, sizeof(float) * 3 * cv);
    return r;
  });
}

int rgbid_denoise_destroy(rgbid_denoise* h) { return destroy_handle(h); }   // a pass may still read the tables

int rgbid_denoise_plan(rgbid_denoise* h, unsigned long long n_vertices, unsigned long long n_triangles, const uint32_t* triangles_dev,
                       unsigned long long counts[4]) {
  if (!h) return RGBID_E_INVALID;
  if (!mesh_in_ok(n_vertices, n_triangles, triangles_dev, h->cap_v, h->cap_t)) return RGBID_E_INVALID;
  if (counts) for (int i = 0; i < 4; ++i) counts[i] = 0;
  h->planned = false;
  h->timed[0] = false;
  const unsigned n_v = (unsigned)n_vertices, n_t = (unsigned)n_triangles;
  h->n_v = n_v; h->n_t = n_t;
  h->tri = triangles_dev;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->w;
  if (n_v == 0) {                                          // no vertex, no triangle: a table of one zero
    RGBID_HIP(hipMemsetAsync(h->offsets, 0, sizeof(unsigned), s));
    h->planned = true;
    return RGBID_OK;
  }
  h->mark(0);
  RGBID_HIP(hipMemsetAsync(w.slots, 0, sizeof(unsigned) * SLOTS, s));
  if (n_t) check_triangles<false>(s, triangles_dev, n_t, n_v, w.slots + SLOT_BAD);
  h->mark(1);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  if (w.slots_host[SLOT_BAD]) return RGBID_E_INVALID;      // a triangle names a vertex that does not exist
  h->mark(2);
  const unsigned long long corners = 3ull * n_t;
  const unsigned* keys = nullptr;
  if (corners) {
    // <unsigned> is no choice: the kernel is a template only so that a file that does not launch it does not compile it
    hipLaunchKernelGGL(k_mesh_corner_keys<unsigned>, dim3(grid_of((corners + VT - 1) / VT)), dim3(VT), 0, s, triangles_dev, corners, n_v, w.keys_as<unsigned>(0),
                       w.idx[0]);
    const int p = w.sort_bits<unsigned>(s, (unsigned)corners, bitlen(n_v), 0);
    keys = w.keys_as<unsigned>(p);
    hipLaunchKernelGGL(k_denoise_faces, dim3(grid_of((corners + VT - 1) / VT)), dim3(VT), 0, s, w.idx[p], corners, h->faces);
  }
  hipLaunchKernelGGL(k_mesh_offsets<false>, dim3(grid_of(((unsigned long long)n_v + 1 + VT - 1) / VT)), dim3(VT), 0, s, keys, (const unsigned*)nullptr,
                     (const unsigned*)nullptr, (unsigned)corners, n_v, h->offsets);
  hipLaunchKernelGGL(k_denoise_rowstats, dim3((n_v + VT - 1) / VT), dim3(VT), 0, s, h->offsets, n_v, w.slots);
  if (n_t) hipLaunchKernelGGL(k_denoise_tristats, dim3((n_t + VT - 1) / VT), dim3(VT), 0, s, triangles_dev, h->offsets, n_t, n_v, w.slots);
  h->mark(3);
  RGBID_HIP(hipGetLastError());
  if (int r = w.read_slots(s)) return r;
  h->timed[0] = h->timer.on;
  if (counts) {
    counts[0] = w.slots_host[SLOT_EMPTY];
    counts[1] = w.slots_host[SLOT_LONGEST];
    counts[2] = w.slots_host[SLOT_REPEATS];
    unsigned long long work;
    memcpy(&work, w.slots_host + SLOT_WORK, sizeof(work));
    counts[3] = work;
  }
  h->planned = true;
  return RGBID_OK;
}

int rgbid_denoise_faces(rgbid_denoise* h, uint32_t* offsets_out, uint32_t* faces_out) {
  if (!h || !h->planned) return RGBID_E_INVALID;
  if (!aligned4(offsets_out) || !aligned4(faces_out)) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  if (offsets_out) RGBID_HIP(hipMemcpyAsync(offsets_out, h->offsets, sizeof(unsigned) * ((size_t)h->n_v + 1), hipMemcpyDeviceToDevice, s));
  if (faces_out && h->n_t) RGBID_HIP(hipMemcpyAsync(faces_out, h->faces, sizeof(unsigned) * 3 * (size_t)h->n_t, hipMemcpyDeviceToDevice, s));
  return RGBID_OK;
}

int rgbid_denoise_normals(rgbid_denoise* h, const float* vertices_dev, float* normals_out, unsigned iterations, double threshold) {
  if (!h || !h->planned) return RGBID_E_INVALID;
  if (iterations > RGBID_DENOISE_MAX_ITERATIONS) return RGBID_E_INVALID;
  if (!(std::isfinite(threshold) && threshold >= 0.0 && threshold < 1.0)) return RGBID_E_INVALID;
  const size_t vbytes = sizeof(float) * 3 * (size_t)h->n_v, nbytes = sizeof(float) * 3 * (size_t)h->n_t;
  if (h->n_t) {
    if (!vertices_dev || !normals_out || !aligned4(vertices_dev) || !aligned4(normals_out)) return RGBID_E_INVALID;
    if (overlap(vertices_dev, vbytes, normals_out, nbytes)) return RGBID_E_INVALID;
  }
  h->timed[1] = false;
  if (h->n_t == 0) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const unsigned n_v = h->n_v, n_t = h->n_t, blocks = (n_t + VT - 1) / VT;
  h->mark(4);
  float* dst = (iterations & 1u) ? h->spare_n : normals_out;   // the last pass writes normals_out
  hipLaunchKernelGGL(k_denoise_raw, dim3(blocks), dim3(VT), 0, s, vertices_dev, h->tri, n_t, n_v, dst);
  for (unsigned i = 0; i < iterations; ++i) {
    const float* src = dst;
    dst = src == normals_out ? h->spare_n : normals_out;
    hipLaunchKernelGGL(k_denoise_normal_pass, dim3(blocks), dim3(VT), 0, s, src, dst, h->tri, h->offsets, h->faces, n_t, n_v, 3ull * n_t, threshold);
  }
  h->mark(5);
  RGBID_HIP(hipGetLastError());
  h->timed[1] = h->timer.on;
  return RGBID_OK;
}

int rgbid_denoise_vertices(rgbid_denoise* h, const float* vertices_in, const float* face_normals_dev, float* vertices_out, unsigned iterations) {
  if (!h || !h->planned) return RGBID_E_INVALID;
  if (iterations > RGBID_DENOISE_MAX_ITERATIONS) return RGBID_E_INVALID;
  const size_t vbytes = sizeof(float) * 3 * (size_t)h->n_v, nbytes = sizeof(float) * 3 * (size_t)h->n_t;
  if (h->n_v) {
    if (!vertices_in || !vertices_out || !aligned4(vertices_in) || !aligned4(vertices_out)) return RGBID_E_INVALID;
    if (h->n_t && (!face_normals_dev || !aligned4(face_normals_dev))) return RGBID_E_INVALID;
    if (overlap(vertices_in, vbytes, vertices_out, vbytes) || overlap(face_normals_dev, nbytes, vertices_out, vbytes)) return RGBID_E_INVALID;
  }
  h->timed[2] = false;
  if (h->n_v == 0) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  h->mark(6);
  if (iterations == 0) RGBID_HIP(hipMemcpyAsync(vertices_out, vertices_in, vbytes, hipMemcpyDeviceToDevice, s));
  const float* src = vertices_in;
  for (unsigned i = 0; i < iterations; ++i) {
    float* dst = ((iterations - 1 - i) & 1u) ? h->spare_v : vertices_out;   // the last pass writes vertices_out
    hipLaunchKernelGGL(k_denoise_vertex_pass, dim3((h->n_v + VT - 1) / VT), dim3(VT), 0, s, src, dst, face_normals_dev, h->tri, h->offsets, h->faces, h->n_t,
                       h->n_v, 3ull * h->n_t);
    src = dst;
  }
  h->mark(7);
  RGBID_HIP(hipGetLastError());
  h->timed[2] = h->timer.on;
  return RGBID_OK;
}

int rgbid_denoise_timing(rgbid_denoise* h, int enable, float ms[3]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  static const int pairs[3][4] = {{0, 1, 2, 3}, {4, 5}, {6, 7}};   // the plan: the check and the rest
  if (ms)
    if (int r = stage_times(h->timer, h->timed, pairs, ms)) return r;
  return h->timer.enable(enable != 0);
}

}  // extern "C"
