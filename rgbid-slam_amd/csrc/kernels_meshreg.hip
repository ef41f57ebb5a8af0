// kernels_meshreg.hip -- point sets and meshes registered to an indexed triangle mesh by point-to-plane ICP (include/rgbid_meshreg.h,
// DESIGN.md section 28).
//
// The judge is tests/meshreg_mirror.py; the result records, the triangles' normals as the sums see them and apply's output are
// byte-identical to it.  The handle owns a rgbid_meshdist and reaches it through its public C-ABI only.
//   target  rgbid_meshdist_plan   the grid of the target
//           k_reg_normals         one thread per triangle: tests every index before it is an address; three doubles, or NaN for a triangle
//                                 without a normal
//   align   k_reg_init            the result records of the starts: pose, RUNNING, zeros
//           per iteration, enqueued without a host wait:
//           k_reg_transform<P>    blockIdx.y the start: step 4's float32 point of every lattice point; NaN bits for a stopped start
//           rgbid_meshdist_query  the nearest triangle, the distance and the closest point of every transformed point
//           k_reg_system          one thread per lattice point, a wave per group of 64, blockIdx.y the start: the 28 terms in registers,
//                                 the __shfl_xor butterfly, lane 0 writes term-major
//           k_reg_solve           one block per start: the upper tree between the two workspace buffers; thread 0 walks steps 8 - 10
//   apply   k_reg_apply           step 12
// The search and the system are two launches on purpose: the search walks its queries in cell order, the tree must see them in input order.
// No float atomics, no wait on another thread, every loop has its bound when it starts.
#include "../../include/rgbid_meshreg.h"
#include "common.h"
#include "hip_host.h"
#include "mesh_device.h"    // mesh_create; voxel_device.h's point sources and records_in_ok
#include "gn_device.h"      // tree64, the upper tree, the solve, the retraction

#include <cmath>

using namespace rgbid;

static_assert(sizeof(rgbid_cloud_point) == 32, "RecordPoints reads the first 16 bytes of a 32-byte record");
static_assert(sizeof(rgbid_meshreg_result) == 560, "step 11");
static_assert(RGBID_MESHREG_TERMS == GN_TERMS && VT == GN_BLOCK, "gn_device.h's tree");

namespace {

constexpr unsigned NONE = RGBID_MESHDIST_NONE;
constexpr unsigned NAN_BITS = RGBID_RENDER_NAN_BITS;
constexpr int MAX_IT = RGBID_MESHREG_MAX_ITERATIONS;

struct RegPose { double m[12]; };                // R00 .. R22 tx ty tz, as a kernel argument

struct RegLevel {
  unsigned n;                     // source points
  unsigned stride, n_l, groups;   // the level's lattice and its groups of 64 (at least one)
  unsigned restart;               // the first iteration of a later level: CONVERGED starts run again
};

struct RegWork {                  // the handle's workspace
  double* a;                      // [V][28][a_stride] group sums, term-major, and the third round of the upper tree
  double* b;                      // [V][28][b_stride] the second and fourth round
  unsigned* used;                 // [V][a_stride] used points per group
  size_t a_stride, b_stride;
};

struct RegRule {
  double damping, eps;
  unsigned min_points;
};

__device__ __forceinline__ int reg_status(const rgbid_meshreg_result* res, unsigned start, unsigned restart) {
  const int s = res[start].status;
  return s == RGBID_MESHREG_CONVERGED && restart ? RGBID_MESHREG_RUNNING : s;
}

// step 4 (and step 12 with t = 0 left out by the caller): one row of the pose on a point, in double
__device__ __forceinline__ double reg_row(const double* m, double x, double y, double z) {
  RGBID_FP_STRICT
  return (m[0] * x + m[1] * y) + m[2] * z;
}

// step 1: one thread per triangle
__global__ __launch_bounds__(VT) void k_reg_normals(const float* __restrict__ v, const unsigned* __restrict__ tri, unsigned n_v, unsigned n_t,
                                                    double* __restrict__ nrm) {
  RGBID_FP_STRICT
  const unsigned t = blockIdx.x * VT + threadIdx.x;
  if (t >= n_t) return;
  const unsigned ia = tri[3 * (size_t)t], ib = tri[3 * (size_t)t + 1], ic = tri[3 * (size_t)t + 2];
  const double nan = __longlong_as_double((long long)RGBID_MESHREG_NAN_BITS);
  double n[3] = {nan, nan, nan};
  if (ia < n_v && ib < n_v && ic < n_v) {
    const float* pa = v + 3 * (size_t)ia;
    const float* pb = v + 3 * (size_t)ib;
    const float* pc = v + 3 * (size_t)ic;
    if (finite3(pa[0], pa[1], pa[2]) && finite3(pb[0], pb[1], pb[2]) && finite3(pc[0], pc[1], pc[2])) {   // it takes part
      const double a[3] = {(double)pa[0], (double)pa[1], (double)pa[2]};
      const double ab[3] = {(double)pb[0] - a[0], (double)pb[1] - a[1], (double)pb[2] - a[2]};
      const double ac[3] = {(double)pc[0] - a[0], (double)pc[1] - a[1], (double)pc[2] - a[2]};
      const double m0 = ab[1] * ac[2] - ab[2] * ac[1], m1 = ab[2] * ac[0] - ab[0] * ac[2], m2 = ab[0] * ac[1] - ab[1] * ac[0];
      const double l2 = (m0 * m0 + m1 * m1) + m2 * m2;
      if (l2 > 0.0 && l2 < (double)INFINITY) {
        const double l = sqrt(l2);
        n[0] = m0 / l; n[1] = m1 / l; n[2] = m2 / l;
      }
    }
  }
  for (int k = 0; k < 3; ++k) nrm[3 * (size_t)t + k] = n[k];
}

__global__ __launch_bounds__(VT) void k_reg_init(const double* __restrict__ poses, int V, rgbid_meshreg_result* __restrict__ res) {
  const int v = blockIdx.x * VT + threadIdx.x;
  if (v >= V) return;
  rgbid_meshreg_result& r = res[v];
  for (int k = 0; k < 12; ++k) r.pose[k] = poses[12 * v + k];
  r.status = RGBID_MESHREG_RUNNING;
  r.iterations = 0;
  r.used[0] = r.used[1] = 0u;
  for (int k = 0; k < GN_TERMS; ++k) r.sums[0][k] = r.sums[1][k] = 0.0;
}

// step 4: lattice point j of start blockIdx.y -> p[start n_l + j]; a stopped start's points are NaN, which the search does not walk
template <class P>
__global__ __launch_bounds__(VT) void k_reg_transform(P pts, RegLevel lv, const rgbid_meshreg_result* __restrict__ res, float* __restrict__ p) {
  RGBID_FP_STRICT
  const unsigned j = blockIdx.x * VT + threadIdx.x, start = blockIdx.y;
  if (j >= lv.n_l) return;
  float* o = p + 3 * ((size_t)start * lv.n_l + j);
  if (reg_status(res, start, lv.restart) != RGBID_MESHREG_RUNNING) {
    o[0] = o[1] = o[2] = __uint_as_float(NAN_BITS);
    return;
  }
  const unsigned i = j * lv.stride;              // < n: n_l = ceil(n / stride); the product is below 2^31
  if (i >= lv.n) return;
  const float4 s = pts.at(i);
  const double* m = res[start].pose;
  const double x = (double)s.x, y = (double)s.y, z = (double)s.z;
  o[0] = (float)(reg_row(m, x, y, z) + m[9]);
  o[1] = (float)(reg_row(m + 3, x, y, z) + m[10]);
  o[2] = (float)(reg_row(m + 6, x, y, z) + m[11]);
}

// steps 5 - 7: one thread per lattice point, a wave per group of 64, a block four groups of the start blockIdx.y.  Lanes beyond the
// lattice and points that are not used stay in the wave with +0.0: the butterflies need all 64.  No LDS, no atomic.
__global__ __launch_bounds__(VT) void k_reg_system(RegLevel lv, float reach, double huber, unsigned n_t, const double* __restrict__ nrm,
                                                   const float* __restrict__ p, const unsigned* __restrict__ tri, const float* __restrict__ dist,
                                                   const float* __restrict__ closest, const rgbid_meshreg_result* __restrict__ res,
                                                   double* __restrict__ sums, unsigned* __restrict__ used, size_t a_stride) {
  RGBID_FP_STRICT
  const unsigned start = blockIdx.y;
  if (reg_status(res, start, lv.restart) != RGBID_MESHREG_RUNNING) return;   // a stopped start's blocks leave at once
  const unsigned group = blockIdx.x * (VT / 64) + (threadIdx.x >> 6);
  if (group >= lv.groups) return;                               // the whole wave
  const unsigned lane = threadIdx.x & 63u, j = group * 64u + lane;
  double tm[GN_TERMS];
#pragma unroll
  for (int k = 0; k < GN_TERMS; ++k) tm[k] = 0.0;
  bool is_used = false;
  if (j < lv.n_l) {
    const size_t q = (size_t)start * lv.n_l + j;
    const unsigned t = tri[q];
    if (t != NONE && t < n_t && dist[q] <= reach) {             // a winner within reach; the index before it is an address
      const double n0 = nrm[3 * (size_t)t], n1 = nrm[3 * (size_t)t + 1], n2 = nrm[3 * (size_t)t + 2];
      if (n0 == n0) {                                           // the triangle has a normal
        is_used = true;
        const double P0 = (double)p[3 * q], P1 = (double)p[3 * q + 1], P2 = (double)p[3 * q + 2];
        const double e0 = P0 - (double)closest[3 * q], e1 = P1 - (double)closest[3 * q + 1], e2 = P2 - (double)closest[3 * q + 2];
        const double f = (n0 * e0 + n1 * e1) + n2 * e2;
        const double J[6] = {n0, n1, n2, P1 * n2 - P2 * n1, P2 * n0 - P0 * n2, P0 * n1 - P1 * n0};
        const double af = fabs(f);
        const double w = af <= huber ? 1.0 : huber / af;
        double a[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) a[i] = w * J[i];
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int jj = i; jj < 6; ++jj) tm[k++] = a[i] * J[jj];
#pragma unroll
        for (int i = 0; i < 6; ++i) tm[21 + i] = a[i] * f;
        tm[27] = (w * f) * f;
      }
    }
  }
  const unsigned n_used = (unsigned)__popcll(__ballot(is_used));
#pragma unroll
  for (int k = 0; k < GN_TERMS; ++k) tm[k] = gn_tree64(tm[k]);
  if (lane == 0) {
    double* o = sums + (size_t)start * GN_TERMS * a_stride + group;
#pragma unroll
    for (int k = 0; k < GN_TERMS; ++k) o[(size_t)k * a_stride] = tm[k];
    used[(size_t)start * a_stride + group] = n_used;
  }
}

// One block per start: the upper rounds of step 7 between the two buffers, then thread 0 walks steps 8 - 10 in double.
__global__ __launch_bounds__(VT) void k_reg_solve(RegWork w, RegRule rule, RegLevel lv, rgbid_meshreg_result* res) {
  RGBID_FP_STRICT
  __shared__ unsigned lds[VT / 64];
  const unsigned start = blockIdx.x;
  if (reg_status(res, start, lv.restart) != RGBID_MESHREG_RUNNING) return;   // the whole block
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // the used points: an integer sum, the same in any order
  unsigned cnt = 0;
  for (unsigned i = threadIdx.x; i < lv.groups; i += VT) cnt += w.used[(size_t)start * w.a_stride + i];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
  if (lane == 0) lds[wave] = cnt;
  double* src = w.a + (size_t)start * GN_TERMS * w.a_stride;
  size_t src_stride = w.a_stride;
  gn_upper_tree(src, src_stride, w.b + (size_t)start * GN_TERMS * w.b_stride, w.b_stride, lv.groups);
  rgbid_meshreg_result& r = res[start];
  const bool first = r.iterations == 0;
  __syncthreads();                                              // everybody has read the count of systems before thread 0 raises it
  if (threadIdx.x < GN_TERMS) {                                 // step 11: the first and the last system built
    const double s = gn_canonical_nan(src[(size_t)threadIdx.x * src_stride]);
    r.sums[1][threadIdx.x] = s;
    if (first) r.sums[0][threadIdx.x] = s;
  }
  if (threadIdx.x != 0) return;
  static_assert(VT / 64 == 4, "four waves left their counts");
  const unsigned n_used = lds[0] + lds[1] + lds[2] + lds[3];
  r.used[1] = n_used;
  if (first) r.used[0] = n_used;
  r.iterations += 1;
  if (n_used < rule.min_points) { r.status = RGBID_MESHREG_FEW; return; }             // step 8
  double x[6], biggest;
  if (!gn_solve(src, src_stride, rule.damping, x, biggest)) { r.status = RGBID_MESHREG_SINGULAR; return; }   // step 9
  double P[12], Q[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = r.pose[k];
  gn_retract(P, x, Q);
#pragma unroll
  for (int k = 0; k < 12; ++k) r.pose[k] = gn_canonical_nan(Q[k]);
  r.status = biggest < rule.eps ? RGBID_MESHREG_CONVERGED : RGBID_MESHREG_RUNNING;    // step 10
}

// step 12: one thread per point; an output may be its input, so nothing here is __restrict__ and a point is read before it is written
__global__ __launch_bounds__(VT) void k_reg_apply(const float* pts, const float* nrm, unsigned n, RegPose pose, float* pts_out, float* nrm_out) {
  RGBID_FP_STRICT
  const double* m = pose.m;
  for (size_t i = (size_t)blockIdx.x * VT + threadIdx.x; i < n; i += (size_t)gridDim.x * VT) {
    const double x = (double)pts[3 * i], y = (double)pts[3 * i + 1], z = (double)pts[3 * i + 2];
    const float o0 = (float)(reg_row(m, x, y, z) + m[9]), o1 = (float)(reg_row(m + 3, x, y, z) + m[10]),
                o2 = (float)(reg_row(m + 6, x, y, z) + m[11]);
    pts_out[3 * i] = o0; pts_out[3 * i + 1] = o1; pts_out[3 * i + 2] = o2;
    if (nrm) {
      const double a = (double)nrm[3 * i], b = (double)nrm[3 * i + 1], c = (double)nrm[3 * i + 2];
      const float q0 = (float)reg_row(m, a, b, c), q1 = (float)reg_row(m + 3, a, b, c), q2 = (float)reg_row(m + 6, a, b, c);
      nrm_out[3 * i] = q0; nrm_out[3 * i + 1] = q1; nrm_out[3 * i + 2] = q2;
    }
  }
}

}  // namespace

struct rgbid_meshreg {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0, cap_t = 0, cap_n = 0, cap_s = 0;
  rgbid_meshdist* dist = nullptr;          // the search, through its public C-ABI
  double* nrm = nullptr;                   // [cap_t][3] step 1's normals, NaN for a triangle without one
  float* p = nullptr;                      // [cap_n cap_s][3] the transformed points of an iteration: the search's queries
  unsigned* tri = nullptr;                 // [cap_n cap_s] and its answers
  float* qdist = nullptr;                  // [cap_n cap_s]
  float* closest = nullptr;                // [cap_n cap_s][3]
  double* poses = nullptr;                 // [cap_s][12] the starts of a call
  double* poses_host = nullptr;            // pinned
  hipEvent_t copied = nullptr;             // the last call's copy has read the pinned table
  RegWork w = {};
  // the last target
  bool has_target = false;
  unsigned n_t = 0;
  float d_max = 0.f;
  // stage timing: event 0 after the init, then one after every launch of an iteration: transform, query, system, solve
  int timed = 0;                           // iterations of the last call that were recorded
  Buffers buf;
  StageTimer<4 * MAX_IT + 1> timer;
  ~rgbid_meshreg() {
    if (dist) (void)rgbid_meshdist_destroy(dist);
    if (copied) (void)hipEventDestroy(copied);
  }
};

namespace {

template <class P>
int align_call(rgbid_meshreg* h, const P& pts, unsigned long long n, int V, const double* poses, float huber, double damping, double eps,
               unsigned min_points, int n_levels, const rgbid_meshreg_level* levels, rgbid_meshreg_result* result_dev) {
  if (!h->has_target || !poses || !levels) return RGBID_E_INVALID;
  if (V < 1 || (unsigned long long)V > h->cap_s) return RGBID_E_INVALID;
  if (!finite_all(poses, 12 * V)) return RGBID_E_INVALID;
  if (!(std::isfinite(huber) && huber > 0.f)) return RGBID_E_INVALID;
  if (!(std::isfinite(damping) && damping >= 0.0)) return RGBID_E_INVALID;
  if (!(std::isfinite(eps) && eps > 0.0)) return RGBID_E_INVALID;
  if (min_points < 6) return RGBID_E_INVALID;
  if (n_levels < 1 || n_levels > RGBID_MESHREG_MAX_LEVELS) return RGBID_E_INVALID;
  int total = 0;
  for (int l = 0; l < n_levels; ++l) {
    const int it = levels[l].iterations;
    if (levels[l].stride < 1 || it < 1 || it > MAX_IT) return RGBID_E_INVALID;
    if (!(std::isfinite(levels[l].reach) && levels[l].reach > 0.f && levels[l].reach <= h->d_max)) return RGBID_E_INVALID;
    total += it;
  }
  if (total > MAX_IT) return RGBID_E_INVALID;
  if (!result_dev || (((uintptr_t)result_dev) & 7)) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const bool timing = h->timer.on;
  h->timed = 0;
  RGBID_HIP(hipEventSynchronize(h->copied));      // the previous call's copy has read the pinned table (nothing was recorded: returns at once)
  for (int k = 0; k < 12 * V; ++k) h->poses_host[k] = poses[k];
  RGBID_HIP(hipMemcpyAsync(h->poses, h->poses_host, sizeof(double) * 12 * (size_t)V, hipMemcpyHostToDevice, s));
  RGBID_HIP(hipEventRecord(h->copied, s));
  hipLaunchKernelGGL(k_reg_init, dim3(((unsigned)V + VT - 1) / VT), dim3(VT), 0, s, h->poses, V, result_dev);
  int e = 0;
  h->timer.mark(e++, s);
  const RegRule rule{damping, eps, min_points};
  for (int l = 0; l < n_levels; ++l) {
    RegLevel lv{};
    lv.n = (unsigned)n;
    lv.stride = (unsigned)levels[l].stride;
    lv.n_l = (unsigned)((n + lv.stride - 1) / lv.stride);
    lv.groups = lv.n_l ? (lv.n_l + 63u) / 64u : 1u;
    const unsigned long long queries = (unsigned long long)V * lv.n_l;
    for (int it = 0; it < levels[l].iterations; ++it) {          // enqueued without waiting: the device decides who still runs
      lv.restart = (l > 0 && it == 0) ? 1u : 0u;
      if (lv.n_l) hipLaunchKernelGGL(k_reg_transform<P>, dim3((lv.n_l + VT - 1) / VT, (unsigned)V), dim3(VT), 0, s, pts, lv, result_dev, h->p);
      h->timer.mark(e++, s);
      if (int r = rgbid_meshdist_query(h->dist, queries, h->p, h->tri, h->qdist, h->closest, nullptr, nullptr)) return r;
      h->timer.mark(e++, s);
      hipLaunchKernelGGL(k_reg_system, dim3((lv.groups + VT / 64 - 1) / (VT / 64), (unsigned)V), dim3(VT), 0, s, lv, levels[l].reach, (double)huber,
                         h->n_t, h->nrm, h->p, h->tri, h->qdist, h->closest, result_dev, h->w.a, h->w.used, h->w.a_stride);
      h->timer.mark(e++, s);
      hipLaunchKernelGGL(k_reg_solve, dim3((unsigned)V), dim3(VT), 0, s, h->w, rule, lv, result_dev);
      h->timer.mark(e++, s);
    }
  }
  RGBID_HIP(hipGetLastError());
  h->timed = timing ? total : 0;
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_meshreg_create(rgbid_meshreg** out, rgbid_ctx* ctx, unsigned long long max_vertices, unsigned long long max_triangles,
                         unsigned long long max_pairs, unsigned long long max_points, unsigned long long max_starts) {
  if (out) *out = nullptr;
  if (max_points < 1 || max_points > RGBID_MESHREG_MAX_QUERIES || max_starts < 1 || max_starts > RGBID_MESHREG_MAX_STARTS ||
      max_points * max_starts > RGBID_MESHREG_MAX_QUERIES)
    return RGBID_E_INVALID;
  if (max_pairs < 1 || max_pairs > RGBID_MESHDIST_MAX_PAIRS) return RGBID_E_INVALID;
  return mesh_create(out, ctx, max_vertices, max_triangles, RGBID_MESHDIST_MAX_VERTICES, RGBID_MESHDIST_MAX_TRIANGLES, [&](rgbid_meshreg* h) {
    h->cap_n = max_points;
    h->cap_s = max_starts;
    const size_t q = (size_t)(max_points * max_starts);
    h->w.a_stride = (size_t)((max_points + 63) / 64);
    h->w.b_stride = (h->w.a_stride + 63) / 64;
    int r = rgbid_meshdist_create(&h->dist, ctx, max_vertices, max_triangles, max_pairs, max_points * max_starts);
    if (!r) r = h->buf.alloc(&h->nrm, sizeof(double) * 3 * (size_t)max_triangles);
    if (!r) r = h->buf.alloc(&h->p, sizeof(float) * 3 * q);
    if (!r) r = h->buf.alloc(&h->tri, sizeof(unsigned) * q);
    if (!r) r = h->buf.alloc(&h->qdist, sizeof(float) * q);
    if (!r) r = h->buf.alloc(&h->closest, sizeof(float) * 3 * q);
    if (!r) r = h->buf.alloc(&h->poses, sizeof(double) * 12 * (size_t)max_starts);
    if (!r) r = h->buf.alloc_host(&h->poses_host, sizeof(double) * 12 * (size_t)max_starts);
    if (!r) r = h->buf.alloc(&h->w.a, sizeof(double) * GN_TERMS * h->w.a_stride * (size_t)max_starts);
    if (!r) r = h->buf.alloc(&h->w.b, sizeof(double) * GN_TERMS * h->w.b_stride * (size_t)max_starts);
    if (!r) r = h->buf.alloc(&h->w.used, sizeof(unsigned) * h->w.a_stride * (size_t)max_starts);
    if (!r) r = hip_status(hipEventCreateWithFlags(&h->copied, hipEventDisableTiming));
    return r;
  });
}

int rgbid_meshreg_destroy(rgbid_meshreg* h) { return destroy_handle(h); }

int rgbid_meshreg_target(rgbid_meshreg* h, unsigned long long n_vertices, const float* vertices_dev, unsigned long long n_triangles,
                         const uint32_t* triangles_dev, float d_max, float cell, long long grid[6], unsigned long long stats[4]) {
  if (!h) return RGBID_E_INVALID;
  if (int r = rgbid_meshdist_plan(h->dist, n_vertices, vertices_dev, n_triangles, triangles_dev, d_max, cell, grid, stats)) {
    // the search says whether its former plan is kept (a query of nothing passes) or gone; the normals were not touched
    h->has_target = h->has_target && rgbid_meshdist_query(h->dist, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RGBID_OK;
    return r;
  }
  h->has_target = false;
  h->n_t = (unsigned)n_triangles;
  h->d_max = d_max;
  if (h->n_t) {
    (void)hipSetDevice(h->ctx->device);
    hipStream_t s = h->ctx->stream;
    hipLaunchKernelGGL(k_reg_normals, dim3((h->n_t + VT - 1) / VT), dim3(VT), 0, s, vertices_dev, triangles_dev, (unsigned)n_vertices, h->n_t, h->nrm);
    RGBID_HIP(hipGetLastError());
    RGBID_HIP(hipStreamSynchronize(s));          // the mesh may be released after the call
  }
  h->has_target = true;
  return RGBID_OK;
}

int rgbid_meshreg_align(rgbid_meshreg* h, unsigned long long n, const float* points_dev, int V, const double* poses, float huber,
                        double damping, double eps, unsigned min_points, int n_levels, const rgbid_meshreg_level* levels,
                        rgbid_meshreg_result* result_dev) {
  if (!h || n > h->cap_n) return RGBID_E_INVALID;
  if (n && (!points_dev || !aligned4(points_dev))) return RGBID_E_INVALID;
  return align_call(h, VertexPoints{points_dev}, n, V, poses, huber, damping, eps, min_points, n_levels, levels, result_dev);
}

int rgbid_meshreg_align_records(rgbid_meshreg* h, unsigned long long n, const rgbid_cloud_point* records_dev, int V, const double* poses,
                                float huber, double damping, double eps, unsigned min_points, int n_levels,
                                const rgbid_meshreg_level* levels, rgbid_meshreg_result* result_dev) {
  if (!h || !records_in_ok(records_dev, n, h->cap_n)) return RGBID_E_INVALID;
  return align_call(h, RecordPoints{reinterpret_cast<const float4*>(records_dev)}, n, V, poses, huber, damping, eps, min_points, n_levels, levels,
                    result_dev);
}

int rgbid_meshreg_apply(rgbid_meshreg* h, unsigned long long n, const float* points_dev, const float* normals_dev, const double pose[12],
                        float* points_out, float* normals_out) {
  if (!h || !pose || n > (1ull << 31) || !finite_all(pose, 12)) return RGBID_E_INVALID;
  if (!aligned4(points_dev) || !aligned4(normals_dev) || !aligned4(points_out) || !aligned4(normals_out)) return RGBID_E_INVALID;
  if ((normals_dev == nullptr) != (normals_out == nullptr)) return RGBID_E_INVALID;
  if (n == 0) return RGBID_OK;
  if (!points_dev || !points_out) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  RegPose P;
  for (int k = 0; k < 12; ++k) P.m[k] = pose[k];
  hipLaunchKernelGGL(k_reg_apply, dim3(grid_of((n + VT - 1) / VT)), dim3(VT), 0, h->ctx->stream, points_dev, normals_dev, (unsigned)n, P, points_out,
                     normals_out);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_meshreg_set_query_sort(rgbid_meshreg* h, int enable) {
  if (!h) return RGBID_E_INVALID;
  return rgbid_meshdist_set_query_sort(h->dist, enable);
}

int rgbid_meshreg_timing(rgbid_meshreg* h, int enable, float ms[4]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  if (ms) {
    for (int k = 0; k < 4; ++k) ms[k] = 0.f;
    for (int i = 0; i < h->timed; ++i)
      for (int k = 0; k < 4; ++k) {
        float one = 0.f;
        RGBID_HIP(h->timer.elapsed(4 * i + k, 4 * i + k + 1, &one));
        ms[k] += one;
      }
  }
  return h->timer.enable(enable != 0);
}

}  // extern "C"
