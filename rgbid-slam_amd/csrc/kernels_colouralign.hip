// kernels_colouralign.hip -- keyframe poses refined against the grey values of a mesh's vertices (include/rgbid_colouralign.h, DESIGN.md
// section 31).
//
// The judge is tests/colouralign_mirror.py; the result records and the targets S, W, used are byte-identical to it.
//   run     k_ca_init      the result records of the views: pose, RUNNING or FIXED, zeros
//           k_ca_pose      one thread per view: step 2's twelve floats from the record's double pose, into the view table
//           per round, enqueued without a host wait:
//           k_ca_target    one thread per lattice vertex: position and normal are read once.  Up to 16 views: all are walked in order with
//                          S, W and used in registers and the state is written once, no atomics.  More views: blockIdx.y walks a chunk
//                          of 16 and adds its integer sums to the cleared state with 64-bit atomics (the same bytes in any order)
//           per iteration:
//           k_ca_system    one thread per (lattice vertex, view) pair, a wave per group of 64, blockIdx.y the view: the view's table entry
//                          is block-uniform (scalar loads); the 28 terms in registers, the __shfl_xor butterfly, lane 0 writes
//                          term-major.  A wave without a used pair stores +0.0 without the butterflies (tree64 of 64 x +0.0 is +0.0)
//           k_ca_solve     one block per view: the upper tree between the two workspace buffers; thread 0 walks step 7
//           k_ca_pose      the moved poses for the next pass
//   targets three device-to-device copies of the state planes
// No float atomics, no wait on another thread, every loop has its bound when it starts.
//
// Exact arithmetic: every function that forms a product followed by a sum opens with RGBID_FP_STRICT (common.h), so the compiler forms no
// FMA from them; division and square root are hipcc's default correctly rounded ones.
#include "../../include/rgbid_colouralign.h"
#include "common.h"
#include "hip_host.h"
#include "view_device.h"    // the view entry, steps 3 and 4 of a pair; the host's checks of camera and views
#include "gn_device.h"      // tree64, the upper tree, the solve, the retraction

#include <cmath>
#include <new>

using namespace rgbid;

static_assert(sizeof(rgbid_colouralign_result) == 560, "step 8");
static_assert(RGBID_COLOURALIGN_TERMS == GN_TERMS, "gn_device.h's tree");
// step 5: S stays exact as a double
static_assert((unsigned long long)RGBID_COLOURALIGN_MAX_VIEWS * RGBID_RECOLOUR_UNIT_WEIGHT * (65280ull * 65536ull) < (1ull << 53), "step 5's bound");

namespace {

constexpr int VT = GN_BLOCK;                                // threads of a block: four waves
constexpr int WAVES = VT / 64;
constexpr int MAX_IT = RGBID_COLOURALIGN_MAX_ITERATIONS;
constexpr int TARGET_CHUNK = 16;                            // views a block of the chunked target pass walks

struct CaView : ViewEntry {                                 // the view table's entry: 80 bytes; m is written by k_ca_pose
  int fixed, pad;
};
static_assert(sizeof(CaView) == 80, "the view table's stride");
struct CaLattice {
  unsigned stride, n_l, groups;   // the lattice and its groups of 64 (at least one)
  unsigned restart;               // the first iteration of a round: CONVERGED views run again
};
struct CaWork {                   // the handle's workspace
  double* a;                      // [V][28][a_stride] group sums, term-major, and the third round of the upper tree
  double* b;                      // [V][28][b_stride] the second and fourth round
  unsigned* used;                 // [V][a_stride] used pairs per group
  size_t a_stride, b_stride;
};
struct CaRule {
  double damping, eps, huber;
  unsigned min_pairs, min_views;
};
// what steps 3 and 4 give for a TAKEN pair
struct CaSample {
  float X, Y, Z;
  unsigned w, s;
  int Gx, Gy;
};

__device__ __forceinline__ int ca_status(const rgbid_colouralign_result* res, unsigned v, unsigned restart) {
  const int s = res[v].status;
  return s == RGBID_COLOURALIGN_CONVERGED && restart ? RGBID_COLOURALIGN_RUNNING : s;
}

__device__ __forceinline__ unsigned grey(const unsigned char* __restrict__ c, size_t t) {
  return 77u * c[3 * t] + 150u * c[3 * t + 1] + 29u * c[3 * t + 2];
}

// steps 3 and 4 of one pair (view_device.h) and its grey sample: true iff it is TAKEN.  fin: the vertex is finite; facing: its normal has
// a finite, non-zero squared length
template <bool GRADIENT>
__device__ __forceinline__ bool ca_pair(const CaView& view, const ViewCam& cam, float x, float y, float z, bool fin, bool facing, float n0, float n1,
                                        float n2, CaSample& o) {
  return VIEW_TAKEN == view_sample(view, cam, x, y, z, fin, facing, n0, n1, n2, [&](const ViewSample& q) {
    const unsigned char* col = view.colour;
    const unsigned ax = q.ax, ay = q.ay;
    const unsigned L00 = grey(col, q.t00), L10 = grey(col, q.t10), L01 = grey(col, q.t01), L11 = grey(col, q.t11);   // <= 65 280
    o.X = q.X; o.Y = q.Y; o.Z = q.Z; o.w = q.w;
    o.s = (256u - ax) * (256u - ay) * L00 + ax * (256u - ay) * L10 + (256u - ax) * ay * L01 + ax * ay * L11;  // <= 65 280 * 65 536
    if (GRADIENT) {
      o.Gx = (int)(256u - ay) * ((int)L10 - (int)L00) + (int)ay * ((int)L11 - (int)L01);
      o.Gy = (int)(256u - ax) * ((int)L01 - (int)L00) + (int)ax * ((int)L11 - (int)L10);
    }
  });
}

// a lattice vertex's position and normal
struct CaVertex {
  float x, y, z, n0, n1, n2;
  bool fin, facing;
};
__device__ __forceinline__ CaVertex ca_vertex(const float* __restrict__ pos, const float* __restrict__ normals, size_t i) {
  RGBID_FP_STRICT
  CaVertex p;
  p.x = pos[3 * i]; p.y = pos[3 * i + 1]; p.z = pos[3 * i + 2];
  p.fin = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
  p.n0 = p.n1 = p.n2 = 0.f;
  p.facing = false;
  if (normals) {
    p.n0 = normals[3 * i]; p.n1 = normals[3 * i + 1]; p.n2 = normals[3 * i + 2];
    const float q = (p.n0 * p.n0 + p.n1 * p.n1) + p.n2 * p.n2;
    p.facing = __builtin_isfinite(q) && q != 0.f;
  }
  return p;
}

__global__ __launch_bounds__(VT) void k_ca_init(const double* __restrict__ poses, const CaView* __restrict__ views, int V,
                                                rgbid_colouralign_result* __restrict__ res) {
  const int v = blockIdx.x * VT + threadIdx.x;
  if (v >= V) return;
  rgbid_colouralign_result& r = res[v];
  for (int k = 0; k < 12; ++k) r.pose[k] = poses[12 * v + k];
  r.status = views[v].fixed ? RGBID_COLOURALIGN_FIXED : RGBID_COLOURALIGN_RUNNING;
  r.iterations = 0;
  r.used[0] = r.used[1] = 0u;
  for (int k = 0; k < GN_TERMS; ++k) r.sums[0][k] = r.sums[1][k] = 0.0;
}

// step 2: one thread per view
__global__ __launch_bounds__(VT) void k_ca_pose(const rgbid_colouralign_result* __restrict__ res, int V, CaView* __restrict__ views) {
  RGBID_FP_STRICT
  const int v = blockIdx.x * VT + threadIdx.x;
  if (v >= V) return;
  const double* R = res[v].pose;
  const double* t = R + 9;
  float* m = views[v].m;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) m[3 * i + j] = (float)R[3 * j + i];
    m[9 + i] = (float)(-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]));
  }
}

// step 5: one thread per lattice vertex, the views in order; state: S [n_l], W [n_l] uint64, used [n_l] uint32
// CHUNKS false: the whole view table, the state written once.  CHUNKS true: blockIdx.y walks TARGET_CHUNK views and adds what it found to
// the cleared state with integer atomics: the sums are integers, so the bytes are the same in any order
template <bool CHUNKS>
__global__ __launch_bounds__(VT) void k_ca_target(const float* __restrict__ pos, const float* __restrict__ normals, CaLattice lt,
                                                  const CaView* __restrict__ views, int V, ViewCam cam, unsigned long long* __restrict__ S_plane,
                                                  unsigned long long* __restrict__ W_plane, unsigned* __restrict__ used_plane) {
  const unsigned j = blockIdx.x * VT + threadIdx.x;
  if (j >= lt.n_l) return;
  const size_t i = (size_t)j * lt.stride;                   // < n: n_l = ceil(n / stride)
  const CaVertex p = ca_vertex(pos, normals, i);
  unsigned long long S = 0, W = 0;
  unsigned used = 0;
  const int v0 = CHUNKS ? (int)blockIdx.y * TARGET_CHUNK : 0;
  const int v1 = CHUNKS ? min(v0 + TARGET_CHUNK, V) : V;
  for (int v = v0; v < v1; ++v) {                            // the view's entry is wave-uniform
    CaSample o;
    if (ca_pair<false>(views[v], cam, p.x, p.y, p.z, p.fin, p.facing, p.n0, p.n1, p.n2, o)) {
      S += (unsigned long long)o.w * o.s;
      W += o.w;
      ++used;
    }
  }
  if (!CHUNKS) {
    S_plane[j] = S; W_plane[j] = W; used_plane[j] = used;
  } else if (used) {
    atomicAdd(S_plane + j, S); atomicAdd(W_plane + j, W); atomicAdd(used_plane + j, used);
  }
}

// step 6: one thread per lattice vertex, a wave per group of 64, a block four groups of the view blockIdx.y.  Lanes beyond the lattice and
// pairs that are not used stay in the wave with +0.0: the butterflies need all 64.  No LDS, no atomic.
__global__ __launch_bounds__(VT) void k_ca_system(const float* __restrict__ pos, const float* __restrict__ normals, CaLattice lt,
                                                  const CaView* __restrict__ views, ViewCam cam, CaRule rule,
                                                  const unsigned long long* __restrict__ S_plane, const unsigned long long* __restrict__ W_plane,
                                                  const unsigned* __restrict__ used_plane, const rgbid_colouralign_result* __restrict__ res,
                                                  double* __restrict__ sums, unsigned* __restrict__ used, size_t a_stride) {
  RGBID_FP_STRICT
  const unsigned view = blockIdx.y;
  if (ca_status(res, view, lt.restart) != RGBID_COLOURALIGN_RUNNING) return;   // a stopped or fixed view's blocks leave at once
  const unsigned group = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (group >= lt.groups) return;                               // the whole wave
  const unsigned lane = threadIdx.x & 63u, j = group * 64u + lane;
  const CaView& vw = views[view];                               // block-uniform
  double tm[GN_TERMS];
#pragma unroll
  for (int k = 0; k < GN_TERMS; ++k) tm[k] = 0.0;
  bool is_used = false;
  if (j < lt.n_l && used_plane[j] >= rule.min_views) {          // the vertex has a target
    const size_t i = (size_t)j * lt.stride;
    const CaVertex p = ca_vertex(pos, normals, i);
    CaSample o;
    if (ca_pair<true>(vw, cam, p.x, p.y, p.z, p.fin, p.facing, p.n0, p.n1, p.n2, o)) {
      is_used = true;
      const double C = (double)S_plane[j] / ((double)W_plane[j] * 16777216.0);
      const double g = (double)o.s / 16777216.0, dx = (double)o.Gx / 65536.0, dy = (double)o.Gy / 65536.0;
      const double f = g - C;
      const double X = (double)o.X, Y = (double)o.Y, Z = (double)o.Z;
      const double iz = 1.0 / Z;
      const double a = (dx * (double)cam.fx) * iz, b = (dy * (double)cam.fy) * iz;
      const double c = -((a * X + b * Y) * iz);
      const float* r = vw.m;
      const double m0 = ((double)r[0] * a + (double)r[3] * b) + (double)r[6] * c;
      const double m1 = ((double)r[1] * a + (double)r[4] * b) + (double)r[7] * c;
      const double m2 = ((double)r[2] * a + (double)r[5] * b) + (double)r[8] * c;
      const double p0 = (double)p.x, p1 = (double)p.y, p2 = (double)p.z;
      const double J[6] = {-m0, -m1, -m2, -(p1 * m2 - p2 * m1), -(p2 * m0 - p0 * m2), -(p0 * m1 - p1 * m0)};
      const double af = fabs(f);
      const double wh = af <= rule.huber ? 1.0 : rule.huber / af;
      double aa[6];
#pragma unroll
      for (int q = 0; q < 6; ++q) aa[q] = wh * J[q];
      int k = 0;
#pragma unroll
      for (int q = 0; q < 6; ++q)
#pragma unroll
        for (int jj = q; jj < 6; ++jj) tm[k++] = aa[q] * J[jj];
#pragma unroll
      for (int q = 0; q < 6; ++q) tm[21 + q] = aa[q] * f;
      tm[27] = (wh * f) * f;
    }
  }
  const unsigned long long any = __ballot(is_used);
  if (any) {                                                    // wave-uniform: a wave without a used pair keeps its 28 x +0.0
#pragma unroll
    for (int k = 0; k < GN_TERMS; ++k) tm[k] = gn_tree64(tm[k]);
  }
  if (lane == 0) {
    double* o = sums + (size_t)view * GN_TERMS * a_stride + group;
#pragma unroll
    for (int k = 0; k < GN_TERMS; ++k) o[(size_t)k * a_stride] = tm[k];
    used[(size_t)view * a_stride + group] = (unsigned)__popcll(any);
  }
}

// One block per view: the upper rounds of step 6 between the two buffers, then thread 0 walks step 7 in double.
__global__ __launch_bounds__(VT) void k_ca_solve(CaWork w, CaRule rule, CaLattice lt, rgbid_colouralign_result* res) {
  RGBID_FP_STRICT
  __shared__ unsigned lds[WAVES];
  const unsigned view = blockIdx.x;
  if (ca_status(res, view, lt.restart) != RGBID_COLOURALIGN_RUNNING) return;   // the whole block
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  // the used pairs: an integer sum, the same in any order
  unsigned cnt = 0;
  for (unsigned i = threadIdx.x; i < lt.groups; i += VT) cnt += w.used[(size_t)view * w.a_stride + i];
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) cnt += __shfl_xor(cnt, m);
  if (lane == 0) lds[wave] = cnt;
  double* src = w.a + (size_t)view * GN_TERMS * w.a_stride;
  size_t src_stride = w.a_stride;
  gn_upper_tree(src, src_stride, w.b + (size_t)view * GN_TERMS * w.b_stride, w.b_stride, lt.groups);
  rgbid_colouralign_result& r = res[view];
  const bool first = r.iterations == 0;
  __syncthreads();                                              // everybody has read the count of systems before thread 0 raises it
  if (threadIdx.x < GN_TERMS) {                                 // step 8: the first and the last system built
    const double s = gn_canonical_nan(src[(size_t)threadIdx.x * src_stride]);
    r.sums[1][threadIdx.x] = s;
    if (first) r.sums[0][threadIdx.x] = s;
  }
  if (threadIdx.x != 0) return;
  static_assert(WAVES == 4, "four waves left their counts");
  const unsigned n_used = lds[0] + lds[1] + lds[2] + lds[3];
  r.used[1] = n_used;
  if (first) r.used[0] = n_used;
  r.iterations += 1;
  if (n_used < rule.min_pairs) { r.status = RGBID_COLOURALIGN_FEW; return; }
  double x[6], biggest;
  if (!gn_solve(src, src_stride, rule.damping, x, biggest)) { r.status = RGBID_COLOURALIGN_SINGULAR; return; }
  double P[12], Q[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = r.pose[k];
  gn_retract(P, x, Q);
#pragma unroll
  for (int k = 0; k < 12; ++k) r.pose[k] = gn_canonical_nan(Q[k]);
  r.status = biggest < rule.eps ? RGBID_COLOURALIGN_CONVERGED : RGBID_COLOURALIGN_RUNNING;
}

// one thread per output texel and channel: the mean over the f x f box, halves rounded up
__global__ __launch_bounds__(VT) void k_ca_downscale(const unsigned char* __restrict__ in, int cols, int f, int orows, int ocols,
                                                     unsigned char* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * VT + threadIdx.x, total = (size_t)orows * ocols * 3;
  if (e >= total) return;
  const int k = (int)(e % 3);
  const size_t t = e / 3;
  const int ox = (int)(t % (size_t)ocols), oy = (int)(t / (size_t)ocols);
  unsigned sum = 0;                                             // <= 255 * 16 * 16
  for (int y = 0; y < f; ++y)                                   // oy f + y <= orows f - 1 < rows, ox f + x < cols
    for (int x = 0; x < f; ++x) sum += in[3 * ((size_t)(oy * f + y) * (size_t)cols + (size_t)(ox * f + x)) + k];
  const unsigned ff = (unsigned)(f * f);
  out[e] = (unsigned char)((2u * sum + ff) / (2u * ff));
}

}  // namespace

struct rgbid_colouralign {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_n = 0;
  int cap_v = 0;
  unsigned long long* S = nullptr;         // [cap_n] the last target pass
  unsigned long long* W = nullptr;         // [cap_n]
  unsigned* used = nullptr;                // [cap_n]
  CaView* views = nullptr;                 // [cap_v] the view table
  CaView* views_host = nullptr;            // pinned
  double* poses = nullptr;                 // [cap_v][12] the poses a call starts from
  double* poses_host = nullptr;            // pinned
  hipEvent_t copied = nullptr;             // the last call's copies have read the pinned tables
  CaWork w = {};
  bool ran = false;
  int target_form = RGBID_COLOURALIGN_TARGET_AUTO;
  unsigned n_l = 0;                        // the last run's lattice
  // stage timing: event 0 after the init and the first pose pass, then per round one after the target and per iteration one after the
  // system and one after the solve and its pose pass
  int timed_rounds = 0, timed_iterations = 0;
  Buffers buf;
  StageTimer<MAX_IT * 3 + 1> timer;
  ~rgbid_colouralign() {
    if (copied) (void)hipEventDestroy(copied);
  }
};

extern "C" {

int rgbid_colouralign_create(rgbid_colouralign** out, rgbid_ctx* ctx, unsigned long long max_vertices, int max_views) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_vertices < 1 || max_vertices > RGBID_COLOURALIGN_MAX_VERTICES || max_views < 1 || max_views > RGBID_COLOURALIGN_MAX_VIEWS)
    return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_colouralign* h = new (std::nothrow) rgbid_colouralign;
  if (!h) return RGBID_E_NOMEM;
  h->ctx = ctx;
  h->cap_n = max_vertices;
  h->cap_v = max_views;
  const size_t n = (size_t)max_vertices, V = (size_t)max_views;
  h->w.a_stride = (n + 63) / 64;
  h->w.b_stride = (h->w.a_stride + 63) / 64;
  int r = h->buf.alloc(&h->S, sizeof(unsigned long long) * n);
  if (!r) r = h->buf.alloc(&h->W, sizeof(unsigned long long) * n);
  if (!r) r = h->buf.alloc(&h->used, sizeof(unsigned) * n);
  if (!r) r = h->buf.alloc(&h->views, sizeof(CaView) * V);
  if (!r) r = h->buf.alloc_host(&h->views_host, sizeof(CaView) * V);
  if (!r) r = h->buf.alloc(&h->poses, sizeof(double) * 12 * V);
  if (!r) r = h->buf.alloc_host(&h->poses_host, sizeof(double) * 12 * V);
  if (!r) r = h->buf.alloc(&h->w.a, sizeof(double) * GN_TERMS * h->w.a_stride * V);
  if (!r) r = h->buf.alloc(&h->w.b, sizeof(double) * GN_TERMS * h->w.b_stride * V);
  if (!r) r = h->buf.alloc(&h->w.used, sizeof(unsigned) * h->w.a_stride * V);
  if (!r) r = hip_status(hipEventCreateWithFlags(&h->copied, hipEventDisableTiming));
  if (r) { destroy_handle(h); return r; }
  *out = h;
  return RGBID_OK;
}

int rgbid_colouralign_destroy(rgbid_colouralign* h) { return destroy_handle(h); }

int rgbid_colouralign_run(rgbid_colouralign* h, const float* vertices_dev, const float* normals_dev, unsigned long long n, int V,
                          const rgbid_colouralign_view* views, const float K[4], int rows, int cols, const rgbid_recolour_params* params,
                          const rgbid_colouralign_rule* rule, rgbid_colouralign_result* result_dev) {
  if (!h || !views || !K || !params || !rule || !result_dev) return RGBID_E_INVALID;
  if (n > h->cap_n || V < 1 || V > h->cap_v) return RGBID_E_INVALID;
  if (!view_camera_ok(K, rows, cols, *params)) return RGBID_E_INVALID;
  if (n && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  if (!aligned4(normals_dev)) return RGBID_E_INVALID;
  const rgbid_colouralign_rule& q = *rule;
  if (!(std::isfinite(q.huber) && q.huber > 0.f)) return RGBID_E_INVALID;
  if (!(std::isfinite(q.damping) && q.damping >= 0.0)) return RGBID_E_INVALID;
  if (!(std::isfinite(q.eps) && q.eps > 0.0)) return RGBID_E_INVALID;
  if (q.min_pairs < 6 || q.min_views < 2) return RGBID_E_INVALID;
  if (q.rounds < 1 || q.iterations < 1 || q.stride < 1 || q.rounds > MAX_IT || q.iterations > MAX_IT || q.rounds * q.iterations > MAX_IT)
    return RGBID_E_INVALID;
  if (((uintptr_t)result_dev) & 7) return RGBID_E_INVALID;
  for (int v = 0; v < V; ++v)
    if ((views[v].fixed != 0 && views[v].fixed != 1) || !view_ok(views[v].view)) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const bool timing = h->timer.on;
  h->timed_rounds = h->timed_iterations = 0;
  RGBID_HIP(hipEventSynchronize(h->copied));      // the previous call's copies have read the pinned tables (nothing was recorded: returns at once)
  for (int v = 0; v < V; ++v) {
    const rgbid_recolour_view& in = views[v].view;
    CaView& o = h->views_host[v];
    for (int k = 0; k < 12; ++k) o.m[k] = 0.f;
    o.colour = in.colour_dev; o.surface = in.surface_dev; o.measured = in.measured_dev;
    o.fixed = views[v].fixed; o.pad = 0;
    for (int k = 0; k < 9; ++k) h->poses_host[12 * v + k] = in.pose.R[k];
    for (int k = 0; k < 3; ++k) h->poses_host[12 * v + 9 + k] = in.pose.t[k];
  }
  RGBID_HIP(hipMemcpyAsync(h->views, h->views_host, sizeof(CaView) * (size_t)V, hipMemcpyHostToDevice, s));
  RGBID_HIP(hipMemcpyAsync(h->poses, h->poses_host, sizeof(double) * 12 * (size_t)V, hipMemcpyHostToDevice, s));
  RGBID_HIP(hipEventRecord(h->copied, s));
  const ViewCam cam = view_cam(K, rows, cols, *params);
  CaLattice lt{};
  lt.stride = (unsigned)q.stride;
  lt.n_l = (unsigned)((n + lt.stride - 1) / lt.stride);         // n is 2^31 at most
  lt.groups = lt.n_l ? (lt.n_l + 63u) / 64u : 1u;
  const CaRule cr{q.damping, q.eps, (double)q.huber, q.min_pairs, q.min_views};
  const dim3 block(VT), per_view(((unsigned)V + VT - 1) / VT);
  // the target pass: a vertex per thread over all views, or, with more views than one chunk, over chunks of views (measured faster at
  // 64 and 512 views from 4 747 to 303 776 vertices; with one chunk it would be the walk plus clearing and atomics)
  const unsigned target_blocks = (lt.n_l + VT - 1) / VT;
  const bool chunked = h->target_form == RGBID_COLOURALIGN_TARGET_CHUNKS || (h->target_form == RGBID_COLOURALIGN_TARGET_AUTO && V > TARGET_CHUNK);
  hipLaunchKernelGGL(k_ca_init, per_view, block, 0, s, h->poses, h->views, V, result_dev);
  hipLaunchKernelGGL(k_ca_pose, per_view, block, 0, s, result_dev, V, h->views);
  int e = 0;
  h->timer.mark(e++, s);
  for (int r = 0; r < q.rounds; ++r) {                           // enqueued without waiting: the device decides who still runs
    if (lt.n_l && chunked) {
      RGBID_HIP(hipMemsetAsync(h->S, 0, sizeof(unsigned long long) * lt.n_l, s));
      RGBID_HIP(hipMemsetAsync(h->W, 0, sizeof(unsigned long long) * lt.n_l, s));
      RGBID_HIP(hipMemsetAsync(h->used, 0, sizeof(unsigned) * lt.n_l, s));
      hipLaunchKernelGGL(k_ca_target<true>, dim3(target_blocks, ((unsigned)V + TARGET_CHUNK - 1) / TARGET_CHUNK), block, 0, s, vertices_dev, normals_dev, lt,
                         h->views, V, cam, h->S, h->W, h->used);
    } else if (lt.n_l) {
      hipLaunchKernelGGL(k_ca_target<false>, dim3(target_blocks), block, 0, s, vertices_dev, normals_dev, lt, h->views, V, cam, h->S, h->W, h->used);
    }
    h->timer.mark(e++, s);
    for (int it = 0; it < q.iterations; ++it) {
      lt.restart = it == 0 ? 1u : 0u;
      hipLaunchKernelGGL(k_ca_system, dim3((lt.groups + WAVES - 1) / WAVES, (unsigned)V), block, 0, s, vertices_dev, normals_dev, lt, h->views, cam, cr,
                         h->S, h->W, h->used, result_dev, h->w.a, h->w.used, h->w.a_stride);
      h->timer.mark(e++, s);
      hipLaunchKernelGGL(k_ca_solve, dim3((unsigned)V), block, 0, s, h->w, cr, lt, result_dev);
      hipLaunchKernelGGL(k_ca_pose, per_view, block, 0, s, result_dev, V, h->views);
      h->timer.mark(e++, s);
    }
  }
  RGBID_HIP(hipGetLastError());
  h->ran = true;
  h->n_l = lt.n_l;
  if (timing) { h->timed_rounds = q.rounds; h->timed_iterations = q.iterations; }
  return RGBID_OK;
}

int rgbid_colouralign_targets(rgbid_colouralign* h, uint64_t* S_out_dev, uint64_t* W_out_dev, uint32_t* used_out_dev) {
  if (!h || !h->ran) return RGBID_E_INVALID;
  if ((((uintptr_t)S_out_dev) & 7) || (((uintptr_t)W_out_dev) & 7) || !aligned4(used_out_dev)) return RGBID_E_INVALID;
  if (!h->n_l) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  const size_t n = h->n_l;
  if (S_out_dev) RGBID_HIP(hipMemcpyAsync(S_out_dev, h->S, sizeof(uint64_t) * n, hipMemcpyDeviceToDevice, s));
  if (W_out_dev) RGBID_HIP(hipMemcpyAsync(W_out_dev, h->W, sizeof(uint64_t) * n, hipMemcpyDeviceToDevice, s));
  if (used_out_dev) RGBID_HIP(hipMemcpyAsync(used_out_dev, h->used, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, s));
  return RGBID_OK;
}

int rgbid_colouralign_set_target_form(rgbid_colouralign* h, int form) {
  if (!h || form < RGBID_COLOURALIGN_TARGET_AUTO || form > RGBID_COLOURALIGN_TARGET_CHUNKS) return RGBID_E_INVALID;
  h->target_form = form;
  return RGBID_OK;
}

int rgbid_colouralign_downscale(rgbid_colouralign* h, const uint8_t* in_dev, int rows, int cols, int f, uint8_t* out_dev) {
  if (!h || !in_dev || !out_dev) return RGBID_E_INVALID;
  if (rows < 1 || cols < 1 || rows > RGBID_RASTER_MAX_DIM || cols > RGBID_RASTER_MAX_DIM) return RGBID_E_INVALID;
  if (f < 1 || f > RGBID_COLOURALIGN_MAX_FACTOR || rows / f < 1 || cols / f < 1) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  const int orows = rows / f, ocols = cols / f;
  const size_t total = (size_t)orows * ocols * 3;               // below 2^30
  hipLaunchKernelGGL(k_ca_downscale, dim3((unsigned)((total + VT - 1) / VT)), dim3(VT), 0, h->ctx->stream, in_dev, cols, f, orows, ocols, out_dev);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_colouralign_timing(rgbid_colouralign* h, int enable, float ms[3]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  if (ms) {
    ms[0] = ms[1] = ms[2] = 0.f;
    int e = 0;                                                  // the event before the stage that follows
    for (int r = 0; r < h->timed_rounds; ++r) {
      float one = 0.f;
      RGBID_HIP(h->timer.elapsed(e, e + 1, &one));
      ms[0] += one; ++e;
      for (int it = 0; it < h->timed_iterations; ++it)
        for (int k = 1; k < 3; ++k) {
          RGBID_HIP(h->timer.elapsed(e, e + 1, &one));
          ms[k] += one; ++e;
        }
    }
  }
  return h->timer.enable(enable != 0);
}

}  // extern "C"
