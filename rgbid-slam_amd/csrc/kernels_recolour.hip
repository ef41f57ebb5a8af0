// kernels_recolour.hip -- the vertices of a mesh coloured from the keyframes that see them (include/rgbid_recolour.h).
//
// The judge is tests/recolour_mirror.py; colours, views_used, best_view and the six counts per view are byte-identical to it.
//   k_recolour_add<BEST>     one thread per vertex, per chunk of up to RGBID_RECOLOUR_VIEW_CHUNK views, whose twelve floats and three plane
//                            pointers each sit in the kernel arguments: position, normal and state are read once, the views are walked in
//                            order with the state in registers, the state is written once.  Nobody else touches a vertex's state: no atomics
//                            on it.  The class of every (vertex, view) pair is counted by ballot and popcount per wave; the block's four
//                            waves meet in LDS and the block issues one 64-bit atomic per view and non-zero class
//   k_recolour_finish<BEST>  one thread per vertex: state -> colour, views_used, best_view; the state is only read
// State, [n_v] each (n_v is begin's): four uint64 planes -- MEAN S_0 S_1 S_2 W, BEST s_0 s_1 s_2 key -- and one uint32 plane `used`.
//
// Exact arithmetic: every function that forms a product followed by a sum opens with RGBID_FP_STRICT (common.h), so the compiler forms no
// FMA from them; division and square root are hipcc's default correctly rounded ones.
#include "../../include/rgbid_recolour.h"
#include "common.h"
#include "hip_host.h"
#include "view_device.h"    // the view entry, rot_row, the texel tests, the accumulation, the class tally, step 7's byte; the host's checks

#include <cmath>
#include <new>

using namespace rgbid;

namespace {

constexpr int VT = VIEW_BLOCK;                              // threads of a block: four waves
constexpr int CHUNK = VIEWS_PER_CHUNK;

// steps 3 - 6 of one chunk of views.  counts: the count lines of the launch's first view
template <bool BEST>
__global__ __launch_bounds__(VT) void k_recolour_add(const float* __restrict__ pos, const float* __restrict__ normals, unsigned n_v, ViewChunk vw,
                                                     ViewCam cam, int nv, unsigned first_view, unsigned long long* __restrict__ state,
                                                     unsigned* __restrict__ used_plane, unsigned long long* __restrict__ counts) {
  RGBID_FP_STRICT
  __shared__ unsigned tally[VIEW_WAVES][CHUNK * VIEW_N_COUNTS];
  const unsigned i = blockIdx.x * VT + threadIdx.x;
  const bool live = i < n_v;
  float x = 0.f, y = 0.f, z = 0.f, n0 = 0.f, n1 = 0.f, n2 = 0.f;
  bool fin = false, facing = false;
  unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;       // MEAN: S_0 S_1 S_2 W; BEST: s_0 s_1 s_2 key
  unsigned used = 0;
  if (live) {
    x = pos[3 * (size_t)i]; y = pos[3 * (size_t)i + 1]; z = pos[3 * (size_t)i + 2];
    fin = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(z);
    if (normals) {
      n0 = normals[3 * (size_t)i]; n1 = normals[3 * (size_t)i + 1]; n2 = normals[3 * (size_t)i + 2];
      const float q = (n0 * n0 + n1 * n1) + n2 * n2;
      facing = __builtin_isfinite(q) && q != 0.f;
    }
    a0 = state[i]; a1 = state[(size_t)n_v + i]; a2 = state[2 * (size_t)n_v + i]; a3 = state[3 * (size_t)n_v + i];
    used = used_plane[i];
  }
  const int last_x = 256 * (cam.cols - 1), last_y = 256 * (cam.rows - 1);   // dims <= 16384: below 2^22
  for (int v = 0; v < nv; ++v) {
    const ViewEntry& view = vw.v[v];                        // wave-uniform: scalar registers
    const float* m = view.m;
    int cls = -1;                                           // a thread behind the last vertex has no class
    if (live) {
      cls = VIEW_GATED;
      if (fin) {
        const float Z = rot_row(m + 6, x, y, z) + m[11];
        if (Z >= cam.z_min && Z <= cam.z_max) {             // NaN fails; z_max is finite, so infinity does too
          const float X = rot_row(m, x, y, z) + m[9];
          const float Y = rot_row(m + 3, x, y, z) + m[10];
          const float u = cam.fx * (X / Z) + cam.cx;
          const float w_ = cam.fy * (Y / Z) + cam.cy;
          const float xf = floorf(u * 256.0f + 0.5f);
          const float yf = floorf(w_ * 256.0f + 0.5f);
          if (fabsf(xf) <= 8388608.f && fabsf(yf) <= 8388608.f) {   // in float: nothing out of range reaches the cast
            const int xs = (int)xf, ys = (int)yf;
            cls = VIEW_OUTSIDE;
            if (xs >= 0 && xs <= last_x && ys >= 0 && ys <= last_y) {
              const int x0 = xs >> 8, y0 = ys >> 8, x1 = min(x0 + 1, cam.cols - 1), y1 = min(y0 + 1, cam.rows - 1);
              const unsigned ax = (unsigned)(xs & 255), ay = (unsigned)(ys & 255);
              // every texel index lies in the plane: 0 <= x0 <= x1 <= cols - 1, 0 <= y0 <= y1 <= rows - 1
              const size_t r0 = (size_t)y0 * (size_t)cam.cols, r1 = (size_t)y1 * (size_t)cam.cols;
              const size_t t00 = r0 + (size_t)x0, t10 = r0 + (size_t)x1, t01 = r1 + (size_t)x0, t11 = r1 + (size_t)x1;
              cls = VIEW_TAKEN;
              if (view.surface) {
                const float* d = view.surface;
                const float d00 = d[t00], d10 = d[t10], d01 = d[t01], d11 = d[t11];
                if (!(surface_ok(d00, Z, cam.tol_surface) && surface_ok(d10, Z, cam.tol_surface) && surface_ok(d01, Z, cam.tol_surface) &&
                      surface_ok(d11, Z, cam.tol_surface)))
                  cls = VIEW_HIDDEN;
              }
              if (cls == VIEW_TAKEN && view.measured) {
                const float* d = view.measured;
                const float m00 = d[t00], m10 = d[t10], m01 = d[t01], m11 = d[t11];
                if (!(measured_ok(m00, Z, cam.tol_measured) && measured_ok(m10, Z, cam.tol_measured) && measured_ok(m01, Z, cam.tol_measured) &&
                      measured_ok(m11, Z, cam.tol_measured)))
                  cls = VIEW_UNMEASURED;
              }
              unsigned w = RGBID_RECOLOUR_UNIT_WEIGHT;
              if (cls == VIEW_TAKEN && facing) {
                const double c0 = (double)rot_row(m, n0, n1, n2), c1 = (double)rot_row(m + 3, n0, n1, n2), c2 = (double)rot_row(m + 6, n0, n1, n2);
                const double Xd = (double)X, Yd = (double)Y, Zd = (double)Z;
                const double dot = -((c0 * Xd + c1 * Yd) + c2 * Zd);
                const double gg = (c0 * c0 + c1 * c1) + c2 * c2;
                const double rr = (Xd * Xd + Yd * Yd) + Zd * Zd;
                double cs = dot / sqrt(gg * rr);
                if (cam.two_sided) cs = fabs(cs);
                if (cs > 0.0 && cs >= cam.min_cos) {        // a NaN fails; cs <= 1 up to rounding, so the cast is in range
                  const unsigned f = (unsigned)floor(cs * 1024.0 + 0.5);
                  w = f < 1u ? 1u : f;
                } else {
                  cls = VIEW_AVERTED;
                }
              }
              if (cls == VIEW_TAKEN)
                view_accumulate<BEST>(view.colour, ViewSample{X, Y, Z, w, ax, ay, t00, t10, t01, t11}, first_view + (unsigned)v, a0, a1, a2, a3, used);
            }
          }
        }
      }
    }
    view_tally(tally, v, cls);
  }
  if (live) {
    state[i] = a0; state[(size_t)n_v + i] = a1; state[2 * (size_t)n_v + i] = a2; state[3 * (size_t)n_v + i] = a3;
    used_plane[i] = used;
  }
  view_tally_add(tally, nv, counts);
}

// step 7.  colours_in and colours_out may be the same buffer: a thread reads its three bytes before it writes them
template <bool BEST>
__global__ __launch_bounds__(VT) void k_recolour_finish(const unsigned long long* __restrict__ state, const unsigned* __restrict__ used_plane, unsigned n_v,
                                                        const unsigned char* colours_in, unsigned char* colours_out, unsigned* __restrict__ views_used,
                                                        unsigned* __restrict__ best_view) {
  const unsigned i = blockIdx.x * VT + threadIdx.x;
  if (i >= n_v) return;
  const unsigned used = used_plane[i];
  if (views_used) views_used[i] = used;
  const unsigned long long a3 = state[3 * (size_t)n_v + i];
  if (BEST && best_view) best_view[i] = used ? 0xFFFFFFFFu - (unsigned)a3 : RGBID_RECOLOUR_NO_VIEW;
  if (!colours_out) return;
  unsigned char rgb[3] = {0, 0, 0};
  if (used) {
    for (int k = 0; k < 3; ++k) rgb[k] = view_state_byte<BEST>(state[(size_t)k * n_v + i], a3);
  } else if (colours_in) {
    for (int k = 0; k < 3; ++k) rgb[k] = colours_in[3 * (size_t)i + k];
  }
  for (int k = 0; k < 3; ++k) colours_out[3 * (size_t)i + k] = rgb[k];
}

enum { M_ADD0 = 0, M_ADD1, M_FIN0, M_FIN1, MARKS };

}  // namespace

struct rgbid_recolour {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_v = 0;
  unsigned long long* state = nullptr;         // 36 bytes per vertex of capacity: [4][n_v] uint64, then [n_v] uint32
  unsigned long long* counts = nullptr;        // [MAX_VIEWS][VIEW_COUNT_LINE]
  bool begun = false;
  unsigned long long n_v = 0;                  // begin's
  int mode = RGBID_RECOLOUR_MEAN, views = 0;   // views since begin
  bool timed[2] = {false, false};              // whether the last add / the last finish was recorded
  Buffers buf;
  StageTimer<MARKS> timer;
  unsigned* used_plane() const { return reinterpret_cast<unsigned*>(state + 4 * n_v); }
};

extern "C" {

int rgbid_recolour_create(rgbid_recolour** out, rgbid_ctx* ctx, unsigned long long max_vertices) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_vertices < 1 || max_vertices > RGBID_RECOLOUR_MAX_VERTICES) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_recolour* r = new (std::nothrow) rgbid_recolour;
  if (!r) return RGBID_E_NOMEM;
  r->ctx = ctx;
  r->cap_v = max_vertices;
  int e = r->buf.alloc(&r->state, (size_t)max_vertices * 36 + 4);   // the uint32 plane ends on a whole 8 bytes
  if (!e) e = r->buf.alloc(&r->counts, sizeof(unsigned long long) * VIEW_COUNT_LINE * RGBID_RECOLOUR_MAX_VIEWS);
  if (e) { destroy_handle(r); return e; }
  *out = r;
  return RGBID_OK;
}

int rgbid_recolour_destroy(rgbid_recolour* r) { return destroy_handle(r); }   // a launch may still read the state

int rgbid_recolour_begin(rgbid_recolour* r, unsigned long long n_vertices, int mode) {
  if (!r || n_vertices > r->cap_v || (mode != RGBID_RECOLOUR_MEAN && mode != RGBID_RECOLOUR_BEST)) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  if (n_vertices) RGBID_HIP(hipMemsetAsync(r->state, 0, (size_t)n_vertices * 36, r->ctx->stream));
  r->begun = true; r->n_v = n_vertices; r->mode = mode; r->views = 0;   // a view's count line is cleared when the view is added
  return RGBID_OK;
}

int rgbid_recolour_add(rgbid_recolour* r, const float* vertices_dev, const float* normals_dev, unsigned long long n_vertices, int V,
                       const rgbid_recolour_view* views, const float K[4], int rows, int cols, const rgbid_recolour_params* params) {
  if (!r || !views || !K || !params || V < 1 || !r->begun || V > RGBID_RECOLOUR_MAX_VIEWS - r->views) return RGBID_E_INVALID;
  if (n_vertices != r->n_v || n_vertices > r->cap_v) return RGBID_E_INVALID;
  if (!view_camera_ok(K, rows, cols, *params)) return RGBID_E_INVALID;
  if (n_vertices && (!vertices_dev || !aligned4(vertices_dev))) return RGBID_E_INVALID;
  if (!aligned4(normals_dev)) return RGBID_E_INVALID;
  for (int v = 0; v < V; ++v) if (!view_ok(views[v])) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  hipStream_t st = r->ctx->stream;
  const unsigned n_v = (unsigned)n_vertices;                // 2^31 at most
  unsigned long long* lines = r->counts + (size_t)r->views * VIEW_COUNT_LINE;
  RGBID_HIP(hipMemsetAsync(lines, 0, sizeof(unsigned long long) * VIEW_COUNT_LINE * (size_t)V, st));
  const ViewCam cam = view_cam(K, rows, cols, *params);
  r->timed[0] = false;
  r->timer.mark(M_ADD0, st);
  ViewChunk vw;
  for (int v0 = 0; n_v && v0 < V; v0 += CHUNK) {
    const int nv = V - v0 < CHUNK ? V - v0 : CHUNK;
    view_pack(views + v0, nv, vw);
    const unsigned first_view = (unsigned)(r->views + v0);  // global index of the launch's first view
    const dim3 grid((n_v + VT - 1) / VT), block(VT);
    if (r->mode == RGBID_RECOLOUR_BEST)
      hipLaunchKernelGGL(k_recolour_add<true>, grid, block, 0, st, vertices_dev, normals_dev, n_v, vw, cam, nv, first_view, r->state, r->used_plane(),
                         lines + (size_t)v0 * VIEW_COUNT_LINE);
    else
      hipLaunchKernelGGL(k_recolour_add<false>, grid, block, 0, st, vertices_dev, normals_dev, n_v, vw, cam, nv, first_view, r->state, r->used_plane(),
                         lines + (size_t)v0 * VIEW_COUNT_LINE);
  }
  r->timer.mark(M_ADD1, st);
  r->timed[0] = r->timer.on;
  RGBID_HIP(hipGetLastError());
  r->views += V;
  return RGBID_OK;
}

int rgbid_recolour_finish(rgbid_recolour* r, const uint8_t* colours_in_dev, uint8_t* colours_out_dev, uint32_t* views_used_dev,
                          uint32_t* best_view_dev) {
  if (!r || !r->begun || !aligned4(views_used_dev) || !aligned4(best_view_dev)) return RGBID_E_INVALID;
  if (best_view_dev && r->mode != RGBID_RECOLOUR_BEST) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  hipStream_t st = r->ctx->stream;
  const unsigned n_v = (unsigned)r->n_v;
  r->timed[1] = false;
  r->timer.mark(M_FIN0, st);
  if (n_v && (colours_out_dev || views_used_dev || best_view_dev)) {
    const dim3 grid((n_v + VT - 1) / VT), block(VT);
    if (r->mode == RGBID_RECOLOUR_BEST)
      hipLaunchKernelGGL(k_recolour_finish<true>, grid, block, 0, st, r->state, r->used_plane(), n_v, colours_in_dev, colours_out_dev, views_used_dev, best_view_dev);
    else
      hipLaunchKernelGGL(k_recolour_finish<false>, grid, block, 0, st, r->state, r->used_plane(), n_v, colours_in_dev, colours_out_dev, views_used_dev, best_view_dev);
  }
  r->timer.mark(M_FIN1, st);
  r->timed[1] = r->timer.on;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_recolour_counts(rgbid_recolour* r, int first_view, int V, unsigned long long* out) {
  if (!r || !out || !r->begun || first_view < 0 || V < 1 || first_view > r->views || V > r->views - first_view) return RGBID_E_INVALID;
  return view_counts_read(r->ctx, r->counts + (size_t)first_view * VIEW_COUNT_LINE, V, out);
}

int rgbid_recolour_timing(rgbid_recolour* r, int enable, float ms[2]) {
  if (!r) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  if (ms) {
    static const int pairs[2][4] = {{M_ADD0, M_ADD1, 0, 0}, {M_FIN0, M_FIN1, 0, 0}};
    if (int e = stage_times(r->timer, r->timed, pairs, ms)) return e;
  }
  return r->timer.enable(enable != 0);
}

}  // extern "C"
