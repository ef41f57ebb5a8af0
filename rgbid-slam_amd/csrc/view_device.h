// view_device.h -- what the operators that sample keyframes at projected points share (kernels_recolour.hip, kernels_texture.hip,
// kernels_colouralign.hip), and rot_row for every file that projects through twelve floats (kernels_raster.hip, kernels_render.hip,
// kernels_tsdf.hip, kernels_consist.hip).  Device half: the view entry and the camera, steps 3 - 4 of include/rgbid_recolour.h for one
// (point, view) pair as kernels_colouralign.hip walks it (the two add kernels keep theirs written out), the MEAN / BEST accumulation of
// steps 5 - 6, the class tally of a block and step 7's byte.  Host half: the checks of K, rows, cols, rgbid_recolour_params and a
// rgbid_recolour_view, the fill of the camera, the packing of a chunk of views and the read-back of the count lines.
// Everything has internal linkage, and nothing here is a kernel: an including file compiles what it calls.
//
// Exact arithmetic: every function that forms a product followed by a sum opens with RGBID_FP_STRICT (common.h), so the compiler forms no
// FMA from them; division and square root are hipcc's default correctly rounded ones.
#pragma once
#include "../../include/rgbid_recolour.h"
#include "common.h"
#include "hip_host.h"

#include <cmath>
#include <vector>

namespace rgbid {
namespace {

constexpr int VIEW_BLOCK = 256, VIEW_WAVES = VIEW_BLOCK / 64;   // the block of a kernel that tallies: four waves
constexpr int VIEWS_PER_CHUNK = RGBID_RECOLOUR_VIEW_CHUNK;
constexpr int VIEW_N_COUNTS = 6, VIEW_COUNT_LINE = 8;           // a view's six counts lie in one 64-byte line
enum { VIEW_GATED = 0, VIEW_OUTSIDE, VIEW_HIDDEN, VIEW_UNMEASURED, VIEW_AVERTED, VIEW_TAKEN };
static_assert(VIEWS_PER_CHUNK * VIEW_N_COUNTS <= VIEW_BLOCK, "one thread per (view, class) adds the block's counts up");

struct ViewEntry {
  float m[12];                                              // r00 r01 r02 r10 r11 r12 r20 r21 r22 tx ty tz
  const unsigned char* colour;
  const float* surface;
  const float* measured;
};
struct ViewChunk {                                          // kernel argument: 16 x 72 bytes
  ViewEntry v[VIEWS_PER_CHUNK];
};
struct ViewCam {
  double min_cos;
  float fx, fy, cx, cy, z_min, z_max, tol_surface, tol_measured;
  int rows, cols, two_sided;
};
// what steps 3 and 4 give for a TAKEN pair
struct ViewSample {
  float X, Y, Z;
  unsigned w, ax, ay;                                       // the weight; the 1/256 fractions of the bilinear sample
  size_t t00, t10, t01, t11;                                // the four texels, each inside the plane
};

__device__ __forceinline__ float rot_row(const float* __restrict__ m, float x, float y, float z) {
  RGBID_FP_STRICT
  return (m[0] * x + m[1] * y) + m[2] * z;
}

// step 4's test of one texel of the surface plane / the inverse-depth plane
__device__ __forceinline__ bool surface_ok(float d, float Z, float tol) { return __builtin_isfinite(d) && !(fabsf(Z - d) > tol); }
__device__ __forceinline__ bool measured_ok(float m, float Z, float tol) {
  if (!(__builtin_isfinite(m) && m > 0.f)) return false;
  const float z = 1.f / m;
  return __builtin_isfinite(z) && !(fabsf(Z - z) > tol);
}

// steps 3 and 4 of one pair -> its class; a TAKEN pair hands its sample to taken(const ViewSample&) before the return.  fin: the point is
// finite; facing: its normal has a finite, non-zero squared length.  kernels_colouralign.hip's pair.  k_recolour_add and k_texture_add
// keep the same sequence written out as nested ifs around rot_row, surface_ok, measured_ok and view_accumulate: through this function
// they lost a wave per SIMD or left the parent's time, so a change to the rule is made here and in those two;
// tests/test_gpu_view_rule.py holds the three to the same boundary table and to each other
template <class F>
__device__ __forceinline__ int view_sample(const ViewEntry& view, const ViewCam& cam, float x, float y, float z, bool fin, bool facing, float n0,
                                           float n1, float n2, F&& taken) {
  RGBID_FP_STRICT
  const float* m = view.m;
  const int last_x = 256 * (cam.cols - 1), last_y = 256 * (cam.rows - 1);   // dims <= 16384: below 2^22
  if (!fin) return VIEW_GATED;
  const float Z = rot_row(m + 6, x, y, z) + m[11];
  if (!(Z >= cam.z_min && Z <= cam.z_max)) return VIEW_GATED;   // NaN fails; z_max is finite, so infinity does too
  const float X = rot_row(m, x, y, z) + m[9];
  const float Y = rot_row(m + 3, x, y, z) + m[10];
  const float u = cam.fx * (X / Z) + cam.cx;
  const float w_ = cam.fy * (Y / Z) + cam.cy;
  const float xf = floorf(u * 256.0f + 0.5f);
  const float yf = floorf(w_ * 256.0f + 0.5f);
  if (!(fabsf(xf) <= 8388608.f && fabsf(yf) <= 8388608.f)) return VIEW_GATED;   // in float: nothing out of range reaches the cast
  const int xs = (int)xf, ys = (int)yf;
  if (!(xs >= 0 && xs <= last_x && ys >= 0 && ys <= last_y)) return VIEW_OUTSIDE;
  const int x0 = xs >> 8, y0 = ys >> 8, x1 = min(x0 + 1, cam.cols - 1), y1 = min(y0 + 1, cam.rows - 1);
  const unsigned ax = (unsigned)(xs & 255), ay = (unsigned)(ys & 255);
  // every texel index lies in the plane: 0 <= x0 <= x1 <= cols - 1, 0 <= y0 <= y1 <= rows - 1
  const size_t r0 = (size_t)y0 * (size_t)cam.cols, r1 = (size_t)y1 * (size_t)cam.cols;
  const size_t t00 = r0 + (size_t)x0, t10 = r0 + (size_t)x1, t01 = r1 + (size_t)x0, t11 = r1 + (size_t)x1;
  if (view.surface) {
    const float* d = view.surface;
    const float d00 = d[t00], d10 = d[t10], d01 = d[t01], d11 = d[t11];
    if (!(surface_ok(d00, Z, cam.tol_surface) && surface_ok(d10, Z, cam.tol_surface) && surface_ok(d01, Z, cam.tol_surface) &&
          surface_ok(d11, Z, cam.tol_surface)))
      return VIEW_HIDDEN;
  }
  if (view.measured) {
    const float* d = view.measured;
    const float m00 = d[t00], m10 = d[t10], m01 = d[t01], m11 = d[t11];
    if (!(measured_ok(m00, Z, cam.tol_measured) && measured_ok(m10, Z, cam.tol_measured) && measured_ok(m01, Z, cam.tol_measured) &&
          measured_ok(m11, Z, cam.tol_measured)))
      return VIEW_UNMEASURED;
  }
  unsigned w = RGBID_RECOLOUR_UNIT_WEIGHT;
  if (facing) {
    const double c0 = (double)rot_row(m, n0, n1, n2), c1 = (double)rot_row(m + 3, n0, n1, n2), c2 = (double)rot_row(m + 6, n0, n1, n2);
    const double Xd = (double)X, Yd = (double)Y, Zd = (double)Z;
    const double dot = -((c0 * Xd + c1 * Yd) + c2 * Zd);
    const double g = (c0 * c0 + c1 * c1) + c2 * c2;
    const double r = (Xd * Xd + Yd * Yd) + Zd * Zd;
    double cs = dot / sqrt(g * r);
    if (cam.two_sided) cs = fabs(cs);
    if (!(cs > 0.0 && cs >= cam.min_cos)) return VIEW_AVERTED;   // a NaN fails
    const unsigned f = (unsigned)floor(cs * 1024.0 + 0.5);       // cs <= 1 up to rounding, so the cast is in range
    w = f < 1u ? 1u : f;
  }
  taken(ViewSample{X, Y, Z, w, ax, ay, t00, t10, t01, t11});
  return VIEW_TAKEN;
}

// steps 5 and 6 for a TAKEN pair of view number `index`: the bilinear colour into the state a0 .. a3 -- MEAN S_0 S_1 S_2 W, BEST s_0 s_1
// s_2 key -- and the count of the views used
template <bool BEST>
__device__ __forceinline__ void view_accumulate(const unsigned char* __restrict__ col, const ViewSample& o, unsigned index, unsigned long long& a0,
                                                unsigned long long& a1, unsigned long long& a2, unsigned long long& a3, unsigned& used) {
  const unsigned ax = o.ax, ay = o.ay, w = o.w;
  const size_t t00 = o.t00, t10 = o.t10, t01 = o.t01, t11 = o.t11;
  const unsigned w00 = (256u - ax) * (256u - ay), w10 = ax * (256u - ay), w01 = (256u - ax) * ay, w11 = ax * ay;   // sum 65 536
  unsigned s[3];
  for (int k = 0; k < 3; ++k)
    s[k] = w00 * col[3 * t00 + k] + w10 * col[3 * t10 + k] + w01 * col[3 * t01 + k] + w11 * col[3 * t11 + k];    // <= 255 * 65 536
  ++used;
  if (BEST) {
    const unsigned long long key = ((unsigned long long)w << 32) | (unsigned long long)(0xFFFFFFFFu - index);
    if (key > a3) { a3 = key; a0 = s[0]; a1 = s[1]; a2 = s[2]; }
  } else {
    a0 += (unsigned long long)w * s[0]; a1 += (unsigned long long)w * s[1]; a2 += (unsigned long long)w * s[2];
    a3 += w;
  }
}

// The classes of a block's pairs with view v of the launch, counted by ballot and popcount per wave.  Every thread of the block is here; a
// thread without a pair has the class -1
__device__ __forceinline__ void view_tally(unsigned (*tally)[VIEWS_PER_CHUNK * VIEW_N_COUNTS], int v, int cls) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int k = 0; k < VIEW_N_COUNTS; ++k) {
    const unsigned n = (unsigned)__popcll(__ballot(cls == k));
    if (lane == 0) tally[wave][v * VIEW_N_COUNTS + k] = n;
  }
}
// behind the walk over the launch's nv views: the waves meet in LDS, one 64-bit atomic per view and non-zero class.  counts: the count
// lines of the launch's first view
__device__ __forceinline__ void view_tally_add(unsigned (*tally)[VIEWS_PER_CHUNK * VIEW_N_COUNTS], int nv, unsigned long long* __restrict__ counts) {
  __syncthreads();
  if ((int)threadIdx.x < nv * VIEW_N_COUNTS) {
    unsigned n = 0;
    for (int w = 0; w < VIEW_WAVES; ++w) n += tally[w][threadIdx.x];
    const unsigned v = threadIdx.x / VIEW_N_COUNTS, k = threadIdx.x - v * VIEW_N_COUNTS;
    if (n) atomicAdd(counts + (size_t)v * VIEW_COUNT_LINE + k, (unsigned long long)n);
  }
}

// step 7's byte of one channel a of a state with used >= 1, a3 its fourth plane
template <bool BEST>
__device__ __forceinline__ unsigned char view_state_byte(unsigned long long a, unsigned long long a3) {
  if (BEST) return (unsigned char)((a + 32768ull) >> 16);
  const unsigned long long D = 65536ull * a3;               // W >= 1 with used >= 1
  return (unsigned char)((2ull * a + D) / (2ull * D));
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// what every call checks about the camera and the thresholds it is given; neither pointer is null
bool view_camera_ok(const float K[4], int rows, int cols, const rgbid_recolour_params& p) {
  if (rows < 1 || cols < 1 || rows > RGBID_RASTER_MAX_DIM || cols > RGBID_RASTER_MAX_DIM) return false;
  if (!(std::isfinite(p.z_min) && std::isfinite(p.z_max) && p.z_min > 0.f && p.z_min <= p.z_max)) return false;
  if (!(std::isfinite(p.surface_tolerance) && p.surface_tolerance >= 0.f && std::isfinite(p.measured_tolerance) && p.measured_tolerance >= 0.f))
    return false;
  if (!(p.min_cos >= 0.f && p.min_cos <= 1.f) || (p.two_sided != 0 && p.two_sided != 1)) return false;
  for (int k = 0; k < 4; ++k) if (!std::isfinite(K[k])) return false;
  return K[0] != 0.f && K[1] != 0.f;
}

// a view: a colour plane, aligned depth planes, a finite pose whose twelve floats are finite too
bool view_ok(const rgbid_recolour_view& in) {
  if (!in.colour_dev || !aligned4(in.surface_dev) || !aligned4(in.measured_dev)) return false;
  if (!finite_all(in.pose.R, 9) || !finite_all(in.pose.t, 3)) return false;
  float cw[12];
  rgbid_render_pose_cw(&in.pose, cw);
  for (int k = 0; k < 12; ++k) if (!std::isfinite(cw[k])) return false;
  return true;
}

ViewCam view_cam(const float K[4], int rows, int cols, const rgbid_recolour_params& p) {
  ViewCam cam;
  cam.min_cos = (double)p.min_cos;
  cam.fx = K[0]; cam.fy = K[1]; cam.cx = K[2]; cam.cy = K[3]; cam.z_min = p.z_min; cam.z_max = p.z_max;
  cam.tol_surface = p.surface_tolerance; cam.tol_measured = p.measured_tolerance;
  cam.rows = rows; cam.cols = cols; cam.two_sided = p.two_sided;
  return cam;
}

// the first nv <= VIEWS_PER_CHUNK of `views` into the kernel argument, zeros behind them
void view_pack(const rgbid_recolour_view* views, int nv, ViewChunk& vw) {
  for (int v = 0; v < VIEWS_PER_CHUNK; ++v) {
    ViewEntry& o = vw.v[v];
    if (v < nv) {
      const rgbid_recolour_view& in = views[v];
      rgbid_render_pose_cw(&in.pose, o.m);
      o.colour = in.colour_dev; o.surface = in.surface_dev; o.measured = in.measured_dev;
    } else {
      for (int k = 0; k < 12; ++k) o.m[k] = 0.f;
      o.colour = nullptr; o.surface = nullptr; o.measured = nullptr;
    }
  }
}

// the six counts of V >= 1 views from their device lines -> out [V][6]; one host synchronisation
int view_counts_read(const rgbid_ctx* ctx, const unsigned long long* lines_dev, int V, unsigned long long* out) {
  (void)hipSetDevice(ctx->device);
  std::vector<unsigned long long> lines((size_t)V * VIEW_COUNT_LINE);
  RGBID_HIP(hipMemcpyAsync(lines.data(), lines_dev, sizeof(unsigned long long) * lines.size(), hipMemcpyDeviceToHost, ctx->stream));
  RGBID_HIP(hipStreamSynchronize(ctx->stream));
  for (int v = 0; v < V; ++v)
    for (int k = 0; k < VIEW_N_COUNTS; ++k) out[(size_t)v * VIEW_N_COUNTS + k] = lines[(size_t)v * VIEW_COUNT_LINE + k];
  return RGBID_OK;
}

}  // namespace
}  // namespace rgbid
