// kernels_render.hip -- the map seen from camera poses (include/rgbid_render.h).
//
// The judge is tests/render_mirror.py; the device output is byte-identical to it.
//   k_render_clear    the key buffer [V][rows][cols] of uint64 is set to all ones, 16 bytes per store
//   k_render_splat    one thread per record; up to RGBID_RENDER_VIEW_CHUNK views per launch in an inner loop, their twelve floats each in the
//                     kernel arguments; camera point, gates, projection in float32; key = bits of Z << 32 | index goes to the (2 s + 1)^2
//                     pixels with a 64-bit atomic minimum on global memory
//   k_render_resolve  one thread per pixel and view: key -> the winner's record -> the requested planes
// No float atomic exists: the minimum of integer keys is the same whatever the order of threads, waves, launches or records.
//
// Exact arithmetic: every function that forms a float32 product followed by a sum opens with RGBID_FP_STRICT (common.h: clang's fp contract
// pragma, off for the compound statement), so the compiler forms no FMA from them whatever flags the file is built with; the division is
// hipcc's default correctly rounded one.  The host part (rgbid_render_pose_cw, in double) does the same.
#include "../../include/rgbid_render.h"
#include "common.h"
#include "hip_host.h"
#include "view_device.h"    // rot_row

#include <cmath>
#include <new>

using namespace rgbid;

static_assert(sizeof(rgbid_cloud_point) == 32, "rgbid_cloud_point is two 16-byte loads");

namespace {

constexpr int RT = 256;                                     // threads per block: four waves
constexpr unsigned long long EMPTY_KEY = ~0ull;
constexpr unsigned long long MAX_PIXEL_VIEWS = 1ull << 38;   // 2 TiB of keys: keeps every grid below 2^31 blocks

struct RenderViews {                                        // kernel argument: 16 x 12 floats = 768 bytes
  float m[RGBID_RENDER_VIEW_CHUNK][12];                     // r00 r01 r02 r10 r11 r12 r20 r21 r22 tx ty tz
};

struct RenderCam {
  float fx, fy, cx, cy, z_min, z_max;
  float lo, hi_u, hi_v;                                     // -s, cols - 1 + s, rows - 1 + s: exact in float32 (RGBID_RENDER_MAX_DIM)
  int rows, cols, s, nv;                                    // nv: views of this launch
};

__global__ __launch_bounds__(RT) void k_render_clear(uint4* __restrict__ keys, size_t n16) {
  const size_t i = (size_t)blockIdx.x * RT + threadIdx.x;
  if (i < n16) keys[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
}

// Only x, y, z decide here and they lie in the record's first 16 bytes; the second half of the record is the resolve's business.  The lines
// fetched are the same either way: 32 bytes per record.
// COUNT: the statistics of rgbid_render_stats (visible pairs, attempted pixel writes, atomics), a variant of its own so that the
// plain kernel carries none of it.
template <bool COUNT>
__global__ __launch_bounds__(RT) void k_render_splat(const float4* __restrict__ in, unsigned n, RenderViews vw, RenderCam cam,
                                                     unsigned long long* __restrict__ keys, unsigned long long* __restrict__ stats) {
  RGBID_FP_STRICT
  const unsigned i = blockIdx.x * RT + threadIdx.x;
  if (i >= n) return;
  const float4 a = in[2 * (size_t)i];
  if (!(__builtin_isfinite(a.x) && __builtin_isfinite(a.y) && __builtin_isfinite(a.z))) return;
  const size_t npix = (size_t)cam.rows * (size_t)cam.cols;
  unsigned c_pairs = 0, c_writes = 0, c_atomics = 0;
  for (int v = 0; v < cam.nv; ++v) {
    const float* m = vw.m[v];                               // wave-uniform: scalar registers
    const float Z = rot_row(m + 6, a.x, a.y, a.z) + m[11];
    if (!(Z >= cam.z_min && Z <= cam.z_max)) continue;      // NaN fails; z_max is finite, so infinity does too
    const float X = rot_row(m, a.x, a.y, a.z) + m[9];
    const float Y = rot_row(m + 3, a.x, a.y, a.z) + m[10];
    const float pu = floorf((cam.fx * (X / Z) + cam.cx) + 0.5f);
    const float pv = floorf((cam.fy * (Y / Z) + cam.cy) + 0.5f);
    if (!(pu >= cam.lo && pu <= cam.hi_u && pv >= cam.lo && pv <= cam.hi_v)) continue;   // in float: nothing out of range reaches the cast
    const int iu = (int)pu, iv = (int)pv;
    const int x0 = max(iu - cam.s, 0), x1 = min(iu + cam.s, cam.cols - 1);
    const int y0 = max(iv - cam.s, 0), y1 = min(iv + cam.s, cam.rows - 1);
    const unsigned long long key = ((unsigned long long)__float_as_uint(Z) << 32) | i;   // Z > 0: its bits order like its value
    unsigned long long* view = keys + (size_t)v * npix;
    if (COUNT) ++c_pairs;
    for (int y = y0; y <= y1; ++y) {
      unsigned long long* row = view + (size_t)y * (size_t)cam.cols;
      for (int x = x0; x <= x1; ++x) {
        if (COUNT) ++c_writes;
        // A plain load first: when the pixel already holds a key that is not larger, this one cannot win and the atomic is skipped.  The
        // load may be stale (another thread lowers the key meanwhile, or this CU's L1 holds an older line); a key only ever decreases, so a
        // stale value is never smaller than the current one: it can cost an atomic that changes nothing, never a result.  On a dense cloud
        // most records lie behind the front surface and leave here, instead of serialising on the pixel's atomic.
        if (row[x] <= key) continue;
        if (COUNT) ++c_atomics;
        (void)__hip_atomic_fetch_min(row + x, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
  if (COUNT) {
    if (c_pairs) atomicAdd(stats + 0, (unsigned long long)c_pairs);
    if (c_writes) atomicAdd(stats + 1, (unsigned long long)c_writes);
    if (c_atomics) atomicAdd(stats + 2, (unsigned long long)c_atomics);
  }
}

__device__ __forceinline__ float one_nan(float f) { return f != f ? __uint_as_float(RGBID_RENDER_NAN_BITS) : f; }

// view = blockIdx.y of this launch; `base` = the launch's first view times rows * cols, in pixels
__global__ __launch_bounds__(RT) void k_render_resolve(const unsigned long long* __restrict__ keys, const uint4* __restrict__ in, RenderViews vw,
                                                       size_t npix, size_t base, unsigned* __restrict__ index, float* __restrict__ depth,
                                                       unsigned char* __restrict__ colour, float* __restrict__ normal) {
  RGBID_FP_STRICT
  const size_t pix = (size_t)blockIdx.x * RT + threadIdx.x;
  if (pix >= npix) return;
  const int v = blockIdx.y;
  const size_t at = base + (size_t)v * npix + pix;          // pixel of the whole batch
  const unsigned long long key = keys[at];
  unsigned idx = RGBID_RENDER_EMPTY, rgb = 0;
  float Z = __uint_as_float(RGBID_RENDER_NAN_BITS), nx = Z, ny = Z, nz = Z;
  if (key != EMPTY_KEY) {
    idx = (unsigned)key;
    Z = __uint_as_float((unsigned)(key >> 32));
    if (colour || normal) {
      const uint4 a = in[2 * (size_t)idx], b = in[2 * (size_t)idx + 1];   // x y z nx | ny nz pixel rgb+flags
      rgb = b.w;
      const float* m = vw.m[v];
      const float px = __uint_as_float(a.w), py = __uint_as_float(b.x), pz = __uint_as_float(b.y);
      nx = one_nan(rot_row(m, px, py, pz));
      ny = one_nan(rot_row(m + 3, px, py, pz));
      nz = one_nan(rot_row(m + 6, px, py, pz));
    }
  }
  if (index) index[at] = idx;
  if (depth) depth[at] = Z;
  if (colour) {
    unsigned char* c = colour + 3 * at;
    c[0] = (unsigned char)rgb; c[1] = (unsigned char)(rgb >> 8); c[2] = (unsigned char)(rgb >> 16);
  }
  if (normal) {
    float* p = normal + 3 * (at - pix) + pix;               // [view][3][rows][cols]
    p[0] = nx; p[npix] = ny; p[2 * npix] = nz;
  }
}

}  // namespace

struct rgbid_render {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap_points = 0, cap_pix = 0;
  unsigned long long* keys = nullptr;          // [cap_pix rounded up to even]
  unsigned long long* stats_dev = nullptr;     // [3]
  unsigned long long* stats_host = nullptr;    // pinned
  bool count = false, counted = false, timed = false;
  Buffers buf;
  StageTimer<4> timer;                          // clear [0, 1], splat [1, 2], resolve [2, 3]
  void mark(int i) { timer.mark(i, ctx->stream); }
};

extern "C" {

int rgbid_render_create(rgbid_render** out, rgbid_ctx* ctx, unsigned long long max_points, unsigned long long max_pixels_times_views) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_points == 0 || max_points > RGBID_RENDER_MAX_POINTS) return RGBID_E_INVALID;
  if (max_pixels_times_views == 0 || max_pixels_times_views > MAX_PIXEL_VIEWS) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_render* r = new (std::nothrow) rgbid_render;
  if (!r) return RGBID_E_NOMEM;
  r->ctx = ctx;
  r->cap_points = max_points;
  r->cap_pix = max_pixels_times_views;
  int e = r->buf.alloc(&r->keys, sizeof(unsigned long long) * (size_t)((max_pixels_times_views + 1) & ~1ull));   // whole 16-byte stores
  if (!e) e = r->buf.alloc(&r->stats_dev, 3 * sizeof(unsigned long long));
  if (!e) e = r->buf.alloc_host(&r->stats_host, 3 * sizeof(unsigned long long));
  if (e) { rgbid_render_destroy(r); return e; }
  *out = r;
  return RGBID_OK;
}

int rgbid_render_destroy(rgbid_render* r) { return destroy_handle(r); }   // a resolve may still read the keys

int rgbid_render_pose_cw(const rgbid_render_pose* pose, float cw[12]) {
  RGBID_FP_STRICT
  if (!pose || !cw) return RGBID_E_INVALID;
  const double* R = pose->R;
  const double* t = pose->t;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) cw[3 * i + j] = (float)R[3 * j + i];
    const double d = (R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2];
    cw[9 + i] = (float)-d;
  }
  return RGBID_OK;
}

int rgbid_render_views(rgbid_render* r, const rgbid_cloud_point* in_dev, unsigned long long n, int V, const rgbid_render_pose* poses,
                       const float K[4], int rows, int cols, int s, float z_min, float z_max, uint32_t* index_dev, float* depth_dev,
                       uint8_t* colour_dev, float* normal_dev) {
  if (!r || !poses || !K || V < 1) return RGBID_E_INVALID;
  if (rows < 1 || cols < 1 || rows > RGBID_RENDER_MAX_DIM || cols > RGBID_RENDER_MAX_DIM) return RGBID_E_INVALID;
  const unsigned long long npix = (unsigned long long)rows * (unsigned long long)cols;
  if (npix > r->cap_pix || (unsigned long long)V > r->cap_pix / npix) return RGBID_E_INVALID;
  if (s < 0 || s > RGBID_RENDER_MAX_SPLAT) return RGBID_E_INVALID;
  if (!(std::isfinite(z_min) && std::isfinite(z_max) && z_min > 0.f && z_min <= z_max)) return RGBID_E_INVALID;
  for (int k = 0; k < 4; ++k) if (!std::isfinite(K[k])) return RGBID_E_INVALID;
  if (K[0] == 0.f || K[1] == 0.f) return RGBID_E_INVALID;
  if (n > r->cap_points || (n > 0 && (!in_dev || (((uintptr_t)in_dev) & 15)))) return RGBID_E_INVALID;
  if ((((uintptr_t)index_dev) | ((uintptr_t)depth_dev) | ((uintptr_t)normal_dev)) & 3) return RGBID_E_INVALID;
  for (int v = 0; v < V; ++v) {
    if (!finite_all(poses[v].R, 9) || !finite_all(poses[v].t, 3)) return RGBID_E_INVALID;
    float cw[12];
    rgbid_render_pose_cw(&poses[v], cw);
    for (int k = 0; k < 12; ++k) if (!std::isfinite(cw[k])) return RGBID_E_INVALID;
  }
  (void)hipSetDevice(r->ctx->device);
  hipStream_t st = r->ctx->stream;
  r->timed = false; r->counted = false;
  const size_t total = (size_t)npix * (size_t)V;
  const size_t n16 = (total + 1) / 2;
  r->mark(0);
  hipLaunchKernelGGL(k_render_clear, dim3((unsigned)((n16 + RT - 1) / RT)), dim3(RT), 0, st, reinterpret_cast<uint4*>(r->keys), n16);
  if (r->count) RGBID_HIP(hipMemsetAsync(r->stats_dev, 0, 3 * sizeof(unsigned long long), st));
  r->mark(1);
  RenderCam cam;
  cam.fx = K[0]; cam.fy = K[1]; cam.cx = K[2]; cam.cy = K[3]; cam.z_min = z_min; cam.z_max = z_max;
  cam.lo = (float)-s; cam.hi_u = (float)(cols - 1 + s); cam.hi_v = (float)(rows - 1 + s);
  cam.rows = rows; cam.cols = cols; cam.s = s;
  RenderViews vw;
  auto chunk = [&](int v0) {
    const int nv = V - v0 < RGBID_RENDER_VIEW_CHUNK ? V - v0 : RGBID_RENDER_VIEW_CHUNK;
    for (int v = 0; v < RGBID_RENDER_VIEW_CHUNK; ++v) {
      if (v < nv) rgbid_render_pose_cw(&poses[v0 + v], vw.m[v]);
      else for (int k = 0; k < 12; ++k) vw.m[v][k] = 0.f;
    }
    return nv;
  };
  if (n > 0) {
    const unsigned nu = (unsigned)n;
    const float4* in = reinterpret_cast<const float4*>(in_dev);
    for (int v0 = 0; v0 < V; v0 += RGBID_RENDER_VIEW_CHUNK) {
      cam.nv = chunk(v0);
      unsigned long long* keys = r->keys + (size_t)v0 * (size_t)npix;
      if (r->count) hipLaunchKernelGGL(k_render_splat<true>, dim3((nu + RT - 1) / RT), dim3(RT), 0, st, in, nu, vw, cam, keys, r->stats_dev);
      else hipLaunchKernelGGL(k_render_splat<false>, dim3((nu + RT - 1) / RT), dim3(RT), 0, st, in, nu, vw, cam, keys, r->stats_dev);
    }
  }
  r->mark(2);
  if (index_dev || depth_dev || colour_dev || normal_dev) {
    for (int v0 = 0; v0 < V; v0 += RGBID_RENDER_VIEW_CHUNK) {
      const int nv = chunk(v0);
      hipLaunchKernelGGL(k_render_resolve, dim3((unsigned)((npix + RT - 1) / RT), (unsigned)nv), dim3(RT), 0, st, r->keys,
                         reinterpret_cast<const uint4*>(in_dev), vw, (size_t)npix, (size_t)v0 * (size_t)npix, index_dev, depth_dev, colour_dev,
                         normal_dev);
    }
  }
  r->mark(3);
  RGBID_HIP(hipGetLastError());
  r->timed = r->timer.on;
  r->counted = r->count;
  return RGBID_OK;
}

int rgbid_render_timing(rgbid_render* r, int enable, float ms[3]) {
  if (!r) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  if (ms) {
    for (int k = 0; k < 3; ++k) {
      ms[k] = 0.f;
      if (r->timed) RGBID_HIP(r->timer.elapsed(k, k + 1, &ms[k]));
    }
  }
  return r->timer.enable(enable != 0);
}

int rgbid_render_stats(rgbid_render* r, int enable, unsigned long long stats[3]) {
  if (!r) return RGBID_E_INVALID;
  (void)hipSetDevice(r->ctx->device);
  if (stats) {
    stats[0] = stats[1] = stats[2] = 0;
    if (r->counted) {
      RGBID_HIP(hipMemcpyAsync(r->stats_host, r->stats_dev, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, r->ctx->stream));
      RGBID_HIP(hipStreamSynchronize(r->ctx->stream));
      for (int k = 0; k < 3; ++k) stats[k] = r->stats_host[k];
    }
  }
  r->count = enable != 0;
  return RGBID_OK;
}

}  // extern "C"
