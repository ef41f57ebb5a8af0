// kernels_cloud.hip -- coloured point clouds of exported keyframes (include/rgbid_cloud.h; KeyframeManager::computeAlignedPointCloud,
// src/keyframe_manager.cpp:438-528).
//
// The reference walks a keyframe in raster order on one CPU thread and pushes every pixel whose 1/iD and normal x are not NaN.  Here one
// launch covers a batch of keyframes (any set of packed export blocks: engine lanes, ring slots), in two passes so that the output is in
// the reference's order and identical from run to run, without atomics:
//   plan  k_cloud_count       one valid-pixel count per tile (TILE contiguous pixels); reads only what the predicate needs (8 - 9 B/px)
//         k_cloud_scan_tiles  one workgroup per keyframe: exclusive scan of its tile counts -> tile offsets, keyframe total
//         k_cloud_scan_kfs    one workgroup: exclusive scan of the keyframe totals -> offsets[n + 1], copied to the host
//   emit  k_cloud_emit        recomputes the predicate, ranks the valid pixels of a tile in pixel order (3 ballots + mbcnt per wave, wave
//                             totals through LDS) and writes one 32-byte record per point as two 16-byte stores (20 B/px read)
// The counting and emitting kernels walk a flat (keyframe, tile) index, grid-strided with the grid capped at CLOUD_MAX_GRID blocks.
#include "../../include/rgbid_cloud.h"
#include "common.h"
#include "cloud_device.h"   // the predicate and the point, shared with kernels_segment.hip
#include "hip_host.h"
#include "wave_device.h"

#include <cstring>
#include <new>

using namespace rgbid;

static_assert(sizeof(rgbid_cloud_point) == 32, "rgbid_cloud_point is two 16-byte stores");
static_assert(sizeof(rgbid_cloud_src) == 104, "rgbid_cloud_src layout");

namespace {

constexpr int CT = 256;                  // threads per block
constexpr int PPT = 4;                   // contiguous pixels per thread
constexpr int TILE = CT * PPT;           // pixels per tile
constexpr int CLOUD_MAX_GRID = 2048;     // cdna_hip_programming guideline 11: 256 CUs x 8 blocks

struct CloudGeom {
  double kinv[9];
  int N, cols, tiles, n, mode;
};

// the 4 pixels p0 .. p0 + 3 of one thread, as far as they lie inside the keyframe
struct Px4 {
  float iD[4], n0[4], n1[4], n2[4];
  unsigned m[4], rgb[4];    // overlap mask byte, colour r | g << 8 | b << 16
};

// packed block: overlap mask u8[N] | colours u8[3N] | inverse depth f32[N] | normals f32[3N planar] (rgbid_engine.h)
__device__ __forceinline__ bool block_vec(const char* blk, int N) { return ((N & 15) == 0) && ((((uintptr_t)blk) & 15) == 0); }

// pixels of a thread that exist: 0 .. 4 (a partial last tile; the vector path never has one, TILE and N both being multiples of 16)
__device__ __forceinline__ int px_here(int p0, int N) { return min(max(N - p0, 0), PPT); }

template <bool FULL>
__device__ __forceinline__ void load_px(const char* blk, int N, int p0, bool vec, bool need_mask, Px4& q) {
  const int cnt = px_here(p0, N);
  const float* iD = reinterpret_cast<const float*>(blk + 4 * (size_t)N);
  const float* nr = reinterpret_cast<const float*>(blk + 8 * (size_t)N);
  if (vec && cnt == PPT) {
    const float4 a = *reinterpret_cast<const float4*>(iD + p0);
    const float4 b = *reinterpret_cast<const float4*>(nr + p0);
    q.iD[0] = a.x; q.iD[1] = a.y; q.iD[2] = a.z; q.iD[3] = a.w;
    q.n0[0] = b.x; q.n0[1] = b.y; q.n0[2] = b.z; q.n0[3] = b.w;
    if (need_mask) {
      const uint32_t mk = *reinterpret_cast<const uint32_t*>(blk + p0);
      for (int j = 0; j < PPT; ++j) q.m[j] = (mk >> (8 * j)) & 0xffu;
    }
    if (FULL) {
      const float4 c = *reinterpret_cast<const float4*>(nr + N + p0);
      const float4 d = *reinterpret_cast<const float4*>(nr + 2 * (size_t)N + p0);
      q.n1[0] = c.x; q.n1[1] = c.y; q.n1[2] = c.z; q.n1[3] = c.w;
      q.n2[0] = d.x; q.n2[1] = d.y; q.n2[2] = d.z; q.n2[3] = d.w;
      const uint32_t* cs = reinterpret_cast<const uint32_t*>(blk + N + 3 * (size_t)p0);   // 4-byte aligned: N and 3 p0 are multiples of 4
      const uint32_t c0 = cs[0], c1 = cs[1], c2 = cs[2];
      q.rgb[0] = c0 & 0xffffffu; q.rgb[1] = (c0 >> 24) | ((c1 & 0xffffu) << 8); q.rgb[2] = (c1 >> 16) | ((c2 & 0xffu) << 16); q.rgb[3] = c2 >> 8;
    }
  } else {
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      q.iD[j] = qnan(); q.n0[j] = qnan(); q.n1[j] = 0.f; q.n2[j] = 0.f; q.m[j] = 1; q.rgb[j] = 0;   // no pixel: invalid
      if (j < cnt) {
        const int p = p0 + j;
        q.iD[j] = iD[p]; q.n0[j] = nr[p];
        if (need_mask) q.m[j] = (unsigned)(uint8_t)blk[p];
        if (FULL) {
          q.n1[j] = nr[N + p]; q.n2[j] = nr[2 * (size_t)N + p];
          const uint8_t* cp = reinterpret_cast<const uint8_t*>(blk) + N + 3 * (size_t)p;
          q.rgb[j] = (unsigned)cp[0] | ((unsigned)cp[1] << 8) | ((unsigned)cp[2] << 16);
        }
      }
    }
  }
}

__device__ __forceinline__ unsigned valid_bits(const Px4& q, int mode) {
  unsigned v = 0;
  float d;
  for (int j = 0; j < PPT; ++j) v |= (cloud_valid(q.iD[j], q.n0[j], q.m[j], mode, d) ? 1u : 0u) << j;
  return v;
}

// count c (0 .. 4) of every lane of a wave as three ballots: the lane's exclusive prefix (mbcnt over the lower lanes) and the wave total
__device__ __forceinline__ void wave_prefix(unsigned c, unsigned& prefix, unsigned& total) {
  prefix = 0; total = 0;
  for (int b = 0; b < 3; ++b) {
    const unsigned long long m = __ballot((c >> b) & 1u);
    prefix += lane_prefix(m) << b;
    total += (unsigned)__popcll(m) << b;
  }
}

__global__ __launch_bounds__(CT) void k_cloud_count(const rgbid_cloud_src* __restrict__ src, CloudGeom g, unsigned* __restrict__ tile_counts) {
  __shared__ unsigned wsum[CT / 64];
  const int items = g.n * g.tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int k = w / g.tiles, t = w - k * g.tiles;
    const char* blk = static_cast<const char*>(src[k].block_dev);
    const int p0 = t * TILE + threadIdx.x * PPT;
    Px4 q;
    load_px<false>(blk, g.N, p0, block_vec(blk, g.N), g.mode != RGBID_CLOUD_ALL, q);
    const unsigned c = __popc(valid_bits(q, g.mode));
    unsigned pre, tot;
    wave_prefix(c, pre, tot);
    if (lane == 0) wsum[wave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[w] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
}

// one block per keyframe: tile counts -> exclusive tile offsets (in place), keyframe total
__global__ __launch_bounds__(CT) void k_cloud_scan_tiles(unsigned* __restrict__ tiles_io, unsigned* __restrict__ kf_total, int tiles) {
  __shared__ unsigned lds[CT / 64];
  unsigned* tc = tiles_io + (size_t)blockIdx.x * tiles;
  unsigned carry = 0;
  for (int base = 0; base < tiles; base += CT) {
    const int i = base + threadIdx.x;
    const unsigned v = i < tiles ? tc[i] : 0u;
    unsigned tot;
    const unsigned incl = block_scan_incl(v, lds, tot);
    if (i < tiles) tc[i] = carry + incl - v;
    carry += tot;
  }
  if (threadIdx.x == 0) kf_total[blockIdx.x] = carry;
}

// one block: keyframe totals -> offsets[n + 1] (64-bit: a batch may hold more than 2^32 points)
__global__ __launch_bounds__(CT) void k_cloud_scan_kfs(const unsigned* __restrict__ kf_total, unsigned long long* __restrict__ offsets, int n) {
  __shared__ unsigned long long lds[CT / 64];
  unsigned long long carry = 0;
  for (int base = 0; base < n; base += CT) {
    const int i = base + threadIdx.x;
    const unsigned long long v = i < n ? kf_total[i] : 0ull;
    unsigned long long tot;
    const unsigned long long incl = block_scan_incl(v, lds, tot);
    if (i < n) offsets[i] = carry + incl - v;
    carry += tot;
  }
  if (threadIdx.x == 0) offsets[n] = carry;
}

__global__ __launch_bounds__(CT) void k_cloud_emit(const rgbid_cloud_src* __restrict__ src, CloudGeom g, const unsigned* __restrict__ tile_off,
                                                   const unsigned long long* __restrict__ kf_off, uint4* __restrict__ out) {
  __shared__ unsigned wsum[CT / 64];
  const int items = g.n * g.tiles;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int w = blockIdx.x; w < items; w += gridDim.x) {
    const int k = w / g.tiles, t = w - k * g.tiles;
    const rgbid_cloud_src& s = src[k];
    const char* blk = static_cast<const char*>(s.block_dev);
    const int p0 = t * TILE + threadIdx.x * PPT;
    Px4 q;
    load_px<true>(blk, g.N, p0, block_vec(blk, g.N), true, q);
    const unsigned v = valid_bits(q, g.mode);
    unsigned pre, tot;
    wave_prefix(__popc(v), pre, tot);
    if (lane == 0) wsum[wave] = tot;
    __syncthreads();
    unsigned before = 0;
    for (int i = 0; i < wave; ++i) before += wsum[i];
    __syncthreads();
    unsigned long long idx = kf_off[k] + tile_off[w] + before + pre;
    const unsigned long long end = kf_off[k + 1];   // the plan's bound: blocks that changed after the plan cannot make the kernel write past it
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      if (!((v >> j) & 1u) || idx >= end) continue;
      const int p = p0 + j, y = p / g.cols, x = p - y * g.cols;
      float d, o[6];
      cloud_valid(q.iD[j], q.n0[j], q.m[j], g.mode, d);
      cloud_point(d, x, y, g.kinv, s.R, s.t, q.n0[j], q.n1[j], q.n2[j], o);
      const unsigned rgbf = q.rgb[j] | ((q.m[j] == 0 ? RGBID_CLOUD_NOVEL : 0u) << 24);
      out[2 * idx] = make_uint4(__float_as_uint(o[0]), __float_as_uint(o[1]), __float_as_uint(o[2]), __float_as_uint(o[3]));
      out[2 * idx + 1] = make_uint4(__float_as_uint(o[4]), __float_as_uint(o[5]), (unsigned)p, rgbf);
      ++idx;
    }
  }
}

}  // namespace

struct rgbid_cloud {
  rgbid_ctx* ctx = nullptr;
  int rows = 0, cols = 0, cap = 0, tiles = 0;
  rgbid_cloud_src* src_dev = nullptr;          // [cap] sources of the last plan
  rgbid_cloud_src* src_host = nullptr;         // pinned staging of the upload
  unsigned* tile_off = nullptr;                // [cap][tiles]: counts, then exclusive offsets inside the keyframe
  unsigned* kf_total = nullptr;                // [cap]
  unsigned long long* kf_off = nullptr;        // [cap + 1]
  unsigned long long* kf_off_host = nullptr;   // pinned
  CloudGeom geom = {};                         // of the last plan (geom.n = 0: none)
  unsigned long long total = 0;
  Buffers buf;
};

namespace {

// Eigen's compute_inverse<3x3> (Eigen/src/LU/InverseImpl.h) of K = [fx 0 cx; 0 fy cy; 0 0 1] in double: cofactors of column 0,
// det = their dot product with column 0 (in index order), invdet = 1 / det, Kinv(i, j) = cofactor(j, i) * invdet
void kinv_eigen(const float K[4], double Kinv[9]) {
  RGBID_FP_STRICT
  const double m[3][3] = {{(double)K[0], 0.0, (double)K[2]}, {0.0, (double)K[1], (double)K[3]}, {0.0, 0.0, 1.0}};
  auto cof = [&](int i, int j) {
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1];
  };
  const double det = (cof(0, 0) * m[0][0] + cof(1, 0) * m[1][0]) + cof(2, 0) * m[2][0];
  const double invdet = 1.0 / det;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Kinv[3 * i + j] = cof(j, i) * invdet;
}

int grid_of(int items) { return items < CLOUD_MAX_GRID ? items : CLOUD_MAX_GRID; }

}  // namespace

extern "C" {

int rgbid_cloud_kinv(const float K[4], double Kinv[9]) {
  if (!K || !Kinv) return RGBID_E_INVALID;
  kinv_eigen(K, Kinv);
  return RGBID_OK;
}

int rgbid_cloud_create(rgbid_cloud** out, rgbid_ctx* ctx, int rows, int cols, int max_keyframes) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || rows <= 0 || cols <= 0 || max_keyframes <= 0 || (long long)rows * cols > (1ll << 30)) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_cloud* c = new (std::nothrow) rgbid_cloud;
  if (!c) return RGBID_E_NOMEM;
  c->ctx = ctx; c->rows = rows; c->cols = cols; c->cap = max_keyframes;
  c->tiles = (rows * cols + TILE - 1) / TILE;
  const size_t cap = (size_t)max_keyframes;
  int r = c->buf.alloc(&c->src_dev, sizeof(rgbid_cloud_src) * cap);
  if (!r) r = c->buf.alloc_host(&c->src_host, sizeof(rgbid_cloud_src) * cap);
  if (!r) r = c->buf.alloc(&c->tile_off, sizeof(unsigned) * cap * c->tiles);
  if (!r) r = c->buf.alloc(&c->kf_total, sizeof(unsigned) * cap);
  if (!r) r = c->buf.alloc(&c->kf_off, sizeof(unsigned long long) * (cap + 1));
  if (!r) r = c->buf.alloc_host(&c->kf_off_host, sizeof(unsigned long long) * (cap + 1));
  if (r) { rgbid_cloud_destroy(c); return r; }
  *out = c;
  return RGBID_OK;
}

int rgbid_cloud_destroy(rgbid_cloud* c) { return destroy_handle(c); }   // an emit may still read the tables

int rgbid_cloud_plan(rgbid_cloud* c, int n, const rgbid_cloud_src* src, const float K[4], int mode, unsigned long long* offsets) {
  if (!c || n < 0 || n > c->cap || (n > 0 && !src) || !K || !offsets || (mode != RGBID_CLOUD_ALL && mode != RGBID_CLOUD_NOVEL_ONLY))
    return RGBID_E_INVALID;
  for (int i = 0; i < n; ++i) if (!src[i].block_dev) return RGBID_E_INVALID;
  (void)hipSetDevice(c->ctx->device);
  hipStream_t s = c->ctx->stream;
  c->geom.n = 0; c->total = 0;
  offsets[0] = 0;
  if (n == 0) return RGBID_OK;
  RGBID_HIP(hipStreamSynchronize(s));   // the previous plan's upload and emit have read the staging area and the tables
  CloudGeom g;
  kinv_eigen(K, g.kinv);
  g.N = c->rows * c->cols; g.cols = c->cols; g.tiles = c->tiles; g.n = n; g.mode = mode;
  memcpy(c->src_host, src, sizeof(rgbid_cloud_src) * n);
  RGBID_HIP(hipMemcpyAsync(c->src_dev, c->src_host, sizeof(rgbid_cloud_src) * n, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_cloud_count, dim3(grid_of(n * g.tiles)), dim3(CT), 0, s, c->src_dev, g, c->tile_off);
  hipLaunchKernelGGL(k_cloud_scan_tiles, dim3(n), dim3(CT), 0, s, c->tile_off, c->kf_total, g.tiles);
  hipLaunchKernelGGL(k_cloud_scan_kfs, dim3(1), dim3(CT), 0, s, c->kf_total, c->kf_off, n);
  RGBID_HIP(hipGetLastError());
  RGBID_HIP(hipMemcpyAsync(c->kf_off_host, c->kf_off, sizeof(unsigned long long) * (n + 1), hipMemcpyDeviceToHost, s));
  RGBID_HIP(hipStreamSynchronize(s));
  memcpy(offsets, c->kf_off_host, sizeof(unsigned long long) * (n + 1));
  c->geom = g;
  c->total = offsets[n];
  return RGBID_OK;
}

int rgbid_cloud_emit(rgbid_cloud* c, rgbid_cloud_point* out_dev, unsigned long long capacity) {
  if (!c) return RGBID_E_INVALID;
  if (c->geom.n == 0 || c->total == 0) return RGBID_OK;
  if (!out_dev || capacity < c->total || (((uintptr_t)out_dev) & 15)) return RGBID_E_INVALID;
  (void)hipSetDevice(c->ctx->device);
  hipLaunchKernelGGL(k_cloud_emit, dim3(grid_of(c->geom.n * c->geom.tiles)), dim3(CT), 0, c->ctx->stream, c->src_dev, c->geom, c->tile_off, c->kf_off,
                     reinterpret_cast<uint4*>(out_dev));
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

}  // extern "C"
