// kernels_voxel.hip -- voxel-grid filter over keyframe point clouds (include/rgbid_voxel.h; pcl::VoxelGrid::applyFilter as the reference's
// savePointCloudInFile runs it, tools/RGBID_SLAMapp.cpp:341-354).
//
// PCL sorts (cell key, point index) pairs with std::sort and averages each run of equal keys.  Here the same steps run on the device,
// with a STABLE sort so that every voxel sums its members in ascending input order, and without atomics on any float:
//   plan  k_vox_box / k_vox_box_final   per-axis min / max and the count of the finite points (exact in any order), copied to the host
//         (host)                        the grid in float32 as PCL forms it, the key width B = bitlen(largest key + 1)
//         k_vox_keys                    one (key, index) pair per record; non-finite records get the sentinel (largest key + 1)
//         LSD radix sort, 8 bits/pass   k_vox_hist (digit counts per tile) -> k_vox_scan_digits (one workgroup per digit: tile offsets)
//                                       -> k_vox_scatter (ranks a tile's keys with 8 ballots + mbcnt per wave: stable)
//         runs                          k_vox_flag_count / k_vox_scan1 / k_vox_flag_write: heads key[i] != key[i - 1] -> run starts;
//                                       the same three over the runs keep those of >= min_points members
//   emit  k_vox_emit                    one thread per voxel: gathers its members through the sorted indices, sums in order, 2 x 16 B stores
// Keys are 32-bit when the largest key + 1 < 2^32 (a 1 cm room map), 64-bit otherwise.
#include "../../include/rgbid_voxel.h"
#include "common.h"
#include "hip_host.h"
#include "voxel_device.h"   // box, grid, keys, radix sort, flag compaction

#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

using namespace rgbid;

static_assert(sizeof(rgbid_voxel_point) == 32, "rgbid_voxel_point is two 16-byte stores");
static_assert(offsetof(rgbid_voxel_point, count) == offsetof(rgbid_cloud_point, pixel), "count sits where the cloud record holds its pixel");

namespace {

// ---- emit -----------------------------------------------------------------------------------------------------------------------
struct VoxSum {
  double x = 0, y = 0, z = 0, nx = 0, ny = 0, nz = 0;
  unsigned long long r = 0, g = 0, b = 0;
  unsigned flags = 0;
  bool normal = false;
};

// one member, in order; the pragma keeps every add a separate rounding (no v_fma_f64 from the sums)
__device__ __forceinline__ void vox_add(VoxSum& s, const uint4& p, const uint4& q) {
  RGBID_FP_STRICT
  s.x += (double)__uint_as_float(p.x); s.y += (double)__uint_as_float(p.y); s.z += (double)__uint_as_float(p.z);
  const float n0 = __uint_as_float(p.w), n1 = __uint_as_float(q.x), n2 = __uint_as_float(q.y);
  if (finite3(n0, n1, n2)) { s.nx += (double)n0; s.ny += (double)n1; s.nz += (double)n2; s.normal = true; }
  s.r += q.w & 0xffu; s.g += (q.w >> 8) & 0xffu; s.b += (q.w >> 16) & 0xffu;
  s.flags |= (q.w >> 24) & RGBID_CLOUD_NOVEL;
}

__global__ __launch_bounds__(VT) void k_vox_emit(const uint4* __restrict__ in, const unsigned* __restrict__ sidx, const unsigned* __restrict__ vbeg,
                                                 const unsigned* __restrict__ vend, unsigned nvox, uint4* __restrict__ out) {
  RGBID_FP_STRICT
  const unsigned v = blockIdx.x * VT + threadIdx.x;
  if (v >= nvox) return;
  const unsigned b = vbeg[v], e = vend[v];
  VoxSum s;
  unsigned m = b;
  for (; m + 4 <= e; m += 4) {                 // the gathers of 4 members are issued before their adds
    unsigned id[4];
    uint4 p[4], q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) id[u] = sidx[m + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) { p[u] = in[2 * (size_t)id[u]]; q[u] = in[2 * (size_t)id[u] + 1]; }
#pragma unroll
    for (int u = 0; u < 4; ++u) vox_add(s, p[u], q[u]);
  }
  for (; m < e; ++m) {
    const unsigned id = sidx[m];
    vox_add(s, in[2 * (size_t)id], in[2 * (size_t)id + 1]);
  }
  const unsigned cnt = e - b;
  const double dc = (double)cnt;
  const float x = (float)(s.x / dc), y = (float)(s.y / dc), z = (float)(s.z / dc);
  float n0 = qnan(), n1 = qnan(), n2 = qnan();
  if (s.normal) {
    const double q = (s.nx * s.nx + s.ny * s.ny) + s.nz * s.nz;
    if (q != 0.0) {
      const double l = sqrt(q);
      n0 = (float)(s.nx / l); n1 = (float)(s.ny / l); n2 = (float)(s.nz / l);
    }
  }
  const unsigned rgbf = (unsigned)(s.r / cnt) | ((unsigned)(s.g / cnt) << 8) | ((unsigned)(s.b / cnt) << 16) | (s.flags << 24);
  out[2 * (size_t)v] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), __float_as_uint(n0));
  out[2 * (size_t)v + 1] = make_uint4(__float_as_uint(n1), __float_as_uint(n2), cnt, rgbf);
}

}  // namespace

struct rgbid_voxel {
  rgbid_ctx* ctx = nullptr;
  unsigned long long cap = 0;
  unsigned sort_tiles = 0, run_tiles = 0;      // at capacity
  unsigned long long* keys[2] = {nullptr, nullptr};   // [cap] 8 B each (32-bit keys use the first half); the free one holds vbeg | vend after the sort
  unsigned* idx[2] = {nullptr, nullptr};       // [cap + 1]; the free one holds the run starts after the sort
  unsigned* hist = nullptr;                    // [RADIX][sort_tiles]
  unsigned* dtotal = nullptr;                  // [RADIX]
  float* box_part = nullptr;                   // [VOX_MAX_GRID][6]
  unsigned* box_cnt = nullptr;                 // [VOX_MAX_GRID]
  unsigned* bc = nullptr;                      // [run_tiles]
  unsigned* slots = nullptr;                   // [SLOTS] box, finite count, runs, voxels
  unsigned* slots_host = nullptr;              // pinned
  // the last plan (voxels == 0: nothing to emit)
  const rgbid_cloud_point* in = nullptr;
  const unsigned* sidx = nullptr;
  const unsigned* vbeg = nullptr;
  const unsigned* vend = nullptr;
  unsigned long long voxels = 0;
  // stage timing (rgbid_voxel_timing): box [0, 1], keys [2, 3], sort [3, 4], runs [4, 5], emit [6, 7]
  bool plan_timed = false, emit_timed = false;
  Buffers buf;
  StageTimer<8> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

template <typename K>
int sort_and_runs(rgbid_voxel* v, const float4* in, unsigned n, unsigned finite, const VoxGrid& g, unsigned min_points) {
  hipStream_t s = v->ctx->stream;
  K* keys[2] = {reinterpret_cast<K*>(v->keys[0]), reinterpret_cast<K*>(v->keys[1])};
  v->mark(2);
  hipLaunchKernelGGL(k_vox_keys<K>, dim3(grid_of((n + VT - 1) / VT)), dim3(VT), 0, s, in, n, g, keys[0], v->idx[0]);
  v->mark(3);
  const int p = radix_sort_pairs<K>(s, keys, v->idx, n, bitlen(g.sentinel), v->hist, v->dtotal);
  v->mark(4);
  // the sorted pairs are in buffer p; the other buffers are free: run starts in idx[p ^ 1], voxel bounds in keys[p ^ 1]
  unsigned* starts = v->idx[p ^ 1];
  unsigned* vbeg = reinterpret_cast<unsigned*>(v->keys[p ^ 1]);
  unsigned* vend = vbeg + v->cap;
  const unsigned rtiles = (finite + RUN_TILE - 1) / RUN_TILE;
  const HeadSrc<K> hs{keys[p], finite, starts};
  hipLaunchKernelGGL(k_vox_flag_count<HeadSrc<K>>, dim3(rtiles), dim3(VT), 0, s, hs, v->bc);
  hipLaunchKernelGGL(k_vox_scan1, dim3(1), dim3(VT), 0, s, v->bc, rtiles, v->slots, (int)SLOT_RUNS, starts, finite);
  hipLaunchKernelGGL(k_vox_flag_write<HeadSrc<K>>, dim3(rtiles), dim3(VT), 0, s, hs, v->bc);
  if (min_points > 1) {
    const KeepSrc ks{starts, v->slots + SLOT_RUNS, min_points, vbeg, vend};
    hipLaunchKernelGGL(k_vox_flag_count<KeepSrc>, dim3(rtiles), dim3(VT), 0, s, ks, v->bc);
    hipLaunchKernelGGL(k_vox_scan1, dim3(1), dim3(VT), 0, s, v->bc, rtiles, v->slots, (int)SLOT_VOXELS, (unsigned*)nullptr, 0u);
    hipLaunchKernelGGL(k_vox_flag_write<KeepSrc>, dim3(rtiles), dim3(VT), 0, s, ks, v->bc);
    v->vbeg = vbeg; v->vend = vend;
  } else {
    v->vbeg = starts; v->vend = starts + 1;     // every run has >= 1 member
  }
  v->mark(5);
  v->sidx = v->idx[p];
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

}  // namespace

extern "C" {

int rgbid_voxel_create(rgbid_voxel** out, rgbid_ctx* ctx, unsigned long long max_points) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || max_points == 0 || max_points > RGBID_VOXEL_MAX_POINTS) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_voxel* v = new (std::nothrow) rgbid_voxel;
  if (!v) return RGBID_E_NOMEM;
  v->ctx = ctx; v->cap = max_points;
  v->sort_tiles = (unsigned)((max_points + SORT_TILE - 1) / SORT_TILE);
  v->run_tiles = (unsigned)((max_points + RUN_TILE - 1) / RUN_TILE);
  const size_t cap = (size_t)max_points;
  int r = RGBID_OK;
  for (int i = 0; i < 2 && !r; ++i) r = v->buf.alloc(&v->keys[i], sizeof(unsigned long long) * cap);
  for (int i = 0; i < 2 && !r; ++i) r = v->buf.alloc(&v->idx[i], sizeof(unsigned) * (cap + 1));
  if (!r) r = v->buf.alloc(&v->hist, sizeof(unsigned) * RADIX * (size_t)v->sort_tiles);
  if (!r) r = v->buf.alloc(&v->dtotal, sizeof(unsigned) * RADIX);
  if (!r) r = v->buf.alloc(&v->box_part, sizeof(float) * 6 * VOX_MAX_GRID);
  if (!r) r = v->buf.alloc(&v->box_cnt, sizeof(unsigned) * VOX_MAX_GRID);
  if (!r) r = v->buf.alloc(&v->bc, sizeof(unsigned) * v->run_tiles);
  if (!r) r = v->buf.alloc(&v->slots, sizeof(unsigned) * SLOTS);
  if (!r) r = v->buf.alloc_host(&v->slots_host, sizeof(unsigned) * SLOTS);
  if (r) { rgbid_voxel_destroy(v); return r; }
  *out = v;
  return RGBID_OK;
}

int rgbid_voxel_destroy(rgbid_voxel* v) {
  if (!v) return RGBID_OK;
  (void)hipSetDevice(v->ctx->device);
  if (v->ctx->stream) (void)hipStreamSynchronize(v->ctx->stream);   // an emit may still read the tables
  delete v;   // its Buffers free the tables, its StageTimer the events
  return RGBID_OK;
}

int rgbid_voxel_plan(rgbid_voxel* v, const rgbid_cloud_point* in_dev, unsigned long long n, const float leaf[3],
                     unsigned min_points, long long grid[6], unsigned long long stats[3], unsigned long long* voxels) {
  if (!v || !leaf || !voxels || n > v->cap || (n > 0 && !in_dev) || (((uintptr_t)in_dev) & 15)) return RGBID_E_INVALID;
  for (int a = 0; a < 3; ++a) if (!(std::isfinite(leaf[a]) && leaf[a] > 0.f)) return RGBID_E_INVALID;
  v->voxels = 0; v->in = nullptr;
  *voxels = 0;
  if (grid) for (int i = 0; i < 6; ++i) grid[i] = 0;
  if (stats) stats[0] = stats[1] = stats[2] = 0;
  if (n == 0) return RGBID_OK;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  RGBID_HIP(hipStreamSynchronize(s));   // the previous emit has read the tables
  const float4* in = reinterpret_cast<const float4*>(in_dev);
  const unsigned nu = (unsigned)n;
  const unsigned nb = grid_of((n + VT - 1) / VT);
  v->plan_timed = false; v->emit_timed = false;
  v->mark(0);
  hipLaunchKernelGGL(k_vox_box, dim3(nb), dim3(VT), 0, s, in, nu, v->box_part, v->box_cnt);
  hipLaunchKernelGGL(k_vox_box_final, dim3(1), dim3(64), 0, s, v->box_part, v->box_cnt, (int)nb, v->slots);
  v->mark(1);
  RGBID_HIP(hipGetLastError());
  RGBID_HIP(hipMemcpyAsync(v->slots_host, v->slots, sizeof(unsigned) * SLOTS, hipMemcpyDeviceToHost, s));
  RGBID_HIP(hipStreamSynchronize(s));
  const unsigned finite = v->slots_host[SLOT_FINITE];
  if (stats) stats[0] = finite;
  if (finite == 0) return RGBID_OK;
  float lo[3], hi[3];
  memcpy(lo, v->slots_host + SLOT_BOX, sizeof lo);
  memcpy(hi, v->slots_host + SLOT_BOX + 3, sizeof hi);
  VoxGrid g;
  long long gr[6];
  const int r = form_grid(lo, hi, leaf, g, gr);
  if (r) return r;
  if (grid) memcpy(grid, gr, sizeof gr);
  const int e = g.sentinel < (1ull << 32) ? sort_and_runs<unsigned>(v, in, nu, finite, g, min_points)
                                          : sort_and_runs<unsigned long long>(v, in, nu, finite, g, min_points);
  if (e) return e;
  RGBID_HIP(hipMemcpyAsync(v->slots_host, v->slots, sizeof(unsigned) * SLOTS, hipMemcpyDeviceToHost, s));
  RGBID_HIP(hipStreamSynchronize(s));
  const unsigned runs = v->slots_host[SLOT_RUNS];
  const unsigned vox = min_points > 1 ? v->slots_host[SLOT_VOXELS] : runs;
  if (stats) { stats[1] = runs; stats[2] = vox; }
  *voxels = vox;
  v->voxels = vox;
  v->in = in_dev;
  v->plan_timed = v->timer.on;
  return RGBID_OK;
}

int rgbid_voxel_emit(rgbid_voxel* v, rgbid_voxel_point* out_dev, unsigned long long capacity) {
  if (!v) return RGBID_E_INVALID;
  if (v->voxels == 0) return RGBID_OK;
  if (!out_dev || capacity < v->voxels || (((uintptr_t)out_dev) & 15)) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  const unsigned nv = (unsigned)v->voxels;
  v->mark(6);
  hipLaunchKernelGGL(k_vox_emit, dim3((nv + VT - 1) / VT), dim3(VT), 0, v->ctx->stream, reinterpret_cast<const uint4*>(v->in), v->sidx, v->vbeg,
                     v->vend, nv, reinterpret_cast<uint4*>(out_dev));
  v->mark(7);
  RGBID_HIP(hipGetLastError());
  v->emit_timed = v->timer.on;
  return RGBID_OK;
}

int rgbid_voxel_timing(rgbid_voxel* v, int enable, float ms[5]) {
  if (!v) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  if (ms) {
    static const int pair[5][2] = {{0, 1}, {2, 3}, {3, 4}, {4, 5}, {6, 7}};
    for (int k = 0; k < 5; ++k) {
      ms[k] = 0.f;
      if ((k < 4 && v->plan_timed) || (k == 4 && v->emit_timed)) RGBID_HIP(v->timer.elapsed(pair[k][0], pair[k][1], &ms[k]));
    }
  }
  return v->timer.enable(enable != 0);
}

}  // extern "C"
