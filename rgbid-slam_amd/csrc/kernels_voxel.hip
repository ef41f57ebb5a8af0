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
#include "voxel_device.h"   // box, grid, keys, radix sort, flag compaction; the sort workspace

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
  for (; m + 4 <= e; m += 4) {                 // gather_in_order's loop, kept here: through it this kernel compiles five instructions longer
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
  SortWorkspace ws;                            // after the sort the free index buffer holds the run starts, the free key buffer vbeg | vend
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
  SortWorkspace& w = v->ws;
  v->mark(2);
  w.make_keys<K>(s, RecordPoints{in}, n, g);
  v->mark(3);
  const SortedPairs<K> sp = w.sort<K>(s, n, g);
  v->mark(4);
  const HeadSrc<K> hs{sp.keys, finite, sp.starts};
  w.count_scan(s, hs, finite, SLOT_RUNS, sp.starts, finite);
  w.write(s, hs, finite);
  if (min_points > 1) {
    unsigned* vbeg = reinterpret_cast<unsigned*>(sp.scratch);
    unsigned* vend = vbeg + w.cap;
    const KeepSrc ks{sp.starts, w.slots + SLOT_RUNS, min_points, vbeg, vend};
    w.count_scan(s, ks, finite, SLOT_VOXELS);
    w.write(s, ks, finite);
    v->vbeg = vbeg; v->vend = vend;
  } else {
    v->vbeg = sp.starts; v->vend = sp.starts + 1;     // every run has >= 1 member
  }
  v->mark(5);
  v->sidx = sp.idx;
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
  v->ctx = ctx;
  if (int r = v->ws.alloc(v->buf, max_points)) { rgbid_voxel_destroy(v); return r; }
  *out = v;
  return RGBID_OK;
}

int rgbid_voxel_destroy(rgbid_voxel* v) { return destroy_handle(v); }   // an emit may still read the tables

int rgbid_voxel_plan(rgbid_voxel* v, const rgbid_cloud_point* in_dev, unsigned long long n, const float leaf[3],
                     unsigned min_points, long long grid[6], unsigned long long stats[3], unsigned long long* voxels) {
  if (!v || !leaf || !voxels || !records_in_ok(in_dev, n, v->ws.cap)) return RGBID_E_INVALID;
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
  v->plan_timed = false; v->emit_timed = false;
  v->mark(0);
  v->ws.box(s, RecordPoints{in}, nu);
  v->mark(1);
  unsigned finite;
  float lo[3], hi[3];
  if (int r = v->ws.read_box(s, finite, lo, hi)) return r;
  if (stats) stats[0] = finite;
  if (finite == 0) return RGBID_OK;
  VoxGrid g;
  long long gr[6];
  if (int r = form_grid(lo, hi, leaf, g, gr)) return r;
  if (grid) memcpy(grid, gr, sizeof gr);
  if (int r = with_key_type(g, [&](auto k) { return sort_and_runs<decltype(k)>(v, in, nu, finite, g, min_points); })) return r;
  if (int r = v->ws.read_slots(s)) return r;
  const unsigned runs = v->ws.slots_host[SLOT_RUNS];
  const unsigned vox = min_points > 1 ? v->ws.slots_host[SLOT_VOXELS] : runs;
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
  if (!records_out_ok(out_dev, capacity, v->voxels)) return RGBID_E_INVALID;
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
