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

#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

using namespace rgbid;

static_assert(sizeof(rgbid_voxel_point) == 32, "rgbid_voxel_point is two 16-byte stores");
static_assert(offsetof(rgbid_voxel_point, count) == offsetof(rgbid_cloud_point, pixel), "count sits where the cloud record holds its pixel");

namespace {

constexpr int VT = 256;                      // threads per block
constexpr int RADIX = 256;                   // 8-bit digits
constexpr int SORT_IPT = 16;                 // keys per thread of a sort tile
constexpr int SORT_TILE = VT * SORT_IPT;     // 4 096 keys; a wave ranks 1 024 contiguous keys in 16 rounds of 64
constexpr int RUN_IPT = 8;
constexpr int RUN_TILE = VT * RUN_IPT;       // 2 048 items per tile of the run compactions
constexpr int VOX_MAX_GRID = 2048;           // grid-strided kernels: 256 CUs x 8 blocks
enum { SLOT_BOX = 0, SLOT_FINITE = 6, SLOT_RUNS = 7, SLOT_VOXELS = 8, SLOTS = 16 };

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

__device__ __forceinline__ unsigned lane_prefix(unsigned long long m) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// inclusive scan of one value per thread over the block (256 threads); returns the block total through `total`
__device__ __forceinline__ unsigned block_scan_incl(unsigned v, unsigned* lds, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  unsigned before = 0;
  for (int i = 0; i < wave; ++i) before += lds[i];
  total = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return v + before;
}

// ---- bounding box of the finite points ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(VT) void k_vox_box(const float4* __restrict__ in, unsigned n, float* __restrict__ part, unsigned* __restrict__ part_cnt) {
  __shared__ float lds[VT / 64][6];
  __shared__ unsigned ldc[VT / 64];
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  unsigned cnt = 0;
  for (unsigned i = blockIdx.x * VT + threadIdx.x; i < n; i += gridDim.x * VT) {
    const float4 a = in[2 * (size_t)i];     // x y z nx of a 32-byte record
    if (finite3(a.x, a.y, a.z)) {
      ++cnt;
      v[0] = fminf(v[0], a.x); v[1] = fminf(v[1], a.y); v[2] = fminf(v[2], a.z);
      v[3] = fmaxf(v[3], a.x); v[4] = fmaxf(v[4], a.y); v[5] = fmaxf(v[5], a.z);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int k = 0; k < 3; ++k) v[k] = fminf(v[k], __shfl_xor(v[k], o, 64));
    for (int k = 3; k < 6; ++k) v[k] = fmaxf(v[k], __shfl_xor(v[k], o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { for (int k = 0; k < 6; ++k) lds[wave][k] = v[k]; ldc[wave] = cnt; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    float r = lds[0][k];
    for (int w = 1; w < VT / 64; ++w) r = k < 3 ? fminf(r, lds[w][k]) : fmaxf(r, lds[w][k]);
    part[6 * blockIdx.x + k] = r;
  }
  if (threadIdx.x == 6) part_cnt[blockIdx.x] = ldc[0] + ldc[1] + ldc[2] + ldc[3];
}

// one wave: the block partials -> box[6] floats | finite count in the slot area
__global__ __launch_bounds__(64) void k_vox_box_final(const float* __restrict__ part, const unsigned* __restrict__ part_cnt, int nb, unsigned* __restrict__ slots) {
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  unsigned cnt = 0;
  for (int b = threadIdx.x; b < nb; b += 64) {
    for (int k = 0; k < 3; ++k) v[k] = fminf(v[k], part[6 * b + k]);
    for (int k = 3; k < 6; ++k) v[k] = fmaxf(v[k], part[6 * b + k]);
    cnt += part_cnt[b];
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int k = 0; k < 3; ++k) v[k] = fminf(v[k], __shfl_xor(v[k], o, 64));
    for (int k = 3; k < 6; ++k) v[k] = fmaxf(v[k], __shfl_xor(v[k], o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (threadIdx.x == 0) {
    for (int k = 0; k < 6; ++k) slots[SLOT_BOX + k] = __float_as_uint(v[k]);
    slots[SLOT_FINITE] = cnt;
  }
}

// ---- keys -----------------------------------------------------------------------------------------------------------------------
struct VoxGrid {
  float inv[3];                 // 1.f / leaf
  float minb[3];                // (float) min_b
  unsigned long long d0, d01;   // div_b_0, div_b_0 div_b_1
  unsigned long long sentinel;  // largest key of a finite point + 1: the key of the non-finite records
};

// PCL's cell index: one float multiply, floorf, a float subtraction, the truncation (the host has checked that it lies in [0, 2^31))
__device__ __forceinline__ unsigned long long cell_key(float x, float y, float z, const VoxGrid& g) {
  RGBID_FP_STRICT
  const unsigned i0 = (unsigned)(int)(floorf(x * g.inv[0]) - g.minb[0]);
  const unsigned i1 = (unsigned)(int)(floorf(y * g.inv[1]) - g.minb[1]);
  const unsigned i2 = (unsigned)(int)(floorf(z * g.inv[2]) - g.minb[2]);
  return (unsigned long long)i0 + (unsigned long long)i1 * g.d0 + (unsigned long long)i2 * g.d01;
}

template <typename K>
__global__ __launch_bounds__(VT) void k_vox_keys(const float4* __restrict__ in, unsigned n, VoxGrid g, K* __restrict__ keys, unsigned* __restrict__ idx) {
  for (unsigned i = blockIdx.x * VT + threadIdx.x; i < n; i += gridDim.x * VT) {
    const float4 a = in[2 * (size_t)i];
    keys[i] = (K)(finite3(a.x, a.y, a.z) ? cell_key(a.x, a.y, a.z, g) : g.sentinel);
    idx[i] = i;
  }
}

// ---- stable LSD radix sort of (key, index), 8 bits per pass -----------------------------------------------------------------------
template <typename K>
__device__ __forceinline__ unsigned digit_of(K k, int shift) { return (unsigned)(k >> shift) & (RADIX - 1); }

// digit counts of one tile -> hist[digit][tile] (digit-major: a scan along a digit's row gives the tiles' offsets)
template <typename K>
__global__ __launch_bounds__(VT) void k_vox_hist(const K* __restrict__ keys, unsigned n, int shift, unsigned* __restrict__ hist, unsigned ntiles) {
  __shared__ unsigned cnt[RADIX];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * SORT_TILE;
  unsigned d[SORT_IPT];
#pragma unroll
  for (int j = 0; j < SORT_IPT; ++j) {
    const size_t i = base + j * VT + threadIdx.x;
    d[j] = i < n ? digit_of(keys[i], shift) : RADIX;
  }
#pragma unroll
  for (int j = 0; j < SORT_IPT; ++j)
    if (d[j] < RADIX) atomicAdd(&cnt[d[j]], 1u);     // integer counts: exact in any order
  __syncthreads();
  hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// one block per digit: exclusive scan of its tile counts in place, the digit's total
__global__ __launch_bounds__(VT) void k_vox_scan_digits(unsigned* __restrict__ hist, unsigned ntiles, unsigned* __restrict__ dtotal) {
  __shared__ unsigned lds[VT / 64];
  unsigned* h = hist + (size_t)blockIdx.x * ntiles;
  unsigned carry = 0;
  for (unsigned base = 0; base < ntiles; base += VT) {
    const unsigned i = base + threadIdx.x;
    const unsigned v = i < ntiles ? h[i] : 0u;
    unsigned tot;
    const unsigned incl = block_scan_incl(v, lds, tot);
    if (i < ntiles) h[i] = carry + incl - v;
    carry += tot;
  }
  if (threadIdx.x == 0) dtotal[blockIdx.x] = carry;
}

// A tile's keys in input order are (wave, round, lane): wave w owns keys [w 1024, (w + 1) 1024) of the tile.  In each round the lanes
// of equal digit find each other with 8 ballots; the lowest of them adds the group's size to the wave's counter of that digit (an LDS
// integer add returning the old value, in program order) and broadcasts the old value.  Position = digit base + tile offset + the
// counts of lower waves + the rank inside the wave: stable.
template <typename K>
__global__ __launch_bounds__(VT) void k_vox_scatter(const K* __restrict__ kin, const unsigned* __restrict__ vin, K* __restrict__ kout,
                                                    unsigned* __restrict__ vout, unsigned n, int shift, const unsigned* __restrict__ hist,
                                                    const unsigned* __restrict__ dtotal, unsigned ntiles) {
  __shared__ unsigned wcnt[VT / 64][RADIX];
  __shared__ unsigned base[RADIX];
  __shared__ unsigned lds[VT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  {
    const unsigned v = dtotal[threadIdx.x];
    unsigned tot;
    const unsigned incl = block_scan_incl(v, lds, tot);
    base[threadIdx.x] = incl - v + hist[(size_t)threadIdx.x * ntiles + blockIdx.x];
  }
  for (int w = 0; w < VT / 64; ++w) wcnt[w][threadIdx.x] = 0;
  __syncthreads();
  const size_t t0 = (size_t)blockIdx.x * SORT_TILE + (size_t)wave * (64 * SORT_IPT);
  K k[SORT_IPT];
  unsigned v[SORT_IPT], rank[SORT_IPT];
#pragma unroll
  for (int j = 0; j < SORT_IPT; ++j) {
    const size_t i = t0 + j * 64 + lane;
    k[j] = i < n ? kin[i] : (K)0;
    v[j] = i < n ? vin[i] : 0u;
  }
#pragma unroll
  for (int j = 0; j < SORT_IPT; ++j) {
    const bool valid = t0 + j * 64 + lane < n;
    const unsigned d = digit_of(k[j], shift);
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const unsigned long long bb = __ballot((d >> b) & 1u);
      m &= ((d >> b) & 1u) ? bb : ~bb;
    }
    const unsigned pre = lane_prefix(m);
    const int leader = m ? __builtin_ctzll(m) : 0;
    unsigned old = 0;
    if (valid && pre == 0) old = atomicAdd(&wcnt[wave][d], (unsigned)__popcll(m));
    old = __shfl(old, leader, 64);
    rank[j] = old + pre;
  }
  __syncthreads();
  {
    const unsigned c0 = wcnt[0][threadIdx.x], c1 = wcnt[1][threadIdx.x], c2 = wcnt[2][threadIdx.x];
    const unsigned b0 = base[threadIdx.x];
    wcnt[0][threadIdx.x] = b0;
    wcnt[1][threadIdx.x] = b0 + c0;
    wcnt[2][threadIdx.x] = b0 + c0 + c1;
    wcnt[3][threadIdx.x] = b0 + c0 + c1 + c2;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SORT_IPT; ++j) {
    if (t0 + j * 64 + lane >= n) continue;
    const unsigned pos = wcnt[wave][digit_of(k[j], shift)] + rank[j];
    kout[pos] = k[j];
    vout[pos] = v[j];
  }
}

// ---- stable compactions: run heads, then the runs of >= min_points members ------------------------------------------------------
// A source says how many items it has (size), which of them are kept (flag) and what a kept item writes at its rank (write).
template <typename K>
struct HeadSrc {                       // item i < finite: key[i] != key[i - 1] -> starts[rank] = i
  const K* keys;
  unsigned finite;
  unsigned* starts;
  __device__ __forceinline__ unsigned size() const { return finite; }
  __device__ __forceinline__ bool flag(unsigned i) const { return i == 0 || keys[i] != keys[i - 1]; }
  __device__ __forceinline__ void write(unsigned pos, unsigned i) const { starts[pos] = i; }
};

struct KeepSrc {                       // run r < runs: starts[r + 1] - starts[r] >= min_points -> (begin, end) of voxel `rank`
  const unsigned* starts;
  const unsigned* runs;                // device slot
  unsigned min_points;
  unsigned* vbeg;
  unsigned* vend;
  __device__ __forceinline__ unsigned size() const { return *runs; }
  __device__ __forceinline__ bool flag(unsigned r) const { return starts[r + 1] - starts[r] >= min_points; }
  __device__ __forceinline__ void write(unsigned pos, unsigned r) const { vbeg[pos] = starts[r]; vend[pos] = starts[r + 1]; }
};

template <class S>
__global__ __launch_bounds__(VT) void k_vox_flag_count(S s, unsigned* __restrict__ bc) {
  __shared__ unsigned lds[VT / 64];
  const unsigned n = s.size();
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  unsigned c = 0;
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    if (i < n && s.flag((unsigned)i)) ++c;
  }
  unsigned tot;
  block_scan_incl(c, lds, tot);
  if (threadIdx.x == 0) bc[blockIdx.x] = tot;
}

// one block: exclusive scan of nb tile counts in place -> slots[slot] = total; tail (optional): tail[total] = tail_val
__global__ __launch_bounds__(VT) void k_vox_scan1(unsigned* __restrict__ bc, unsigned nb, unsigned* __restrict__ slots, int slot,
                                                  unsigned* __restrict__ tail, unsigned tail_val) {
  __shared__ unsigned lds[VT / 64];
  unsigned carry = 0;
  for (unsigned base = 0; base < nb; base += VT) {
    const unsigned i = base + threadIdx.x;
    const unsigned v = i < nb ? bc[i] : 0u;
    unsigned tot;
    const unsigned incl = block_scan_incl(v, lds, tot);
    if (i < nb) bc[i] = carry + incl - v;
    carry += tot;
  }
  if (threadIdx.x == 0) {
    slots[slot] = carry;
    if (tail) tail[carry] = tail_val;
  }
}

// items of a tile in (round, wave, lane) order: rank = tile offset + earlier rounds + lower waves + mbcnt
template <class S>
__global__ __launch_bounds__(VT) void k_vox_flag_write(S s, const unsigned* __restrict__ bc) {
  __shared__ unsigned wsum[VT / 64];
  const unsigned n = s.size();
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  if (t0 >= n) return;                 // uniform over the block
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned carry = bc[blockIdx.x];
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    const bool f = i < n && s.flag((unsigned)i);
    const unsigned long long m = __ballot(f);
    if (lane == 0) wsum[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    const unsigned tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    if (f) s.write(carry + before + lane_prefix(m), (unsigned)i);
    carry += tot;
  }
}

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

unsigned grid_of(unsigned long long items) { return items < VOX_MAX_GRID ? (unsigned)(items ? items : 1) : VOX_MAX_GRID; }

int bitlen(unsigned long long x) { return x ? 64 - __builtin_clzll(x) : 0; }

// the grid of DESIGN.md section 12 from the box, in float32 as PCL forms it; RGBID_E_INVALID when a bound leaves the int32 range, a
// cell index could not be held by an int, or the grid has 2^62 cells or more
int form_grid(const float lo[3], const float hi[3], const float leaf[3], VoxGrid& g, long long grid[6]) {
  RGBID_FP_STRICT
  unsigned long long div[3], ijk_max[3];
  for (int a = 0; a < 3; ++a) {
    const float inv = 1.0f / leaf[a];
    const float flo = floorf(lo[a] * inv), fhi = floorf(hi[a] * inv);
    if (!(flo >= -2147483648.f && flo < 2147483648.f && fhi >= -2147483648.f && fhi < 2147483648.f)) return RGBID_E_INVALID;
    const int min_b = (int)flo, max_b = (int)fhi;
    const float span = fhi - (float)min_b;   // the largest cell index a point can get (the float operations are monotone)
    if (!(span < 2147483648.f)) return RGBID_E_INVALID;
    g.inv[a] = inv;
    g.minb[a] = (float)min_b;
    div[a] = (unsigned long long)((long long)max_b - min_b + 1);
    ijk_max[a] = (unsigned long long)(int)span;
    grid[a] = min_b;
    grid[3 + a] = (long long)div[a];
  }
  const unsigned __int128 cells = (unsigned __int128)div[0] * div[1] * div[2];
  if (cells >= ((unsigned __int128)1 << 62)) return RGBID_E_INVALID;
  g.d0 = div[0];
  g.d01 = div[0] * div[1];
  const unsigned __int128 kmax = (unsigned __int128)ijk_max[0] + (unsigned __int128)ijk_max[1] * g.d0 + (unsigned __int128)ijk_max[2] * g.d01;
  if (kmax >= ((unsigned __int128)1 << 63)) return RGBID_E_INVALID;
  g.sentinel = (unsigned long long)kmax + 1;
  return RGBID_OK;
}

template <typename K>
int sort_and_runs(rgbid_voxel* v, const float4* in, unsigned n, unsigned finite, const VoxGrid& g, unsigned min_points) {
  hipStream_t s = v->ctx->stream;
  K* keys[2] = {reinterpret_cast<K*>(v->keys[0]), reinterpret_cast<K*>(v->keys[1])};
  v->mark(2);
  hipLaunchKernelGGL(k_vox_keys<K>, dim3(grid_of((n + VT - 1) / VT)), dim3(VT), 0, s, in, n, g, keys[0], v->idx[0]);
  v->mark(3);
  const unsigned ntiles = (n + SORT_TILE - 1) / SORT_TILE;
  const int passes = (bitlen(g.sentinel) + 7) / 8;
  int p = 0;
  for (int pass = 0; pass < passes; ++pass, p ^= 1) {
    hipLaunchKernelGGL(k_vox_hist<K>, dim3(ntiles), dim3(VT), 0, s, keys[p], n, 8 * pass, v->hist, ntiles);
    hipLaunchKernelGGL(k_vox_scan_digits, dim3(RADIX), dim3(VT), 0, s, v->hist, ntiles, v->dtotal);
    hipLaunchKernelGGL(k_vox_scatter<K>, dim3(ntiles), dim3(VT), 0, s, keys[p], v->idx[p], keys[p ^ 1], v->idx[p ^ 1], n, 8 * pass, v->hist,
                       v->dtotal, ntiles);
  }
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
