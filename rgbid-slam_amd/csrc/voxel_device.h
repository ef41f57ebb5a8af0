// voxel_device.h -- what the map filters over rgbid_cloud_point records share (kernels_voxel.hip, kernels_outlier.hip, kernels_consist.hip),
// and the mesh operators with them (mesh_device.h).  Device half: the box of the finite points of a point source (32-byte records or
// 12-byte vertices), the float32 grid and its cell keys, the stable LSD radix sort of (key, index) pairs, the keys of a sort by a tuple,
// the ordered sum over gathered members, the stable flag compaction and the exclusive value scan (the wave and block primitives they stand on are
// wave_device.h's).  Host half: SortWorkspace, the buffers of one handle and the launches over them, and the argument checks every
// plan / emit of a filter makes.
// Everything has internal linkage: each including file compiles its own copy of the kernels it launches.
#pragma once
#include "../../include/rgbid.h"
#include "common.h"
#include "hip_host.h"
#include "wave_device.h"

#include <cmath>
#include <cstddef>
#include <cstring>
#include <initializer_list>

namespace rgbid {
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

// ---- point sources --------------------------------------------------------------------------------------------------------------
// A source says where the position of point i lies: at(i) -> x y z (and a fourth float that nobody reads).
struct RecordPoints {                  // the first float4 of a 32-byte record: x y z nx
  const float4* in;
  __device__ __forceinline__ float4 at(unsigned i) const { return in[2 * (size_t)i]; }
};

struct VertexPoints {                  // three dwords of a 12-byte vertex
  const float* in;
  __device__ __forceinline__ float4 at(unsigned i) const {
    const size_t o = 3 * (size_t)i;
    return make_float4(in[o], in[o + 1], in[o + 2], 0.f);
  }
};

// ---- bounding box of the finite points ------------------------------------------------------------------------------------------
template <class P>
__global__ __launch_bounds__(VT) void k_vox_box(P in, unsigned n, float* __restrict__ part, unsigned* __restrict__ part_cnt) {
  __shared__ float lds[VT / 64][6];
  __shared__ unsigned ldc[VT / 64];
  float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  unsigned cnt = 0;
  for (unsigned i = blockIdx.x * VT + threadIdx.x; i < n; i += gridDim.x * VT) {
    const float4 a = in.at(i);
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

template <typename K, class P>
__global__ __launch_bounds__(VT) void k_vox_keys(P in, unsigned n, VoxGrid g, K* __restrict__ keys, unsigned* __restrict__ idx) {
  for (unsigned i = blockIdx.x * VT + threadIdx.x; i < n; i += gridDim.x * VT) {
    const float4 a = in.at(i);
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

// ---- sorting by a tuple: one stable sort per component, the last component first ------------------------------------------------------
// A key source says how many items it has (size) and the key of an item in round r (key(item, r)): it reads nothing through an item
// that is none and answers the sentinel, the largest key, for it.
// The keys of round r for the items in the order the last round left (order == null: the input order, and the items are written too).
template <class F>
__global__ __launch_bounds__(VT) void k_vox_round_keys(F key, int r, const unsigned* __restrict__ order, unsigned* __restrict__ keys,
                                                       unsigned* __restrict__ idx) {
  for (size_t m = (size_t)blockIdx.x * VT + threadIdx.x; m < key.size(); m += (size_t)gridDim.x * VT) {
    keys[m] = key(order ? order[m] : (unsigned)m, r);
    if (!order) idx[m] = (unsigned)m;
  }
}

// ---- sums over a row of gathered members, in the row's order -----------------------------------------------------------------------
// add(acc, load(ids[m])) for m = b .. e - 1, in that order: the bytes of a floating-point sum depend on it.  The gathers of 4 members are
// issued before their adds; add keeps every sum a separate rounding (RGBID_FP_STRICT).
template <class Acc, class Load, class Add>
__device__ __forceinline__ void gather_in_order(const unsigned* __restrict__ ids, unsigned b, unsigned e, Acc& acc, Load load, Add add) {
  unsigned m = b;
  for (; e - m >= 4; m += 4) {
    unsigned id[4];
    decltype(load(0u)) x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) id[u] = ids[m + u];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = load(id[u]);
#pragma unroll
    for (int u = 0; u < 4; ++u) add(acc, x[u]);
  }
  for (; m < e; ++m) add(acc, load(ids[m]));
}

// s / |s| in float; zeros when |s|^2 is 0 or not finite
__device__ __forceinline__ void unit_of(const double s[3], float n[3]) {
  RGBID_FP_STRICT
  n[0] = n[1] = n[2] = 0.f;
  const double q = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2];
  if (q != 0.0 && isfinite(q)) {
    const double l = sqrt(q);
    for (int a = 0; a < 3; ++a) n[a] = (float)(s[a] / l);
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
  __shared__ unsigned lds[VT / 64];
  const unsigned n = s.size();
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  if (t0 >= n) return;                 // uniform over the block
  unsigned carry = bc[blockIdx.x];
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    const bool f = i < n && s.flag((unsigned)i);
    unsigned tot;
    const unsigned rank = block_rank(f, lds, tot);
    if (f) s.write(carry + rank, (unsigned)i);
    carry += tot;
  }
}

// ---- the exclusive scan of one value per item, in the tile order of the flag compaction ------------------------------------------------
// A source says how many items it has (size), the value of an item (value) and what an item does with the sum before it (write).
template <class S>
__global__ __launch_bounds__(VT) void k_vox_sum_count(S s, unsigned* __restrict__ bc) {
  __shared__ unsigned lds[VT / 64];
  const unsigned n = s.size();
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  unsigned c = 0;
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    if (i < n) c += s.value((unsigned)i);
  }
  unsigned tot;
  block_scan_incl(c, lds, tot);
  if (threadIdx.x == 0) bc[blockIdx.x] = tot;
}

template <class S>
__global__ __launch_bounds__(VT) void k_vox_sum_write(S s, const unsigned* __restrict__ bc) {
  __shared__ unsigned lds[VT / 64];
  const unsigned n = s.size();
  const size_t t0 = (size_t)blockIdx.x * RUN_TILE;
  if (t0 >= n) return;                 // uniform over the block
  unsigned carry = bc[blockIdx.x];
  for (int j = 0; j < RUN_IPT; ++j) {
    const size_t i = t0 + j * VT + threadIdx.x;
    const unsigned v = i < n ? s.value((unsigned)i) : 0u;
    unsigned tot;
    const unsigned incl = block_scan_incl(v, lds, tot);
    if (i < n) s.write((unsigned)i, carry + incl - v, v);
    carry += tot;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
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

// calls f with a value of the key type the grid needs: 32-bit keys when the largest key + 1 < 2^32, 64-bit otherwise
template <class F>
int with_key_type(const VoxGrid& g, F&& f) { return g.sentinel < (1ull << 32) ? f(0u) : f(0ull); }

// what every plan checks about its input records and every emit about its output: count against capacity, null, 16-byte alignment
bool records_in_ok(const void* in_dev, unsigned long long n, unsigned long long cap) {
  return n <= cap && (n == 0 || in_dev) && !(((uintptr_t)in_dev) & 15);
}
bool records_out_ok(const void* out_dev, unsigned long long capacity, unsigned long long records) {
  return out_dev && capacity >= records && !(((uintptr_t)out_dev) & 15);
}

// the ping-pong buffers after a sort, for keys of type K
template <typename K>
struct SortedPairs {
  const K* keys;           // [n] ascending, the non-finite records' sentinel last
  const unsigned* idx;     // [n] their record indices, stable
  unsigned* starts;        // the free index buffer [cap + 1]
  K* scratch;              // the free key buffer: 8 B x cap whatever K is
};

// The buffers one filter handle sorts and compacts with, and the launches over them.  It launches and reads back; the stage marks and
// the launch check (hipGetLastError) stay with the caller.  24 B per point of capacity + the tables.
struct SortWorkspace {
  unsigned long long cap = 0;
  unsigned sort_tiles = 0, run_tiles = 0;             // at capacity
  unsigned long long* keys[2] = {nullptr, nullptr};   // [cap] 8 B each (32-bit keys use the first half)
  unsigned* idx[2] = {nullptr, nullptr};              // [cap + 1]
  unsigned* hist = nullptr;                           // [RADIX][sort_tiles]
  unsigned* dtotal = nullptr;                         // [RADIX]
  float* box_part = nullptr;                          // [VOX_MAX_GRID][6]
  unsigned* box_cnt = nullptr;                        // [VOX_MAX_GRID]
  unsigned* bc = nullptr;                             // [run_tiles] tile offsets of the last count_scan: valid until the next one
  unsigned* slots = nullptr;                          // [SLOTS] box, finite count, two compaction totals
  unsigned* slots_host = nullptr;                     // pinned

  // what count_scan / write / read_slots need, for a handle that compacts up to max_items items and sorts nothing
  int alloc_compaction(Buffers& buf, unsigned long long max_items) {
    cap = max_items;
    run_tiles = (unsigned)((max_items + RUN_TILE - 1) / RUN_TILE);
    int r = buf.alloc(&bc, sizeof(unsigned) * run_tiles);
    if (!r) r = buf.alloc(&slots, sizeof(unsigned) * SLOTS);
    if (!r) r = buf.alloc_host(&slots_host, sizeof(unsigned) * SLOTS);
    return r;
  }

  int alloc(Buffers& buf, unsigned long long max_points) {
    sort_tiles = (unsigned)((max_points + SORT_TILE - 1) / SORT_TILE);
    const size_t c = (size_t)max_points;
    int r = alloc_compaction(buf, max_points);
    for (int i = 0; i < 2 && !r; ++i) r = buf.alloc(&keys[i], sizeof(unsigned long long) * c);
    for (int i = 0; i < 2 && !r; ++i) r = buf.alloc(&idx[i], sizeof(unsigned) * (c + 1));
    if (!r) r = buf.alloc(&hist, sizeof(unsigned) * RADIX * (size_t)sort_tiles);
    if (!r) r = buf.alloc(&dtotal, sizeof(unsigned) * RADIX);
    if (!r) r = buf.alloc(&box_part, sizeof(float) * 6 * VOX_MAX_GRID);
    if (!r) r = buf.alloc(&box_cnt, sizeof(unsigned) * VOX_MAX_GRID);
    return r;
  }

  // the slot area as the stream leaves it -> slots_host; one host synchronisation
  int read_slots(hipStream_t s) {
    RGBID_HIP(hipMemcpyAsync(slots_host, slots, sizeof(unsigned) * SLOTS, hipMemcpyDeviceToHost, s));
    RGBID_HIP(hipStreamSynchronize(s));
    return RGBID_OK;
  }

  // box and count of the finite points of a source of n points -> slots
  template <class P>
  void box(hipStream_t s, const P& in, unsigned n) {
    const unsigned nb = grid_of(((unsigned long long)n + VT - 1) / VT);
    hipLaunchKernelGGL(k_vox_box<P>, dim3(nb), dim3(VT), 0, s, in, n, box_part, box_cnt);
    hipLaunchKernelGGL(k_vox_box_final, dim3(1), dim3(64), 0, s, box_part, box_cnt, (int)nb, slots);
  }
  int read_box(hipStream_t s, unsigned& finite, float lo[3], float hi[3]) {
    RGBID_HIP(hipGetLastError());
    if (int r = read_slots(s)) return r;
    finite = slots_host[SLOT_FINITE];
    memcpy(lo, slots_host + SLOT_BOX, 3 * sizeof(float));
    memcpy(hi, slots_host + SLOT_BOX + 3, 3 * sizeof(float));
    return RGBID_OK;
  }

  template <typename K>
  K* keys_as(int p) const { return reinterpret_cast<K*>(keys[p]); }   // key buffer p for keys of type K

  // one (key, index) pair per point into buffer 0
  template <typename K, class P>
  void make_keys(hipStream_t s, const P& in, unsigned n, const VoxGrid& g) {
    hipLaunchKernelGGL((k_vox_keys<K, P>), dim3(grid_of(((unsigned long long)n + VT - 1) / VT)), dim3(VT), 0, s, in, n, g, keys_as<K>(0), idx[0]);
  }

  // the stable sort of the n pairs in buffer p by the lowest `bits` bits of their keys, ping-ponging between the two buffers: three
  // launches per 8-bit pass -> the buffer that holds them afterwards
  template <typename K>
  int sort_bits(hipStream_t s, unsigned n, int bits, int p) {
    const unsigned ntiles = (n + SORT_TILE - 1) / SORT_TILE;
    const int passes = (bits + 7) / 8;
    for (int pass = 0; pass < passes; ++pass, p ^= 1) {
      hipLaunchKernelGGL(k_vox_hist<K>, dim3(ntiles), dim3(VT), 0, s, keys_as<K>(p), n, 8 * pass, hist, ntiles);
      hipLaunchKernelGGL(k_vox_scan_digits, dim3(RADIX), dim3(VT), 0, s, hist, ntiles, dtotal);
      hipLaunchKernelGGL(k_vox_scatter<K>, dim3(ntiles), dim3(VT), 0, s, keys_as<K>(p), idx[p], keys_as<K>(p ^ 1), idx[p ^ 1], n, 8 * pass, hist, dtotal, ntiles);
    }
    return p;
  }

  // the sort of make_keys' pairs by the bits a key of the grid can have
  template <typename K>
  SortedPairs<K> sort(hipStream_t s, unsigned n, const VoxGrid& g) {
    const int p = sort_bits<K>(s, n, bitlen(g.sentinel), 0);
    return SortedPairs<K>{keys_as<K>(p), idx[p], idx[p ^ 1], keys_as<K>(p ^ 1)};
  }

  // The n items 0 .. n - 1 sorted by a tuple of 32-bit keys: one stable sort per round of `rounds` (the tuple's last component first) by
  // key(item, round) <= sentinel, the keys recomputed in the order the round before left -> the buffer p that holds the result:
  // keys_as<unsigned>(p) the keys of the last round, idx[p] the items; the other buffer is free
  template <class F>
  int sort_rounds(hipStream_t s, const F& key, unsigned sentinel, unsigned n, std::initializer_list<int> rounds) {
    const unsigned g = grid_of(((unsigned long long)n + VT - 1) / VT);
    int p = 0;
    const unsigned* order = nullptr;
    for (int r : rounds) {
      hipLaunchKernelGGL(k_vox_round_keys<F>, dim3(g), dim3(VT), 0, s, key, r, order, keys_as<unsigned>(p), idx[p]);
      p = sort_bits<unsigned>(s, n, bitlen(sentinel), p);
      order = idx[p];
    }
    return p;
  }

  // The stable compaction of the flagged items of a source of at most `items` items, in two calls that may lie in different API calls.
  // count_scan: tile counts -> exclusive tile offsets in bc, the total in slots[slot]; with a tail, tail[total] = tail_val.
  template <class S>
  void count_scan(hipStream_t s, const S& src, unsigned items, int slot, unsigned* tail = nullptr, unsigned tail_val = 0u) {
    const unsigned tiles = (items + RUN_TILE - 1) / RUN_TILE;
    hipLaunchKernelGGL(k_vox_flag_count<S>, dim3(tiles), dim3(VT), 0, s, src, bc);
    hipLaunchKernelGGL(k_vox_scan1, dim3(1), dim3(VT), 0, s, bc, tiles, slots, slot, tail, tail_val);
  }
  // write: every flagged item at its rank, with the bc of the count_scan over the same flags
  template <class S>
  void write(hipStream_t s, const S& src, unsigned items) {
    hipLaunchKernelGGL(k_vox_flag_write<S>, dim3((items + RUN_TILE - 1) / RUN_TILE), dim3(VT), 0, s, src, bc);
  }
  // The exclusive scan of a value source of at most `items` > 0 items: tile sums, the one-block scan of them (the total in slots[slot]),
  // every item's write with the sum before it.  It uses bc as a count_scan does
  template <class S>
  void value_scan(hipStream_t s, const S& src, unsigned items, int slot) {
    const unsigned tiles = (items + RUN_TILE - 1) / RUN_TILE;
    hipLaunchKernelGGL(k_vox_sum_count<S>, dim3(tiles), dim3(VT), 0, s, src, bc);
    hipLaunchKernelGGL(k_vox_scan1, dim3(1), dim3(VT), 0, s, bc, tiles, slots, slot, (unsigned*)nullptr, 0u);
    hipLaunchKernelGGL(k_vox_sum_write<S>, dim3(tiles), dim3(VT), 0, s, src, bc);
  }
};

}  // namespace
}  // namespace rgbid
