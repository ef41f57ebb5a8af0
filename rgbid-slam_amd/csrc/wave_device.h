// wave_device.h -- the wave64 and block primitives of the scan / compaction kernels, each written once: a lane's rank in a ballot, the
// butterfly sum of a wave and that sum added to a count slot, the inclusive scan and the flag rank of a block of BLOCK_WAVES waves (256 threads: VT, CT, LT and BT).
// Everything has internal linkage and is inlined into the kernels of the including file.
#pragma once
#include "common.h"

namespace rgbid {
namespace {

constexpr int BLOCK_WAVES = 4;   // the block primitives take an LDS array of this many values

// set bits of a ballot below this lane
__device__ __forceinline__ unsigned lane_prefix(unsigned long long ballot) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// wave total in every lane, for integers and double; float has the DPP overload of common.h
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the wave's total of c added to *slot, when it is not 0: one integer atomic per wave.  Called by all lanes of the wave together
template <typename S, typename T>
__device__ __forceinline__ void wave_add_to(S* slot, T c) {
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(slot, (S)c);
}

// inclusive scan of one value per thread over the block; returns the block total through `total`.  Two barriers: lds is free again
template <typename T>
__device__ __forceinline__ T block_scan_incl(T v, T* lds, T& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  if (lane == 63) lds[wave] = v;
  __syncthreads();
  T before = 0;
  for (int i = 0; i < wave; ++i) before += lds[i];
  total = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return v + before;
}

// exclusive rank of this thread among the flagged threads of the block in (wave, lane) order: one ballot, the waves' popcounts through
// LDS, mbcnt.  Returns the number of flagged threads through `total`.  Two barriers: lds is free again
__device__ __forceinline__ unsigned block_rank(bool flag, unsigned* lds, unsigned& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) lds[wave] = (unsigned)__popcll(m);
  __syncthreads();
  unsigned before = 0;
  for (int w = 0; w < wave; ++w) before += lds[w];
  total = lds[0] + lds[1] + lds[2] + lds[3];
  __syncthreads();
  return before + lane_prefix(m);
}

}  // namespace
}  // namespace rgbid
