// segment_host.h -- the host half of the segmenter that needs no device (include/rgbid_segment.h): the argument checks of create and run, the
// bin table and the sizing of the workspace.  Plain C++ with no HIP call, so that it also builds into a stand-alone program under the
// host sanitizers (tools/segment_host_check.cpp).
#pragma once
#include "../../include/rgbid_segment.h"

#include <cmath>
#include <cstddef>

namespace rgbid {
namespace seghost {

constexpr unsigned long long SORT_TILE_KEYS = 4096, RUN_TILE_ITEMS = 2048, SORT_RADIX = 256, BOX_GRID = 2048, WS_SLOTS = 16;   // voxel_device.h

// rows x cols keyframes, max_keyframes of them: edge ids 4 * pixel + nb of the whole batch are 32-bit, 0xffffffff is no edge
inline bool create_args_ok(int rows, int cols, int max_keyframes, int max_segments) {
  if (rows < 1 || cols < 1 || max_keyframes < 1 || max_segments < 1) return false;
  const unsigned long long P = (unsigned long long)rows * (unsigned long long)cols;
  if (P > (1ull << 28)) return false;
  if ((unsigned long long)max_segments > P) return false;
  return 4ull * P * (unsigned long long)max_keyframes < 0xffffffffull;
}

inline bool run_args_ok(int n, int max_keyframes, const void* src, const float* K, float k_th, int min_size, int nbins, int levels) {
  if (n < 1 || n > max_keyframes || !src || !K) return false;
  if (!(std::isfinite(k_th) && k_th >= 0.f)) return false;
  if (min_size < 1) return false;
  if (nbins < 1 || nbins > RGBID_SEGMENT_MAX_BINS) return false;
  return levels >= 1 && levels <= RGBID_SEGMENT_MAX_LEVELS;
}

// the golden-section spiral of the reference (src/util_funcs.cpp:157-173), every operation in float
inline void bins(int nbins, float* c) {
  const float inc = 3.141592f * (3.f - sqrtf(5.f));
  const float off = 2.f / (float)nbins;
  for (int i = 0; i < nbins; ++i) {
    const float y = ((float)i * off - 1.f) + off / 2.f;
    const float r = sqrtf(1.f - y * y);
    const float phi = (float)i * inc;
    c[3 * i] = cosf(phi) * r;
    c[3 * i + 1] = y;
    c[3 * i + 2] = sinf(phi) * r;
  }
}

// device bytes of a handle: the sort workspace over 4 P max_keyframes edge slots (SortWorkspace::alloc) and the segmenter's own tables
inline unsigned long long workspace_bytes(int rows, int cols, int max_keyframes, int max_segments) {
  const unsigned long long P = (unsigned long long)rows * cols, kf = (unsigned long long)max_keyframes, S = (unsigned long long)max_segments;
  const unsigned long long E = 4 * P * kf;
  unsigned long long b = 2 * 8 * E + 2 * 4 * (E + 1);                                        // keys, indices
  b += 4 * SORT_RADIX * ((E + SORT_TILE_KEYS - 1) / SORT_TILE_KEYS) + 4 * SORT_RADIX;        // digit histograms
  b += 4 * 6 * BOX_GRID + 4 * BOX_GRID + 4 * ((E + RUN_TILE_ITEMS - 1) / RUN_TILE_ITEMS) + 4 * WS_SLOTS;
  b += 16 * P * kf;                                                                          // points
  b += 4 * 4 * P * kf;                                                                       // parent, size, th, reservation / segment index
  b += 4 * S * kf;                                                                           // entropies
  b += 8 * kf + 4 * kf + 4 * 2 * kf + 4 * RGBID_SEGMENT_THRESHOLDS * kf;                     // block pointers, edge counts, rounds, c_k
  b += 4 * 3 * RGBID_SEGMENT_MAX_BINS;                                                       // bin centres
  return b;
}

}  // namespace seghost
}  // namespace rgbid
