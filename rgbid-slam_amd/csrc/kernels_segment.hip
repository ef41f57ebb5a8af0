// kernels_segment.hip -- superjut segmentation of keyframes, normal histograms, negentropy image and masks (include/rgbid_segment.h,
// DESIGN.md section 16; the reference's CloudSegmenter / Segmentation::Graph, Superjut::computeHistogramOfNormalsAndEntropy and
// Keyframe::computeMaskedDescriptors).
//
// One run over a batch of n keyframes of P = rows x cols pixels:
//   edges   k_seg_points        the camera-frame point of every pixel (cloud_device.h), the union-find state of every point
//           k_seg_edges         4 edge slots per pixel: key = keyframe << 32 | order-preserving bits of the weight (-0 folded onto +0; a slot
//                               without an edge gets 0xffffffff, above every weight), value = the slot's index in the batch; edges per keyframe
//   sort    SortWorkspace       stable LSD radix sort: keyframe k's edges are the first ecount[k] entries of [4 P k, 4 P (k + 1)), ascending
//                               by (weight, edge id)
//   pass 1  k_seg_unionfind<1>  one workgroup per keyframe walks its run in rounds of deterministic reservations (below)
//   pass 2  k_seg_unionfind<2>  the same with the small-component predicate
//   labels  k_seg_flatten, k_seg_label   every pixel's root (into the labels output); the roots (each the smallest pixel of its segment)
//                               ranked in raster order
//   rest    k_seg_hist, k_seg_entropy, k_seg_image, k_seg_levels   labels + integer histogram, entropies, negentropy + c_k, the k*
//
// Rounds.  The window is the first W undecided edges of the run, in order, one per thread.  Every window edge finds its two roots; equal
// roots decide it (dropped).  Every other one writes its position into both roots' reservation words with an atomic min.  After a barrier
// an edge that reads its own position in both words is the earliest undecided edge touching either component, so no undecided edge before
// it can change what it is about to read: it is decided against size / th exactly as the sequential loop decides it.  Winners own
// disjoint pairs of roots, so their merges do not meet.  The first undecided edge always wins: a pass of E edges ends within E rounds.
// The survivors are compacted to the front in order and the window is refilled from the run.
// A merge keeps the smaller pixel as the root, so a segment's root is its first pixel in raster order.
#include "../../include/rgbid_segment.h"
#include "cloud_device.h"
#include "common.h"
#include "hip_host.h"
#include "segment_host.h"
#include "voxel_device.h"   // the radix sort and its workspace; wave_device.h

#include <cmath>
#include <cstring>
#include <new>

using namespace rgbid;

namespace {

constexpr unsigned NONE = 0xffffffffu;
constexpr int NTH = RGBID_SEGMENT_THRESHOLDS;
static_assert(RGBID_SEGMENT_MAX_WINDOW == VT, "one window edge per thread");
static_assert(seghost::SORT_TILE_KEYS == SORT_TILE && seghost::RUN_TILE_ITEMS == RUN_TILE && seghost::SORT_RADIX == RADIX &&
              seghost::BOX_GRID == VOX_MAX_GRID && seghost::WS_SLOTS == SLOTS, "segment_host.h sizes the sort workspace");

struct SegGeom {
  double kinv[9];
  int rows, cols, P, n, S;
};

struct Thresholds { float t[NTH]; };

__device__ __forceinline__ unsigned aload(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void astore(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// order-preserving bits of a weight that is not NaN, -0 folded onto +0; and back
__device__ __forceinline__ unsigned weight_key(float w) {
  const unsigned b = w == 0.f ? 0u : __float_as_uint(w);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_weight(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

__device__ __forceinline__ int neighbour(int x, int y, int nb, int rows, int cols) {
  const int x2 = nb == 1 ? x : x + 1;
  const int y2 = nb == 0 ? y : (nb == 2 ? y - 1 : y + 1);
  return (x2 < cols && y2 >= 0 && y2 < rows) ? y2 * cols + x2 : -1;
}

// grid (tiles, n): the point of every pixel, w = 1 where the pixel is a point; every point its own component
__global__ __launch_bounds__(VT) void k_seg_points(const char* const* __restrict__ blocks, SegGeom g, float kth, float4* __restrict__ pts,
                                                   int* __restrict__ parent, int* __restrict__ size, float* __restrict__ th,
                                                   unsigned* __restrict__ resv) {
  const int i = blockIdx.x * VT + threadIdx.x, k = blockIdx.y;
  if (i >= g.P) return;
  const char* blk = blocks[k];
  const float* iD = reinterpret_cast<const float*>(blk + 4 * (size_t)g.P);
  const float* nr = reinterpret_cast<const float*>(blk + 8 * (size_t)g.P);
  const float n0 = nr[i], n1 = nr[g.P + i], n2 = nr[2 * (size_t)g.P + i];
  float d;
  const bool valid = cloud_valid(iD[i], n0, 0u, RGBID_CLOUD_ALL, d);
  const double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  float o[6];
  cloud_point(d, i % g.cols, i / g.cols, g.kinv, R, t, n0, n1, n2, o);
  const size_t q = (size_t)k * g.P + i;
  pts[q] = make_float4(o[0], o[1], o[2], valid ? 1.f : 0.f);
  parent[q] = i;
  size[q] = 1;
  th[q] = kth;
  resv[q] = NONE;
}

// grid (tiles, n): the 4 edge slots of every pixel
template <typename K>
__global__ __launch_bounds__(VT) void k_seg_edges(const char* const* __restrict__ blocks, SegGeom g, const float4* __restrict__ pts,
                                                  K* __restrict__ keys, unsigned* __restrict__ idx, unsigned* __restrict__ ecount) {
  RGBID_FP_STRICT
  const int i = blockIdx.x * VT + threadIdx.x, k = blockIdx.y;
  unsigned cnt = 0;
  if (i < g.P) {
    const float* nr = reinterpret_cast<const float*>(blocks[k] + 8 * (size_t)g.P);
    const float4* pk = pts + (size_t)k * g.P;
    const float4 p1 = pk[i];
    const float n1x = nr[i], n1y = nr[g.P + i], n1z = nr[2 * (size_t)g.P + i];
    const int x = i % g.cols, y = i / g.cols;
    const size_t e0 = 4 * ((size_t)k * g.P + i);
    for (int nb = 0; nb < 4; ++nb) {
      unsigned u = NONE;
      const int j = p1.w != 0.f ? neighbour(x, y, nb, g.rows, g.cols) : -1;
      if (j >= 0) {
        const float4 p2 = pk[j];
        if (p2.w != 0.f) {
          const float n2x = nr[j], n2y = nr[g.P + j], n2z = nr[2 * (size_t)g.P + j];
          const float dx = p2.x - p1.x, dy = p2.y - p1.y, dz = p2.z - p1.z;
          const float norm = sqrtf((dx * dx + dy * dy) + dz * dz);
          const float dot = (n1x * n2x + n1y * n2y) + n1z * n2z;
          const float dot2 = (1.f / norm) * ((n2x * dx + n2y * dy) + n2z * dz);
          float c = 1.f - dot;
          if (dot2 > 0.f) c = c * c;
          if (!isnan(c)) { u = weight_key(c); ++cnt; }
        }
      }
      keys[e0 + nb] = (K)(((unsigned long long)k << 32) | u);   // a 32-bit key (one keyframe) keeps u
      idx[e0 + nb] = (unsigned)(e0 + nb);
    }
  }
  wave_add_to(&ecount[k], cnt);   // integer count: exact in any order
}

__device__ __forceinline__ int find_root(int* par, int x) {
  int p = par[x];
  while (p != x) {                 // path halving: whatever a racing find writes here is an ancestor too
    const int gp = par[p];
    par[x] = gp;
    x = gp;
    p = par[x];
  }
  return x;
}

// one workgroup per keyframe; PASS 1 merges by the thresholds, PASS 2 the small components
template <int PASS, typename K>
__global__ __launch_bounds__(VT) void k_seg_unionfind(const K* __restrict__ keys, const unsigned* __restrict__ idx,
                                                      const unsigned* __restrict__ ecount, SegGeom g, unsigned W, float kth, int min_size,
                                                      int* parent, int* size, float* th, unsigned* resv, unsigned* __restrict__ rounds) {
  RGBID_FP_STRICT
  __shared__ unsigned q[VT];
  __shared__ unsigned lds[BLOCK_WAVES];
  const unsigned t = threadIdx.x;
  const int k = blockIdx.x;
  const unsigned E = ecount[k];
  const size_t base = 4 * (size_t)k * g.P;
  int* par = parent + (size_t)k * g.P;
  int* sz = size + (size_t)k * g.P;
  float* tk = th + (size_t)k * g.P;
  unsigned* rs = resv + (size_t)k * g.P;
  unsigned live = 0, next = 0, nrounds = 0;
  for (unsigned it = 0; it <= E; ++it) {          // every round decides its first edge: at most E rounds, then the empty one
    if (t >= live && t < W) q[t] = next + (t - live);
    const unsigned added = min(W - live, E - next);
    next += added;
    live += added;
    if (live == 0) break;                         // uniform
    __syncthreads();                              // the window; the merges of the last round
    const bool active = t < live;
    const unsigned pos = active ? q[t] : NONE;
    int a = 0, b = 0;
    bool open = false;
    if (active) {
      const unsigned e = idx[base + pos] - (unsigned)base;
      const int pix = (int)(e >> 2);
      a = find_root(par, pix);
      b = find_root(par, neighbour(pix % g.cols, pix / g.cols, (int)(e & 3u), g.rows, g.cols));
      open = a != b;
      if (open) { atomicMin(&rs[a], pos); atomicMin(&rs[b], pos); }
    }
    __syncthreads();
    const bool win = open && aload(&rs[a]) == pos && aload(&rs[b]) == pos;
    __syncthreads();                              // every reservation is read before any is cleared
    if (open) { astore(&rs[a], NONE); astore(&rs[b], NONE); }
    if (win) {
      const int sa = sz[a], sb = sz[b];
      bool merge;
      const float w = key_weight((unsigned)keys[base + pos]);
      if (PASS == 1) merge = w <= tk[a] && w <= tk[b];
      else merge = sa < min_size || sb < min_size;
      if (merge) {
        const int r = min(a, b), c = max(a, b);
        par[c] = r;
        sz[r] = sa + sb;
        if (PASS == 1) tk[r] = w + kth / (float)(sa + sb);
      }
    }
    const bool stay = open && !win;
    unsigned tot;
    const unsigned rank = block_rank(stay, lds, tot);
    if (stay) q[rank] = pos;                      // after block_rank's barriers: every thread has read its q[t]
    live = tot;
    ++nrounds;
  }
  if (t == 0) rounds[k] = nrounds;
}

// grid (tiles, n): root[i] = the root of i.  It only reads the forest: a find that compresses could overwrite, with an ancestor it read
// earlier, the root another thread has just stored, and every pixel needs its root itself here
__global__ __launch_bounds__(VT) void k_seg_flatten(SegGeom g, const int* __restrict__ parent, int* __restrict__ root) {
  const int i = blockIdx.x * VT + threadIdx.x, k = blockIdx.y;
  if (i >= g.P) return;
  const int* par = parent + (size_t)k * g.P;
  int x = i;
  for (int p = par[x]; p != x; p = par[x]) x = p;
  root[(size_t)k * g.P + i] = x;
}

// one workgroup per keyframe: the roots among the points, ranked in raster order -> segidx[root], the sizes, the count
__global__ __launch_bounds__(VT) void k_seg_label(SegGeom g, const float4* __restrict__ pts, const int* __restrict__ parent,
                                                  const int* __restrict__ size, unsigned* __restrict__ segidx, int* __restrict__ seg_counts,
                                                  int* __restrict__ seg_sizes) {
  __shared__ unsigned lds[BLOCK_WAVES];
  const int k = blockIdx.x;
  const size_t o = (size_t)k * g.P;
  unsigned carry = 0;
  for (int base = 0; base < g.P; base += VT) {
    const int i = base + threadIdx.x;
    const bool f = i < g.P && pts[o + i].w != 0.f && parent[o + i] == i;
    unsigned tot;
    const unsigned rank = carry + block_rank(f, lds, tot);
    if (f) {
      segidx[o + i] = rank;
      if (rank < (unsigned)g.S) seg_sizes[(size_t)k * g.S + rank] = size[o + i];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) seg_counts[k] = (int)carry;
}

// grid (tiles, n): the label of every pixel; one integer add per point into its segment's histogram
__global__ __launch_bounds__(VT) void k_seg_hist(const char* const* __restrict__ blocks, SegGeom g, const float4* __restrict__ pts,
                                                 const unsigned* __restrict__ segidx, const float* __restrict__ centres, int nbins,
                                                 int* labels, int* __restrict__ hist) {
  RGBID_FP_STRICT
  __shared__ float c[3 * RGBID_SEGMENT_MAX_BINS];
  for (int j = threadIdx.x; j < 3 * nbins; j += VT) c[j] = centres[j];
  __syncthreads();
  const int i = blockIdx.x * VT + threadIdx.x, k = blockIdx.y;
  if (i >= g.P) return;
  const size_t o = (size_t)k * g.P;
  if (pts[o + i].w == 0.f) { labels[o + i] = -1; return; }
  const unsigned s = segidx[o + labels[o + i]];   // labels holds the roots (k_seg_flatten)
  labels[o + i] = (int)s;
  if (s >= (unsigned)g.S) return;
  const float* nr = reinterpret_cast<const float*>(blocks[k] + 8 * (size_t)g.P);
  const float nx = nr[i], ny = nr[g.P + i], nz = nr[2 * (size_t)g.P + i];
  float best = -1.1f;
  int bin = -1;
  for (int j = 0; j < nbins; ++j) {
    const float d = (nx * c[3 * j] + ny * c[3 * j + 1]) + nz * c[3 * j + 2];
    if (d > best) { best = d; bin = j; }
  }
  if (bin >= 0) atomicAdd(&hist[((size_t)k * g.S + s) * nbins + bin], 1);
}

// one thread per (keyframe, segment below S)
__global__ __launch_bounds__(VT) void k_seg_entropy(SegGeom g, const int* __restrict__ seg_counts, const int* __restrict__ seg_sizes,
                                                    const int* __restrict__ hist, int nbins, float* __restrict__ entropy) {
  RGBID_FP_STRICT
  const int s = blockIdx.x * VT + threadIdx.x, k = blockIdx.y;
  if (s >= g.S || s >= seg_counts[k]) return;
  const size_t o = (size_t)k * g.S + s;
  const int size = seg_sizes[o];
  const float fs = (float)size, small = 1.f / (float)(2 * size);
  float sum = 0.f;
  for (int j = 0; j < nbins; ++j) {
    const float freq = (float)hist[o * nbins + j] / fs;
    const float term = freq < small ? 0.f : -freq * logf(freq);
    sum = sum + term;
  }
  entropy[o] = sum / logf(fs);
}

// grid (tiles, n): the negentropy image and the counts c_k of the pixels below each threshold
__global__ __launch_bounds__(VT) void k_seg_image(SegGeom g, const int* __restrict__ labels, const float* __restrict__ entropy, Thresholds th,
                                                  float* __restrict__ negentropy, unsigned* __restrict__ ck) {
  RGBID_FP_STRICT
  const int i = blockIdx.x * VT + threadIdx.x, k = blockIdx.y;
  const bool here = i < g.P;
  float v = 0.f;
  if (here) {
    const int s = labels[(size_t)k * g.P + i];
    if (s >= 0) v = s < g.S ? 1.f - entropy[(size_t)k * g.S + s] : qnan();
    negentropy[(size_t)k * g.P + i] = v;
  }
  for (int j = 0; j < NTH; ++j) {
    const unsigned long long m = __ballot(here && v < th.t[j]);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&ck[k * NTH + j], (unsigned)__popcll(m));
  }
}

// one thread per (keyframe, level)
__global__ __launch_bounds__(VT) void k_seg_levels(SegGeom g, const unsigned* __restrict__ ck, int M, int* __restrict__ levels) {
  RGBID_FP_STRICT
  const int j = blockIdx.x * VT + threadIdx.x;
  if (j >= g.n * M) return;
  const int k = j / M, m = j - k * M;
  int ks = -1;
  if (m > 0) {
    const float frac = (float)m / (float)M;
    for (int i = 0; i < NTH; ++i)
      if ((float)ck[k * NTH + i] / (float)g.P < frac) ks = i;
  }
  levels[j] = ks;
}

// one thread per keypoint record
__global__ __launch_bounds__(VT) void k_seg_mask_keypoints(int rows, int cols, int n, int M, int max_kp, Thresholds th, const float* __restrict__ negentropy,
                                                           const int* __restrict__ levels, const rgbid_loopfeat_kp* __restrict__ kps,
                                                           const int* __restrict__ counts, unsigned char* __restrict__ bits) {
  const long long j = (long long)blockIdx.x * VT + threadIdx.x;
  if (j >= (long long)n * max_kp) return;
  const int k = (int)(j / max_kp), r = (int)(j - (long long)k * max_kp);
  unsigned b = 0;
  if (r < counts[k]) {
    b = 1;
    const int x = kps[j].x, y = kps[j].y;
    if (x >= 0 && x < cols && y >= 0 && y < rows) {
      const float v = negentropy[((size_t)k * rows + y) * cols + x];
      for (int m = 1; m < M; ++m) {
        const int ks = levels[k * M + m];
        if (ks < 0 || !(v < th.t[ks])) b |= 1u << m;
      }
    }
  }
  bits[j] = (unsigned char)b;
}

Thresholds thresholds() { return Thresholds{{0.f, 0.1f, 0.2f, 0.3f, 0.4f, 0.5f, 0.6f, 0.7f, 0.8f, 0.9f}}; }

}  // namespace

struct rgbid_segment {
  rgbid_ctx* ctx = nullptr;
  int rows = 0, cols = 0, P = 0, max_kf = 0, S = 0;
  unsigned window = RGBID_SEGMENT_MAX_WINDOW;
  SortWorkspace ws;                 // 4 P max_kf edge slots
  float4* pts = nullptr;            // [max_kf][P] x, y, z, 1 where the pixel is a point
  int* parent = nullptr;            // [max_kf][P]
  int* size = nullptr;              // [max_kf][P] at the roots
  float* th = nullptr;              // [max_kf][P] at the roots
  unsigned* resv = nullptr;         // [max_kf][P] reservation words of the rounds; then the segment index of every root
  float* entropy = nullptr;         // [max_kf][S]
  const char** blocks = nullptr;    // [max_kf]
  const char** blocks_host = nullptr;   // pinned
  unsigned* ecount = nullptr;       // [max_kf]
  unsigned* rounds = nullptr;       // [2][max_kf]
  unsigned* rounds_host = nullptr;  // pinned
  unsigned* ck = nullptr;           // [max_kf][NTH]
  float* centres = nullptr;         // [MAX_BINS][3]
  int centres_bins = 0;             // the table on the device
  int last_n = 0;
  bool timed = false;
  Buffers buf;
  StageTimer<7> timer;
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

template <typename K>
void launch_run(rgbid_segment* h, const SegGeom& g, float kth, int min_size, int nbins, int M, int* labels, int* seg_counts, int* seg_sizes, int* hist,
                float* negentropy, int* levels) {
  hipStream_t s = h->ctx->stream;
  SortWorkspace& w = h->ws;
  const unsigned n = (unsigned)g.n;
  const dim3 px((g.P + VT - 1) / VT, n);
  const unsigned E = 4u * (unsigned)g.P * n;
  h->mark(0);
  hipLaunchKernelGGL(k_seg_points, px, dim3(VT), 0, s, h->blocks, g, kth, h->pts, h->parent, h->size, h->th, h->resv);
  hipLaunchKernelGGL(k_seg_edges<K>, px, dim3(VT), 0, s, h->blocks, g, h->pts, reinterpret_cast<K*>(w.keys[0]), w.idx[0], h->ecount);
  h->mark(1);
  VoxGrid vg{};
  vg.sentinel = ((unsigned long long)(n - 1) << 32) | 0xffffffffull;   // the largest key: the sort walks its bits
  const SortedPairs<K> sp = w.sort<K>(s, E, vg);
  h->mark(2);
  hipLaunchKernelGGL((k_seg_unionfind<1, K>), dim3(n), dim3(VT), 0, s, sp.keys, sp.idx, h->ecount, g, h->window, kth, min_size, h->parent, h->size,
                     h->th, h->resv, h->rounds);
  h->mark(3);
  hipLaunchKernelGGL((k_seg_unionfind<2, K>), dim3(n), dim3(VT), 0, s, sp.keys, sp.idx, h->ecount, g, h->window, kth, min_size, h->parent, h->size,
                     h->th, h->resv, h->rounds + h->max_kf);
  h->mark(4);
  hipLaunchKernelGGL(k_seg_flatten, px, dim3(VT), 0, s, g, h->parent, labels);
  hipLaunchKernelGGL(k_seg_label, dim3(n), dim3(VT), 0, s, g, h->pts, h->parent, h->size, h->resv, seg_counts, seg_sizes);
  h->mark(5);
  hipLaunchKernelGGL(k_seg_hist, px, dim3(VT), 0, s, h->blocks, g, h->pts, h->resv, h->centres, nbins, labels, hist);
  hipLaunchKernelGGL(k_seg_entropy, dim3((g.S + VT - 1) / VT, n), dim3(VT), 0, s, g, seg_counts, seg_sizes, hist, nbins, h->entropy);
  hipLaunchKernelGGL(k_seg_image, px, dim3(VT), 0, s, g, labels, h->entropy, thresholds(), negentropy, h->ck);
  hipLaunchKernelGGL(k_seg_levels, dim3((n * M + VT - 1) / VT), dim3(VT), 0, s, g, h->ck, M, levels);
  h->mark(6);
}

}  // namespace

extern "C" {

int rgbid_segment_workspace_bytes(int rows, int cols, int max_keyframes, int max_segments, unsigned long long* bytes) {
  if (!bytes || !seghost::create_args_ok(rows, cols, max_keyframes, max_segments)) return RGBID_E_INVALID;
  *bytes = seghost::workspace_bytes(rows, cols, max_keyframes, max_segments);
  return RGBID_OK;
}

int rgbid_segment_bins(int nbins, float* centres) {
  if (!centres || nbins < 1 || nbins > RGBID_SEGMENT_MAX_BINS) return RGBID_E_INVALID;
  seghost::bins(nbins, centres);
  return RGBID_OK;
}

int rgbid_segment_create(rgbid_segment** out, rgbid_ctx* ctx, int rows, int cols, int max_keyframes, int max_segments) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  if (!ctx || !seghost::create_args_ok(rows, cols, max_keyframes, max_segments)) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_segment* h = new (std::nothrow) rgbid_segment;
  if (!h) return RGBID_E_NOMEM;
  h->ctx = ctx;
  h->rows = rows; h->cols = cols; h->P = rows * cols; h->max_kf = max_keyframes; h->S = max_segments;
  const size_t kf = (size_t)max_keyframes, pix = (size_t)h->P * kf;
  int r = h->ws.alloc(h->buf, 4ull * pix);
  if (!r) r = h->buf.alloc(&h->pts, sizeof(float4) * pix);
  if (!r) r = h->buf.alloc(&h->parent, sizeof(int) * pix);
  if (!r) r = h->buf.alloc(&h->size, sizeof(int) * pix);
  if (!r) r = h->buf.alloc(&h->th, sizeof(float) * pix);
  if (!r) r = h->buf.alloc(&h->resv, sizeof(unsigned) * pix);
  if (!r) r = h->buf.alloc(&h->entropy, sizeof(float) * (size_t)max_segments * kf);
  if (!r) r = h->buf.alloc(&h->blocks, sizeof(char*) * kf);
  if (!r) r = h->buf.alloc(&h->ecount, sizeof(unsigned) * kf);
  if (!r) r = h->buf.alloc(&h->rounds, sizeof(unsigned) * 2 * kf);
  if (!r) r = h->buf.alloc(&h->ck, sizeof(unsigned) * NTH * kf);
  if (!r) r = h->buf.alloc(&h->centres, sizeof(float) * 3 * RGBID_SEGMENT_MAX_BINS);
  if (!r) r = h->buf.alloc_host(&h->blocks_host, sizeof(char*) * kf);
  if (!r) r = h->buf.alloc_host(&h->rounds_host, sizeof(unsigned) * 2 * kf);
  if (r) { rgbid_segment_destroy(h); return r; }
  *out = h;
  return RGBID_OK;
}

int rgbid_segment_destroy(rgbid_segment* h) { return destroy_handle(h); }

int rgbid_segment_device_bytes(const rgbid_segment* h, unsigned long long* bytes) {
  if (!h || !bytes) return RGBID_E_INVALID;
  *bytes = h->buf.bytes();
  return RGBID_OK;
}

int rgbid_segment_set_window(rgbid_segment* h, int window) {
  if (!h || window < 1 || window > RGBID_SEGMENT_MAX_WINDOW) return RGBID_E_INVALID;
  h->window = (unsigned)window;
  return RGBID_OK;
}

int rgbid_segment_run(rgbid_segment* h, int n, const rgbid_cloud_src* src, const float K[4], float k_th, int min_size, int nbins, int levels,
                      int32_t* labels_dev, int32_t* seg_counts_dev, int32_t* seg_sizes_dev, int32_t* hist_dev, float* negentropy_dev,
                      int32_t* mask_levels_dev) {
  if (!h || !seghost::run_args_ok(n, h->max_kf, src, K, k_th, min_size, nbins, levels)) return RGBID_E_INVALID;
  if (!labels_dev || !seg_counts_dev || !seg_sizes_dev || !hist_dev || !negentropy_dev || !mask_levels_dev) return RGBID_E_INVALID;
  for (int k = 0; k < n; ++k)
    if (!src[k].block_dev || (((uintptr_t)src[k].block_dev) & 3)) return RGBID_E_INVALID;
  SegGeom g;
  if (int r = rgbid_cloud_kinv(K, g.kinv)) return r;
  g.rows = h->rows; g.cols = h->cols; g.P = h->P; g.n = n; g.S = h->S;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  RGBID_HIP(hipStreamSynchronize(s));   // the previous run has read the staged block pointers and the bin table
  for (int k = 0; k < n; ++k) h->blocks_host[k] = static_cast<const char*>(src[k].block_dev);
  RGBID_HIP(hipMemcpyAsync(h->blocks, h->blocks_host, sizeof(char*) * (size_t)n, hipMemcpyHostToDevice, s));
  if (h->centres_bins != nbins) {
    float c[3 * RGBID_SEGMENT_MAX_BINS];
    seghost::bins(nbins, c);
    RGBID_HIP(hipMemcpyAsync(h->centres, c, sizeof(float) * 3 * (size_t)nbins, hipMemcpyHostToDevice, s));
    RGBID_HIP(hipStreamSynchronize(s));   // c is pageable stack memory
    h->centres_bins = nbins;
  }
  RGBID_HIP(hipMemsetAsync(h->ecount, 0, sizeof(unsigned) * (size_t)n, s));
  RGBID_HIP(hipMemsetAsync(h->ck, 0, sizeof(unsigned) * NTH * (size_t)n, s));
  RGBID_HIP(hipMemsetAsync(seg_sizes_dev, 0, sizeof(int32_t) * (size_t)h->S * n, s));
  RGBID_HIP(hipMemsetAsync(hist_dev, 0, sizeof(int32_t) * (size_t)h->S * n * nbins, s));
  h->timed = false;
  if (n == 1) launch_run<unsigned>(h, g, k_th, min_size, nbins, levels, labels_dev, seg_counts_dev, seg_sizes_dev, hist_dev, negentropy_dev, mask_levels_dev);
  else launch_run<unsigned long long>(h, g, k_th, min_size, nbins, levels, labels_dev, seg_counts_dev, seg_sizes_dev, hist_dev, negentropy_dev, mask_levels_dev);
  RGBID_HIP(hipGetLastError());
  h->last_n = n;
  h->timed = h->timer.on;
  return RGBID_OK;
}

int rgbid_segment_mask_keypoints(rgbid_segment* h, const float* negentropy_dev, const int32_t* mask_levels_dev, int n, int levels,
                                 const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int max_keypoints, uint8_t* bits_dev) {
  if (!h || !negentropy_dev || !mask_levels_dev || !kps_dev || !counts_dev || !bits_dev) return RGBID_E_INVALID;
  if (n < 1 || levels < 1 || levels > RGBID_SEGMENT_MAX_LEVELS || max_keypoints < 1) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  const long long items = (long long)n * max_keypoints;
  hipLaunchKernelGGL(k_seg_mask_keypoints, dim3((unsigned)((items + VT - 1) / VT)), dim3(VT), 0, h->ctx->stream, h->rows, h->cols, n, levels,
                     max_keypoints, thresholds(), negentropy_dev, mask_levels_dev, kps_dev, counts_dev, bits_dev);
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_segment_last_rounds(rgbid_segment* h, unsigned long long rounds[2]) {
  if (!h || !rounds) return RGBID_E_INVALID;
  rounds[0] = rounds[1] = 0;
  if (h->last_n == 0) return RGBID_OK;
  (void)hipSetDevice(h->ctx->device);
  hipStream_t s = h->ctx->stream;
  RGBID_HIP(hipMemcpyAsync(h->rounds_host, h->rounds, sizeof(unsigned) * 2 * (size_t)h->max_kf, hipMemcpyDeviceToHost, s));
  RGBID_HIP(hipStreamSynchronize(s));
  for (int p = 0; p < 2; ++p)
    for (int k = 0; k < h->last_n; ++k)
      if (h->rounds_host[p * h->max_kf + k] > rounds[p]) rounds[p] = h->rounds_host[p * h->max_kf + k];
  return RGBID_OK;
}

int rgbid_segment_timing(rgbid_segment* h, int enable, float ms[6]) {
  if (!h) return RGBID_E_INVALID;
  (void)hipSetDevice(h->ctx->device);
  if (ms)
    for (int k = 0; k < 6; ++k) {
      ms[k] = 0.f;
      if (h->timed) RGBID_HIP(h->timer.elapsed(k, k + 1, &ms[k]));
    }
  return h->timer.enable(enable != 0);
}

}  // extern "C"
