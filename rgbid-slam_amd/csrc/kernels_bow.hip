// kernels_bow.hip -- the binary vocabulary that shortlists loop candidates (include/rgbid_bow.h; the reference ranks its database by DBoW2's
// score, src/loop_closer.cpp:183-271).  All device arithmetic is integer: votes are integer sums, every arg-max / arg-min is one integer key,
// so integer atomics and any reduction shape give the same bytes.
//
//   training   level-synchronous: every node of a level is split by the same launches.  Per slot (keyframe, slot) arrays hold the node a
//              descriptor sits in, its minimum distance to the seeds and its child; the children of a level live in `rows` (node of the
//              level x child) until the level is finished and numbered by one scan.
//              k_bow_seed_*    farthest-point seeds: one 64-bit atomicMax key (distance << 32 | ~index) per node and round
//              k_bow_assign    one thread per descriptor, 4 x 64-bit registers against the node's <= 16 row centroids
//              k_bow_vote      one thread per bit: a block walks 64 descriptors, thread t adds bit t to votes[row][t] (the 64 lanes of a
//                              wave-instruction add to 256 contiguous bytes)
//              k_bow_centroid  one block per row: majority per bit, assembled by 4 ballots
//   transform  k_bow_descend   one thread per descriptor in 4 x 64-bit registers; the first 273 nodes (root, <= 16, <= 256) are staged in LDS
//              k_bow_vector    one block per keyframe: bitonic sort of its <= 1 536 words in LDS, run heads compacted by ballots, the
//                              integer normalisation
//   score      k_bow_score     one wave per pair, binary search of the candidate's words in the query's list
//   shortlist  k_bow_shortlist one block per query, its vector in LDS; a wave streams candidates and keeps its best 64 keys
//                              (score << 32 | candidate) one per lane, sorted, inserted by a ballot and a shuffle
#include "../../include/rgbid_bow.h"
#include "common.h"
#include "hip_host.h"
#include "wave_device.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

using namespace rgbid;

static_assert(sizeof(rgbid_bow_entry) == 8, "rgbid_bow_entry is 8 bytes");
static_assert(sizeof(rgbid_loopfeat_kp) == 120 && offsetof(rgbid_loopfeat_kp, desc) == 16, "descriptor at byte 16 of a 120-byte record");

namespace {

typedef unsigned long long u64;
constexpr int BT = 256;                   // threads per block
constexpr int MAXD = RGBID_BOW_MAX_DEPTH;
constexpr int STAGED = 1 + 16 + 256;      // nodes whose centroids the descent keeps in LDS
constexpr int VCHUNK = 64;                // descriptors a vote block walks
constexpr int SORTN = 2048;               // >= RGBID_LOOPFEAT_MAX_KEYPOINTS, a power of two
constexpr int NO_CHILD = 0xFF;
static_assert(SORTN >= RGBID_LOOPFEAT_MAX_KEYPOINTS, "a keyframe's words are sorted in LDS");
static_assert((u64)RGBID_LOOPFEAT_MAX_KEYPOINTS * RGBID_BOW_MAX_WEIGHT < (1ull << 31), "a_w = c_w * W_w < 2^31: a_w << 30 stays inside 64 bits");

// what the training kernels share: the tree, the per-node, per-slot and per-row state
struct BowTrain {
  u64* cent; int2* child; int* lvls; int* n_nodes;       // tree: centroids [nodes][4], (first child, children), level starts, node count
  int *count, *nseeds, *stamp; u64* far;                 // per node: descriptors held, seeds, last pass that changed, arg-max key
  int *node_of, *mind; uint8_t* assign;                  // per slot
  u64* rowcent; int *votes, *members;                    // per row = (node - level start) * k + child
  const rgbid_loopfeat_kp* kps; const int* counts;
  int n_kf, max_kp, n_slots, k;
};

__device__ __forceinline__ void load_desc(const rgbid_loopfeat_kp* kp, u64 a[4]) {
  for (int j = 0; j < 4; ++j) a[j] = *reinterpret_cast<const u64*>(kp->desc + 8 * j);
}
__device__ __forceinline__ int ham(const u64 a[4], const u64* c) {
  return __popcll(a[0] ^ c[0]) + __popcll(a[1] ^ c[1]) + __popcll(a[2] ^ c[2]) + __popcll(a[3] ^ c[3]);
}

// atomicMax of per-lane keys on far[node]: when every active lane of the wave names the same node (the whole root level, most of the next)
// the wave reduces first and one lane goes to memory.  Called by all 64 lanes.
__device__ __forceinline__ void wave_atomic_max(u64* far, int node, bool act, u64 key) {
  const u64 m = __ballot(act);
  if (m == 0) return;
  const int first = __builtin_amdgcn_readlane(node, (int)__builtin_ctzll(m));
  if (__all(!act || node == first)) {
    u64 v = act ? key : 0ull;
    for (int o = 32; o > 0; o >>= 1) { const u64 w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    if ((threadIdx.x & 63) == 0) atomicMax(&far[first], v);
  } else if (act) {
    atomicMax(&far[node], key);
  }
}

// ---- training ----
__global__ __launch_bounds__(BT) void k_bow_node_init(BowTrain T, int max_nodes, int depth) {
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i < max_nodes) {
    for (int j = 0; j < 4; ++j) T.cent[4 * (size_t)i + j] = 0ull;
    T.child[i] = make_int2(0, 0);
    T.count[i] = 0; T.nseeds[i] = 0; T.stamp[i] = 0; T.far[i] = 0ull;
  }
  if (i == 0) {
    T.lvls[0] = 0;
    for (int d = 1; d <= MAXD + 1; ++d) T.lvls[d] = 1;
    *T.n_nodes = 1;
  }
}

// every slot: in the root or unused; the root's count
__global__ __launch_bounds__(BT) void k_bow_slot_init(BowTrain T) {
  const int i = blockIdx.x * BT + threadIdx.x;
  bool valid = false;
  if (i < T.n_slots) {
    const int kf = i / T.max_kp, slot = i - kf * T.max_kp;
    valid = slot < min(max(T.counts[kf], 0), T.max_kp);
    T.node_of[i] = valid ? 0 : -1;
    T.mind[i] = 0;
    T.assign[i] = NO_CHILD;
  }
  const u64 m = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&T.count[0], (int)__popcll(m));
}

// the node of slot i when it is being split at level d, else -1
__device__ __forceinline__ int split_node(const BowTrain& T, int i, int start) {
  if (i >= T.n_slots) return -1;
  const int node = T.node_of[i];
  return (node >= start && T.count[node] >= 2) ? node : -1;
}

__global__ __launch_bounds__(BT) void k_bow_seed_first(BowTrain T, int d) {
  const int i = blockIdx.x * BT + threadIdx.x;
  const int node = split_node(T, i, T.lvls[d]);
  // the lowest slot as the largest key: one path for both arg-extrema
  wave_atomic_max(T.far, max(node, 0), node >= 0, (u64)(0xFFFFFFFFu - (unsigned)i));
}

// round r of the seeding, one thread per node of the level: the slot the last round's key names becomes seed r
__global__ __launch_bounds__(BT) void k_bow_seed_set(BowTrain T, int d, int r) {
  const int start = T.lvls[d], end = T.lvls[d + 1];
  const int node = start + blockIdx.x * BT + threadIdx.x;
  if (node >= end || T.count[node] < 2 || T.nseeds[node] != r) return;
  const u64 key = T.far[node];
  T.far[node] = 0ull;
  if (r > 0 && (key >> 32) == 0) return;   // every descriptor equals a seed
  const unsigned slot = 0xFFFFFFFFu - (unsigned)key;
  if (slot >= (unsigned)T.n_slots) return;
  u64 a[4];
  load_desc(T.kps + slot, a);
  u64* c = T.rowcent + 4 * ((size_t)(node - start) * T.k + r);
  for (int j = 0; j < 4; ++j) c[j] = a[j];
  T.nseeds[node] = r + 1;
}

__global__ __launch_bounds__(BT) void k_bow_seed_dist(BowTrain T, int d, int r) {
  const int i = blockIdx.x * BT + threadIdx.x;
  const int start = T.lvls[d];
  const int node = split_node(T, i, start);
  const bool act = node >= 0 && T.nseeds[node] == r + 1;
  u64 key = 0ull;
  if (act) {
    u64 a[4];
    load_desc(T.kps + i, a);
    const int dd = ham(a, T.rowcent + 4 * ((size_t)(node - start) * T.k + r));
    const int m = r == 0 ? dd : min(T.mind[i], dd);
    T.mind[i] = m;
    key = ((u64)(unsigned)m << 32) | (u64)(0xFFFFFFFFu - (unsigned)i);
  }
  wave_atomic_max(T.far, max(node, 0), act, key);
}

// a node of the level takes part in pass p of its Lloyd iteration when it has children and its assignment changed in pass p - 1
__device__ __forceinline__ bool lloyd_active(const BowTrain& T, int node, int p) {
  return node >= 0 && T.nseeds[node] >= 2 && T.stamp[node] >= p - 1;
}

__global__ __launch_bounds__(BT) void k_bow_assign(BowTrain T, int d, int p) {
  const int i = blockIdx.x * BT + threadIdx.x;
  const int start = T.lvls[d];
  const int node = split_node(T, i, start);
  if (!lloyd_active(T, node, p)) return;
  u64 a[4];
  load_desc(T.kps + i, a);
  const u64* c = T.rowcent + 4 * (size_t)(node - start) * T.k;
  const int s = T.nseeds[node];
  int best = 0, bd = 1 << 20;
  for (int j = 0; j < s; ++j) {
    const int dd = ham(a, c + 4 * j);
    if (dd < bd) { bd = dd; best = j; }   // strict: the lower child stays in front on a tie
  }
  if (best != (int)T.assign[i]) {
    T.assign[i] = (uint8_t)best;
    if (p > 0) atomicMax(&T.stamp[node], p);
  }
}

__global__ __launch_bounds__(BT) void k_bow_vote(BowTrain T, int d, int p) {
  const int start = T.lvls[d];
  const int t = threadIdx.x;
  const int base = blockIdx.x * VCHUNK;
  for (int j = 0; j < VCHUNK; ++j) {
    const int i = base + j;   // uniform over the block
    const int node = split_node(T, i, start);
    if (!lloyd_active(T, node, p)) continue;
    const size_t row = (size_t)(node - start) * T.k + T.assign[i];
    const unsigned w = reinterpret_cast<const unsigned*>(T.kps[i].desc)[t >> 5];
    if ((w >> (t & 31)) & 1u) atomicAdd(&T.votes[row * 256 + t], 1);
    if (t == 0) atomicAdd(&T.members[row], 1);
  }
}

__global__ __launch_bounds__(BT) void k_bow_centroid(BowTrain T, int d, int p) {
  const int start = T.lvls[d], end = T.lvls[d + 1];
  const size_t row = blockIdx.x;
  const int node = start + (int)(row / T.k), c = (int)(row % T.k);
  if (node >= end || T.count[node] < 2 || c >= T.nseeds[node] || !lloyd_active(T, node, p)) return;   // uniform over the block
  const int t = threadIdx.x;
  const int m = T.members[row];
  const int v = T.votes[row * 256 + t];
  T.votes[row * 256 + t] = 0;
  const u64 bits = __ballot(2 * v > m);
  if (m > 0 && (t & 63) == 0) T.rowcent[4 * row + (t >> 6)] = bits;
  __syncthreads();
  if (t == 0) T.members[row] = 0;
}

// number the children of the level: one block, a thread sums the seeds of a contiguous run of nodes
__global__ __launch_bounds__(BT) void k_bow_finish_scan(BowTrain T, int d, int depth) {
  __shared__ int part[BT];
  const int start = T.lvls[d], end = T.lvls[d + 1];
  const int N = end - start, per = (N + BT - 1) / BT;
  const int lo = start + threadIdx.x * per, hi = min(lo + per, end);
  int sum = 0;
  for (int n = lo; n < hi; ++n) sum += (T.count[n] >= 2 && T.nseeds[n] >= 2) ? T.nseeds[n] : 0;
  part[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int j = 0; j < BT; ++j) { const int s = part[j]; part[j] = run; run += s; }
    T.lvls[d + 2] = end + run;
    if (d == depth - 1) *T.n_nodes = end + run;
  }
  __syncthreads();
  int off = end + part[threadIdx.x];
  for (int n = lo; n < hi; ++n) {
    const int s = (T.count[n] >= 2 && T.nseeds[n] >= 2) ? T.nseeds[n] : 0;
    T.child[n] = s ? make_int2(off, s) : make_int2(0, 0);
    off += s;
  }
}

__global__ __launch_bounds__(BT) void k_bow_finish_rows(BowTrain T, int d, int max_nodes) {
  const int start = T.lvls[d], end = T.lvls[d + 1];
  const size_t row = (size_t)blockIdx.x * BT + threadIdx.x;
  const size_t n = row / T.k;
  if (n >= (size_t)(end - start)) return;
  const int node = start + (int)n, c = (int)(row % T.k);
  const int2 ch = T.child[node];
  if (c >= ch.y) return;
  const int nn = ch.x + c;
  if (nn >= max_nodes) return;
  for (int j = 0; j < 4; ++j) T.cent[4 * (size_t)nn + j] = T.rowcent[4 * row + j];
}

__global__ __launch_bounds__(BT) void k_bow_finish_assign(BowTrain T, int d, int max_nodes) {
  const int i = blockIdx.x * BT + threadIdx.x;
  const int node = split_node(T, i, T.lvls[d]);
  if (node < 0) return;
  const int2 ch = T.child[node];
  const int a = T.assign[i];
  T.assign[i] = NO_CHILD;
  if (a >= ch.y) return;   // the node stayed a leaf
  const int nn = ch.x + a;
  if (nn >= max_nodes) return;
  T.node_of[i] = nn;
  atomicAdd(&T.count[nn], 1);
}

// ---- transform ----
__global__ __launch_bounds__(BT) void k_bow_descend(const u64* __restrict__ cent, const int2* __restrict__ child, const int* __restrict__ n_nodes,
                                                    const rgbid_loopfeat_kp* __restrict__ kps, const int* __restrict__ counts, int n_slots, int max_kp,
                                                    int* __restrict__ words) {
  __shared__ u64 top[STAGED * 4];
  const int nodes = *n_nodes, staged = min(nodes, STAGED);
  for (int j = threadIdx.x; j < staged * 4; j += BT) top[j] = cent[j];
  __syncthreads();
  const int i = blockIdx.x * BT + threadIdx.x;
  if (i >= n_slots) return;
  const int kf = i / max_kp, slot = i - kf * max_kp;
  if (slot >= min(max(counts[kf], 0), max_kp)) { words[i] = -1; return; }
  u64 a[4];
  load_desc(kps + i, a);
  int node = 0;
  for (int l = 0; l < MAXD; ++l) {
    const int2 ch = child[node];
    if (ch.y <= 0 || ch.x <= node || ch.x + ch.y > nodes) break;
    int best = 0, bd = 1 << 20;
    for (int c = 0; c < ch.y; ++c) {
      const int n = ch.x + c;
      const int dd = n < staged ? ham(a, top + 4 * n) : ham(a, cent + 4 * (size_t)n);
      if (dd < bd) { bd = dd; best = c; }
    }
    node = ch.x + best;
  }
  words[i] = node;
}

// the words of one keyframe into w[0 .. P), ascending, P = the power of two >= max(cnt, 2); unused places hold INT_MAX
__device__ __forceinline__ void sort_words(int* w, const int* __restrict__ words, int cnt) {
  int P = 2;
  while (P < cnt) P <<= 1;
  for (int i = threadIdx.x; i < P; i += BT) w[i] = i < cnt ? words[i] : 0x7FFFFFFF;
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += BT) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const int x = w[i], y = w[l];
        if ((x > y) == ((i & k2) == 0)) { w[i] = y; w[l] = x; }
      }
      __syncthreads();
    }
}

// the places where a run of equal words starts, compacted in order into hp[0 .. ne), hp[ne] = cnt; returns ne (uniform)
__device__ __forceinline__ int run_heads(const int* w, int cnt, int* hp, unsigned* wtot) {
  unsigned running = 0;
  for (int base = 0; base < cnt; base += BT) {
    const int i = base + threadIdx.x;
    const bool head = i < cnt && (i == 0 || w[i] != w[i - 1]);
    unsigned tot;
    const unsigned pos = running + block_rank(head, wtot, tot);
    if (head) hp[pos] = i;   // pos < cnt
    running += tot;
  }
  if (threadIdx.x == 0) hp[running] = cnt;
  __syncthreads();
  return (int)running;
}

// keyframes that hold each word
__global__ __launch_bounds__(BT) void k_bow_df(const int* __restrict__ words, const int* __restrict__ counts, int max_kp, int nodes_cap,
                                               unsigned* __restrict__ df) {
  __shared__ int w[SORTN];
  const int kf = blockIdx.x, cnt = min(max(counts[kf], 0), max_kp);
  if (cnt == 0) return;
  sort_words(w, words + (size_t)kf * max_kp, cnt);
  for (int i = threadIdx.x; i < cnt; i += BT)
    if ((i == 0 || w[i] != w[i - 1]) && w[i] >= 0 && w[i] < nodes_cap) atomicAdd(&df[w[i]], 1u);
}

__global__ __launch_bounds__(BT) void k_bow_vector(const int* __restrict__ words, const int* __restrict__ counts, int max_kp, int nodes_cap,
                                                   const unsigned* __restrict__ weight, rgbid_bow_entry* __restrict__ bow, int* __restrict__ bow_counts) {
  __shared__ int w[SORTN];
  __shared__ int hp[RGBID_LOOPFEAT_MAX_KEYPOINTS + 1];
  __shared__ unsigned wtot[BT / 64];
  __shared__ u64 wsum[BT / 64];
  const int kf = blockIdx.x, cnt = min(max(counts[kf], 0), max_kp);
  rgbid_bow_entry* out = bow + (size_t)kf * max_kp;
  int ne = 0;
  u64 A = 0ull;
  if (cnt > 0) {   // uniform over the block
    sort_words(w, words + (size_t)kf * max_kp, cnt);
    ne = run_heads(w, cnt, hp, wtot);
    u64 part = 0ull;
    for (int e = threadIdx.x; e < ne; e += BT) {
      const int i = hp[e], word = w[i];
      part += (u64)(unsigned)(hp[e + 1] - i) * (u64)((word >= 0 && word < nodes_cap) ? weight[word] : 0u);
    }
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = part;
    __syncthreads();
    A = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    if (A == 0ull) ne = 0;
  }
  for (int e = threadIdx.x; e < max_kp; e += BT) {
    rgbid_bow_entry o{0u, 0u};
    if (e < ne) {
      const int i = hp[e], word = w[i];
      const u64 a = (u64)(unsigned)(hp[e + 1] - i) * (u64)((word >= 0 && word < nodes_cap) ? weight[word] : 0u);
      o.word = (unsigned)word;
      o.value = (unsigned)((a << 30) / A);   // a < 2^31: the shift stays inside 64 bits
    }
    out[e] = o;
  }
  if (threadIdx.x == 0) bow_counts[kf] = ne;
}

// ---- score ----
// sum of min(v) over the words of list c that list q holds too (q by word and value arrays, sorted by word); the wave's total in every lane
template <class QW, class QV>
__device__ __forceinline__ u64 wave_score(QW qw, QV qv, int nq, const rgbid_bow_entry* __restrict__ cl, int nc, int lane) {
  u64 s = 0ull;
  for (int e = lane; e < nc; e += 64) {
    const rgbid_bow_entry ce = cl[e];
    int lo = 0, hi = nq;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (qw(mid) < ce.word) lo = mid + 1; else hi = mid;
    }
    if (lo < nq && qw(lo) == ce.word) s += (u64)min(qv(lo), ce.value);
  }
  return wave_sum(s);
}

__global__ __launch_bounds__(BT) void k_bow_score(const rgbid_bow_entry* __restrict__ bow, const int* __restrict__ bow_counts, int n_kf, int max_kp,
                                                  const int* __restrict__ pairs, int n_pairs, u64* __restrict__ scores) {
  const int lane = threadIdx.x & 63, pair = blockIdx.x * (BT / 64) + (threadIdx.x >> 6);
  if (pair >= n_pairs) return;   // uniform over the wave
  const int q = pairs[2 * pair], c = pairs[2 * pair + 1];
  u64 s = 0ull;
  if (q >= 0 && q < n_kf && c >= 0 && c < n_kf) {
    const rgbid_bow_entry* ql = bow + (size_t)q * max_kp;
    const int nq = min(max(bow_counts[q], 0), max_kp), nc = min(max(bow_counts[c], 0), max_kp);
    s = wave_score([ql](int i) { return ql[i].word; }, [ql](int i) { return ql[i].value; }, nq, bow + (size_t)c * max_kp, nc, lane);
  }
  if (lane == 0) scores[pair] = s;
}

// ---- shortlist ----
__global__ __launch_bounds__(BT) void k_bow_shortlist(const rgbid_bow_entry* __restrict__ bow, const int* __restrict__ bow_counts, int n_kf, int max_kp,
                                                      int min_sep, int T, int* __restrict__ cand, u64* __restrict__ cand_scores) {
  __shared__ unsigned qw[RGBID_LOOPFEAT_MAX_KEYPOINTS], qv[RGBID_LOOPFEAT_MAX_KEYPOINTS];
  __shared__ u64 keys[BT];
  const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nq = min(max(bow_counts[q], 0), max_kp);
  const int ncand = nq > 0 ? q - min_sep + 1 : 0;
  for (int i = threadIdx.x; i < nq; i += BT) {
    const rgbid_bow_entry e = bow[(size_t)q * max_kp + i];
    qw[i] = e.word; qv[i] = e.value;
  }
  __syncthreads();
  u64 mine = 0ull;   // the wave's keys, descending over its lanes
  for (int c = wave; c < ncand; c += BT / 64) {
    const int nc = min(max(bow_counts[c], 0), max_kp);
    const unsigned *pw = qw, *pv = qv;
    const u64 s = wave_score([pw](int i) { return pw[i]; }, [pv](int i) { return pv[i]; }, nq, bow + (size_t)c * max_kp, nc, lane);
    if (s == 0ull) continue;   // uniform over the wave
    const u64 x = (s << 32) | (u64)(unsigned)c;   // s <= 2^30
    const int pos = (int)__popcll(__ballot(mine > x));
    const u64 up = __shfl_up(mine, 1, 64);
    mine = lane < pos ? mine : (lane == pos ? x : up);
  }
  keys[threadIdx.x] = mine;
  __syncthreads();
  int rank = 0, valid = 0;
  for (int j = 0; j < BT; ++j) {
    const u64 o = keys[j];
    rank += o > mine;
    valid += o != 0ull;
  }
  if (mine != 0ull && rank < T) {
    cand[(size_t)q * T + rank] = (int)(unsigned)(mine & 0xFFFFFFFFull);
    cand_scores[(size_t)q * T + rank] = mine >> 32;
  }
  if ((int)threadIdx.x < T && (int)threadIdx.x >= valid) {
    cand[(size_t)q * T + threadIdx.x] = -1;
    cand_scores[(size_t)q * T + threadIdx.x] = 0ull;
  }
}

long long ipow(int k, int e) {
  long long p = 1;
  for (int i = 0; i < e; ++i) p *= k;
  return p;
}

}  // namespace

struct rgbid_bow {
  rgbid_ctx* ctx = nullptr;
  int k = 0, depth = 0, max_nodes = 0;
  u64* cent = nullptr; int2* child = nullptr; unsigned* weight = nullptr; unsigned* df = nullptr;
  int *lvls = nullptr, *n_nodes = nullptr;
  BowTrain T{};                 // training scratch for cap_train slots
  int cap_train = 0;
  int* words = nullptr;         // a word per slot, for cap_run slots
  int cap_run = 0;
  Buffers tree, train, run;
  StageTimer<8> timer;          // 0-1 train, 2-3 transform, 4-5 score, 6-7 shortlist
  bool timed[4] = {false, false, false, false};
  void mark(int i) { timer.mark(i, ctx->stream); }
};

namespace {

bool bow_limits(int k, int depth) {
  return k >= 2 && k <= RGBID_BOW_MAX_K && depth >= 1 && depth <= RGBID_BOW_MAX_DEPTH && ipow(k, depth) <= RGBID_BOW_MAX_LEAVES;
}

bool bow_batch_ok(int n_kf, int max_kp) {
  return n_kf >= 0 && n_kf <= 65535 && max_kp >= 1 && max_kp <= RGBID_LOOPFEAT_MAX_KEYPOINTS;
}

// nodes a level at depth d can hold when the batch has n_slots descriptors
long long level_nodes(const rgbid_bow* v, int d, long long n_slots) { return std::min(ipow(v->k, d), std::max(n_slots, 1ll)); }

int bow_reserve_run(rgbid_bow* v, int n_slots) {
  if (n_slots <= v->cap_run) return RGBID_OK;
  RGBID_HIP(hipStreamSynchronize(v->ctx->stream));
  v->run.release();
  v->words = nullptr; v->cap_run = 0;
  if (int r = v->run.alloc(&v->words, sizeof(int) * (size_t)n_slots)) return r;
  v->cap_run = n_slots;
  return RGBID_OK;
}

int bow_reserve_train(rgbid_bow* v, int n_slots) {
  if (n_slots <= v->cap_train) return RGBID_OK;
  RGBID_HIP(hipStreamSynchronize(v->ctx->stream));
  v->train.release();
  v->cap_train = 0;
  BowTrain& T = v->T;
  const size_t nodes = (size_t)v->max_nodes, rows = (size_t)(v->k * level_nodes(v, v->depth - 1, n_slots));
  int r = v->train.alloc(&T.count, sizeof(int) * nodes);
  if (!r) r = v->train.alloc(&T.nseeds, sizeof(int) * nodes);
  if (!r) r = v->train.alloc(&T.stamp, sizeof(int) * nodes);
  if (!r) r = v->train.alloc(&T.far, sizeof(u64) * nodes);
  if (!r) r = v->train.alloc(&T.node_of, sizeof(int) * (size_t)n_slots);
  if (!r) r = v->train.alloc(&T.mind, sizeof(int) * (size_t)n_slots);
  if (!r) r = v->train.alloc(&T.assign, (size_t)n_slots);
  if (!r) r = v->train.alloc(&T.rowcent, sizeof(u64) * 4 * rows);
  if (!r) r = v->train.alloc(&T.votes, sizeof(int) * 256 * rows);
  if (!r) r = v->train.alloc(&T.members, sizeof(int) * rows);
  if (!r) r = hip_status(hipMemsetAsync(T.votes, 0, sizeof(int) * 256 * rows, v->ctx->stream));
  if (!r) r = hip_status(hipMemsetAsync(T.members, 0, sizeof(int) * rows, v->ctx->stream));
  if (r) { v->train.release(); return r; }
  v->cap_train = n_slots;
  return RGBID_OK;
}

inline int blocks(long long n) { return (int)((n + BT - 1) / BT); }

void bow_descend(rgbid_bow* v, const rgbid_loopfeat_kp* kps, const int32_t* counts, int n_slots, int max_kp, int* words) {
  hipLaunchKernelGGL(k_bow_descend, dim3(blocks(n_slots)), dim3(BT), 0, v->ctx->stream, v->cent, v->child, v->n_nodes, kps, counts, n_slots, max_kp,
                     words);
}

}  // namespace

extern "C" {

int rgbid_bow_max_nodes(int k, int depth, int32_t* nodes) {
  if (!nodes || !bow_limits(k, depth)) return RGBID_E_INVALID;
  long long s = 0;
  for (int l = 0; l <= depth; ++l) s += ipow(k, l);
  *nodes = (int32_t)s;
  return RGBID_OK;
}

int rgbid_bow_create(rgbid_bow** out, rgbid_ctx* ctx, int k, int depth) {
  if (!out) return RGBID_E_INVALID;
  *out = nullptr;
  int32_t nodes = 0;
  if (!ctx || rgbid_bow_max_nodes(k, depth, &nodes)) return RGBID_E_INVALID;
  (void)hipSetDevice(ctx->device);
  rgbid_bow* v = new (std::nothrow) rgbid_bow;
  if (!v) return RGBID_E_NOMEM;
  v->ctx = ctx; v->k = k; v->depth = depth; v->max_nodes = nodes;
  int r = v->tree.alloc(&v->cent, sizeof(u64) * 4 * (size_t)nodes);
  if (!r) r = v->tree.alloc(&v->child, sizeof(int2) * (size_t)nodes);
  if (!r) r = v->tree.alloc(&v->weight, sizeof(unsigned) * (size_t)nodes);
  if (!r) r = v->tree.alloc(&v->df, sizeof(unsigned) * (size_t)nodes);
  if (!r) r = v->tree.alloc(&v->lvls, sizeof(int) * (MAXD + 2));
  if (!r) r = v->tree.alloc(&v->n_nodes, sizeof(int));
  if (!r) {   // the root alone
    const int one = 1;
    hipError_t e = hipMemset(v->cent, 0, sizeof(u64) * 4 * (size_t)nodes);
    if (e == hipSuccess) e = hipMemset(v->child, 0, sizeof(int2) * (size_t)nodes);
    if (e == hipSuccess) e = hipMemset(v->weight, 0, sizeof(unsigned) * (size_t)nodes);
    if (e == hipSuccess) e = hipMemcpy(v->n_nodes, &one, sizeof(int), hipMemcpyHostToDevice);
    r = hip_status(e);
  }
  if (r) { rgbid_bow_destroy(v); return r; }
  *out = v;
  return RGBID_OK;
}

int rgbid_bow_destroy(rgbid_bow* v) { return destroy_handle(v); }

int rgbid_bow_set_weights(rgbid_bow* v, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, int max_keypoints) {
  if (!v || !bow_batch_ok(n_kf, max_keypoints)) return RGBID_E_INVALID;
  if (n_kf > 0 && (!kps_dev || !counts_dev || (((uintptr_t)kps_dev) & 7))) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  const size_t nodes = (size_t)v->max_nodes;
  RGBID_HIP(hipMemsetAsync(v->df, 0, sizeof(unsigned) * nodes, s));
  if (n_kf > 0) {
    const int n_slots = n_kf * max_keypoints;
    if (int r = bow_reserve_run(v, n_slots)) return r;
    bow_descend(v, kps_dev, counts_dev, n_slots, max_keypoints, v->words);
    hipLaunchKernelGGL(k_bow_df, dim3(n_kf), dim3(BT), 0, s, v->words, counts_dev, max_keypoints, v->max_nodes, v->df);
    RGBID_HIP(hipGetLastError());
  }
  std::vector<unsigned> h;
  try { h.resize(nodes); } catch (...) { return RGBID_E_NOMEM; }
  RGBID_HIP(hipMemcpyAsync(h.data(), v->df, sizeof(unsigned) * nodes, hipMemcpyDeviceToHost, s));
  RGBID_HIP(hipStreamSynchronize(s));
  for (size_t w = 0; w < nodes; ++w) {
    const unsigned nw = h[w];
    h[w] = (nw == 0 || nw >= (unsigned)n_kf) ? 0u : (unsigned)std::floor(std::log((double)n_kf / (double)nw) * 65536.0 + 0.5);
  }
  RGBID_HIP(hipMemcpy(v->weight, h.data(), sizeof(unsigned) * nodes, hipMemcpyHostToDevice));
  return RGBID_OK;
}

int rgbid_bow_train(rgbid_bow* v, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, int max_keypoints, int iters) {
  if (!v || !bow_batch_ok(n_kf, max_keypoints) || iters < 1 || iters > RGBID_BOW_MAX_ITERS) return RGBID_E_INVALID;
  if (n_kf > 0 && (!kps_dev || !counts_dev || (((uintptr_t)kps_dev) & 7))) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  const int n_slots = n_kf * max_keypoints;
  if (int r = bow_reserve_train(v, std::max(n_slots, 1))) return r;
  BowTrain T = v->T;
  T.cent = v->cent; T.child = v->child; T.lvls = v->lvls; T.n_nodes = v->n_nodes;
  T.kps = kps_dev; T.counts = counts_dev; T.n_kf = n_kf; T.max_kp = max_keypoints; T.n_slots = n_slots; T.k = v->k;
  v->timed[0] = false;
  v->mark(0);
  hipLaunchKernelGGL(k_bow_node_init, dim3(blocks(v->max_nodes)), dim3(BT), 0, s, T, v->max_nodes, v->depth);
  if (n_slots > 0) {
    const dim3 gs(blocks(n_slots)), b(BT);
    hipLaunchKernelGGL(k_bow_slot_init, gs, b, 0, s, T);
    for (int d = 0; d < v->depth; ++d) {
      const long long ln = level_nodes(v, d, n_slots), rows = ln * v->k;
      const dim3 gn(blocks(ln));
      hipLaunchKernelGGL(k_bow_seed_first, gs, b, 0, s, T, d);
      for (int r = 0; r < v->k; ++r) {
        hipLaunchKernelGGL(k_bow_seed_set, gn, b, 0, s, T, d, r);
        if (r + 1 < v->k) hipLaunchKernelGGL(k_bow_seed_dist, gs, b, 0, s, T, d, r);
      }
      hipLaunchKernelGGL(k_bow_assign, gs, b, 0, s, T, d, 0);
      for (int p = 1; p <= iters; ++p) {
        hipLaunchKernelGGL(k_bow_vote, dim3((n_slots + VCHUNK - 1) / VCHUNK), b, 0, s, T, d, p);
        hipLaunchKernelGGL(k_bow_centroid, dim3((unsigned)rows), b, 0, s, T, d, p);
        hipLaunchKernelGGL(k_bow_assign, gs, b, 0, s, T, d, p);
      }
      hipLaunchKernelGGL(k_bow_finish_scan, dim3(1), b, 0, s, T, d, v->depth);
      hipLaunchKernelGGL(k_bow_finish_rows, dim3(blocks(rows)), b, 0, s, T, d, v->max_nodes);
      hipLaunchKernelGGL(k_bow_finish_assign, gs, b, 0, s, T, d, v->max_nodes);
    }
  }
  v->mark(1);
  v->timed[0] = v->timer.on;
  RGBID_HIP(hipGetLastError());
  return rgbid_bow_set_weights(v, kps_dev, counts_dev, n_kf, max_keypoints);
}

int rgbid_bow_export(rgbid_bow* v, int32_t* nodes, uint8_t* centroids, int32_t* children, uint32_t* weights) {
  if (!v) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  RGBID_HIP(hipStreamSynchronize(v->ctx->stream));
  int n = 0;
  RGBID_HIP(hipMemcpy(&n, v->n_nodes, sizeof(int), hipMemcpyDeviceToHost));
  if (n < 1 || n > v->max_nodes) return RGBID_E_INVALID;
  if (nodes) *nodes = n;
  if (centroids) RGBID_HIP(hipMemcpy(centroids, v->cent, 32 * (size_t)n, hipMemcpyDeviceToHost));
  if (children) RGBID_HIP(hipMemcpy(children, v->child, sizeof(int2) * (size_t)n, hipMemcpyDeviceToHost));
  if (weights) RGBID_HIP(hipMemcpy(weights, v->weight, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToHost));
  return RGBID_OK;
}

int rgbid_bow_import(rgbid_bow* v, int32_t nodes, const uint8_t* centroids, const int32_t* children, const uint32_t* weights) {
  if (!v || nodes < 1 || nodes > v->max_nodes || !centroids || !children || !weights) return RGBID_E_INVALID;
  // the numbering of the contract: children follow each other level by level, every parent before its children, no node deeper than depth
  std::vector<int> dep;
  try { dep.assign((size_t)nodes, 0); } catch (...) { return RGBID_E_NOMEM; }
  int next = 1;
  for (int i = 0; i < nodes; ++i) {
    const int first = children[2 * i], cnt = children[2 * i + 1];
    if (cnt == 0) { if (first != 0) return RGBID_E_INVALID; continue; }
    if (cnt < 2 || cnt > v->k || first != next || first <= i || dep[i] >= v->depth || cnt > nodes - next) return RGBID_E_INVALID;
    for (int c = 0; c < cnt; ++c) dep[first + c] = dep[i] + 1;
    next += cnt;
  }
  if (next != nodes) return RGBID_E_INVALID;
  // the transform's a_w = c_w * W_w stays below 2^31 (and a_w << 30 inside 64 bits) only for weights training can produce
  for (int i = 0; i < nodes; ++i)
    if (weights[i] > RGBID_BOW_MAX_WEIGHT) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  RGBID_HIP(hipStreamSynchronize(v->ctx->stream));
  RGBID_HIP(hipMemcpy(v->cent, centroids, 32 * (size_t)nodes, hipMemcpyHostToDevice));
  RGBID_HIP(hipMemcpy(v->child, children, sizeof(int2) * (size_t)nodes, hipMemcpyHostToDevice));
  RGBID_HIP(hipMemset(v->weight, 0, sizeof(unsigned) * (size_t)v->max_nodes));
  RGBID_HIP(hipMemcpy(v->weight, weights, sizeof(unsigned) * (size_t)nodes, hipMemcpyHostToDevice));
  const int n = nodes;
  RGBID_HIP(hipMemcpy(v->n_nodes, &n, sizeof(int), hipMemcpyHostToDevice));
  return RGBID_OK;
}

int rgbid_bow_transform(rgbid_bow* v, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, int max_keypoints,
                        int32_t* words_dev, rgbid_bow_entry* bow_dev, int32_t* bow_counts_dev) {
  if (!v || !bow_batch_ok(n_kf, max_keypoints)) return RGBID_E_INVALID;
  if (n_kf == 0) return RGBID_OK;
  if (!kps_dev || !counts_dev || !bow_dev || !bow_counts_dev || (((uintptr_t)kps_dev) & 7) || (((uintptr_t)bow_dev) & 7) ||
      (((uintptr_t)words_dev) & 3))
    return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  const int n_slots = n_kf * max_keypoints;
  int* words = words_dev;
  if (!words) {
    if (int r = bow_reserve_run(v, n_slots)) return r;
    words = v->words;
  }
  v->timed[1] = false;
  v->mark(2);
  bow_descend(v, kps_dev, counts_dev, n_slots, max_keypoints, words);
  hipLaunchKernelGGL(k_bow_vector, dim3(n_kf), dim3(BT), 0, s, words, counts_dev, max_keypoints, v->max_nodes, v->weight, bow_dev, bow_counts_dev);
  v->mark(3);
  v->timed[1] = v->timer.on;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_bow_score(rgbid_bow* v, const rgbid_bow_entry* bow_dev, const int32_t* bow_counts_dev, int n_kf, int max_keypoints,
                    const int32_t* pairs_dev, int n_pairs, uint64_t* scores_dev) {
  if (!v || !bow_batch_ok(n_kf, max_keypoints) || n_pairs < 0) return RGBID_E_INVALID;
  if (n_pairs == 0) return RGBID_OK;
  if (!pairs_dev || !scores_dev || (((uintptr_t)scores_dev) & 7) || (n_kf > 0 && (!bow_dev || !bow_counts_dev || (((uintptr_t)bow_dev) & 7))))
    return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  v->timed[2] = false;
  v->mark(4);
  hipLaunchKernelGGL(k_bow_score, dim3((n_pairs + BT / 64 - 1) / (BT / 64)), dim3(BT), 0, s, bow_dev, bow_counts_dev, n_kf, max_keypoints, pairs_dev,
                     n_pairs, (u64*)scores_dev);
  v->mark(5);
  v->timed[2] = v->timer.on;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_bow_shortlist(rgbid_bow* v, const rgbid_bow_entry* bow_dev, const int32_t* bow_counts_dev, int n_kf, int max_keypoints,
                        int min_separation, int T, int32_t* cand_dev, uint64_t* cand_scores_dev) {
  if (!v || !bow_batch_ok(n_kf, max_keypoints) || min_separation < 1 || T < 1 || T > RGBID_BOW_MAX_SHORTLIST) return RGBID_E_INVALID;
  if (n_kf == 0) return RGBID_OK;
  if (!bow_dev || !bow_counts_dev || !cand_dev || !cand_scores_dev || (((uintptr_t)bow_dev) & 7) || (((uintptr_t)cand_scores_dev) & 7))
    return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  hipStream_t s = v->ctx->stream;
  v->timed[3] = false;
  v->mark(6);
  hipLaunchKernelGGL(k_bow_shortlist, dim3(n_kf), dim3(BT), 0, s, bow_dev, bow_counts_dev, n_kf, max_keypoints, min_separation, T, cand_dev,
                     (u64*)cand_scores_dev);
  v->mark(7);
  v->timed[3] = v->timer.on;
  RGBID_HIP(hipGetLastError());
  return RGBID_OK;
}

int rgbid_bow_timing(rgbid_bow* v, int enable, float ms[4]) {
  if (!v) return RGBID_E_INVALID;
  (void)hipSetDevice(v->ctx->device);
  if (ms)
    for (int i = 0; i < 4; ++i) {
      ms[i] = 0.f;
      if (v->timed[i]) {
        RGBID_HIP(hipEventSynchronize(v->timer.ev[2 * i + 1]));
        RGBID_HIP(v->timer.elapsed(2 * i, 2 * i + 1, &ms[i]));
      }
    }
  return v->timer.enable(enable != 0);
}

}  // extern "C"
