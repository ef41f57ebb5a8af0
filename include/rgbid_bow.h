/*
 * rgbid_bow.h -- C-ABI of the binary vocabulary that shortlists loop candidates before the descriptors are matched (the reference ranks its
 * database by DBoW2's bag-of-words score, LoopCloser::detectLoopClosures, src/loop_closer.cpp:183-271, TemplatedVocabulary::transform / score;
 * here the vocabulary is a k-majority tree over this project's own 256-bit descriptors, rgbid_loopfeat_kp::desc).  Every call is batched over
 * keyframes or pairs and works on the context's stream; all device arithmetic is integer and independent of the order of its reductions,
 * so every result is bitwise the same from run to run and independent of the batch a keyframe is computed in.  No library sort and no
 * floating-point atomics.
 *
 * Contract (tests/bow_mirror.py restates it in numpy).
 *  vocabulary  a tree of branching factor k (2 .. 16) and depth L (1 .. 6), k^L <= 2^20.  Node 0 is the root (depth 0, centroid zero).
 *              Nodes are numbered level by level; within a level by their parent's number, then by child index.  A node has 0 children
 *              (a leaf) or 2 .. k consecutive ones.  Every node holds a 32-byte centroid (bit t = byte t / 8, bit t % 8, as the
 *              descriptors).  The words are the leaves; a word's number is its node number.
 *  distance    Hamming distance of 256 bits.  "Nearest" among the children of a node is by (distance, child index).
 *  training    over the n descriptors of the keyframes in (keyframe, slot) order (slot < count), level by level from the root.  A node
 *              of depth < L that holds at least 2 descriptors is seeded: seed 0 is its first descriptor in input order; each further seed
 *              is the descriptor of the node with the largest minimum distance to the seeds so far, the lowest input index on a tie;
 *              seeding stops at k seeds or when that largest distance is 0.  A node with fewer than 2 seeds stays a leaf.  Otherwise the
 *              seeds are the first centroids of its children, a = assign(centroids), and at most `iters` times: centroids =
 *              update(a), b = assign(centroids), stop if b == a, a = b.  assign: the nearest child.  update: bit t of a child's centroid
 *              is set iff 2 * (members with bit t set) > members; a child without members keeps its centroid.  The children then hold
 *              the descriptors a assigns them.  n = 0 or 1 leaves the root a leaf (one word, 0); n < k or equal descriptors give fewer
 *              children.
 *  weights     over N keyframes, n_w of which hold word w at least once: W_w = (uint32) floor(log((double) N / n_w) * 65536 + 0.5) on
 *              the host, 0 when n_w is 0 or N (DBoW2's IDF in Q16.16; the only floating-point step).  Nodes that are no leaves carry 0.
 *  transform   every descriptor descends from the root to a word by the nearest child.  A keyframe's vector lists its distinct words in
 *              ascending order; with c_w descriptors in word w, a_w = c_w * W_w and A = sum a_w (uint64), the entry's value is
 *              v_w = (uint32) ((a_w << 30) / A); entries of value 0 stay.  A = 0 gives an empty vector.  c_w <= RGBID_LOOPFEAT_MAX_KEYPOINTS
 *              = 1 536 and W_w <= RGBID_BOW_MAX_WEIGHT give a_w < 2^31, so a_w << 30 stays inside 64 bits.
 *  score       S(q, c) = sum over the common words of min(v_q, v_c) in uint64: DBoW2's L1 score 1 - 0.5 sum |v - w| of L1-normalised
 *              vectors, scaled by 2^30.
 *  shortlist   for query q the candidates c <= q - min_separation with S(q, c) > 0, the T largest by (S descending, c descending).
 */
#ifndef RGBID_BOW_H_
#define RGBID_BOW_H_

#include <stdint.h>
#include "rgbid.h"
#include "rgbid_loopfeat.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_BOW_MAX_K 16
#define RGBID_BOW_MAX_DEPTH 6
#define RGBID_BOW_MAX_LEAVES (1 << 20)
#define RGBID_BOW_MAX_ITERS 64
#define RGBID_BOW_MAX_SHORTLIST 64        /* a wave keeps its best candidates one per lane */
/* the largest weight: a batch holds at most 65 535 keyframes, so W_w <= floor(log(65535 / 1) * 65536 + 0.5) = 726 816 (N = 65 535, n_w = 1).
 * 1 536 * 726 816 = 1 116 389 376 < 2^31 is what the transform's a_w << 30 rests on; rgbid_bow_import refuses anything larger. */
#define RGBID_BOW_MAX_WEIGHT 726816

/* one entry of a keyframe's vector, 8 bytes */
typedef struct rgbid_bow_entry {
  uint32_t word;     /* node number of the leaf */
  uint32_t value;    /* v_w, the entries of a vector sum to at most 2^30 */
} rgbid_bow_entry;

typedef struct rgbid_bow rgbid_bow;

/* an untrained vocabulary (the root alone: one word of weight 0) of branching factor k and depth `depth`.  RGBID_E_INVALID outside the
 * limits above. */
int rgbid_bow_create(rgbid_bow** v, rgbid_ctx* ctx, int k, int depth);
int rgbid_bow_destroy(rgbid_bow* v);
/* most nodes a tree of (k, depth) can have: sum of k^l, l = 0 .. depth; RGBID_E_INVALID outside the limits.  Needs no device. */
int rgbid_bow_max_nodes(int k, int depth, int32_t* nodes);
/* train on the descriptors of n_kf keyframes kps_dev [n_kf][max_keypoints], counts_dev [n_kf] (1 <= max_keypoints <=
 * RGBID_LOOPFEAT_MAX_KEYPOINTS, 1 <= iters <= RGBID_BOW_MAX_ITERS), then set the weights from the same keyframes.  Here and wherever a call
 * takes counts_dev, a count below 0 reads as 0 and one above max_keypoints as max_keypoints.  Scratch is allocated for the batch on first use
 * and grown on demand; the final step (the weights) waits for the stream. */
int rgbid_bow_train(rgbid_bow* v, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, int max_keypoints, int iters);
/* recompute the weights from another set of keyframes (N = n_kf; n_kf = 0 zeroes them; counts_dev clamped to 0 .. max_keypoints as in
 * rgbid_bow_train).  Waits for the stream. */
int rgbid_bow_set_weights(rgbid_bow* v, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, int max_keypoints);
/* the tree to host buffers (each optional): *nodes; centroids [nodes][32]; children [nodes][2] = first child, number of children (0, 0 for a
 * leaf); weights [nodes].  Waits for the stream.  Call it once for *nodes, then with buffers of that size. */
int rgbid_bow_export(rgbid_bow* v, int32_t* nodes, uint8_t* centroids, int32_t* children, uint32_t* weights);
/* the reverse: a tree in the numbering above that fits this handle's k and depth, with no weight above RGBID_BOW_MAX_WEIGHT; anything else
 * is RGBID_E_INVALID and leaves the vocabulary as it was. */
int rgbid_bow_import(rgbid_bow* v, int32_t nodes, const uint8_t* centroids, const int32_t* children, const uint32_t* weights);
/* vectors of n_kf keyframes: bow_dev [n_kf][max_keypoints] entries (unused ones zeroed), bow_counts_dev [n_kf]; words_dev [n_kf][max_keypoints]
 * (optional) receives the word of every descriptor, -1 in unused slots; counts_dev clamped to 0 .. max_keypoints as in rgbid_bow_train.
 * Asynchronous. */
int rgbid_bow_transform(rgbid_bow* v, const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int n_kf, int max_keypoints,
                        int32_t* words_dev, rgbid_bow_entry* bow_dev, int32_t* bow_counts_dev);
/* scores_dev [n_pairs] = S(q, c) of pairs_dev [n_pairs][2]; a pair naming a keyframe outside 0 .. n_kf - 1 scores 0.  Asynchronous. */
int rgbid_bow_score(rgbid_bow* v, const rgbid_bow_entry* bow_dev, const int32_t* bow_counts_dev, int n_kf, int max_keypoints,
                    const int32_t* pairs_dev, int n_pairs, uint64_t* scores_dev);
/* cand_dev [n_kf][T] (-1 padded) and cand_scores_dev [n_kf][T] (0 padded), min_separation >= 1, 1 <= T <= RGBID_BOW_MAX_SHORTLIST.  One
 * workgroup per query streams its candidates; no pair list and no score table is formed.  Asynchronous. */
int rgbid_bow_shortlist(rgbid_bow* v, const rgbid_bow_entry* bow_dev, const int32_t* bow_counts_dev, int n_kf, int max_keypoints,
                        int min_separation, int T, int32_t* cand_dev, uint64_t* cand_scores_dev);
/* stage timing: enable != 0 records HIP events around the following calls; ms (optional, host) receives the device milliseconds of the last
 * ones: train (without its weights), transform, score, shortlist.  Call it for ms after the work has completed. */
int rgbid_bow_timing(rgbid_bow* v, int enable, float ms[4]);

#ifdef __cplusplus
}
#endif
#endif
