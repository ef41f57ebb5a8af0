/*
 * rgbid_segment.h -- C-ABI of the keyframe segmenter: the first step of the reference's KeyframeManager::processNewKeyframe
 * (src/keyframe_manager.cpp:300-385).  A keyframe's camera-frame cloud is cut into "superjuts" by a Felzenszwalb-style graph segmentation
 * over pixel-neighbour edges weighted by normal curvature (CloudSegmenter, Segmentation::Graph), every segment gets a histogram of its
 * normals and the entropy of that histogram (Superjut::computeHistogramOfNormalsAndEntropy), the entropies make the negentropy image, and
 * the negentropy masks choose which keypoints feed the masked bags of words (Keyframe::computeMaskedDescriptors, src/keyframe.cpp:135-203).
 * Every call is batched over keyframes in the packed export layout rgbid_cloud_src names (overlap mask u8[N] | colours u8[3N] | inverse
 * depth f32[N] | normals f32[3N planar]; R and t of the source are not read: the reference segments the camera-frame cloud), works on the
 * context's stream, uses no library sort and no floating-point atomics, and gives results that are bitwise the same from run to run and
 * independent of the batch a keyframe is computed in.  Every float operation is rounded once (no contraction).
 *
 * Contract.
 *  points    A pixel is a point when the predicate of rgbid_cloud.h holds: d = 1.f / iD and the normal's x are not NaN.  Its position is
 *            the rgbid_cloud point of the identity pose, R = I and t = 0 ((d Kinv) p in double, rounded to float); its normal is the
 *            exported one.
 *  edges     For the point at pixel (x, y) the neighbours nb = 0 .. 3 are (x + 1, y), (x, y + 1), (x + 1, y - 1), (x + 1, y + 1); one
 *            counts when it lies inside the image and is a point.  Edge id e = 4 * pixel + nb, pixel = y * cols + x.  Weight, in float,
 *            p1 / n1 the pixel and p2 / n2 the neighbour: dp = p2 - p1, norm = sqrtf((dx dx + dy dy) + dz dz), dot = (n1x n2x + n1y n2y) +
 *            n1z n2z, dot2 = (1.f / norm) ((n2x dx + n2y dy) + n2z dz), c = 1.f - dot, and c = c c when dot2 > 0.  A NaN weight drops the edge.
 *  order     Ascending by float comparison of the weight (-0 equals +0; weights are negative when dot rounds above 1), ties by ascending
 *            edge id.  (The reference's std::sort leaves ties unspecified.)
 *  segments  The result of the sequential loop: every point starts as its own component with size = 1 and th = k_th.  Pass 1 over the
 *            edges in order, a != b the roots of an edge's ends: when w <= th[a] and w <= th[b] the two merge, the sizes add up and th =
 *            w + k_th / (float) size.  Pass 2 over the edges in the same order: when a != b and (size[a] < min_size or size[b] < min_size)
 *            the two merge.  The partition and the sizes are the contract (th after pass 1); parents and ranks are not.
 *  labels    labels [n][rows][cols] int32: -1 where the pixel is no point, else the segment's index in order of first appearance in raster
 *            order (the reference's superjut index).  seg_counts [n]: segments per keyframe.  seg_sizes [n][max_segments]: points per
 *            segment.  Labels and counts are always complete; sizes, histograms and entropies exist for the segments of index below
 *            max_segments, and a pixel of a later segment has negentropy NaN (a caller that sees seg_counts > max_segments asks for more).
 *  histogram Bin centres: the golden-section spiral of src/util_funcs.cpp:157-173 in float (rgbid_segment_bins).  A point counts in the
 *            first bin of the largest (nx cx + ny cy) + nz cz, by strict > starting from -1.1f; a point no bin wins (a NaN dot) counts
 *            nowhere.  hist [n][max_segments][nbins] int32, exact.  Entropy: freq = (float) count / (float) size; the term is 0 when freq <
 *            1.f / (float) (2 * size), else -freq logf(freq); terms added in bin order; the sum divided by logf((float) size).  A segment
 *            of one point gives NaN, as the reference does.  (The reference adds 1.f / size once per point; the quotient differs from
 *            that by at most about count 2^-24 relative.)
 *  image     negentropy [n][rows][cols] float: 0 where the pixel is no point, else 1.f - entropy of its segment.
 *  masks     Thresholds t_k = 0.f, 0.1f, .. 0.9f; c_k = pixels of the whole image with negentropy < t_k.  For level m = 1 .. M - 1, k*(m) is
 *            the largest k with (float) c_k / (float) (rows cols) < (float) m / (float) M, -1 when there is none.  Mask m keeps a pixel
 *            unless negentropy < t_k*(m); k* = -1 and level 0 keep everything.  mask_levels [n][M] int32 holds the k* (entry 0 is -1).
 */
#ifndef RGBID_SEGMENT_H_
#define RGBID_SEGMENT_H_

#include <stdint.h>
#include "rgbid.h"
#include "rgbid_cloud.h"
#include "rgbid_loopfeat.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_SEGMENT_MAX_BINS 128
#define RGBID_SEGMENT_DEFAULT_BINS 80
#define RGBID_SEGMENT_MAX_LEVELS 8      /* mask levels M: one bit each of a keypoint's byte */
#define RGBID_SEGMENT_DEFAULT_LEVELS 4
#define RGBID_SEGMENT_THRESHOLDS 10
#define RGBID_SEGMENT_MAX_WINDOW 256    /* edges a keyframe's workgroup decides side by side */
#define RGBID_SEGMENT_DEFAULT_K 0.6f
#define RGBID_SEGMENT_DEFAULT_MIN_SIZE 300

typedef struct rgbid_segment rgbid_segment;

/* a segmenter for keyframes of rows x cols pixels, up to max_keyframes per call, with tables for max_segments (1 .. rows cols) segments
 * per keyframe.  4 rows cols max_keyframes must stay below 2^32.  RGBID_E_INVALID otherwise. */
int rgbid_segment_create(rgbid_segment** s, rgbid_ctx* ctx, int rows, int cols, int max_keyframes, int max_segments);
int rgbid_segment_destroy(rgbid_segment* s);
/* the device bytes rgbid_segment_create allocates for these arguments, or its refusal.  Needs no device. */
int rgbid_segment_workspace_bytes(int rows, int cols, int max_keyframes, int max_segments, unsigned long long* bytes);
/* the device bytes this handle holds: rgbid_segment_workspace_bytes of its arguments */
int rgbid_segment_device_bytes(const rgbid_segment* s, unsigned long long* bytes);
/* the bin centres: centres[nbins][3], nbins in 1 .. RGBID_SEGMENT_MAX_BINS.  Needs no device. */
int rgbid_segment_bins(int nbins, float* centres);
/* test hook: the window of the union-find rounds, 1 .. RGBID_SEGMENT_MAX_WINDOW (the default).  No window changes a result. */
int rgbid_segment_set_window(rgbid_segment* s, int window);
/* segment n (1 <= n <= max_keyframes) keyframes.  K = fx, fy, cx, cy (host).  k_th finite and >= 0, min_size >= 1, nbins in 1 ..
 * RGBID_SEGMENT_MAX_BINS, levels (M) in 1 .. RGBID_SEGMENT_MAX_LEVELS.  Outputs, device memory: labels_dev [n][rows][cols], seg_counts_dev
 * [n], seg_sizes_dev [n][max_segments], hist_dev [n][max_segments][nbins], negentropy_dev [n][rows][cols], mask_levels_dev [n][levels].
 * It first waits for the work already on the context's stream (the previous run reads the staged block pointers), then enqueues its
 * own and returns: the blocks and the outputs must stay valid until that has run. */
int rgbid_segment_run(rgbid_segment* s, int n, const rgbid_cloud_src* src, const float K[4], float k_th, int min_size, int nbins, int levels,
                      int32_t* labels_dev, int32_t* seg_counts_dev, int32_t* seg_sizes_dev, int32_t* hist_dev, float* negentropy_dev,
                      int32_t* mask_levels_dev);
/* one byte per keypoint record of n keyframes (kps_dev [n][max_keypoints], counts_dev [n]): bit m < levels is set when mask m keeps the
 * keypoint's pixel (x, y); a keypoint outside the image is in level 0 only, as in the reference; bytes of unused records are 0.
 * bits_dev [n][max_keypoints].  Asynchronous. */
int rgbid_segment_mask_keypoints(rgbid_segment* s, const float* negentropy_dev, const int32_t* mask_levels_dev, int n, int levels,
                                 const rgbid_loopfeat_kp* kps_dev, const int32_t* counts_dev, int max_keypoints, uint8_t* bits_dev);
/* the largest number of rounds a keyframe of the last run needed in pass 1 and in pass 2.  Synchronises. */
int rgbid_segment_last_rounds(rgbid_segment* s, unsigned long long rounds[2]);
/* stage timing: enable != 0 records HIP events around the following runs; ms (optional, host) receives the device milliseconds of the
 * last one: edges (points + weights), sort, pass 1, pass 2, labels, histogram + image + masks.  Call it for ms after the work has completed. */
int rgbid_segment_timing(rgbid_segment* s, int enable, float ms[6]);

#ifdef __cplusplus
}
#endif
#endif
