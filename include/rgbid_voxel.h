/*
 * rgbid_voxel.h -- C-ABI of the voxel-grid filter over keyframe point clouds (the map the reference writes for its user).
 *
 * The reference writes its final map through pcl::VoxelGrid<pcl::PointXYZRGB> with a 1 cm leaf (savePointCloudInFile,
 * tools/RGBID_SLAMapp.cpp:341-354): every occupied cell of a regular grid becomes the centroid of the points inside it.  Here the same
 * filter runs on the device over rgbid_cloud_point records (rgbid_cloud.h), deterministically: a plan pass forms the grid, sorts the
 * points' cell keys with a stable radix sort and counts the voxels; an emit pass writes one 32-byte record per voxel, in ascending key
 * order, summing each voxel's members in ascending input order.  No floating-point atomics: the output is the same from run to run.
 *
 * Contract: a record takes part iff x, y, z are finite.  inv_a = 1.f / leaf_a; min_b_a / max_b_a =
 * (int) floorf(min / max of p_a over the finite points * inv_a); div_b = max_b - min_b + 1; a point's cell ijk_a =
 * (int)(floorf(p_a * inv_a) - (float) min_b_a) and its key ijk_0 + ijk_1 div_b_0 + ijk_2 div_b_0 div_b_1 (64-bit).  Centroid: sums in
 * double in member order without contraction, divided by the member count n_v and rounded to float once; colour floor(sum / n_v);
 * normal s / sqrt((s0 s0 + s1 s1) + s2 s2) over the members whose normal is finite (NaN when there is none or the sum is 0); flags bit 0
 * when any member has RGBID_CLOUD_NOVEL.  Voxels of fewer than min_points members are dropped.
 */
#ifndef RGBID_VOXEL_H_
#define RGBID_VOXEL_H_

#include <stdint.h>
#include "rgbid_cloud.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one voxel: centroid, mean normal, member count, mean colour, flags.  32 bytes, the offsets of rgbid_cloud_point (count where the
 * cloud record holds its pixel). */
typedef struct rgbid_voxel_point {
  float x, y, z, nx, ny, nz;
  uint32_t count;
  uint8_t r, g, b, flags;
} rgbid_voxel_point;

#define RGBID_VOXEL_MAX_POINTS (1ull << 31)   /* indices fit in 32 bits */

typedef struct rgbid_voxel rgbid_voxel;

/* a filter for up to max_points (1 .. RGBID_VOXEL_MAX_POINTS) input records per plan; it works on the context's stream */
int rgbid_voxel_create(rgbid_voxel** v, rgbid_ctx* ctx, unsigned long long max_points);
int rgbid_voxel_destroy(rgbid_voxel* v);
/* grid and count the voxels of n records at in_dev (device memory, 16-byte aligned) with leaf sizes leaf[3] (finite, > 0).
 * grid (optional, host): min_b[3], div_b[3]; stats (optional, host): finite points, voxels before and after min_points;
 * voxels: the number of records the emit writes.  RGBID_E_INVALID for a refused leaf, n > max_points, a grid whose bounds leave the
 * int32 range or whose cell count is 2^62 or more.  Synchronises. */
int rgbid_voxel_plan(rgbid_voxel* v, const rgbid_cloud_point* in_dev, unsigned long long n, const float leaf[3],
                     unsigned min_points, long long grid[6], unsigned long long stats[3], unsigned long long* voxels);
/* write the voxels of the last plan to out_dev (device memory of `capacity` records, 16-byte aligned; RGBID_E_INVALID when capacity
 * < voxels).  Asynchronous on the context's stream: the input records must stay valid and unchanged until it has run. */
int rgbid_voxel_emit(rgbid_voxel* v, rgbid_voxel_point* out_dev, unsigned long long capacity);
/* stage timing: enable != 0 records HIP events around the stages of the following plans and emits; ms (optional, host) receives the
 * device milliseconds of the last ones: box, keys, sort, runs (incl. min_points), emit.  Call it for ms after the emit has completed. */
int rgbid_voxel_timing(rgbid_voxel* v, int enable, float ms[5]);

#ifdef __cplusplus
}
#endif
#endif
