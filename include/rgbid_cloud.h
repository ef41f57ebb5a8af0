/*
 * rgbid_cloud.h -- C-ABI of the keyframe point-cloud builder (the map a dense RGB-D front-end hands its user).
 *
 * The reference turns every keyframe it receives into a coloured point cloud (KeyframeManager::computeAlignedPointCloud,
 * src/keyframe_manager.cpp:438-528): in raster order, every pixel whose depth 1/iD and normal x are not NaN becomes one
 * point  Xworld = R_WC (d Kinv (x, y, 1)) + t_WC  with its world normal R_WC n and colour; the "novel" cloud its viewer draws
 * keeps the pixels whose overlap mask is 0 (surface the previous keyframe did not see).  Here the same step runs on the device,
 * batched over any set of keyframes in the packed export layout of rgbid_engine.h (overlap mask u8[N] | colours u8[3N] |
 * inverse depth f32[N] | normals f32[3N planar], N = rows * cols): a plan pass counts the points of every keyframe, an emit pass
 * writes them, in keyframe order and raster order inside each keyframe, with no atomics -- the output is deterministic.
 *
 * Arithmetic: d = 1.f / iD (IEEE float division), Kinv = the 3x3 cofactor inverse of K in double as Eigen
 * forms it (rgbid_cloud_kinv), every dot product ((a0 b0 + a1 b1) + a2 b2) in double without contraction, results rounded to float.
 */
#ifndef RGBID_CLOUD_H_
#define RGBID_CLOUD_H_

#include <stdint.h>
#include "rgbid.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one point: world position, world normal, source pixel (y * cols + x), colour, flags.  32 bytes. */
typedef struct rgbid_cloud_point {
  float x, y, z, nx, ny, nz;
  uint32_t pixel;
  uint8_t r, g, b, flags;
} rgbid_cloud_point;
#define RGBID_CLOUD_NOVEL 1u           /* flags bit: the pixel's overlap mask is 0 */

enum { RGBID_CLOUD_ALL = 0, RGBID_CLOUD_NOVEL_ONLY = 1 };

/* one keyframe: its packed export block (device memory, 20 N bytes) and its world pose R_WC (row-major) | t_WC */
typedef struct rgbid_cloud_src {
  const void* block_dev;
  double R[9], t[3];
} rgbid_cloud_src;

typedef struct rgbid_cloud rgbid_cloud;

/* a builder for keyframes of rows x cols pixels, up to max_keyframes per plan; it works on the context's stream */
int rgbid_cloud_create(rgbid_cloud** c, rgbid_ctx* ctx, int rows, int cols, int max_keyframes);
int rgbid_cloud_destroy(rgbid_cloud* c);
/* the inverse of K = [fx 0 cx; 0 fy cy; 0 0 1] (K = fx, fy, cx, cy as floats, widened to double) as the plan uses it: row-major */
int rgbid_cloud_kinv(const float K[4], double Kinv[9]);
/* count the points of n (1 <= n <= max_keyframes) keyframes in `mode` (RGBID_CLOUD_ALL / RGBID_CLOUD_NOVEL_ONLY).
 * offsets (host, n + 1 entries): the first record of each keyframe, offsets[n] = total.  Synchronises. */
int rgbid_cloud_plan(rgbid_cloud* c, int n, const rgbid_cloud_src* src, const float K[4], int mode, unsigned long long* offsets);
/* write the points of the last plan to out_dev (device memory of `capacity` records; RGBID_E_INVALID when capacity < offsets[n]).
 * Asynchronous on the context's stream: the source blocks must stay valid and unchanged until it has run. */
int rgbid_cloud_emit(rgbid_cloud* c, rgbid_cloud_point* out_dev, unsigned long long capacity);

#ifdef __cplusplus
}
#endif
#endif
