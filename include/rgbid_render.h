/*
 * rgbid_render.h -- C-ABI of the headless view of the map: the 32-byte records of a keyframe point cloud (rgbid_cloud.h, or what
 * rgbid_outlier.h / a caller left of them) are projected into V pinhole cameras and every pixel keeps the nearest record.  The reference
 * looks at its map through a PCL / VTK window (VisualizationManager, CameraView) and has no program text for this; only the pose and
 * intrinsics conventions are the ones the project mirrors already.
 *
 * Contract (byte-identical to tests/render_mirror.py).  Integers decide and nothing depends on execution order.
 *  1. Per view, on the host, in double without contraction: R_CW = R_WC^T and t_CW[i] = -((R_WC[0][i] t0 + R_WC[1][i] t1) + R_WC[2][i] t2),
 *     every entry then rounded once to float32 (rgbid_render_pose_cw).  These twelve floats r00 .. r22, tx, ty, tz are the only form in
 *     which a pose reaches the device.
 *  2. A record takes part in a view iff x, y, z are finite.  A non-finite normal excludes nothing.
 *  3. Camera point, float32, no contraction: X = ((r00 x + r01 y) + r02 z) + tx, Y and Z likewise with rows 1 and 2.
 *  4. Depth gate: the record is visible iff z_min <= Z <= z_max (a NaN or infinite Z fails it).
 *  5. Projection: u = fx (X / Z) + cx, v = fy (Y / Z) + cy with IEEE division, one product and one sum each; pu = floorf(u + 0.5f),
 *     pv = floorf(v + 0.5f).  In float: the record is dropped unless -s <= pu <= cols - 1 + s and -s <= pv <= rows - 1 + s (NaN and
 *     infinity fail); only then are pu, pv converted to int.
 *  6. Splat: the record writes to the (2 s + 1)^2 pixels around (pu, pv), clipped to the image.
 *  7. Winner: key = (uint64(bits of Z) << 32) | record index.  Z > 0, so its bits order like its value.  Every pixel of every view keeps the
 *     minimum key written to it: the smallest Z, and among equal Z the smallest index.
 *  8. Resolve: an empty pixel has index RGBID_RENDER_EMPTY, depth NaN, colour 0 0 0, normal NaN NaN NaN; another one the winner's index,
 *     its Z, its r g b bytes unchanged and its normal R_CW n = ((r00 nx + r01 ny) + r02 nz), ... in float32 without contraction.  Every
 *     NaN written -- an empty pixel's, or a normal component that came out NaN -- has the bits RGBID_RENDER_NAN_BITS, the project's
 *     invalid-pixel NaN: which NaN an invalid operation or a NaN operand yields differs between processors, the stored bits do not.
 *  9. Outputs (device memory, each may be NULL to skip it), view v at element offset v * rows * cols * {1, 1, 3, 3}:
 *     index uint32 [V][rows][cols], depth float32 [V][rows][cols], colour uint8 [V][rows][cols][3], normal float32 [V][3][rows][cols].
 */
#ifndef RGBID_RENDER_H_
#define RGBID_RENDER_H_

#include <stdint.h>
#include "rgbid_cloud.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_RENDER_MAX_SPLAT 4                /* the largest splat half-width s: (2 s + 1)^2 <= 81 pixels per record and view */
#define RGBID_RENDER_MAX_POINTS 2147483647ull   /* 2^31 - 1: indices fit in 32 bits and RGBID_RENDER_EMPTY is nobody's index */
#define RGBID_RENDER_MAX_DIM 1048576            /* 2^20: rows and cols at most; cols - 1 + s is then exact in float32 */
#define RGBID_RENDER_VIEW_CHUNK 16              /* views one splat / resolve launch handles; further views go in further launches */
#define RGBID_RENDER_EMPTY 0xFFFFFFFFu          /* index of a pixel no record wrote to */
#define RGBID_RENDER_NAN_BITS 0x7FFFFFFFu       /* bits of every NaN in the depth and normal planes */

/* one view: the camera's world pose R_WC (row-major) | t_WC, as rgbid_cloud_src carries it */
typedef struct rgbid_render_pose {
  double R[9], t[3];
} rgbid_render_pose;

typedef struct rgbid_render rgbid_render;

/* a renderer for up to max_points (1 .. RGBID_RENDER_MAX_POINTS) records and rows * cols * V <= max_pixels_times_views per call; it
 * works on the context's stream and holds 8 bytes per pixel and view */
int rgbid_render_create(rgbid_render** r, rgbid_ctx* ctx, unsigned long long max_points, unsigned long long max_pixels_times_views);
int rgbid_render_destroy(rgbid_render* r);
/* step 1 of the contract: pose -> r00 r01 r02 r10 .. r22 tx ty tz as float32.  Host only, touches no device. */
int rgbid_render_pose_cw(const rgbid_render_pose* pose, float cw[12]);
/* render n records at in_dev (device memory, 16-byte aligned) into V >= 1 views of rows x cols pixels with K = fx, fy, cx, cy, splat
 * half-width s (0 .. RGBID_RENDER_MAX_SPLAT) and depth gate [z_min, z_max].  RGBID_E_INVALID before any launch, the handle usable
 * afterwards, for: rows or cols < 1 or > RGBID_RENDER_MAX_DIM; rows * cols * V above the handle's capacity; s out of range; z_min or
 * z_max not finite, <= 0 or z_min > z_max; a pose or intrinsic that is not finite (as double or once rounded to float32), fx or fy equal
 * to 0; n above the handle's capacity; a NULL or misaligned record pointer with n > 0; an output pointer that is not 4-byte aligned.
 * n = 0 is no error and gives all-empty views.  Asynchronous on the context's stream: records and outputs must stay valid until it ran. */
int rgbid_render_views(rgbid_render* r, const rgbid_cloud_point* in_dev, unsigned long long n, int V, const rgbid_render_pose* poses,
                       const float K[4], int rows, int cols, int s, float z_min, float z_max, uint32_t* index_dev, float* depth_dev,
                       uint8_t* colour_dev, float* normal_dev);
/* stage timing: enable != 0 records HIP events around the stages of the following calls; ms (optional, host) receives the device
 * milliseconds of the last one: clear, splat, resolve.  Call it for ms after the call has completed. */
int rgbid_render_timing(rgbid_render* r, int enable, float ms[3]);
/* splat statistics: enable != 0 makes the following calls count, at some cost in the splat; stats (optional, host) receives the counts of
 * the last one: (record, view) pairs that passed the gates of steps 4 and 5, pixel writes they attempted, and those of them that reached
 * the 64-bit atomic minimum (the others saw a key that was not larger already).  The first two are a function of the input; the third
 * depends on timing.  Synchronises when stats is given. */
int rgbid_render_stats(rgbid_render* r, int enable, unsigned long long stats[3]);

#ifdef __cplusplus
}
#endif
#endif
