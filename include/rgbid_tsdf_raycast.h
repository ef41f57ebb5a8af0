/*
 * rgbid_tsdf_raycast.h -- the second half of the C-ABI of rgbid_tsdf.h, which includes this file at its end: the volume read back by ray
 * casting (a predicted depth, normal and colour image of the fused surface at a pose) and a normal per mesh vertex.  Both evaluate the
 * gradient of D.  The reference has no program text for either.
 *
 * Contract, continued from rgbid_tsdf.h (byte-identical to tests/raycast_mirror.py).  float32 without contraction,
 * IEEE division and square root; integers and comparisons decide and nothing depends on execution order.
 *
 * Ray cast.  V views (rgbid_render_pose), K = fx, fy, cx, cy, rows, cols, a gate 0 < z_min <= z_max, step > 0 (metres of camera depth
 * per sample), min_weight in 1 .. 65 535.  The volume is the handle's current state.
 * 13. Pose: the twelve floats R00 .. R22, tx, ty, tz are the entries of R_WC (row-major) and t_WC, each rounded once from double to
 *     float32 (rgbid_tsdf_pose_wc).  Nothing is inverted.  This is the only form in which a pose reaches the device.
 * 14. Ray of pixel (pu, pv): dx = ((float)pu - cx) / fx, dy = ((float)pv - cy) / fy; world direction per unit depth
 *     wx = (R00 dx + R01 dy) + R02, wy and wz with rows 1 and 2; in voxel units, once per ray: ax = (tx - ox) / voxel, bx = wx / voxel, and
 *     likewise for y and z.
 * 15. Samples: Z_n = z_min + (float)n step for n = 0, 1, ... while n <= RGBID_TSDF_MAX_STEPS and Z_n <= z_max (the call is refused when
 *     (z_max - z_min) / step, in double, exceeds RGBID_TSDF_MAX_STEPS; the bound on n only ends the walk where step is below the
 *     spacing of float32 at z_max).  Position gx = ax + Z bx, one product and one sum; gy, gz likewise.  i0 = floorf(gx), j0 = floorf(gy),
 *     k0 = floorf(gz).  A sample is DEFINED iff 0 <= i0 <= nx - 2, 0 <= j0 <= ny - 2, 0 <= k0 <= nz - 2 (the float against the integer,
 *     exactly; NaN fails) and all 8 corner voxels have W >= min_weight.  Only after the range test are i0, j0, k0 converted to int.  The
 *     domain is half-open: gx = nx - 1 exactly is undefined.
 * 16. Value and gradient.  Corners D_ijk, i, j, k in {0, 1} offset from (i0, j0, k0); fx_ = gx - i0, fy_ = gy - j0, fz_ = gz - k0.  Every
 *     lerp is a + f (b - a).  x first, then y, then z:
 *       Lx_jk = lerp(D_0jk, D_1jk, fx_), Ly_k = lerp(Lx_0k, Lx_1k, fy_), f = lerp(Ly_0, Ly_1, fz_)
 *     The gradient is the interpolant's own derivative inside the cell:
 *       Gx = lerp_z(lerp_y(D_100 - D_000, D_110 - D_010), lerp_y(D_101 - D_001, D_111 - D_011))
 *       Gy = lerp_z(Lx_10 - Lx_00, Lx_11 - Lx_01),  Gz = Ly_1 - Ly_0
 * 17. March: walk n upwards and remember the previous sample.  If samples n - 1 and n are both defined: f_{n-1} > 0 and f_n <= 0 is a
 *     HIT; otherwise !(f_{n-1} > 0) and f_n > 0 is an EXIT (the ray came out of a surface from behind): the pixel is empty and the march
 *     ends.  An undefined sample only breaks the pair.  No hit by the last n: the pixel is empty.
 * 18. Hit: t = f_{n-1} / (f_{n-1} - f_n), Z* = Z_{n-1} + t (Z_n - Z_{n-1}), depth = Z*.  The volume is sampled once more at Z* (steps 15
 *     and 16): this re-sample gives the normal and the colour.
 * 19. Normal, in the camera frame as in rgbid_render.h: L = sqrtf((Gx Gx + Gy Gy) + Gz Gz), n_w = (Gx / L, Gy / L, Gz / L) (from inside to
 *     outside: towards the camera on a front face), n_c = R_WC^T n_w = ((R00 nwx + R10 nwy) + R20 nwz, ...) with the floats of step 13.
 *     An undefined re-sample, or L zero or not finite: all three components are NaN.
 * 20. Colour: per corner the mean of step 11.  All 8 corners have one: per channel the trilinear value in the order of step 16 over the
 *     means as float32, then fminf(fmaxf(floorf(c + 0.5f), 0.f), 255.f) (a NaN gives 0).  Otherwise the mean of the corner
 *     (fx_ >= 0.5f, fy_ >= 0.5f, fz_ >= 0.5f) if that corner has one.  Otherwise, with an undefined re-sample, or on a handle without
 *     colour: 0 0 0.
 * 21. Outputs (device memory, each may be NULL), view v at element offset v rows cols {1, 3, 3}: depth float32 [V][rows][cols], normal
 *     float32 [V][3][rows][cols], colour uint8 [V][rows][cols][3], the layouts of rgbid_render_views.  An empty pixel has depth NaN,
 *     normal NaN and colour 0.  Every NaN written has the bits RGBID_RENDER_NAN_BITS.
 *     This holds on any state (rgbid_tsdf.h): a NaN f is neither a hit nor an exit's first half (f > 0 and f <= 0 both fail; !(f > 0)
 *     holds), a Z* that is NaN is a hit whose re-sample is undefined, and the sampler masks Cn out of every count it compares.
 * The contract visits every n; the kernel skips the n whose sample it can prove undefined (DESIGN.md section 20 holds the proof).
 *
 * Vertex normals, world frame, at the vertex ranks of step 9, under the plan's min_weight.
 * 22. Voxel gradient, per axis with the neighbours p +- e; a neighbour counts iff it is inside the volume and valid.  Both count:
 *     D+ - D-.  Only p + e: 2.f (D+ - D).  Only p - e: 2.f (D - D-).  Neither: 0.
 * 23. Vertex of the active edge (a inside, b outside, t of step 10): g = g_a + t (g_b - g_a) per component, L as in step 19; the normal
 *     is g / L, or 0 0 0 when L is zero or not finite (not NaN: it goes into a PLY).  A NaN t or a D that is not finite makes L NaN or
 *     infinite, so no normal component is ever NaN; the vertex itself may be (step 10).
 */
#ifndef RGBID_TSDF_RAYCAST_H_
#define RGBID_TSDF_RAYCAST_H_

#ifndef RGBID_TSDF_H_
#error "include rgbid_tsdf.h: it declares the handle and includes this file"
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RGBID_TSDF_MAX_STEPS 65536              /* (z_max - z_min) / step at most, and the largest n a ray visits */

/* step 13: pose -> R00 R01 R02 R10 .. R22 tx ty tz of R_WC | t_WC as float32.  Host only, touches no device. */
int rgbid_tsdf_pose_wc(const rgbid_render_pose* pose, float wc[12]);
/* steps 13 - 21 for V views of rows x cols pixels.  RGBID_E_INVALID before any launch, the handle usable afterwards and the outputs
 * untouched, for: V < 1 or above the handle's max_views; rows or cols out of 1 .. RGBID_TSDF_MAX_DIM; rows cols V >= 2^31; z_min or z_max
 * not finite, <= 0 or z_min > z_max; step not finite or <= 0; (z_max - z_min) / step above RGBID_TSDF_MAX_STEPS; min_weight out of
 * 1 .. RGBID_TSDF_MAX_WEIGHT; a pose or intrinsic that is not finite (as double or as float32), fx or fy equal to 0; depth or normal not
 * 4-byte aligned.  All three outputs NULL is a valid call that launches nothing.  Asynchronous on the context's stream.  It reads the
 * state only: a plan of rgbid_tsdf_extract_plan survives it. */
int rgbid_tsdf_raycast(rgbid_tsdf* v, int V, const rgbid_render_pose* poses, const float K[4], int rows, int cols,
                       float z_min, float z_max, float step, unsigned min_weight,
                       float* depth_dev, float* normal_dev, uint8_t* colour_dev);
/* stage timing of the ray cast, beside rgbid_tsdf_timing (the two share one switch): enable != 0 records HIP events around the following
 * calls; ms (optional, host) receives the device milliseconds of the last one (the pose table's upload and the launch). */
int rgbid_tsdf_raycast_timing(rgbid_tsdf* v, int enable, float ms[1]);
/* steps 22 and 23 for the last plan's vertices: normals float32 [n_vertices][3] (device memory, 4-byte aligned).  The refusals are those of
 * rgbid_tsdf_extract_emit: RGBID_E_INVALID without a plan, for a NULL or misaligned buffer and when vertex_capacity < n_vertices; nothing
 * is written past the count; a plan of 0 vertices writes nothing and takes any pointer.  Asynchronous. */
int rgbid_tsdf_extract_normals(rgbid_tsdf* v, float* normals_dev, unsigned long long vertex_capacity);

#ifdef __cplusplus
}
#endif
#endif
