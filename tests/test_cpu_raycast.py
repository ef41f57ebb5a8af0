"""CPU checks of the TSDF ray cast and the vertex normals (include/rgbid_tsdf_raycast.h, rgbid.tsdf): the numpy restatement the GPU tests
compare the kernels against (tests/raycast_mirror.py) against the plain scalar loops of the contract; a sphere whose hit set, depth and
normals are known analytically; a wall whose depth and normal are derived by hand; the threshold scene of the GPU tests, every case
asserted on the mirror; the vertex normals' one-sided forms; the Python argument checks one by one; the header as C99; the library's
exports; the command line's option errors; the PLY with normals."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from rgbid import _lib
from rgbid import tsdf as TS
from tests import raycast_mirror as RM
from tests import tsdf_mirror as TM
from tests.test_cpu_consist import COLS, K, ROWS, cameras
from tests.test_cpu_tsdf import GATE, SPHERE, TH_GRID, TH_K, mixed_scene, mixed_volume, sphere_volume, wall_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32
U = 2.0 ** -24                           # half the spacing of float32 at 1
BACK = np.diag([-1.0, 1.0, -1.0])        # a camera turned by pi about y: entries 0 and +-1
SPHERE_CAM = dict(R=np.eye(3), t=(0.6, 0.5, -1.0), K=(64.0, 64.0, 31.5, 23.5), rows=48, cols=64, z_min=0.3, z_max=5.0)


@functools.lru_cache(maxsize=None)
def mixed_state():
    """the mixed volume of tests/test_cpu_tsdf.py after its three views: weights 0 .. 3, colours, both signs"""
    sc = mixed_scene(3)
    return TM.integrate(mixed_volume(), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)


def ray_cameras(V):
    """V cameras around the mixed volume: the first sees the surface with the identity pose, the second looks back at it from behind, the
    third stands outside and looks past the volume, the others are moved and turned a little"""
    rng = np.random.default_rng(900 + V)
    R, t = cameras(rng, V)
    if V > 1:
        R[1], t[1] = BACK @ R[1], np.array([0.1, -0.05, 3.4])
    if V > 2:
        t[2] = t[2] + np.array([5.0, 0.0, 0.0])
    return R, t


def analytic_sphere(cam=SPHERE_CAM):
    """-> (meets bool [rows, cols], depth of the first intersection, unit ray directions [rows, cols, 3]) of the sphere tests' camera"""
    fx, fy, cx, cy = cam["K"]
    pu, pv = np.meshgrid(np.arange(cam["cols"], dtype=np.float64), np.arange(cam["rows"], dtype=np.float64))
    d = np.stack([(pu - cx) / fx, (pv - cy) / fy, np.ones_like(pu)], -1)
    oc = np.array(cam["t"]) - np.array(SPHERE["centre"])
    A, B, Cc = (d * d).sum(-1), 2 * (d @ oc), oc @ oc - SPHERE["radius"] ** 2
    disc = B * B - 4 * A * Cc
    meets = disc > 0
    return meets, (-B - np.sqrt(np.where(meets, disc, 0))) / (2 * A), d


# ---- the threshold scene: everything exact in float32 ---------------------------------------------------------------------------------
# TH_GRID: voxel = trunc = 1 / 8, centres at multiples of 1 / 8, z = 1.5 .. 2.5 (k = 0 .. 8).  D = clip(2 - z, +-trunc): + 1 / 8 for k <= 3,
# 0 at k = 4, - 1 / 8 behind; W = 1 for k <= 5.  An identity camera at the origin with z_min = 1.5 and step = 1 / 8 has gz = n exactly: sample
# n lies on the voxel plane k = n, is defined for n <= 4 and f_n = D_n there.
def th_volume(kind="wall"):
    vol = TM.Volume(**TH_GRID)
    z = vol.centres()[2].astype(np.float64)
    D = np.broadcast_to(np.clip(2.0 - z, -0.125, 0.125).astype(F)[:, None, None], vol.shape).copy()
    W = np.broadcast_to((z <= 2.125)[:, None, None], vol.shape).astype(np.uint32).copy()
    if kind == "block":                                     # (g): weight 2 in a block of voxels
        W[:6, 3:10, 4:12] = 2
    if kind == "holes":                                     # (h): W = 0 in the plane k = 1 (a pair broken, the march goes on to the hit)
        W[1, :, 2:6] = 0                                    # and in the plane k = 3 (the pair of the crossing broken: no hit there)
        W[3, :, 10:14] = 0
    if kind == "slit":                                      # (j): one column of the plane k = 3 that only the re-sample's cell touches
        W[3, :, 12] = 0
    rng = np.random.default_rng(11)
    Cn = (W > 0).astype(np.uint32)
    Cn[:, :, :3] = 0                                        # the first columns carry no colour: the nearest-corner rule, and 0
    rgb = rng.integers(0, 256, (3,) + vol.shape).astype(np.uint32) * Cn
    vol.set_state(D, W | (Cn << np.uint32(16)), rgb)
    return vol


TH_BASE = dict(kind="wall", z_min=1.5, z_max=2.5, step=0.125, min_weight=1)
TH_MAIN = [(np.eye(3), (0, 0, 0)),                          # 0 (a) f_4 = 0 exactly: a hit with t = 1
           (np.eye(3), (0, 0, 2.0 ** -23)),                 # 1 (b) one ulp forward: gz = n + 2^-20
           (np.eye(3), (0, 0, -2.0 ** -23)),                # 2 (b) one ulp back: gz = n - 2^-20, the crossing is the pair (4, 5)
           (np.eye(3), (-2.0 ** -6, 0, 0)),                 # 3 (c) gx of pixel column 0 at n = 4 is 0 exactly: defined
           (np.eye(3), (-2.0 ** -6 - 2.0 ** -24, 0, 0)),    # 4 (c) one ulp below 0: undefined
           (np.eye(3), (2.0 ** -6, 0, 0)),                  # 5 (d) gx of pixel column 63 at n = 4 is nx - 1 = 16 exactly: undefined
           (np.eye(3), (2.0 ** -6 - 2.0 ** -23, 0, 0)),     # 6 (d) one ulp below 16: defined
           (BACK, (0, 0, 4.0)),                             # 7 (e) from behind, on the planes: f = 0 then + 1 / 8: an exit
           (BACK, (0, 0, 4.0625)),                          # 8 (e) from behind, between the planes: f < 0 then > 0
           (BACK, (0, 0, 3.5625))]                          # 9 (f) inside the negative band: the first defined sample is n = 0 with f < 0
TH_CASES = {"main": dict(TH_BASE, views=TH_MAIN),
            "weight": dict(TH_BASE, kind="block", min_weight=2, views=[TH_MAIN[0]]),                        # (g)
            "holes": dict(TH_BASE, kind="holes", views=[TH_MAIN[0]]),                                       # (h)
            "zmax_on": dict(TH_BASE, z_max=2.0, views=[TH_MAIN[0], TH_MAIN[7]]),                            # (i), and (e) ending on the last n
            "zmax_below": dict(TH_BASE, z_max=2.0 - 2.0 ** -23, views=[TH_MAIN[0]]),                        # (i)
            "resample": dict(TH_BASE, kind="slit", step=0.25, views=[(np.eye(3), (0, 0, 0.0625))])}         # (j)


def th_cast(name, views=None):
    """the mirror's planes of a case of the threshold scene (of some of its views) -> (volume, dict)"""
    c = TH_CASES[name]
    vw = c["views"] if views is None else [c["views"][i] for i in views]
    vol = th_volume(c["kind"])
    return vol, RM.raycast(vol, np.stack([v[0] for v in vw]), np.array([v[1] for v in vw], np.float64), TH_K, ROWS, COLS, c["z_min"], c["z_max"],
                           c["step"], c["min_weight"])


def test_threshold_scene_hits_every_case():
    vol, r = th_cast("main")
    d, hn, en, nrm = r["depth"], r["hit_n"], r["exit_n"], r["normal"]
    assert (hn[0] == 4).all() and (d[0] == F(2)).all() and r["redefined"][0].all()                      # (a): t = 1, Z* = Z_4 = 2
    assert (nrm[0, 2] == F(-1)).all() and not nrm[0, :2].any()                                          # G = (0, 0, -1 / 8) exactly
    assert r["colour"][0][:, 8:].any() and not r["colour"][0][:, 0].any()                               # gx < 2 at column 0: no corner has colour
    assert (hn[1] == 4).all() and (d[1] < F(2)).all() and (d[1] > F(2) - F(1e-5)).all()                  # (b): f_4 < 0, t < 1
    mid = (slice(2, ROWS - 2), slice(2, COLS - 2))          # at Z_5 the outermost rays have left the volume sideways
    assert (hn[2][mid] == 5).all() and (np.abs(d[2][mid] - F(2)) < F(1e-5)).all() and (hn[2][0] == -1).all() and set(np.unique(hn[2])) == {-1, 5}
    assert (hn[3][:, 0] == 4).all() and (hn[4][:, 0] == -1).all() and (hn[4][:, 1] == 4).all()           # (c)
    assert np.isnan(d[4][:, 0]).all() and d[4].view(np.uint32)[0, 0] == RM.NAN_BITS
    assert (hn[5][:, 63] == -1).all() and (hn[5][:, 62] == 4).all() and (hn[6][:, 63] == 4).all()         # (d): the domain is half-open
    for v in (7, 8):                                                                                    # (e): nobody hits, everybody exits
        assert (hn[v] == -1).all() and (en[v][mid] == 5).all() and set(np.unique(en[v])) == {-1, 5} and np.isnan(d[v]).all() and np.isnan(nrm[v]).all() and not r["colour"][v].any()
    assert (hn[9] == -1).all() and (en[9] == 1).all()                                                    # (f)
    # every view alone gives the planes it has in the common call
    for v in range(len(TH_MAIN)):
        one = th_cast("main", [v])[1]
        assert all(one[k][0].tobytes() == r[k][v].tobytes() for k in ("depth", "normal", "colour"))
    vol, r = th_cast("weight")                                                                          # (g)
    hit = r["hit_n"][0] == 4
    assert hit.any() and not hit.all() and (r["hit_n"][0][~hit] == -1).all()
    assert hit.sum() < (th_cast("main", [0])[1]["hit_n"][0] == 4).sum()
    vol, r = th_cast("holes")                                                                           # (h)
    a, b = RM.rays(vol, RM.pose_wc(np.eye(3), (0, 0, 0)), TH_K, ROWS, COLS)
    gx1 = (a[0] + F(1.625) * b[0]).reshape(ROWS, COLS)          # sample 1 lies on the plane k = 1: its cell touches the first hole
    through = (np.floor(gx1) >= 2) & (np.floor(gx1) <= 4)
    assert through.any() and (r["hit_n"][0][through] == 4).all()                                        # the pair (0, 1) is broken, (3, 4) hits
    gx3 = (a[0] + F(1.875) * b[0]).reshape(ROWS, COLS)
    lost = (np.floor(gx3) >= 10) & (np.floor(gx3) <= 12)
    assert lost.any() and (r["hit_n"][0][lost] == -1).all() and (r["exit_n"][0][lost] == -1).all()       # sample 3 undefined: no pair at 4
    vol, r = th_cast("zmax_on")                                                                         # (i)
    assert RM.last_step(1.5, 2.0, 0.125) == 4 and (r["hit_n"][0] == 4).all()
    assert (r["hit_n"][1] == -1).all() and (r["exit_n"][1] == -1).all()                                  # (e): ended on the last n, no exit
    vol, r = th_cast("zmax_below")
    assert RM.last_step(1.5, 2.0 - 2.0 ** -23, 0.125) == 3 and (r["hit_n"][0] == -1).all()
    vol, r = th_cast("resample")                                                                        # (j): it can be built
    lone = (r["hit_n"][0] >= 0) & ~r["redefined"][0]
    assert lone.any() and (r["hit_n"][0] >= 0).sum() > lone.sum()
    assert np.isfinite(r["depth"][0][lone]).all() and np.isnan(r["normal"][0][:, lone]).all() and not r["colour"][0][lone].any()


# ---- mirror against the scalar loops ----------------------------------------------------------------------------------------------------
def test_mirror_equals_the_scalar_loop():
    vol = mixed_state()
    R = np.stack([np.eye(3), BACK])
    t = np.array([[0.0, 0.0, 0.0], [0.1, -0.05, 3.4]])       # the second looks back at the surface from behind
    Ks = (15.0, 14.5, 7.5, 5.5)                              # the mixed scene's camera at a quarter of its size
    for mw in (1, 2):
        r = RM.raycast(vol, R, t, Ks, 12, 16, 0.3, 5.0, 0.05, mw)
        depth, normal, colour = RM.raycast_loop(vol, R, t, Ks, 12, 16, 0.3, 5.0, 0.05, mw)
        assert r["depth"].tobytes() == depth.tobytes() and r["normal"].tobytes() == normal.tobytes() and r["colour"].tobytes() == colour.tobytes()
        hits = np.isfinite(r["depth"]).reshape(2, -1).sum(1)
        print(f"mixed volume, min_weight {mw}: {hits[0]} and {hits[1]} hits of 192 pixels, {(r['exit_n'][1] >= 0).sum()} exits from behind")
        assert hits[0] > 40 and (r["exit_n"][1] >= 0).sum() > 40 and r["colour"][0].any()
    assert hits[0] < np.isfinite(RM.raycast(vol, R, t, Ks, 12, 16, 0.3, 5.0, 0.05, 1)["depth"][0]).sum()      # min_weight decides


def test_sphere_depth_and_normals():
    """the figures of DESIGN.md section 20: 616 hits, exactly the pixels whose analytic ray meets the sphere; the largest |depth - analytic|
    0.0337 m (at grazing rays), the median 0.0023 m; the smallest cosine between normal and radial direction 0.99569"""
    vol = sphere_volume()
    cam = SPHERE_CAM
    r = RM.raycast(vol, cam["R"], cam["t"], cam["K"], cam["rows"], cam["cols"], cam["z_min"], cam["z_max"], 0.05)
    meets, z, d = analytic_sphere()
    hit = np.isfinite(r["depth"][0])
    err = np.abs(r["depth"][0][hit] - z[hit])
    p = np.array(cam["t"]) + d[hit] * r["depth"][0][hit][:, None].astype(np.float64)
    radial = (p - SPHERE["centre"]) / np.linalg.norm(p - SPHERE["centre"], axis=1)[:, None]
    world = r["normal"][0][:, hit].T.astype(np.float64)      # R = I: the camera frame is the world frame
    cos = (world * radial).sum(1)
    print(f"sphere: {hit.sum()} hits, {meets.sum()} analytic, largest |depth - analytic| {err.max():.4f} m, median {np.median(err):.4f} m, "
          f"smallest cosine {cos.min():.5f}")
    assert np.array_equal(hit, meets) and hit.sum() == 616
    assert err.max() < float(vol.voxel) and cos.min() > 0.99
    assert r["redefined"][0][hit].all() and (world[:, 2] < 0).all()                                     # the normals look at the camera
    coarse = RM.raycast(vol, cam["R"], cam["t"], cam["K"], cam["rows"], cam["cols"], cam["z_min"], cam["z_max"], 0.3)
    assert np.isfinite(coarse["depth"]).sum() < meets.sum()                                             # a step above the band may miss


def test_wall_depth_and_normal():
    R, t, planes, colours, Kw = wall_scene()
    vol = TM.Volume(25, 13, 17, (-0.6, -0.3, 1.62), 0.05, 0.15)
    TM.integrate(vol, planes, colours, R, t, Kw, **GATE)
    r = RM.raycast(vol, R, t, Kw, 24, 32, 0.3, 5.0, 0.05)
    # Bound on |depth - 2|, u = 2^-24, h = 0.05.  A hit's two samples lie within h of the wall, their cells' corners within 2 h < trunc:
    # every camera added d = s = 2 - z_k there, so (tests/test_cpu_tsdf.py) |D_k - (2 - z_k)| <= 2 u |s| <= 0.3 u with z_k the float32
    # centre, which is within 3 u of the real o_z + k h (product 0.85 u, sum 2 u).  R = I, t_z = 0: the sample's real depth is Z_n.  Its
    # position in voxels, a_z + Z b_z, carries u |a_z| from the division (32.4 u), 2 u |Z b_z| from b_z and the product (100 u), half an
    # ulp of the product (32 u) and of the sum (16 u): 180.4 u voxels = 9.1 u metres.  The seven lerps of step 16 round 3 times each at
    # values <= 0.15: 3.2 u.  So |f_n - (2 - Z_n)| <= e = (3.3 + 9.1 + 3.2) u = 15.6 u.  D is linear in z there, so the exact crossing of
    # the exact f is at depth 2; t = f_a / (f_a - f_b) with f_a - f_b = h carries e (|f_a| + |f_b|) / h^2 = e / h = 312 u, and 2 u from
    # its difference and division; times Z_n - Z_{n-1} = h (exact by Sterbenz): 15.7 u; the product rounds by 0.05 u and the sum lands
    # next to 2, where half an ulp is at most 2 u: 17.8 u < 20 u.
    bound = 20 * U
    # Normal: G_z = Ly_1 - Ly_0 = -h and G_x = G_y = 0 up to twice (3.3 u + 3.2 u) = 13 u each; over L >= h - 13 u that is 260 u per
    # component, the divisions and the (exact) rotation add less than 2 u: 300 u.
    nbound = 300 * U
    for v in range(3):
        hit = np.isfinite(r["depth"][v])
        err = np.abs(r["depth"][v][hit].astype(np.float64) - 2.0).max()
        nerr = np.abs(r["normal"][v][:, hit].astype(np.float64) - np.array([[0.0], [0.0], [-1.0]])).max()
        print(f"wall, camera {v}: {hit.sum()} hits of 768, largest |depth - 2| = {err:.3e} (bound {bound:.3e}), normal off by {nerr:.3e} (bound {nbound:.3e})")
        assert hit.sum() > 300 and err <= bound and nerr <= nbound
        assert (r["colour"][v][hit] == np.array([200, 100, 50], np.uint8)).all() and not r["colour"][v][~hit].any()


# ---- vertex normals ---------------------------------------------------------------------------------------------------------------------
def test_vertex_normals_mirror_equals_the_scalar_loop():
    sc = mixed_scene(3)
    grid = dict(nx=7, ny=6, nz=5, origin=(-0.45, -0.35, 1.45), voxel=0.15, trunc=0.3)
    vol = TM.integrate(TM.Volume(**grid), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)
    for mw in (1, 2):
        n = RM.vertex_normals(vol, mw)
        assert len(n) == len(TM.extract(vol, mw)[0]) > 20
        assert n.tobytes() == np.array(RM.normals_loop(vol, mw), F).reshape(-1, 3).tobytes()
        L = np.linalg.norm(n.astype(np.float64), axis=1)
        assert ((np.abs(L - 1) < 1e-6) | (L == 0)).all()
    _, form = RM.voxel_gradient(vol, 1)
    _, form2 = RM.voxel_gradient(vol, 2)
    assert (form != form2).any()                                                                        # min_weight changes the form taken


def test_vertex_normals_of_the_sphere_and_the_wall():
    vol = sphere_volume()
    v, _, _ = TM.extract(vol, 1)
    n = RM.vertex_normals(vol, 1)
    radial = (v - np.array(SPHERE["centre"])) / np.linalg.norm(v - np.array(SPHERE["centre"]), axis=1)[:, None]
    cos = (n.astype(np.float64) * radial).sum(1)
    print(f"sphere: {len(n)} vertex normals, smallest cosine with the radial direction {cos.min():.5f}")
    assert len(n) == 2002 and cos.min() > 0.99991 - 0.01        # measured on the mirror: 0.99991
    # the wall of tests/test_cpu_tsdf.py: D depends on z only, so g_x = g_y = 0 exactly (equal values subtract to 0) and the normal is
    # (0, 0, -1) exactly: g_z / |g_z|
    R, t, planes, colours, Kw = wall_scene()
    wall = TM.integrate(TM.Volume(25, 13, 17, (-0.6, -0.3, 1.62), 0.05, 0.15), planes, colours, R, t, Kw, **GATE)
    inner = TM.Volume(25, 13, 17, (-0.6, -0.3, 1.62), 0.05, 0.15)
    seen = (wall.W == 3)                                       # where all three cameras agree D is a function of z alone
    inner.set_state(wall.D, np.where(seen, 3, 0).astype(np.uint32))
    n = RM.vertex_normals(inner, 3)
    a, b, _ = RM.active_edges(inner, 3)
    g, form = RM.voxel_gradient(inner, 3)
    flat = (form[:2, a] == 3).all(0) & (form[:2, b] == 3).all(0)      # both ends have both x and y neighbours
    assert flat.sum() > 100 and (n[flat] == np.array([0, 0, -1], F)).all()


def test_vertex_normals_take_the_one_sided_forms():
    """a 3 x 3 x 3 volume whose 27 values of D all differ, the centre voxel's neighbours invalidated one by one: each form per axis"""
    vol = TM.Volume(3, 3, 3, (0, 0, 0), 1.0, 2.0)
    D = np.arange(27, dtype=F).reshape(3, 3, 3) ** F(1.5) - F(40)
    c = 13                                                  # the centre voxel, linear index (1 * 3 + 1) * 3 + 1
    for axis, stride in ((0, 1), (1, 3), (2, 9)):
        for W_lo, W_hi, want, code in ((1, 1, D.reshape(-1)[c + stride] - D.reshape(-1)[c - stride], 3),
                                       (0, 1, F(2) * (D.reshape(-1)[c + stride] - D.reshape(-1)[c]), 2),
                                       (1, 0, F(2) * (D.reshape(-1)[c] - D.reshape(-1)[c - stride]), 1), (0, 0, F(0), 0)):
            W = np.ones(27, np.uint32)
            W[c - stride], W[c + stride] = W_lo, W_hi
            vol.set_state(D, W)
            g, form = RM.voxel_gradient(vol, 1)
            assert g[axis, c] == want and form[axis, c] == code, (axis, W_lo, W_hi)
            W2 = np.full(27, 2, np.uint32)                  # the same through min_weight: weight 1 no longer counts
            W2[c - stride], W2[c + stride] = 1 + W_lo, 1 + W_hi
            vol.set_state(D, W2)
            g2, form2 = RM.voxel_gradient(vol, 2)
            assert g2[axis, c] == want and form2[axis, c] == code and RM.voxel_gradient(vol, 1)[1][axis, c] == 3
    # at the volume's faces the missing neighbour is outside: one-sided without any invalid voxel
    vol.set_state(D, np.ones(27, np.uint32))
    g, form = RM.voxel_gradient(vol, 1)
    assert form[0, 12] == 2 and form[0, 14] == 1 and form[1, 10] == 2 and form[2, 22] == 1
    assert g[0, 12] == F(2) * (D.reshape(-1)[13] - D.reshape(-1)[12])


# ---- the Python checkers, one by one --------------------------------------------------------------------------------------------------
def test_step_checker():
    assert TS.step_arg(0.05, 0.3, 5.0) == float(F(0.05)) and TS.step_arg(np.float32(1.0), 1.0, 1.0) == 1.0
    assert TS.step_arg((20.0 - 0.05) / 65536 * 1.001, 0.05, 20.0) > 0
    for step, lo, hi in ((0, 0.3, 5.0), (-0.05, 0.3, 5.0), (NAN, 0.3, 5.0), (INF, 0.3, 5.0), (1e39, 0.3, 5.0), ("x", 0.3, 5.0), (None, 0.3, 5.0),
                         ((20.0 - 0.05) / 65536 * 0.999, 0.05, 20.0), (1e-6, 0.3, 5.0), (0.05, 0.0, 5.0), (0.05, 3.0, 2.0), (0.05, 0.3, INF)):
        with pytest.raises(ValueError):
            TS.step_arg(step, lo, hi)


def test_outputs_checker():
    assert TS.raycast_outputs_arg("depth") == ("depth",) and TS.raycast_outputs_arg(["normal", "colour"]) == ("normal", "colour")
    assert TS.raycast_outputs_arg(TS.RAYCAST_PLANES) == ("depth", "normal", "colour")
    for outs in ((), [], "index", ("depth", "index"), ("Depth",)):
        with pytest.raises(ValueError):
            TS.raycast_outputs_arg(outs)


def test_shade():
    n = np.full((3, 2, 3), NAN, F)
    n[:, 0, 0] = (0, 0, -1); n[:, 0, 1] = (0, 0, 1); n[:, 0, 2] = (0.6, 0, -0.8); n[:, 1, 0] = (NAN, 0, -1); n[:, 1, 1] = (0, 0, -0.5)
    assert TS.shade(n).tolist() == [[255, 0, 204], [0, 128, 0]] and TS.shade(n).dtype == np.uint8
    import torch
    assert TS.shade(torch.from_numpy(n)).tolist() == [[255, 0, 204], [0, 128, 0]]


def test_checks_come_before_the_library():
    class Ctx:
        device = 0
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels, vol.voxel = Ctx(), 2, 1000, 0.05
    good = dict(R=np.eye(3), t=np.zeros(3), K=K, rows=ROWS, cols=COLS)
    for change in (dict(z_min=0.0), dict(z_min=3.0, z_max=2.0), dict(z_max=INF), dict(K=(0, 58, 31.5, 23.5)), dict(K=(60, 58, NAN, 23.5)),
                   dict(t=[NAN, 0, 0]), dict(R=np.full((3, 3), 1e300)), dict(rows=0), dict(cols=(1 << 20) + 1), dict(rows=1 << 16, cols=1 << 15),
                   dict(R=np.zeros((0, 3, 3)), t=np.zeros((0, 3))), dict(R=np.stack([np.eye(3)] * 3), t=np.zeros((3, 3))), dict(step=0.0),
                   dict(step=NAN), dict(step=1e-5), dict(min_weight=0), dict(min_weight=65536), dict(min_weight=1.0), dict(outputs=("index",)),
                   dict(outputs=())):
        with pytest.raises(ValueError):
            vol.raycast(**dict(good, **change))
    for bad in (dict(depth=np.zeros((1, ROWS, COLS), F)), dict(normal=5), dict(colour="x")):                # planes that are no CUDA tensors
        with pytest.raises(ValueError):
            vol.raycast_into(np.eye(3), np.zeros(3), K, ROWS, COLS, 0.05, 1, 0.3, 5.0, **bad)
    vol._h = None                                           # nothing to destroy


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_raycast.c"
    src.write_text('#include "rgbid_tsdf.h"\n'
                   "int use(rgbid_tsdf* v, const rgbid_render_pose* poses, float* depth, float* normal, uint8_t* colour, float* normals) {\n"
                   "  const float K[4] = {525.f, 525.f, 319.5f, 239.5f}; float wc[12], ms[1];\n"
                   "  return rgbid_tsdf_pose_wc(poses, wc) + rgbid_tsdf_raycast(v, 16, poses, K, 480, 640, 0.05f, 20.f, 0.02f, 1u, depth, normal, colour)\n"
                   "       + rgbid_tsdf_raycast_timing(v, 1, ms) + rgbid_tsdf_extract_normals(v, normals, 1000ull) + (RGBID_TSDF_MAX_STEPS == 65536 ? 0 : 1); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_tsdf_raycast.h")).read()
    assert int(re.search(r"RGBID_TSDF_MAX_STEPS\s+(\d+)", txt).group(1)) == TS.MAX_STEPS == RM.MAX_STEPS
    assert '#include "rgbid_tsdf_raycast.h"' in open(os.path.join(ROOT, "include", "rgbid_tsdf.h")).read()


def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_library_exports_raycast_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_tsdf_raycast.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_tsdf_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(TS.RAYCAST_EXPORTS) and len(declared) == 4, set(declared) ^ set(TS.RAYCAST_EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_pose_wc_and_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    rng = np.random.default_rng(3)
    R, t = rng.normal(size=(3, 3)), rng.normal(size=3) * 1e3
    assert TS.pose_wc(R, t).tobytes() == RM.pose_wc(R, t).tobytes() == np.concatenate([R.reshape(9), t]).astype(F).tobytes()
    L.rgbid_tsdf_raycast.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_float, c.c_float, c.c_float, c.c_uint,
                                     c.c_void_p, c.c_void_p, c.c_void_p]
    L.rgbid_tsdf_raycast_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_tsdf_extract_normals.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong]
    L.rgbid_tsdf_pose_wc.argtypes = [c.c_void_p, c.c_void_p]
    pose, k, wc = TS.Pose(), (c.c_float * 4)(*K), (c.c_float * 12)()
    assert L.rgbid_tsdf_pose_wc(None, wc) == -1 and L.rgbid_tsdf_pose_wc(c.byref(pose), None) == -1
    assert L.rgbid_tsdf_raycast(None, 1, c.byref(pose), k, ROWS, COLS, 0.3, 5.0, 0.05, 1, None, None, None) == -1
    assert L.rgbid_tsdf_raycast_timing(None, 0, None) == -1 and L.rgbid_tsdf_extract_normals(None, None, 0) == -1


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-normals"], "need --mesh"), (["--mesh-render", str(tmp_path / "v")], "need --mesh"), (["--mesh-render-check"], "need --mesh"),
                      (["--mesh-render-step", "0.05"], "need --mesh"), (mesh + ["--mesh-render-step", "0.05"], "needs --mesh-render or --mesh-render-check"),
                      (mesh + ["--mesh-render-check", "--mesh-render-step", "0"], "step must be > 0"),
                      (mesh + ["--mesh-render", str(tmp_path / "v"), "--mesh-render-step", "nan"], "step must be finite"),
                      (mesh + ["--mesh-render-check", "--mesh-render-step", "1e-5"], "more than 65536 samples")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists() and not (tmp_path / "v").exists()


def test_mesh_ply_with_normals_is_parsed_back():
    vol = sphere_volume()
    v, c, tr = TM.extract(vol, 1)
    n = RM.vertex_normals(vol, 1)
    data = TS.mesh_ply_bytes(v, c, tr, n)
    head = data[:data.index(b"end_header\n")].decode("ascii").split("\n")
    assert head.index("property float z") + 1 == head.index("property float nx") and head.index("property float nz") + 1 == head.index("property uchar red")
    assert len(data) == data.index(b"end_header\n") + 11 + 2002 * 27 + 4000 * 13
    pv, pc, pt, pn = TS.read_mesh_ply(data)
    assert pv.tobytes() == v.tobytes() and pc.tobytes() == c.tobytes() and pt.tobytes() == tr.tobytes() and pn.tobytes() == n.tobytes()
    import torch
    assert TS.mesh_ply_bytes(torch.from_numpy(v), torch.from_numpy(c), torch.from_numpy(tr.view(np.int32)), torch.from_numpy(n)) == data
    # without normals the file is what it was: no normal property, 15 bytes per vertex, three planes read back
    plain = TS.mesh_ply_bytes(v, c, tr)
    assert plain == TS.mesh_ply_bytes(v, c, tr, None) and b"property float nx" not in plain
    assert len(plain) == plain.index(b"end_header\n") + 11 + 2002 * 15 + 4000 * 13 and len(TS.read_mesh_ply(plain)) == 3
    want = ("ply\nformat binary_little_endian 1.0\ncomment rgbid fused keyframe mesh\nelement vertex 2002\nproperty float x\nproperty float y\n"
            "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 4000\n"
            "property list uchar uint vertex_indices\nend_header\n")
    assert plain.startswith(want.encode("ascii"))
