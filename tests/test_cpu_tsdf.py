"""CPU checks of the TSDF volume (include/rgbid_tsdf.h, rgbid.tsdf): the numpy restatement the GPU tests compare the kernels against
(tests/tsdf_mirror.py) against the plain scalar loops of the contract; the case table re-derived from its orientation rule; a sphere whose
mesh must be closed, consistently oriented and of the right volume; a wall whose weights and vertex positions are derived by hand; the
threshold scene of the GPU tests; the Python argument checks one by one; the header as C99; the library's exports; refusals that need no
device; the command line's option errors; the PLY writer."""
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
from tests import tsdf_mirror as TM
from tests.test_cpu_consist import COLS, K, ROWS, cameras, surface_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32
GATE = dict(z_min=0.3, z_max=5.0)
# 24 x 20 x 16 voxels of 0.05 m around the surface of tests/test_cpu_consist.py: unequal dimensions expose an index transposition
MIXED = dict(nx=24, ny=20, nz=16, origin=(-0.575, -0.475, 1.425), voxel=0.05, trunc=0.15)
SPHERE = dict(centre=(0.6, 0.5, 0.4), radius=0.3)
HALF = 524288                           # 128 x 64 x 64: one full grid of the strided kernels; its 7 flags per voxel are 1 792 compaction tiles


def mixed_volume(**kw):
    return TM.Volume(**dict(MIXED, **kw))


@functools.lru_cache(maxsize=None)
def mixed_scene(V):
    """V cameras that see the smooth surface through the mixed volume, planes with every kind of hole, random colours"""
    rng = np.random.default_rng(700 + V)
    R, t = cameras(rng, V)
    planes = surface_planes(rng, R, t)
    colours = rng.integers(0, 256, (V, ROWS, COLS, 3), dtype=np.uint8)
    return dict(R=R, t=t, planes=planes, colours=colours)


def sphere_volume(nx=24, ny=20, nz=16):
    vol = TM.Volume(nx, ny, nz, (0.0, 0.0, 0.0), 0.05, 0.2)
    vol.set_state(*TM.sphere_state(vol, **SPHERE))
    return vol


def large_volume(nx):
    """nx x 64 x 64 voxels of 0.02 m around the surface (nx = 128: exactly one grid of 2 048 x 256 threads; 129: one more row)"""
    return TM.Volume(nx, 64, 64, (-1.27, -0.63, 1.2), 0.02, 0.08)


@functools.lru_cache(maxsize=None)
def large_scene():
    rng = np.random.default_rng(710)
    R, t = cameras(rng, 3)
    return dict(R=R, t=t, planes=surface_planes(rng, R, t), colours=rng.integers(0, 256, (3, ROWS, COLS, 3), dtype=np.uint8))


def assert_every_third_has_work(vol, verts, tris):
    """a trip of the stride or of the scan that did nothing must not pass: each third of the volume (in linear order) holds touched voxels,
    vertices and triangles"""
    n, W = vol.n, vol.W.reshape(-1)
    z = np.asarray(verts)[:, 2]
    cz = vol.centres()[2]
    tz = z[np.asarray(tris, np.int64)[:, 0]]
    for a in range(3):
        lo, hi = a * n // 3, (a + 1) * n // 3
        zlo, zhi = cz[lo // (vol.nx * vol.ny)], cz[(hi - 1) // (vol.nx * vol.ny)]
        assert (W[lo:hi] > 0).sum() > 1000, (a, int((W[lo:hi] > 0).sum()))
        assert ((z >= zlo) & (z <= zhi)).sum() > 100 and ((tz >= zlo) & (tz <= zhi)).sum() > 100, a


# ---- the threshold scene: identity cameras, a constant plane, voxel centres and shifts that are exact in float32 -----------------------
TH_K = (64.0, 64.0, 31.5, 23.5)          # u + 0.5 = 32 X / (Z / 2) + 32: at Z = 2 the image spans X in [-1, 1), Y in [-0.75, 0.75)
TH_GRID = dict(nx=17, ny=13, nz=9, origin=(-1.0, -0.75, 1.5), voxel=0.125, trunc=0.125)   # centres: multiples of 1 / 8; z = 1.5 .. 2.5
TH_GATE = dict(z_min=1.5, z_max=2.5)
U22, U23, U20 = 2.0 ** -22, 2.0 ** -23, 2.0 ** -20
# camera-frame shifts t_CW (Z = z + tz, X = x + tx exactly): the plane measures 2 m, so s = 2 - Z
TH_SHIFTS = [(0, 0, 0), (0, 0, 0.125), (0, 0, 0.125 + U22), (0, 0, 0.125 - U22), (0, 0, -0.125), (0, 0, -0.125 - U23), (0, 0, -0.125 + U23),
             (0, 0, -U23), (0, 0, U22), (-U20, 0, 0), (U20, 0, 0), (0, -U20, 0), (0, U20, 0), (0, 0, 0)]
TH_FAR = (7, 8, 13)                      # these views measure 4 m instead: nothing is hidden, so that only the depth gate decides


def threshold_scene():
    V = len(TH_SHIFTS)
    R = np.stack([np.eye(3)] * V)
    t = -np.array(TH_SHIFTS, np.float64)                   # R = I: t_CW = -t_WC
    planes = np.full((V, ROWS, COLS), 0.5, F)
    planes[list(TH_FAR)] = 0.25
    colours = np.random.default_rng(5).integers(1, 256, (V, ROWS, COLS, 3), dtype=np.uint8)
    return dict(R=R, t=t, planes=planes, colours=colours)


def test_threshold_scene_hits_every_case():
    sc = threshold_scene()
    def one(v):
        vol = TM.Volume(**TH_GRID)
        TM.integrate(vol, sc["planes"][v:v + 1], sc["colours"][v:v + 1], sc["R"][v:v + 1], sc["t"][v:v + 1], TH_K, **TH_GATE)
        return vol
    mid = (4, 6, 8)                                        # the voxel at (0, 0, 2)
    v = one(0); assert v.W[mid] == 1 and v.D[mid] == 0 and v.Cn[mid] == 1
    assert v.W[4, 6, 0] == 1 and v.W[4, 6, 16] == 0        # pu = 0 is inside, pu = 64 is not
    assert v.W[4, 0, 8] == 1 and v.W[4, 12, 8] == 0        # pv = 0 is inside, pv = 48 is not
    v = one(1); assert v.W[mid] == 1 and v.D[mid] == F(-0.125) and v.Cn[mid] == 1      # s = -trunc: not hidden, coloured
    v = one(2); assert v.W[mid] == 0                                                   # one ulp behind: hidden
    v = one(3); assert v.W[mid] == 1 and v.D[mid] == F(-0.125 + U22) and v.Cn[mid] == 1
    v = one(4); assert v.W[mid] == 1 and v.D[mid] == F(0.125) and v.Cn[mid] == 1       # s = +trunc: coloured
    v = one(5); assert v.W[mid] == 1 and v.D[mid] == F(0.125) and v.Cn[mid] == 0       # one ulp more: truncated, no colour
    v = one(6); assert v.W[mid] == 1 and v.D[mid] == F(0.125 - U23) and v.Cn[mid] == 1
    v = one(7); assert v.W[0, 6, 8] == 0 and v.W[1, 6, 8] == 1                         # Z one ulp below z_min
    v = one(8); assert v.W[8, 6, 8] == 0 and v.W[0, 6, 8] == 1                         # Z one ulp above z_max
    v = one(9); assert v.W[4, 6, 0] == 0 and v.W[4, 6, 16] == 1                        # X a little smaller: pu = -1 and pu = 63
    v = one(10); assert v.W[4, 6, 0] == 1 and v.W[4, 6, 16] == 0
    v = one(11); assert v.W[4, 0, 8] == 0 and v.W[4, 12, 8] == 1                       # Y a little smaller: pv = -1 and pv = 47
    v = one(12); assert v.W[4, 0, 8] == 1 and v.W[4, 12, 8] == 0
    v = one(13); assert v.W[0, 6, 8] == 1 and v.W[8, 6, 8] == 1 and v.D[8, 6, 8] == F(0.125)   # Z = z_min and Z = z_max pass the gate


# ---- mirror against the scalar loops ----------------------------------------------------------------------------------------------------
def test_mirror_equals_the_scalar_loop():
    rng = np.random.default_rng(41)
    R, t = cameras(rng, 3)
    planes = surface_planes(rng, R, t)
    colours = [rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8), None, rng.integers(0, 256, (ROWS, COLS, 3), dtype=np.uint8)]
    grid = dict(nx=7, ny=6, nz=5, origin=(-0.45, -0.35, 1.45), voxel=0.15, trunc=0.3)
    a, b = TM.Volume(**grid), TM.Volume(**grid)
    TM.integrate(a, planes, colours, R, t, K, **GATE)
    TM.integrate_loop(b, planes, colours, R, t, K, **GATE)
    assert a.state_bytes() == b.state_bytes()
    assert a.W.max() == 3 and (a.W == 0).any() and a.Cn.max() == 2 and (a.D < 0).any() and (a.D > 0).any()
    for mw in (1, 2):
        v, c, tr = TM.extract(a, mw)
        lv, lc, lt = TM.extract_loop(a, mw)
        assert len(v) > 20 and len(tr) > 20
        assert v.tobytes() == np.array(lv, F).reshape(-1, 3).tobytes() and c.tolist() == lc and tr.tolist() == lt
    assert c.any()


def test_case_table_follows_from_the_orientation_rule():
    assert np.array_equal(TM.derive_swap(), TM.SWAP) and TM.SWAP.shape == (6, 16)
    assert [len(TM.case_rows(m)) for m in range(16)] == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
    # the kernel holds the table as one 16-bit mask per tetrahedron (bit = case)
    src = open(os.path.join(ROOT, "rgbid-slam_amd", "csrc", "kernels_tsdf.hip")).read()
    masks = [int(x, 16) for x in re.search(r"TET_SWAP\[6\] = \{([^}]*)\}", src).group(1).split(",")]
    assert masks == [sum(int(TM.SWAP[t, m]) << m for m in range(16)) for t in range(6)]
    corners = re.search(r"TET_CORNER\[6\]\[4\] = \{(.*?)\};", src).group(1)
    assert tuple(tuple(int(x) for x in g.split(",")) for g in re.findall(r"\{([^{}]*)\}", corners)) == TM.TETS
    # the six tetrahedra are the monotone paths, and they fill the cell: every path's volume is 1 / 6
    for tet in TM.TETS:
        P = np.array([TM.offset(c) for c in tet])
        assert abs(np.linalg.det(P[1:] - P[0])) == 1 and all(bin(b ^ a).count("1") == 1 and b > a for a, b in zip(tet, tet[1:]))


def test_sphere_mesh_is_closed_oriented_and_of_the_right_volume():
    vol = sphere_volume()
    v, c, tr = TM.extract(vol, 1)
    edges, two, repeated = TM.mesh_topology(tr)
    assert (len(v), edges, len(tr)) == (2002, 6000, 4000) and two == edges       # every undirected edge in exactly two triangles
    assert repeated == 0                                                         # every directed edge once: consistently oriented
    assert len(v) - edges + len(tr) == 2
    assert not c.any()                                                           # no colour was integrated
    # Every vertex lies on a lattice edge whose ends are on either side of the sphere: within one cell diagonal, sqrt(3) voxel, of
    # the sphere (the interpolated D is exact to first order only, the edge's ends bound it).  The mesh is a closed surface inside the shell
    # between the radii r -+ sqrt(3) voxel, so its volume lies between the volumes of the two balls.
    vol_mesh = TM.signed_volume(v, tr)
    r, h = SPHERE["radius"], float(vol.voxel)
    lo, hi = 4 / 3 * np.pi * (r - 3 ** 0.5 * h) ** 3, 4 / 3 * np.pi * (r + 3 ** 0.5 * h) ** 3
    print(f"sphere: {len(v)} vertices, {len(tr)} triangles, volume {vol_mesh:.5f} (analytic {4 / 3 * np.pi * r ** 3:.5f}, shell {lo:.5f} .. {hi:.5f})")
    assert 0 < lo < vol_mesh < hi
    dist = np.linalg.norm(v.astype(np.float64) - np.array(SPHERE["centre"]), axis=1)
    assert (np.abs(dist - r) <= 3 ** 0.5 * h).all()


def test_min_weight_decides_validity():
    vol = sphere_volume()
    vol.W[:, :, :12] = 2                                    # the half x < 0.6 has weight 2
    v1, _, t1 = TM.extract(vol, 1)
    v2, _, t2 = TM.extract(vol, 2)
    assert len(t1) == 4000 and 0 < len(t2) < 2000 and len(v2) < len(v1) and (v2[:, 0] <= 0.55 + 1e-6).all()
    assert TM.mesh_topology(t2)[1] < TM.mesh_topology(t2)[0]        # open along the cut
    v3, _, t3 = TM.extract(vol, 3)
    assert len(v3) == 0 and len(t3) == 0 and t3.shape == (0, 3)


def wall_scene():
    """three identity-rotation cameras, translated in x and y only, before a wall at z = 2 (iD = 0.5 everywhere) in images of 24 x 32"""
    R = np.stack([np.eye(3)] * 3)
    t = np.array([[0, 0, 0], [0.25, 0, 0], [-0.125, 0.0625, 0]], np.float64)
    planes = np.full((3, 24, 32), 0.5, F)
    colours = np.full((3, 24, 32, 3), (200, 100, 50), np.uint8)
    return R, t, planes, colours, (60.0, 58.0, 15.5, 11.5)


def test_wall():
    R, t, planes, colours, Kw = wall_scene()
    vol = TM.Volume(25, 13, 17, (-0.6, -0.3, 1.62), 0.05, 0.15)
    TM.integrate(vol, planes, colours, R, t, Kw, **GATE)
    x, y, z = (c.astype(np.float64) for c in vol.centres())
    # W = the cameras that see the voxel, from the projection in float64 (voxels within 1e-3 pixels of an image border are left out:
    # there the float32 rounding decides), and 0 for every voxel more than trunc behind the wall
    seen = np.zeros(vol.shape, np.int64); sure = np.ones(vol.shape, bool)
    for v in range(3):
        u = Kw[0] * (x[None, None, :] - t[v, 0]) / z[:, None, None] + Kw[2] + 0.5 + 0 * y[None, :, None]
        w = Kw[1] * (y[None, :, None] - t[v, 1]) / z[:, None, None] + Kw[3] + 0.5 + 0 * x[None, None, :]
        seen += (u >= 0) & (u < 32) & (w >= 0) & (w < 24)
        sure &= (np.abs(u) > 1e-3) & (np.abs(u - 32) > 1e-3) & (np.abs(w) > 1e-3) & (np.abs(w - 24) > 1e-3)
    behind = (z > 2 + float(vol.trunc) + 1e-6)[:, None, None] & np.ones(vol.shape, bool)
    front = (z < 2 + float(vol.trunc) - 1e-6)[:, None, None] & np.ones(vol.shape, bool)
    assert behind.any() and not vol.W[behind].any()
    assert np.array_equal(vol.W[front & sure], seen[front & sure]) and set(np.unique(seen[front & sure])) == {0, 1, 2, 3}
    near = (np.abs(z - 2) < float(vol.trunc) - 1e-6)[:, None, None] & np.ones(vol.shape, bool)
    assert np.array_equal(vol.Cn[near], vol.W[near]) and not vol.Cn[front & ~near].any() and vol.W[front & ~near].any()   # colour within trunc only
    v, c, tr = TM.extract(vol, 1)
    # Bound on |z_vertex - 2|, u = 2^-24.  R = I and t_z = 0 give Z = z exactly; z_m = 1 / 0.5 = 2 exactly; s = fl(2 - z) is exact
    # (Sterbenz: z in [1, 4]).  An active edge joins z_a > 2 (inside) and z_b = z_a - voxel < 2: |s| <= voxel < trunc at both ends, no
    # truncation, so every camera adds d = s and step 7 gives D = s for W = 1, 2 and fl(fl(3 s) / 3) for W = 3: |D - s| <= 2 u |s|.
    # t = D_a / (D_a - D_b) then carries 2 u |D_a| |D_b| 2 / (D_a - D_b)^2 <= u from the two D (|D_a| |D_b| <= voxel^2 / 4), u from the
    # difference and u from the division: |t - t*| <= 3 u, where z_a + t* (z_b - z_a) = 2.  z_b - z_a is exact (Sterbenz), the product
    # rounds by at most u voxel, and the final sum lands next to 2 where half an ulp is at most 2^-23.
    bound = 2.0 ** -23 + 4 * 2.0 ** -24 * float(vol.voxel)
    err = np.abs(v[:, 2].astype(np.float64) - 2.0).max()
    print(f"wall: {len(v)} vertices, {len(tr)} triangles, largest |z - 2| = {err:.3e} (bound {bound:.3e})")
    assert len(v) > 200 and len(tr) > 300 and err <= bound
    assert (c == np.array([200, 100, 50], np.uint8)).all()
    nrm = np.cross(v[tr[:, 1]] - v[tr[:, 0]], v[tr[:, 2]] - v[tr[:, 0]])
    assert (nrm[:, 2] < 0).all()                                   # inside is behind the wall: the normals look at the cameras


def test_integrating_in_pieces_equals_integrating_at_once():
    sc = mixed_scene(19)
    cols = list(sc["colours"]); cols[2] = None; cols[17] = None
    whole = TM.integrate(mixed_volume(), sc["planes"], cols, sc["R"], sc["t"], K, **GATE)
    parts = mixed_volume()
    for a, b in ((0, 1), (1, 7), (7, 19)):
        TM.integrate(parts, sc["planes"][a:b], cols[a:b], sc["R"][a:b], sc["t"][a:b], K, **GATE)
    assert whole.state_bytes() == parts.state_bytes()
    assert whole.W.max() >= 10 and (whole.W == 0).any() and (whole.Cn < whole.W).any() and whole.Cn.max() >= 8
    # order matters: the running mean of step 7 does not commute
    swapped = TM.integrate(mixed_volume(), sc["planes"][::-1], cols[::-1], sc["R"][::-1], sc["t"][::-1], K, **GATE)
    assert np.array_equal(swapped.W, whole.W) and np.array_equal(swapped.rgb, whole.rgb) and swapped.D.tobytes() != whole.D.tobytes()
    v, c, tr = TM.extract(whole, 2)
    edges, two, repeated = TM.mesh_topology(tr)
    print(f"mixed volume, 19 views: {int((whole.W > 0).sum())} of {whole.n} voxels touched, {len(v)} vertices, {len(tr)} triangles, "
          f"{two} of {edges} edges in two triangles")
    assert len(v) > 500 and len(tr) > 800 and repeated == 0 and c.any()


def test_state_round_trip():
    sc = mixed_scene(3)
    a = TM.integrate(mixed_volume(), sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)
    b = mixed_volume()
    b.set_state(a.D, a.counts(), a.rgb)
    assert a.state_bytes() == b.state_bytes() and np.array_equal(a.W, b.W) and np.array_equal(a.Cn, b.Cn)
    b.set_state(a.D, np.full(a.shape, 0xFFFFFFFF, np.uint32))
    assert (b.W == 65535).all() and (b.Cn == 65535).all() and not b.rgb.any()
    TM.integrate(b, sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)     # a full weight takes nothing more
    assert b.D.tobytes() == a.D.tobytes() and (b.W == 65535).all()
    b.reset()
    assert not b.D.any() and not b.W.any() and not b.Cn.any() and not b.rgb.any()


def test_large_volumes_have_work_in_every_third():
    sc = large_scene()
    for nx in (128, 129):
        vol = large_volume(nx)
        assert (vol.n == HALF) == (nx == 128)
        TM.integrate(vol, sc["planes"], sc["colours"], sc["R"], sc["t"], K, **GATE)
        v, c, tr = TM.extract(vol, 1)
        print(f"{nx} x 64 x 64, 3 views: {int((vol.W > 0).sum())} voxels touched, {len(v)} vertices, {len(tr)} triangles")
        assert_every_third_has_work(vol, v, tr)


# ---- the Python checkers, one by one --------------------------------------------------------------------------------------------------
def test_capacity_checker():
    assert TS.capacity_arg(8, 1) == (8, 1) and TS.capacity_arg(1 << 29, np.int32(65535)) == (1 << 29, 65535)
    for n, v in ((7, 1), ((1 << 29) + 1, 1), (8, 0), (8, 65536), (8.0, 1), (8, "1"), (None, 1), (True, 1)):
        with pytest.raises(ValueError):
            TS.capacity_arg(n, v)


def test_grid_checker():
    good = dict(nx=24, ny=20, nz=16, origin=(0, 0, 0), voxel=0.05, trunc=0.2)
    assert TS.grid_arg(**good) == (24, 20, 16, [0.0, 0.0, 0.0], float(F(0.05)), float(F(0.2)))
    assert TS.grid_arg(**dict(good, nx=2, ny=2, nz=2), max_voxels=8)[:3] == (2, 2, 2)
    for change in (dict(nx=1), dict(ny=1), dict(nz=1), dict(nx=2.0), dict(nz=None), dict(voxel=0), dict(voxel=-0.05), dict(voxel=NAN), dict(voxel=INF),
                   dict(trunc=0), dict(trunc=-1), dict(trunc=NAN), dict(trunc=1e39), dict(origin=(0, 0)), dict(origin=(0, NAN, 0)),
                   dict(origin=(INF, 0, 0)), dict(origin=5), dict(origin=("a", 0, 0)), dict(voxel="x"), dict(max_voxels=24 * 20 * 16 - 1)):
        with pytest.raises(ValueError):
            TS.grid_arg(**dict(good, **change))


def test_weight_checker():
    assert [TS.weight_arg(w) for w in (1, 65535, np.int64(3))] == [1, 65535, 3]
    for w in (0, 65536, -1, 1.0, "1", None, True):
        with pytest.raises(ValueError):
            TS.weight_arg(w)


def test_colours_checker_needs_cuda_uint8_planes_of_the_image_size():
    import torch
    assert TS.colours_arg(None, 3, ROWS, COLS) == [None, None, None] and TS.colours_arg([None, None], 2, ROWS, COLS) == [None, None]
    good = torch.zeros((ROWS, COLS, 3), dtype=torch.uint8)
    for colours, V in (([good], 1),                         # a host tensor
                       ([good.numpy()], 1), ([], 1), (5, 1), ([None], 2), ([good.to(torch.float32)], 1)):
        with pytest.raises(ValueError):
            TS.colours_arg(colours, V, ROWS, COLS)


def test_bounds_grid():
    assert TS.bounds_grid((0, 0, 0, 1, 0.5, 0.25), 0.25) == (5, 3, 2, [0.0, 0.0, 0.0])
    assert TS.bounds_grid((-1, -1, -1, -1, -1, -1), 0.1) == (2, 2, 2, [-1.0, -1.0, -1.0])      # a point still gets a volume
    with pytest.raises(ValueError) as e:
        TS.bounds_grid((0, 0, 0, 10, 10, 10), 0.01, 1 << 27)
    m = re.search(r"a voxel of ([0-9.e+-]+) m would fit", str(e.value))
    assert m and "more than 134217728" in str(e.value)
    fit = float(m.group(1))
    assert 0.01 < fit < 0.03 and np.prod(TS.bounds_grid((0, 0, 0, 10, 10, 10), fit * 1.001, 1 << 27)[:3]) <= 1 << 27
    for b, h in (((0, 0, 0, 1, 1), 0.1), ((0, 0, 0, -1, 1, 1), 0.1), ((0, 0, NAN, 1, 1, 1), 0.1), ((0, 0, 0, 1, 1, INF), 0.1), ("abc", 0.1),
                 ((0, 0, 0, 1, 1, 1), 0), ((0, 0, 0, 1, 1, 1), -1), ((0, 0, 0, 1, 1, 1), NAN), (None, 0.1)):
        with pytest.raises(ValueError):
            TS.bounds_grid(b, h)


def test_checks_come_before_the_library():
    for n, v in ((7, 1), (8, 0), ((1 << 29) + 1, 4)):
        with pytest.raises(ValueError):
            TS.Volume(None, n, v)
    with pytest.raises(ValueError):
        TS.fuse(None, [], K, ROWS, COLS, bounds=(0, 0, 0, 1, 1, 1))
    kf = [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)]
    for change in (dict(min_weight=0), dict(bounds=None), dict(bounds=(0, 0, 0, 1, 1)), dict(voxel=-1.0), dict(trunc=0.0), dict(trunc=NAN),
                   dict(voxel=0.001, max_voxels=1 << 20)):
        with pytest.raises(ValueError):
            TS.fuse(None, kf, K, ROWS, COLS, **dict(dict(bounds=(0, 0, 0, 1, 1, 1)), **change))

    class Ctx:                                              # integrate's own checks need no library either
        device = 0
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels = Ctx(), 2, 1000
    good = dict(planes=[], colours=None, R=np.eye(3), t=np.zeros(3), K=K, rows=ROWS, cols=COLS)
    for change in (dict(z_min=0.0), dict(z_min=3.0, z_max=2.0), dict(z_max=INF), dict(K=(0, 58, 31.5, 23.5)), dict(K=(60, 58, NAN, 23.5)),
                   dict(t=[NAN, 0, 0]), dict(R=np.full((3, 3), 1e300)), dict(rows=0), dict(cols=(1 << 20) + 1),
                   dict(R=np.zeros((0, 3, 3)), t=np.zeros((0, 3))), dict(R=np.stack([np.eye(3)] * 3), t=np.zeros((3, 3))), dict(planes=[]),
                   dict(planes=[np.zeros((ROWS, COLS), F)])):
        with pytest.raises(ValueError):
            vol.integrate(**dict(good, **change))
    for w in (0, 65536):
        with pytest.raises(ValueError):
            vol.extract(w)
    with pytest.raises(ValueError):
        vol.configure(1, 2, 2, (0, 0, 0), 0.1, 0.4)
    with pytest.raises(ValueError):
        vol.configure(10, 10, 11, (0, 0, 0), 0.1, 0.4)     # above the capacity
    vol._h = None                                           # nothing to destroy


# ---- the boundary -----------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_tsdf.c"
    src.write_text('#include "rgbid_tsdf.h"\n'
                   "typedef char view_is_a_pose_and_two_pointers[sizeof(rgbid_tsdf_view) == 96 + 2 * sizeof(void*) ? 1 : -1];\n"
                   "int use(rgbid_tsdf* v, rgbid_ctx* ctx, const rgbid_tsdf_view* views, float* D, uint32_t* counts, uint32_t* rgb, float* verts,\n"
                   "        uint8_t* cols, uint32_t* tris) {\n"
                   "  const float K[4] = {525.f, 525.f, 319.5f, 239.5f}, origin[3] = {0.f, 0.f, 0.f}; float ms[3]; unsigned long long nv, nt;\n"
                   "  return rgbid_tsdf_create(&v, ctx, RGBID_TSDF_MAX_VOXELS, RGBID_TSDF_MAX_VIEWS, 1) + rgbid_tsdf_configure(v, 2, 2, 2, origin, 0.02f, 0.08f)\n"
                   "       + rgbid_tsdf_reset(v) + rgbid_tsdf_integrate(v, RGBID_TSDF_VIEW_CHUNK, views, K, 480, RGBID_TSDF_MAX_DIM, 0.05f, 20.f)\n"
                   "       + rgbid_tsdf_get_state(v, D, counts, rgb) + rgbid_tsdf_set_state(v, D, counts, rgb)\n"
                   "       + rgbid_tsdf_extract_plan(v, RGBID_TSDF_MAX_WEIGHT, &nv, &nt) + rgbid_tsdf_extract_emit(v, verts, cols, tris, nv, nt)\n"
                   "       + rgbid_tsdf_timing(v, 1, ms) + rgbid_tsdf_destroy(v); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_tsdf.h")).read()
    assert int(re.search(r"RGBID_TSDF_MAX_VOXELS\s+(\d+)ull", txt).group(1)) == TS.MAX_VOXELS == 1 << 29 and 7 * TS.MAX_VOXELS < 1 << 32
    assert int(re.search(r"RGBID_TSDF_MAX_VIEWS\s+(\d+)", txt).group(1)) == TS.MAX_VIEWS
    assert int(re.search(r"RGBID_TSDF_MAX_WEIGHT\s+(\d+)", txt).group(1)) == TS.MAX_WEIGHT == TM.MAX_W
    assert int(re.search(r"RGBID_TSDF_VIEW_CHUNK\s+(\d+)", txt).group(1)) == TS.VIEW_CHUNK
    assert ctypes.sizeof(TS.View) == 112


def test_library_exports_tsdf_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_tsdf.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_tsdf_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(TS.EXPORTS) and len(declared) == 10, set(declared) ^ set(TS.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    """argument checks come before the library touches the runtime: a null volume, a null context, capacities past the bounds"""
    L = _lib_handle()
    c = ctypes
    L.rgbid_tsdf_create.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_int, c.c_int]
    L.rgbid_tsdf_configure.argtypes = [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_float, c.c_float]
    L.rgbid_tsdf_integrate.argtypes = [c.c_void_p, c.c_int, c.c_void_p, c.c_void_p, c.c_int, c.c_int, c.c_float, c.c_float]
    L.rgbid_tsdf_get_state.argtypes = L.rgbid_tsdf_set_state.argtypes = [c.c_void_p] * 4
    L.rgbid_tsdf_extract_plan.argtypes = [c.c_void_p, c.c_uint, c.c_void_p, c.c_void_p]
    L.rgbid_tsdf_extract_emit.argtypes = [c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_ulonglong]
    L.rgbid_tsdf_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_tsdf_reset.argtypes = L.rgbid_tsdf_destroy.argtypes = [c.c_void_p]
    h = c.c_void_p()
    assert L.rgbid_tsdf_create(c.byref(h), None, 1000, 2, 1) == -1 and not h.value
    assert L.rgbid_tsdf_create(None, None, 1000, 2, 1) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for n, v in ((7, 2), ((1 << 29) + 1, 2), (1000, 0), (1000, 65536)):
        assert L.rgbid_tsdf_create(c.byref(h), fake, n, v, 1) == -1 and not h.value
    origin = (c.c_float * 3)(0, 0, 0); k = (c.c_float * 4)(*K); view = TS.View(); nv, nt = c.c_ulonglong(), c.c_ulonglong()
    assert L.rgbid_tsdf_configure(None, 2, 2, 2, origin, 0.1, 0.4) == -1 and L.rgbid_tsdf_reset(None) == -1
    assert L.rgbid_tsdf_integrate(None, 1, c.byref(view), k, ROWS, COLS, 0.05, 20.0) == -1
    assert L.rgbid_tsdf_get_state(None, None, None, None) == -1 and L.rgbid_tsdf_set_state(None, None, None, None) == -1
    assert L.rgbid_tsdf_extract_plan(None, 1, c.byref(nv), c.byref(nt)) == -1 and L.rgbid_tsdf_extract_emit(None, None, None, None, 0, 0) == -1
    assert L.rgbid_tsdf_timing(None, 0, None) == -1 and L.rgbid_tsdf_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-voxel", "0.05"], "need --mesh"), (["--mesh-bounds", "0", "0", "0", "1", "1", "1"], "need --mesh"),
                      (["--mesh-trunc", "0.2", "--mesh-min-weight", "2", "--mesh-max-voxels", "1000"], "need --mesh"),
                      (mesh + ["--mesh-voxel", "0"], "voxel and trunc must be > 0"), (mesh + ["--mesh-trunc", "nan"], "trunc must be finite"),
                      (mesh + ["--mesh-min-weight", "65536"], "min_weight must lie in"), (mesh + ["--mesh-max-voxels", "7"], "max_voxels must lie in"),
                      (mesh + ["--mesh-bounds", "0", "0", "0", "-1", "1", "1"], "bounds: six finite numbers"),
                      (mesh + ["--mesh-bounds", "0", "0", "0", "10", "10", "10", "--mesh-voxel", "0.01"], "would fit")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()


def test_mesh_ply_is_parsed_back():
    vol = sphere_volume()
    v, c, tr = TM.extract(vol, 1)
    c = np.random.default_rng(3).integers(0, 256, c.shape, dtype=np.uint8)
    data = TS.mesh_ply_bytes(v, c, tr)
    head = data[:data.index(b"end_header\n")].decode("ascii").split("\n")
    assert head[:2] == ["ply", "format binary_little_endian 1.0"] and "element vertex 2002" in head and "element face 4000" in head
    assert head.index("element vertex 2002") < head.index("property float x") < head.index("property uchar blue") < head.index("element face 4000")
    assert head[-2] == "property list uchar uint vertex_indices"
    assert len(data) == data.index(b"end_header\n") + 11 + 2002 * 15 + 4000 * 13
    pv, pc, pt = TS.read_mesh_ply(data)
    assert pv.tobytes() == v.tobytes() and pc.tobytes() == c.tobytes() and pt.tobytes() == tr.tobytes() and pt.dtype == np.uint32
    import torch
    assert TS.mesh_ply_bytes(torch.from_numpy(v), torch.from_numpy(c), torch.from_numpy(tr.view(np.int32))) == data
    black = TS.read_mesh_ply(TS.mesh_ply_bytes(v, None, tr))[1]
    assert not black.any()
    e = TS.mesh_ply_bytes(np.zeros((0, 3), F), None, np.zeros((0, 3), np.uint32))
    assert b"element vertex 0\n" in e and b"element face 0\n" in e and e.endswith(b"end_header\n")
