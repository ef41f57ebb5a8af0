"""CPU checks of the mesh rasteriser (include/rgbid_raster.h, rgbid.raster): the numpy restatement the GPU tests compare the kernels
against (tests/raster_mirror.py) against the plain scalar loops of the contract on every mesh of the GPU tests; the sphere of section 19,
whose covered pixels are known analytically; a wall whose pixels, depths and winners are derived by hand; hand-built threshold cases,
everything exact in float32; the Python argument checks one by one; the header as C99; the library's exports and NULL-handle refusals; the
command line's option errors."""
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
from rgbid import raster as RS
from tests import raster_mirror as XM
from tests import raycast_mirror as RM
from tests import tsdf_mirror as TM
from tests.test_cpu_raycast import SPHERE_CAM, analytic_sphere
from tests.test_cpu_tsdf import sphere_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
F = np.float32
EYE, ZERO = np.eye(3)[None], np.zeros((1, 3))
UNIT = (1.0, 1.0, 0.0, 0.0)              # with Z = 1 and the identity pose u = x and v = y exactly: a vertex is given in pixels


def case(vertices, triangles, rows, cols, K=UNIT, R=EYE, t=ZERO, colours=None, normals=None, z_min=0.5, z_max=4.0):
    v = np.array(vertices, F).reshape(-1, 3)
    return dict(vertices=v, triangles=np.array(triangles, np.uint32).reshape(-1, 3), R=np.asarray(R, np.float64).reshape(-1, 3, 3),
                t=np.asarray(t, np.float64).reshape(-1, 3), K=K, rows=rows, cols=cols, z_min=z_min, z_max=z_max,
                colours=None if colours is None else np.array(colours, np.uint8).reshape(-1, 3),
                normals=None if normals is None else np.array(normals, F).reshape(-1, 3))


def flat(points, z=1.0):
    """pixel positions -> vertices on the plane Z = z of the identity camera with K = UNIT"""
    return [(x * z, y * z, z) for x, y in points]


def attributes(n, seed):
    rng = np.random.default_rng(seed)
    nr = rng.normal(size=(n, 3))
    return rng.integers(0, 256, (n, 3)).astype(np.uint8), (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(F)


@functools.lru_cache(maxsize=None)
def sphere_mesh():
    vol = sphere_volume()
    v, c, tr = TM.extract(vol, 1)
    return v, c, tr, RM.vertex_normals(vol, 1)


def sphere_case():
    v, c, tr, n = sphere_mesh()
    cam = SPHERE_CAM
    return case(v, tr, cam["rows"], cam["cols"], cam["K"], cam["R"], cam["t"], c, n, cam["z_min"], cam["z_max"])


WALL_V = [(-0.5, -0.25, 2), (0.5, -0.25, 2), (0.5, 0.25, 2), (-0.5, 0.25, 2)]
WALL_K = (64.0, 64.0, 32.0, 24.0)


def wall_case(triangles=((0, 1, 2), (0, 2, 3))):
    col, nr = attributes(4, 5)
    return case(WALL_V, triangles, 48, 64, WALL_K, colours=col, normals=nr, z_min=0.05, z_max=20.0)


X0 = 3 + 0.5 / 256                       # u 256 + 0.5 = 769 exactly
GUARD = 32768.0                          # 2^23 / 256


def threshold_case():
    """one 24 x 40 image of hand-built triangles on the plane Z = 1, see test_threshold_cases"""
    pts = [(2, 2), (5, 2), (2, 5),                                                  # 0: centres on a vertex and on edges
           (10 + 1 / 256, 2 + 1 / 256), (13, 2 + 1 / 256), (10 + 1 / 256, 5),       # 1: the same one sub-pixel inside: its first centre is outside
           (1, 10), (2, 11), (3, 12.001),                                           # 2: the corners differ, the snapped ones are collinear
           (X0, 14), (X0 + 3, 14), (X0, 17),                                        # 3: u 256 + 0.5 on an integer
           (float(np.nextafter(F(X0), F(0))), 18), (X0 + 3, 18), (X0, 21),          # 4: one ulp below it
           (20, 2), (24, 2), (20, 6),                                               # 5: colours 0 2 0: .5 at every odd pixel of its first row
           (28, 2), (32, 2), (28, 6), (NAN, 2), (32, INF),                          # 6, 7, 8: a NaN and an inf vertex gate their triangles only
           (20, 10), (26, 10), (20, 16)]                                            # 9: a NaN vertex normal
    tris = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (9, 10, 11), (12, 13, 14), (15, 16, 17), (18, 19, 20), (18, 19, 21), (18, 22, 20), (23, 24, 25)]
    col, nr = attributes(len(pts), 7)
    col[15:18] = [(0, 0, 0), (2, 2, 2), (0, 0, 0)]
    nr[23] = (NAN, 0, 1)
    return case(flat(pts), tris, 24, 40, colours=col, normals=nr)


def depth_gate_case():
    """four triangles at Z = z_min, one ulp below it, z_max and one ulp above it"""
    lo, hi = F(1.0), F(2.0)
    zs = [lo, np.nextafter(lo, F(0)), hi, np.nextafter(hi, F(3))]
    v, tr = [], []
    for i, z in enumerate(zs):
        tr.append((3 * i, 3 * i + 1, 3 * i + 2))
        v += [(F(4 * i) * z, F(1) * z, z), (F(4 * i + 3) * z, F(1) * z, z), (F(4 * i) * z, F(4) * z, z)]
    col, nr = attributes(len(v), 17)
    return case(v, tr, 6, 16, colours=col, normals=nr, z_min=1.0, z_max=2.0)


def crossing_case():
    """triangle 0 at Z = 1.5, triangle 1 over the same pixels with 1 / Z falling from 1 to 1 / 2 along x: they cross at px = 16 / 3"""
    v = flat([(0, 0), (8, 0), (0, 8)], 1.5) + [(0, 0, 1), (16, 0, 2), (0, 8, 1)]
    col, nr = attributes(6, 9)
    return case(v, [(0, 1, 2), (3, 4, 5)], 9, 9, colours=col, normals=nr)


def duplicate_case():
    col, nr = attributes(3, 11)
    return case(flat([(1, 1), (6, 2), (2, 6)]), [(0, 1, 2), (0, 1, 2), (1, 2, 0), (2, 1, 0)], 8, 8, colours=col, normals=nr)


def guard_case(rows=7, cols=9):
    """a triangle much larger than the image, its corners at the guard and inside it; two beyond the guard that are gated"""
    up = float(np.nextafter(F(GUARD), F(INF)))
    v = flat([(-GUARD, -GUARD), (GUARD, -GUARD), (0, GUARD), (-30000, -30000), (30000, -30000), (1, 30000), (up, -GUARD), (-GUARD - 2 / 256, -GUARD)])
    col, nr = attributes(8, 13)
    return case(v, [(0, 1, 2), (3, 4, 5), (0, 6, 2), (7, 1, 2)], rows, cols, colours=col, normals=nr)


def random_case(n_v, n_t, rows, cols, seed, size=6.0, bad=0):
    """random triangles of a few pixels over the image and beyond its rim, at depths across both gates, some vertices not finite"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.4, 4.5, n_v)
    centre = rng.uniform(-4, max(rows, cols) + 4, (n_v, 2))
    v = np.concatenate([centre * z[:, None], z[:, None]], 1).astype(F)
    first = rng.integers(0, n_v, n_t)
    tri = np.stack([first, rng.integers(0, n_v, n_t), rng.integers(0, n_v, n_t)], 1)
    near = rng.random(n_t) < 0.9                                                 # most triangles are small: their corners are neighbours
    for k in (1, 2):
        tri[near, k] = (first[near] + rng.integers(1, 4, near.sum())) % n_v
    order = np.argsort(centre[:, 0] // size * 1000 + centre[:, 1] // size, kind="stable")   # neighbours in index are neighbours in the image
    v = v[order]
    if bad:
        at = rng.choice(n_v, bad, replace=False)
        v[at[::2], rng.integers(0, 3)] = NAN
        v[at[1::2], rng.integers(0, 3)] = INF
    col, nr = attributes(n_v, seed + 1)
    return case(v, tri, rows, cols, colours=col, normals=nr)


def with_views(c, V, seed=0):
    """the case seen from V poses: its own first, the others turned and moved a little"""
    rng = np.random.default_rng(100 + seed + V)
    R, t = [c["R"][0]], [c["t"][0]]
    for _ in range(V - 1):
        w = rng.normal(size=3) * 0.03
        Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        R.append(c["R"][0] @ (np.eye(3) + Kx + Kx @ Kx / 2))
        t.append(c["t"][0] + rng.normal(size=3) * 0.05)
    return dict(c, R=np.stack(R), t=np.stack(t))


CASES = {"sphere": sphere_case, "wall": wall_case, "wall_reversed": lambda: wall_case(((0, 2, 3), (0, 1, 2))),
         "wall_flipped": lambda: wall_case(((0, 2, 1), (0, 3, 2))), "threshold": threshold_case, "depth_gate": depth_gate_case,
         "crossing": crossing_case, "duplicate": duplicate_case, "guard_7x9": guard_case, "guard_1x1": lambda: guard_case(1, 1),
         "guard_8x8": lambda: guard_case(8, 8), "random_13x29": lambda: random_case(60, 150, 13, 29, 3, bad=6)}


def mirror(c):
    return XM.raster_numpy(c["vertices"], c["triangles"], c["R"], c["t"], c["K"], c["rows"], c["cols"], c["colours"], c["normals"], c["z_min"], c["z_max"])


def counts_of(out, v=0):
    return dict(zip(XM.COUNTS, out["counts"][v].tolist()))


@pytest.mark.parametrize("name", sorted(CASES))
def test_mirror_equals_the_scalar_loop(name):
    c = with_views(CASES[name](), 2)
    a = mirror(c)
    b = XM.raster_loop(c["vertices"], c["triangles"], c["R"], c["t"], c["K"], c["rows"], c["cols"], c["colours"], c["normals"], c["z_min"], c["z_max"])
    assert set(a) == set(b) == {"index", "depth", "colour", "normal", "counts"}
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (name, k)
    assert a["index"].shape == (2, c["rows"], c["cols"]) and a["normal"].shape == (2, 3, c["rows"], c["cols"])
    assert not np.isnan(a["normal"][:, :, a["index"][0] != XM.EMPTY][0]).any()              # a covered pixel never stores a NaN


def test_sphere_is_the_analytic_pixel_set():
    c = sphere_case()
    assert c["vertices"].shape == (2002, 3) and c["triangles"].shape == (4000, 3)
    out = mirror(c)
    n = counts_of(out)
    xs, ys, Z, ok = XM.project(c["vertices"], XM.pose_cw(c["R"][0], c["t"][0]), c["K"], c["z_min"], c["z_max"])
    cl = XM.classify(c["triangles"].astype(np.int64), xs, ys, ok, c["rows"], c["cols"])
    d = cl["cls"] == 3
    largest = int(((cl["x1"] - cl["x0"] + 1) * (cl["y1"] - cl["y0"] + 1))[d].max())
    print(f"sphere: {n}, largest box {largest} pixels")
    assert n == dict(gated=0, degenerate=342, empty_box=1566, drawn=2092, fragments=1292, pixels=616) and largest == 9
    meets, depth, _ = analytic_sphere()
    drawn = out["index"][0] != XM.EMPTY
    assert (drawn == meets).all()                                                # exactly the pixels whose ray meets the sphere
    inner = ~drawn[1:-1, 1:-1] & drawn[:-2, 1:-1] & drawn[2:, 1:-1] & drawn[1:-1, :-2] & drawn[1:-1, 2:]
    assert inner.sum() == 0                                                      # no hole
    err = np.sort(np.abs(out["depth"][0][drawn].astype(np.float64) - depth[drawn]))
    print(f"sphere: |depth - analytic| median {err[len(err) // 2] * 1e3:.2f} mm, 90 % {err[int(0.9 * len(err))] * 1e3:.2f} mm")
    assert err[len(err) // 2] < 0.0021 * 1.5 and err[int(0.9 * len(err))] < 0.0054 * 1.5   # the prototype's figures: 2.1 mm and 5.4 mm


@pytest.mark.parametrize("name", ["wall", "wall_reversed", "wall_flipped"])
def test_wall(name):
    out = mirror(CASES[name]())
    idx, depth = out["index"][0], out["depth"][0]
    drawn = idx != XM.EMPTY
    want = np.zeros((48, 64), bool)
    want[16:33, 16:49] = True
    assert (drawn == want).all() and drawn.sum() == 561 and (depth[drawn] == F(2.0)).all()
    n = counts_of(out)
    assert n == dict(gated=0, degenerate=0, empty_box=0, drawn=2, fragments=578, pixels=561)     # the 17 centres on the diagonal twice
    assert (idx == 0).sum() == 289 and (idx == 1).sum() == 272
    diag = [(16 + k, 16 + 2 * k) for k in range(17)]
    assert all(idx[r, c] == 0 for r, c in diag)                                  # the diagonal goes to index 0, whichever triangle that is


def test_threshold_cases():
    c = threshold_case()
    out = mirror(c)
    idx, col, nrm = out["index"][0].astype(np.int64), out["colour"][0], out["normal"][0]
    idx[idx == int(XM.EMPTY)] = -1
    pix = lambda tri: sorted(zip(*(a.tolist() for a in np.nonzero(idx == tri)[::-1])))       # (px, py)
    tri0 = sorted((x, y) for y in range(2, 6) for x in range(2, 6) if x + y <= 7)
    assert pix(0) == tri0 and (2, 2) in tri0 and (5, 2) in tri0 and (3, 4) in tri0           # vertices and edges are covered
    assert pix(1) == sorted((x + 8, y) for x, y in tri0 if x > 2 and y > 2)                  # both legs moved one sub-pixel inwards
    assert (10, 2) not in pix(1) and (11, 3) in pix(1) and idx[2, 10] == -1 and idx[3, 10] == -1 and idx[2, 11] == -1
    assert pix(2) == []                                                                      # degenerate after the snap
    xs = XM.project(c["vertices"], XM.pose_cw(np.eye(3), np.zeros(3)), UNIT, 0.5, 4.0)[0]
    assert xs[9] == 769 and xs[12] == 768 and XM.project_loop(c["vertices"][9], XM.pose_cw(np.eye(3), np.zeros(3)), UNIT, 0.5, 4.0)[0] == 769
    assert idx[14, 3] == -1 and idx[14, 4] == 3                                              # xs = 769: the centre 768 is outside
    assert idx[18, 3] == 4                                                                   # xs = 768: on the vertex
    assert col[2, 20:25, 0].tolist() == [0, 1, 1, 2, 2] and idx[2, 20:25].tolist() == [5] * 5          # .5 rounds up
    assert pix(6) == sorted((x, y) for y in range(2, 7) for x in range(28, 33) if x + y <= 34)          # its neighbours are gated, it is not
    assert pix(7) == [] and pix(8) == []
    assert counts_of(out) == dict(gated=2, degenerate=1, empty_box=0, drawn=7, fragments=sum(len(pix(k)) for k in range(10)),
                                  pixels=int((idx >= 0).sum()))
    own = idx == 9
    assert own.sum() == 28 and (nrm[:, own] == 0).all() and not np.isnan(nrm[:, idx >= 0]).any()          # the NaN vertex normal
    assert (np.abs(np.linalg.norm(nrm[:, (idx >= 0) & ~own].astype(np.float64), axis=0) - 1) < 1e-6).all()
    empty = idx < 0
    assert (out["depth"][0].view(np.uint32)[empty] == XM.NAN_BITS).all() and (nrm.view(np.uint32)[:, empty] == XM.NAN_BITS).all()
    assert (col[empty] == 0).all()


def test_depth_gate():
    out = mirror(depth_gate_case())
    idx = out["index"][0]
    assert counts_of(out)["gated"] == 2 and counts_of(out)["drawn"] == 2
    assert set(np.unique(idx).tolist()) == {0, 2, int(XM.EMPTY)}                 # Z = z_min and Z = z_max are drawn, one ulp outside is not
    assert (out["depth"][0][idx == 0] == F(1)).all() and (out["depth"][0][idx == 2] == F(2)).all()


def test_crossing_and_duplicate():
    out = mirror(crossing_case())
    idx = out["index"][0]
    assert idx[0].tolist() == [1] * 6 + [0] * 3                                  # 1 / Z is what is linear: the crossing lies at 16 / 3, not at 4
    assert idx[2, :7].tolist() == [1] * 6 + [0]
    assert counts_of(out)["fragments"] == 90 and counts_of(out)["pixels"] == 45
    d = out["depth"][0]
    assert d[0, 0] == F(1) and d[0, 4] == F(1 / (1 - 4 / 16)) and d[0, 6] == F(1.5)
    out = mirror(duplicate_case())
    assert set(np.unique(out["index"][0]).tolist()) == {0, int(XM.EMPTY)}         # equal depths: the smallest index, both windings drawn
    assert counts_of(out)["fragments"] == 4 * counts_of(out)["pixels"] and counts_of(out)["drawn"] == 4


def test_guard_and_small_images():
    for rows, cols in ((7, 9), (1, 1), (8, 8)):
        out = mirror(guard_case(rows, cols))
        n = counts_of(out)
        assert n == dict(gated=2, degenerate=0, empty_box=0, drawn=2, fragments=2 * rows * cols, pixels=rows * cols)
        assert (out["index"][0] == 0).all() and (out["depth"][0] == F(1)).all()
        assert out["colour"].shape == (1, rows, cols, 3)
    m = XM.pose_cw(np.eye(3), np.zeros(3))
    xs, _, _, ok = XM.project(guard_case()["vertices"], m, UNIT, 0.5, 4.0)
    assert xs[:2].tolist() == [-(1 << 23), 1 << 23] and ok[:6].all() and not ok[6] and not ok[7]
    # rows != cols: a transposed image would put the wall elsewhere
    c = wall_case()
    out = mirror(c)
    assert out["index"][0].shape == (48, 64) and (out["index"][0][:, 49:] == XM.EMPTY).all() and (out["index"][0][33:] == XM.EMPTY).all()


def test_empty_meshes():
    for v, tr in ((np.zeros((0, 3), F), np.zeros((0, 3), np.uint32)), (np.zeros((5, 3), F) + 1, np.zeros((0, 3), np.uint32))):
        out = XM.raster_numpy(v, tr, EYE, ZERO, UNIT, 3, 4)
        assert (out["index"] == XM.EMPTY).all() and (out["depth"].view(np.uint32) == XM.NAN_BITS).all() and (out["counts"] == 0).all()
    with pytest.raises(ValueError):
        XM.raster_numpy(np.zeros((3, 3), F), [(0, 1, 3)], EYE, ZERO, UNIT, 3, 4)


# ---- the Python checkers, one by one ------------------------------------------------------------------------------------------------------
def test_checkers():
    assert RS.capacity_arg(1, 1, 1) == (1, 1, 1) and RS.capacity_arg(1 << 31, (1 << 31) - 1, 1 << 38) == (1 << 31, (1 << 31) - 1, 1 << 38)
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), ((1 << 31) + 1, 1, 1), (1, 1 << 31, 1), (1, 1, (1 << 38) + 1), (1.0, 1, 1), (1, "2", 1), (True, 1, 1)):
        with pytest.raises(ValueError):
            RS.capacity_arg(*bad)
    assert RS.image_size(16384, 1) == (16384, 1) and RS.image_size(480, 640, 16, 480 * 640 * 16) == (480, 640)
    for bad in ((0, 4), (4, 0), (16385, 4), (4, 16385), (4.0, 4), (4, 4, 0), (4, 4, 4097), (4, 4, 2, 31)):
        with pytest.raises(ValueError):
            RS.image_size(*bad)
    import torch
    for v, t in ((np.zeros((3, 3), F), None), (torch.zeros((3, 3)), torch.zeros((1, 3), dtype=torch.int32)), (None, None)):
        with pytest.raises(ValueError):
            RS.mesh_arg(v, t)                                                    # no CUDA tensors
    assert RS.EMPTY == int(XM.EMPTY) and RS.NAN_BITS == int(XM.NAN_BITS) and RS.SUB == XM.SUB and RS.MAX_DIM == XM.MAX_DIM
    assert RS.COUNTS == XM.COUNTS and len(RS.STAGES) == 4


def test_checks_come_before_the_library():
    for caps in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1 << 31, 1)):
        with pytest.raises(ValueError):
            RS.Rasteriser(None, *caps)

    class Ctx:
        device = 0
    rs = RS.Rasteriser.__new__(RS.Rasteriser)
    rs.ctx, rs.max_vertices, rs.max_triangles, rs.max_pixels, rs._views = Ctx(), 10, 10, 100, 0
    good = dict(R=np.eye(3), t=np.zeros(3), K=(60.0, 58.0, 4.5, 3.5), rows=8, cols=10)
    for change in (dict(z_min=0.0), dict(z_min=3.0, z_max=2.0), dict(z_max=INF), dict(K=(0, 58, 4.5, 3.5)), dict(K=(60, 58, NAN, 3.5)),
                   dict(t=[NAN, 0, 0]), dict(R=np.full((3, 3), 1e300)), dict(rows=0), dict(cols=16385), dict(rows=11), dict(outputs=("splat",)),
                   dict(outputs=()), dict(R=np.zeros((0, 3, 3)), t=np.zeros((0, 3))), dict(R=np.stack([np.eye(3)] * 2), t=np.zeros((2, 3))), dict()):
        with pytest.raises(ValueError):
            rs.render(np.zeros((3, 3), F), np.zeros((1, 3), np.int32), **dict(good, **change))    # the last one: the mesh is no CUDA tensor
    with pytest.raises(ValueError):
        rs.render(None, None, outputs=("normal",), **good)                       # a plane without its attribute
    with pytest.raises(ValueError):
        rs.render(None, None, outputs=("depth", "colour"), **good)
    with pytest.raises(ValueError):
        rs.counts()                                                              # nothing was rendered
    rs._h = None
    for call in (lambda: RS.render_mesh(None, None, None, np.eye(3), np.zeros(3), good["K"], 8, 10, outputs=("depth",)),
                 lambda: RS.render_mesh(None, None, None, np.eye(3), np.zeros(3), good["K"], 8, 10, z_min=-1, outputs=("depth",)),
                 lambda: RS.mesh_agreement(None, None, None, [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)], good["K"], 8, 10),
                 lambda: RS.mesh_agreement(None, None, None, [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)], good["K"], 0, 10)):
        with pytest.raises(ValueError):
            call()
    assert RS.mesh_agreement(None, None, None, [], good["K"], 8, 10) == []
    assert "cannot be excluded" in RS.mesh_agreement.__doc__


def test_agreement_statistic():
    import torch
    depth = torch.tensor([[1.0, 2.0, NAN], [4.0, 1.5, 3.0]])
    iD = np.array([[1.0, 0.25, 1.0], [NAN, 0.0, 0.5]], F)
    f = RS.agreement_of(depth, iD)                                               # |1 - 1|, |2 - 4|, |3 - 2|: the others lack one side
    assert f == dict(pixels=3, median=1.0, p90=2.0)
    assert RS.agreement_of(depth, np.full((2, 3), NAN, F))["pixels"] == 0


def test_nothing_is_imported_without_the_options():
    code = ("import sys; sys.path[:0] = [%r, %r]; from rgbid import tsdf, render, mesh, simplify, smooth; "
            "assert 'rgbid.raster' not in sys.modules") % (ROOT, os.path.join(ROOT, "rgbid-slam_amd"))
    subprocess.check_call([sys.executable, "-c", code])
    src = open(os.path.join(ROOT, "tools", "track_dataset.py")).read()
    assert src.count("from rgbid import raster as RS") == 1
    head = src[:src.index("from rgbid import raster as RS")].rstrip().splitlines()[-1]
    assert head.strip() == "if args.mesh_raster or args.mesh_raster_check:"     # the one import stands behind the options


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_raster.c"
    src.write_text('#include "rgbid_raster.h"\n'
                   "int use(rgbid_raster* r, rgbid_ctx* ctx, const float* v, const uint32_t* tris, const uint8_t* col, const float* nrm,\n"
                   "        const rgbid_render_pose* poses, uint32_t* index, float* depth, uint8_t* colour, float* normal) {\n"
                   "  const float K[4] = {525.f, 525.f, 319.5f, 239.5f}; unsigned long long counts[6 * RGBID_RASTER_VIEW_CHUNK]; float ms[4];\n"
                   "  return rgbid_raster_create(&r, ctx, RGBID_RASTER_MAX_VERTICES, RGBID_RASTER_MAX_TRIANGLES, 640ull * 480ull * 16ull)\n"
                   "       + rgbid_raster_views(r, v, 10, tris, 5, col, nrm, 16, poses, K, 480, 640, 0.05f, 20.f, index, depth, colour, normal)\n"
                   "       + rgbid_raster_counts(r, 16, counts) + rgbid_raster_timing(r, 1, ms) + rgbid_raster_destroy(r)\n"
                   "       + (RGBID_RASTER_EMPTY == 0xFFFFFFFFu ? 0 : 1); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_raster.h")).read()
    value = lambda name: int(re.search(r"#define RGBID_RASTER_%s\s+(0x[0-9A-Fa-f]+|\d+)" % name, txt).group(1), 0)
    assert value("MAX_TRIANGLES") == RS.MAX_TRIANGLES == (1 << 31) - 1 and value("MAX_VERTICES") == RS.MAX_VERTICES
    assert value("MAX_DIM") == RS.MAX_DIM == 16384 and value("SUB") == RS.SUB == 256 and value("VIEW_CHUNK") == RS.VIEW_CHUNK == 16
    assert value("SMALL_BOX") == RS.SMALL_BOX and value("TILE") == RS.TILE == 8 and value("MAX_VIEWS") == RS.MAX_VIEWS
    assert value("TIMED_CHUNKS") == RS.TIMED_CHUNKS and value("EMPTY") == RS.EMPTY and value("NAN_BITS") == RS.NAN_BITS


def test_library_exports_raster_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_raster.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_raster_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(RS.EXPORTS) and len(declared) == 5, set(declared) ^ set(RS.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    L.rgbid_raster_create.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_ulonglong, c.c_ulonglong]
    L.rgbid_raster_views.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_void_p, c.c_ulonglong, c.c_void_p, c.c_void_p, c.c_int, c.c_void_p,
                                     c.c_void_p, c.c_int, c.c_int, c.c_float, c.c_float, c.c_void_p, c.c_void_p, c.c_void_p, c.c_void_p]
    L.rgbid_raster_counts.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_raster_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_raster_destroy.argtypes = [c.c_void_p]
    h = c.c_void_p()
    assert L.rgbid_raster_create(c.byref(h), None, 10, 10, 100) == -1 and not h.value and L.rgbid_raster_create(None, None, 10, 10, 100) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for v, t, p in ((0, 10, 100), (10, 0, 100), (10, 10, 0), ((1 << 31) + 1, 10, 100), (10, 1 << 31, 100), (10, 10, (1 << 38) + 1)):
        assert L.rgbid_raster_create(c.byref(h), fake, v, t, p) == -1 and not h.value
    pose, k = RS.Pose(), (c.c_float * 4)(60, 58, 4.5, 3.5)
    assert L.rgbid_raster_views(None, None, 0, None, 0, None, None, 1, c.byref(pose), k, 8, 10, 0.05, 20.0, None, None, None, None) == -1
    out = (c.c_ulonglong * 6)()
    assert L.rgbid_raster_counts(None, 1, out) == -1 and L.rgbid_raster_timing(None, 0, None) == -1 and L.rgbid_raster_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    for bad, word in ((["--mesh-raster", str(tmp_path / "v")], "need --mesh"), (["--mesh-raster-check"], "need --mesh"),
                      (["--mesh-raster"], "expected one argument")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "v").exists()
