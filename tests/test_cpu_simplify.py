"""CPU checks of the vertex clustering stage (include/rgbid_simplify.h, rgbid.simplify): the vectorised numpy restatement the GPU tests
compare the kernels against (tests/simplify_mirror.py) against its scalar loops on every mesh below, and by hand what each mesh is about:
cell borders, floorf on negative coordinates, every way a triangle collapses, duplicates of either orientation, lost before collapsed,
non-finite vertices, the normal and colour rules, section 19's sphere with the figures of the issue, two sheets closer than the cell,
random triangles; the Python argument checks one by one; the header as C99; the library's exports; the command line's option errors; a
simplified mesh through the PLY writer."""
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
from rgbid import simplify as SP
from rgbid import tsdf as TS
from tests import simplify_mirror as SM
from tests.test_cpu_mesh import tsdf_meshes
from tests.test_cpu_tsdf import SPHERE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32 = np.float32, np.uint32
NO = SM.NO_CLUSTER
NAN, INF = float("nan"), float("inf")
SNAN = np.array([0x7F800001], U32).view(F)[0]            # a signalling NaN


def mesh(vertices, triangles, cell, colours=None, normals=None):
    v = np.array(vertices, F).reshape(-1, 3)
    return dict(vertices=v, triangles=np.array(triangles, U32).reshape(-1, 3), cell=cell,
                colours=None if colours is None else np.array(colours, np.uint8).reshape(-1, 3),
                normals=None if normals is None else np.array(normals, F).reshape(-1, 3))


def default_attributes(n_v, seed):
    """colours and normals for a mesh that brings none: random bytes, random normals with non-finite rows among them"""
    rng = np.random.default_rng(500 + seed)
    nrm = rng.normal(size=(n_v, 3)).astype(F)
    if n_v:
        nrm[::7, 1] = NAN
        nrm[3::11, 0] = INF
    return rng.integers(0, 256, (n_v, 3), dtype=np.uint8), nrm


# ---- the meshes: name -> dict(vertices, triangles, cell, colours, normals) -----------------------------------------------------------------
HAND_CLASSES = [3, 1, 1, 1, 1, 1, 1, 2, 2, 3, 2, 0, 0, 3]


def hand_mesh():
    """cell 1: clusters A .. E at x = 0 .. 3 and 5; vertices 7 .. 10 do not take part; vertex 11 is a cluster no triangle names"""
    v = [(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (2.5, 0.5, 0.5), (0.25, 0.25, 0.25), (1.25, 0.5, 0.5), (2.75, 0.5, 0.5), (3.5, 0.5, 0.5),
         (NAN, 0, 0), (0.5, INF, 0.5), (0.5, 0.5, -INF), (SNAN, 0.5, 0.5), (5.5, 0.5, 0.5)]
    t = [(0, 4, 2),       # A B C: kept
         (0, 3, 2),       # A A C: the pair (0, 1)
         (0, 1, 4),       # A B B: the pair (1, 2)
         (0, 1, 3),       # A B A: the pair (0, 2)
         (0, 3, 0),       # A A A
         (1, 1, 2),       # the input triangle (a, a, b)
         (6, 6, 6),       # the input triangle (a, a, a)
         (3, 1, 5),       # A B C again, the same orientation: duplicate
         (5, 4, 3),       # C B A, the opposite orientation: the third equal triple
         (1, 2, 6),       # B C D: kept
         (6, 2, 1),       # D C B: duplicate of the smaller input index 9
         (7, 0, 0),       # lost, and would be collapsed
         (0, 1, 8),       # lost
         (2, 6, 0)]       # C D A: kept
    col = np.zeros((12, 3), np.uint8)
    col[0], col[3] = (0, 255, 10), (1, 254, 11)           # sums 1 and 509 over 2 members: the means on .5 round up
    col[1], col[4] = (7, 0, 200), (8, 0, 100)
    nrm = np.zeros((12, 3), F)
    nrm[0], nrm[3] = (0, 0, 1), (0, 0, -1)                # opposite: the sum is 0
    nrm[1], nrm[4] = (NAN, 0, 0), (0, 3, 4)               # one member without a normal
    nrm[2], nrm[5] = (NAN, NAN, NAN), (0, INF, 0)         # no member with one
    nrm[6] = (3e38, 3e38, 0)                              # huge
    nrm[11] = (1, 2, 2)
    return mesh(v, t, 1.0, col, nrm)


def border_mesh():
    """cell 0.5: the border at x = 1 between cells 1 and 2; below it by one ulp, on it, above it by one ulp; and -0.25, whose cell is -1"""
    one = F(1.0)
    xs = [0.25, np.nextafter(one, F(0)), one, np.nextafter(one, F(2)), -0.25, -0.5, np.nextafter(F(-0.5), F(-1))]
    return mesh([(x, 0.1, 0.1) for x in xs], [(0, 1, 2), (0, 2, 3), (4, 0, 1), (4, 5, 6), (6, 0, 2)], 0.5)


def anisotropic_mesh():
    rng = np.random.default_rng(11)
    v = rng.uniform(-1, 1, (400, 3)).astype(F)
    return mesh(v, rng.integers(0, 400, (900, 3)), (0.5, 0.125, 0.3))


def sheets_mesh():
    """two copies of a triangulated plane 3 mm apart under a 10 mm cell, the second with the opposite orientation"""
    n = 40
    g = np.arange(n) * 0.004 + 0.001
    x, y = np.meshgrid(g, g, indexing="ij")
    sheet = lambda z: np.stack([x.ravel(), y.ravel(), np.full(n * n, z)], 1)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a, b, c, d = (i * n + j).ravel(), ((i + 1) * n + j).ravel(), (i * n + j + 1).ravel(), ((i + 1) * n + j + 1).ravel()
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    return mesh(np.concatenate([sheet(0.002), sheet(0.005)]), np.concatenate([tri, tri[:, ::-1] + n * n]), 0.01)


def random_mesh():
    rng = np.random.default_rng(7)
    return mesh(rng.random((3000, 3)).astype(F), rng.integers(0, 3000, (20000, 3)), 0.2)


def sphere(cell):
    v, c, tri = tsdf_meshes()["sphere"]
    return mesh(v, tri, cell, c)


def min_distance(v):
    d2 = ((v.astype(np.float64)[:, None, :] - v.astype(np.float64)[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    return float(np.sqrt(d2.min()))


def distinct_mesh():
    """random vertices, no two alike, under a cell whose diagonal is below their smallest distance: nothing can share a cell"""
    rng = np.random.default_rng(13)
    v = rng.uniform(-1, 1, (500, 3)).astype(F)
    tri = np.array([t for t in rng.integers(0, 500, (1500, 3)) if len(set(t)) == 3])
    tri = tri[np.unique(np.sort(tri, 1), axis=0, return_index=True)[1]]          # a mesh without duplicates
    return mesh(v, tri, min_distance(v) / 2.0)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = {
        "hand": hand_mesh(), "border": border_mesh(), "anisotropic": anisotropic_mesh(), "sheets": sheets_mesh(), "random": random_mesh(),
        "no_triangles": mesh([(0.1, 0.2, 0.3), (0.1, 0.2, 0.3), (4, 5, 6)], [], 0.5),
        "no_vertices": mesh([], [], 0.5),
        "nobody_takes_part": mesh([(NAN, 0, 0), (0, INF, 0), (1, 1, -INF)], [(0, 1, 2), (2, 2, 2)], 0.5),
        "distinct": distinct_mesh(), "sphere_tiny": sphere(1e-4), "sphere_huge": sphere(2.0),
    }
    cases.update({f"sphere_{c}": sphere(c) for c in (0.05, 0.1, 0.02, 0.15)})
    for k, (name, m) in enumerate(sorted(cases.items())):
        col, nrm = default_attributes(len(m["vertices"]), k)
        m["colours"] = col if m["colours"] is None else m["colours"]
        m["normals"] = nrm if m["normals"] is None else m["normals"]
    return cases


@functools.lru_cache(maxsize=None)
def mirrored(name, keep_duplicates=False):
    """the vectorised mirror's result of a case, computed once and shared with the GPU tests"""
    m = all_cases()[name]
    return SM.simplify(m["vertices"], m["triangles"], m["cell"], m["colours"], m["normals"], keep_duplicates)


# ---- mirror against loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_mirror_equals_the_loops(name):
    m = all_cases()[name]
    for keep in (False, True):
        a = mirrored(name, keep)
        b = SM.simplify_loop(m["vertices"], m["triangles"], m["cell"], m["colours"], m["normals"], keep)
        assert SM.same(a, b) == [], (name, keep, SM.same(a, b), a["counts"], b["counts"])
        c = a["counts"]
        assert c["lost"] + c["collapsed"] + c["duplicate"] + c["kept"] == len(m["triangles"]) and (keep is False or c["duplicate"] == 0)
        assert a["vertices"].dtype == F and a["triangles"].dtype == U32 and a["cluster_of"].dtype == U32 and a["members"].dtype == U32
        assert int(a["members"].sum()) == c["participating"] and len(a["vertices"]) == c["clusters"]


def test_sums_are_sequential_in_member_order():
    """100 000 members of one cluster whose values lose bits in any other order of adding: np.add.at against the scalar loop"""
    rng = np.random.default_rng(3)
    v = (rng.random((100000, 3)) * np.array([1.0, 1e-3, 1e3])).astype(F)
    a, b = SM.simplify(v, [], 2000.0, normals=v), SM.simplify_loop(v, [], 2000.0, normals=v)
    assert a["counts"]["clusters"] == 1 and SM.same(a, b) == []
    s = [0.0, 0.0, 0.0]
    for row in v[::-1]:
        for k in range(3):
            s[k] += float(row[k])
    fwd = [0.0, 0.0, 0.0]
    for row in v:
        for k in range(3):
            fwd[k] += float(row[k])
    assert fwd != s                                           # the order matters on this input ...
    assert a["vertices"][0].tolist() == [F(x / 100000.0) for x in fwd]      # ... and the mirror's is the ascending one


# ---- hand-built meshes ----------------------------------------------------------------------------------------------------------------------
def test_hand_built_mesh():
    r = mirrored("hand")
    assert r["cluster_of"].tolist() == [0, 1, 2, 0, 1, 2, 3, NO, NO, NO, NO, 4] and r["grid"].tolist() == [0, 0, 0, 6, 1, 1]
    assert r["counts"] == dict(participating=8, clusters=5, lost=2, collapsed=6, duplicate=3, kept=3)
    assert r["classes"].tolist() == HAND_CLASSES
    assert r["triangles"].tolist() == [[0, 1, 2], [1, 2, 3], [2, 3, 0]]          # t' in input order, the orientation as it was
    assert r["members"].tolist() == [2, 2, 2, 1, 1]
    assert r["vertices"].tolist() == [[0.375, 0.375, 0.375], [1.375, 0.5, 0.5], [2.625, 0.5, 0.5], [3.5, 0.5, 0.5], [5.5, 0.5, 0.5]]
    assert r["colours"][0].tolist() == [1, 255, 11] and r["colours"][1].tolist() == [8, 0, 150]      # 0.5 -> 1, 254.5 -> 255, 7.5 -> 8
    n = r["normals"]
    assert n[0].tolist() == [0, 0, 0] and n[2].tolist() == [0, 0, 0]            # opposite members; no member with a finite normal
    assert n[1].tolist() == [0, F(0.6), F(0.8)] and n[4].tolist() == [F(1 / 3), F(2 / 3), F(2 / 3)]
    # q of a huge normal is 1.8e77, far below the largest double: 2^31 members of float32 normals cannot make q infinite, the rule's
    # last clause guards arithmetic that the inputs cannot reach
    assert n[3].tolist() == [F(3e38 / np.sqrt(2 * float(F(3e38)) ** 2))] * 2 + [0]
    k = mirrored("hand", True)
    assert k["classes"].tolist() == [3 if c == 2 else c for c in HAND_CLASSES] and k["counts"]["kept"] == 6 and k["counts"]["duplicate"] == 0
    assert k["triangles"].tolist() == [[0, 1, 2], [0, 1, 2], [2, 1, 0], [1, 2, 3], [3, 2, 1], [2, 3, 0]]


def test_cell_borders_and_negative_coordinates():
    r = mirrored("border")
    # cells -2 (below -0.5), -1 (-0.5 and -0.25: floorf, not truncation, which would put -0.25 into cell 0), 0, 1 (below 1), 2 (1 and above)
    assert r["grid"].tolist() == [-2, 0, 0, 5, 1, 1]
    assert r["cluster_of"].tolist() == [2, 3, 4, 4, 1, 1, 0]
    assert r["classes"].tolist() == [3, 1, 3, 1, 3] and r["triangles"].tolist() == [[2, 3, 4], [1, 2, 3], [0, 2, 4]]


def test_degenerate_inputs():
    r = mirrored("no_triangles")
    assert r["counts"] == dict(participating=3, clusters=2, lost=0, collapsed=0, duplicate=0, kept=0) and r["members"].tolist() == [2, 1]
    assert r["triangles"].shape == (0, 3) and r["cluster_of"].tolist() == [0, 0, 1]
    r = mirrored("no_vertices")
    assert r["counts"] == dict.fromkeys(SM.COUNTS, 0) and r["vertices"].shape == (0, 3) and r["grid"].tolist() == [0] * 6
    r = mirrored("nobody_takes_part")
    assert r["counts"] == dict(participating=0, clusters=0, lost=2, collapsed=0, duplicate=0, kept=0) and r["cluster_of"].tolist() == [NO] * 3
    assert r["grid"].tolist() == [0] * 6
    r = mirrored("anisotropic")
    assert r["grid"][3:].tolist() == [4, 16, 8] and r["counts"]["clusters"] > 200 and r["counts"]["kept"] > 500
    for bad in ((0, 1, 3), (0, 1, -1)):
        with pytest.raises(ValueError):
            SM.simplify(np.zeros((3, 3), F), [bad], 1.0)
        with pytest.raises(ValueError):
            SM.simplify_loop(np.zeros((3, 3), F), [bad], 1.0)


# ---- the two consequences ----------------------------------------------------------------------------------------------------------------------
def test_a_tiny_cell_permutes_the_mesh():
    m, r = all_cases()["distinct"], mirrored("distinct")
    n_v, n_t = len(m["vertices"]), len(m["triangles"])
    assert 0 < m["cell"] * np.sqrt(3) < min_distance(m["vertices"]) and n_t > 1400
    assert r["counts"] == dict(participating=n_v, clusters=n_v, lost=0, collapsed=0, duplicate=0, kept=n_t)
    perm = r["cluster_of"]
    assert sorted(perm.tolist()) == list(range(n_v)) and (r["members"] == 1).all()
    assert r["triangles"].tobytes() == perm[m["triangles"]].tobytes()
    assert r["vertices"][perm].tobytes() == m["vertices"].tobytes() and r["colours"][perm].tobytes() == m["colours"].tobytes()


def test_a_tiny_cell_on_the_sphere_welds_its_coincident_vertices():
    """Section 19's sphere does not meet the premise of the permutation: marching tetrahedra puts up to seven vertices on one lattice point
    where D is 0 there (1 929 distinct positions among the 2 002 vertices, and others up to 3e-7 m apart that differ in their last bits).
    Under a 0.1 mm cell the clusters are those groups, 1 885 of them: every representative lies within 1e-6 m of all its members, and the triangles that stay
    are the input's over cluster_of."""
    m, r = all_cases()["sphere_tiny"], mirrored("sphere_tiny", True)
    assert min_distance(m["vertices"]) == 0.0 and len(np.unique(m["vertices"], axis=0)) == 1929
    perm = r["cluster_of"].astype(np.int64)
    assert 1850 <= r["counts"]["clusters"] <= 1929 and r["counts"]["lost"] == 0
    assert np.abs(r["vertices"][perm].astype(np.float64) - m["vertices"]).max() < 1e-6
    t = perm[m["triangles"]]
    stay = (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])
    assert r["triangles"].tobytes() == t[stay].astype(U32).tobytes() and r["counts"]["collapsed"] == int((~stay).sum())
    one = r["members"] == 1
    first = np.zeros(len(one), np.int64)
    first[perm[::-1]] = np.arange(len(perm))[::-1]
    assert one.sum() > 1800 and r["vertices"][one].tobytes() == m["vertices"][first[one]].tobytes()      # one member: its bits


def test_a_huge_cell_leaves_one_cluster():
    r = mirrored("sphere_huge")
    assert r["counts"] == dict(participating=2002, clusters=1, lost=0, collapsed=4000, duplicate=0, kept=0) and r["members"].tolist() == [2002]


# ---- section 19's sphere ----------------------------------------------------------------------------------------------------------------------
def edges_of(tri):
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64), 1)
    return np.unique(e, axis=0, return_counts=True)


def signed_volume(v, tri):
    p = v.astype(np.float64)[tri.astype(np.int64)]
    return float(np.einsum("ij,ij->i", p[:, 0], np.cross(p[:, 1], p[:, 2])).sum() / 6.0)


@pytest.mark.parametrize("cell, clusters, collapsed, duplicates, kept", [(0.05, 656, 2692, 0, 1308), (0.1, 152, 3700, 0, 300), (0.02, 1306, 1380, 6, 2614)])
def test_sphere_figures(cell, clusters, collapsed, duplicates, kept):
    r = mirrored(f"sphere_{cell}")
    assert r["counts"] == dict(participating=2002, clusters=clusters, lost=0, collapsed=collapsed, duplicate=duplicates, kept=kept)


@pytest.mark.parametrize("cell, n_edges", [(0.05, 1962), (0.1, 450)])
def test_sphere_stays_closed(cell, n_edges):
    r = mirrored(f"sphere_{cell}")
    edges, uses = edges_of(r["triangles"])
    named = len(np.unique(r["triangles"]))
    assert len(edges) == n_edges and (uses == 2).all() and named - len(edges) + len(r["triangles"]) == 2 and named == r["counts"]["clusters"]


def test_sphere_volume_and_orientation():
    r = mirrored("sphere_0.05")
    radius, slack = SPHERE["radius"], np.sqrt(3) * 0.05 + np.sqrt(3) * 0.05
    ball = lambda x: 4.0 / 3.0 * np.pi * x ** 3
    vol = signed_volume(r["vertices"], r["triangles"])
    v, _, tri = tsdf_meshes()["sphere"]
    assert signed_volume(v, tri) > 0 and ball(radius - slack) < vol < ball(radius + slack), (vol, ball(radius))


def test_sphere_has_one_cluster_without_a_triangle_at_015():
    r = mirrored("sphere_0.15")
    assert r["counts"]["clusters"] == 77 and len(np.unique(r["triangles"])) == 76


# ---- where the duplicate search works ---------------------------------------------------------------------------------------------------------
def test_two_sheets_closer_than_the_cell():
    m, r = all_cases()["sheets"], mirrored("sheets")
    half = len(m["triangles"]) // 2
    c = r["counts"]
    assert c["lost"] == 0 and c["duplicate"] == c["kept"] > 100 and 3 * c["duplicate"] >= c["duplicate"] + c["kept"]
    assert (r["classes"][:half] != 2).all() and (r["classes"][half:] != 3).all()           # the earlier sheet's copy stays
    k = mirrored("sheets", True)["triangles"].astype(np.int64)
    fwd = {tuple(t) for t in k[:c["kept"]].tolist()}
    assert k[:c["kept"]].tobytes() == r["triangles"].astype(np.int64).tobytes()
    assert all(tuple(t[::-1]) in fwd for t in k[c["kept"]:].tolist())                         # every triple twice, opposite orientation


def test_random_triangles():
    r = mirrored("random")
    cand = mirrored("random", True)["triangles"]
    _, sizes = np.unique(np.sort(cand, 1), axis=0, return_counts=True)
    # 125 clusters: a triangle collapses with probability about 3 / 125 (480 of 20 000); the 19 500 others fall on C(125, 3) = 317 750
    # sets, 0.061 per set: about 600 sets are hit twice and about 12 three times
    assert r["counts"]["clusters"] == 125 and r["counts"]["collapsed"] > 400 and (sizes == 2).sum() > 500 and (sizes >= 3).sum() > 10
    assert r["counts"]["kept"] == len(sizes) and r["counts"]["duplicate"] == len(cand) - len(sizes)


# ---- the Python checkers, one by one ------------------------------------------------------------------------------------------------------
def test_capacity_and_cell_checkers():
    assert SP.capacity_arg(1, 1) == (1, 1) and SP.capacity_arg(1 << 31, np.int64(1 << 31)) == (1 << 31, 1 << 31)
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 1), (1, (1 << 31) + 1), (-1, 1), (1.0, 1), (1, "1"), (None, 1), (True, 1)):
        with pytest.raises(ValueError):
            SP.capacity_arg(v, t)
    assert SP.cell_arg(0.5) == (0.5, 0.5, 0.5) and SP.cell_arg((0.5, 0.25, 1)) == (0.5, 0.25, 1.0) and SP.cell_arg(np.float32(0.1)) == (float(F(0.1)),) * 3
    assert SP.cell_arg([1, 2, 3]) == (1.0, 2.0, 3.0) and SP.cell_arg(0.1) == (float(F(0.1)),) * 3
    for c in (0, -1, NAN, INF, -INF, 1e-50, 1e39, (1, 2), (1, 2, 3, 4), (1, 0, 1), (1, NAN, 1), "0.1", None, True, [[1, 2, 3]], (1, "x", 2)):
        with pytest.raises(ValueError):
            SP.cell_arg(c)
    assert TS.simplify_arg(None) is None and TS.simplify_arg(0.25) == (0.25, 0.25, 0.25)
    for c in (0, NAN, (1, 2)):
        with pytest.raises(ValueError):
            TS.simplify_arg(c)


def test_mesh_checker_needs_cuda_tensors():
    import torch
    hv, ht = torch.zeros((5, 3), dtype=torch.float32), torch.zeros((4, 3), dtype=torch.int32)
    for v, t in ((hv, ht), (hv.numpy(), ht), (None, ht), (hv, None), ([[0.0, 1.0, 2.0]], ht)):
        with pytest.raises(ValueError):
            SP.mesh_arg(v, t)


def test_checks_come_before_the_library():
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 4)):
        with pytest.raises(ValueError):
            SP.Simplifier(None, v, t)

    class Ctx:
        device = 0
    sp = SP.Simplifier.__new__(SP.Simplifier)
    sp.ctx, sp.max_vertices, sp.max_triangles, sp._mesh, sp.counts = Ctx(), 10, 10, None, None
    for cell in (0, NAN, (1, 2)):
        with pytest.raises(ValueError):
            sp.plan(None, None, cell)
    with pytest.raises(ValueError):
        sp.plan(np.zeros((3, 3), F), np.zeros((1, 3), np.int32), 0.1)
    with pytest.raises(ValueError):
        sp.emit()                                                   # nothing is planned
    sp._h = None
    for kw in (dict(cell=0), dict(cell=-1.0), dict(cell="x")):
        with pytest.raises(ValueError):
            SP.simplify_mesh(None, None, None, None, **kw)
    with pytest.raises(ValueError):
        SP.simplify_mesh(None, None, None, None, cell=0.1)          # no tensors
    kf = [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)]
    for c in (0, -0.1, NAN, INF, (1, 2)):
        with pytest.raises(ValueError):
            TS.fuse(None, kf, (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), simplify=c)
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels = Ctx(), 2, 1000
    for c in (0, NAN):
        with pytest.raises(ValueError):
            vol.extract(1, simplify=c)
    vol._h = None


def test_nothing_is_imported_without_the_option():
    code = ("import sys; sys.path[:0] = [%r, %r]; from rgbid import tsdf as TS; assert TS.simplify_arg(None) is None; "
            "assert 'rgbid.simplify' not in sys.modules; TS.simplify_arg(0.1); assert 'rgbid.simplify' in sys.modules") % (
                ROOT, os.path.join(ROOT, "rgbid-slam_amd"))
    subprocess.check_call([sys.executable, "-c", code])


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_simplify.c"
    src.write_text('#include "rgbid_simplify.h"\n'
                   "int use(rgbid_simplify* h, rgbid_ctx* ctx, const float* v, const uint32_t* tris, const uint8_t* c, const float* n, float* vo,\n"
                   "        uint8_t* co, float* no, uint32_t* mo, uint32_t* cl, uint32_t* to) {\n"
                   "  long long grid[6]; unsigned long long counts[6]; float ms[3]; const float cell[3] = {0.1f, 0.1f, 0.1f};\n"
                   "  return rgbid_simplify_create(&h, ctx, RGBID_SIMPLIFY_MAX_VERTICES, RGBID_SIMPLIFY_MAX_TRIANGLES)\n"
                   "       + rgbid_simplify_plan(h, 10, v, 5, tris, cell, RGBID_SIMPLIFY_KEEP_DUPLICATES, grid, counts)\n"
                   "       + rgbid_simplify_emit(h, c, n, vo, co, no, mo, cl, to, counts[1], counts[5]) + rgbid_simplify_timing(h, 1, ms)\n"
                   "       + rgbid_simplify_destroy(h) + (cl[0] == RGBID_SIMPLIFY_NO_CLUSTER); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_simplify.h")).read()
    assert int(re.search(r"RGBID_SIMPLIFY_MAX_VERTICES\s+(\d+)ull", txt).group(1)) == SP.MAX_VERTICES == 1 << 31
    assert int(re.search(r"RGBID_SIMPLIFY_MAX_TRIANGLES\s+(\d+)ull", txt).group(1)) == SP.MAX_TRIANGLES == 1 << 31
    assert int(re.search(r"RGBID_SIMPLIFY_NO_CLUSTER\s+0x([0-9A-F]+)u", txt).group(1), 16) == SP.NO_CLUSTER == SM.NO_CLUSTER
    assert int(re.search(r"RGBID_SIMPLIFY_KEEP_DUPLICATES\s+(\d+)u", txt).group(1)) == SP.KEEP_DUPLICATES


def test_library_exports_simplify_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_simplify.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_simplify_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(SP.EXPORTS) and len(declared) == 5, set(declared) ^ set(SP.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    L.rgbid_simplify_create.argtypes = [c.c_void_p, c.c_void_p, c.c_ulonglong, c.c_ulonglong]
    L.rgbid_simplify_plan.argtypes = [c.c_void_p, c.c_ulonglong, c.c_void_p, c.c_ulonglong, c.c_void_p, c.c_void_p, c.c_uint32, c.c_void_p, c.c_void_p]
    L.rgbid_simplify_emit.argtypes = [c.c_void_p] * 9 + [c.c_ulonglong] * 2
    L.rgbid_simplify_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_simplify_destroy.argtypes = [c.c_void_p]
    h = c.c_void_p()
    assert L.rgbid_simplify_create(c.byref(h), None, 10, 10) == -1 and not h.value and L.rgbid_simplify_create(None, None, 10, 10) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 31) + 1)):
        assert L.rgbid_simplify_create(c.byref(h), fake, v, t) == -1 and not h.value
    cell = (c.c_float * 3)(0.1, 0.1, 0.1)
    assert L.rgbid_simplify_plan(None, 0, None, 0, None, cell, 0, None, None) == -1
    assert L.rgbid_simplify_emit(None, *([None] * 8), 0, 0) == -1
    assert L.rgbid_simplify_timing(None, 0, None) == -1 and L.rgbid_simplify_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-simplify", "0.05"], "--mesh-simplify needs --mesh"), (mesh_opt + ["--mesh-simplify", "0"], "cell: every edge finite"),
                      (mesh_opt + ["--mesh-simplify", "-0.05"], "cell: every edge finite"), (mesh_opt + ["--mesh-simplify", "nan"], "cell: every edge finite"),
                      (mesh_opt + ["--mesh-simplify", "inf"], "cell: every edge finite"), (mesh_opt + ["--mesh-simplify", "x"], "invalid float value")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()


def test_simplified_mesh_through_the_ply_writer(tmp_path):
    r = mirrored("sphere_0.05")
    path = tmp_path / "simplified.ply"
    TS.write_mesh_ply(str(path), r["vertices"], r["colours"], r["triangles"], r["normals"])
    pv, pc, pt, pn = TS.read_mesh_ply(path.read_bytes())
    assert pv.tobytes() == r["vertices"].tobytes() and pc.tobytes() == r["colours"].tobytes() and pt.tobytes() == r["triangles"].tobytes()
    assert pn.tobytes() == r["normals"].tobytes() and len(pt) == 1308 and len(pv) == 656
