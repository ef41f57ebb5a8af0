"""CPU checks of the point-to-mesh distance stage (include/rgbid_meshdist.h, rgbid.meshdist): the vectorised numpy restatement the GPU tests
compare the kernels against (tests/meshdist_mirror.py) against its scalar loops; the unit triangle's seven regions by hand; degenerate
triangles; ties; truncation at d_max to the ulp; vertices on their own mesh; section 19's sphere against the analytic one; the grid's
cover statement on adversarial pairs, its restatement against a dictionary of lists, the pair count and its refusal; the Python argument
checks one by one; the header as C99; the library's exports; the command lines' option errors; `summary` on a hand-made tensor."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from rgbid import _lib
from rgbid import meshdist as MD
from tests import meshdist_mirror as DM
from tests.test_cpu_mesh import tsdf_meshes
from tests.test_cpu_tsdf import SPHERE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, F64, U32 = np.float32, np.float64, np.uint32
NAN, INF = float("nan"), float("inf")
NONE = DM.NONE
UNIT = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
SEVEN = [(.25, .25, .5), (-1, -1, 0), (.5, -1, 0), (1, 1, 0), (2, -1, 0), (-1, .5, 0), (-1, 2, 0)]
VOXEL = 0.05                                                # of section 19's sphere


def up(x, towards=INF):
    return np.nextafter(F(x), F(towards))


# ---- the cases the GPU tests share: name -> dict(vertices, triangles, points, d_max) -------------------------------------------------------------
def case(vertices, triangles, points, d_max):
    return dict(vertices=np.array(vertices, F).reshape(-1, 3), triangles=np.array(triangles, U32).reshape(-1, 3),
                points=np.array(points, F).reshape(-1, 3), d_max=d_max)


def region_mesh():
    """about 40 random triangles and 60 queries around them that reach all seven regions, with duplicates, a sliver and a point triangle"""
    rng = np.random.default_rng(26)
    v = rng.uniform(-1, 1, (60, 3)).astype(F)
    t = rng.integers(0, 60, (36, 3))
    t = np.concatenate([t, t[:2], [(0, 0, 1), (5, 5, 5), (7, 8, 7)]])
    c = v[t[rng.integers(0, 36, 60)]].astype(F64)
    w = rng.dirichlet((0.3, 0.3, 0.3), 60)
    q = np.einsum("ik,ikj->ij", w * 1.6 - 0.2, c) + rng.normal(0, 0.05, (60, 3))
    return case(v, t, q, 0.75)


def plane_mesh(n=6, h=0.5):
    """a plane of 2 n n triangles at z = 0 over [0, n h]^2"""
    g = np.arange(n + 1) * h
    x, y = np.meshgrid(g, g, indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), np.zeros(x.size)], 1)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a, b, c, d = (i * (n + 1) + j).ravel(), ((i + 1) * (n + 1) + j).ravel(), (i * (n + 1) + j + 1).ravel(), ((i + 1) * (n + 1) + j + 1).ravel()
    return v.astype(F), np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)]).astype(U32)


def truncation_case():
    """d_max = 0.25 over the plane: heights 0.25 (d2 = 0.0625 exactly) and one ulp above; x = lo - 0.25 beside a corner and one ulp out"""
    v, t = plane_mesh()
    q = [(1.3, 1.1, 0.25), (1.3, 1.1, up(0.25)), (1.3, 1.1, -0.25), (1.3, 1.1, -up(0.25)), (-0.25, 0.0, 0.0), (up(-0.25, -INF), 0.0, 0.0),
         (-0.25, 0.7, 0.0), (3.25, 3.0, 0.0), (up(3.25), 3.0, 0.0), (1.0, 1.0, 0.0), (0.5, 0.25, 0.125)]
    return case(v, t, q, 0.25)


def tie_case():
    """the unit triangle three times (the second with its corners rotated) behind a far one: the smallest index among equal d2 wins"""
    v = UNIT + [(5, 5, 5), (6, 5, 5), (5, 6, 5)]
    return case(v, [(3, 4, 5), (0, 1, 2), (1, 2, 0), (0, 1, 2)], SEVEN + [(5.1, 5.1, 5.2)], 4.0)


def degenerate_case():
    """the collinear triangle, the point triangle, and a = b != c whose edge region divides 0 by 0, each alone in its corner of space"""
    v = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (10, 0, 0), (20, 0, 0), (20, 0, 0), (20, 1, 0)]
    t = [(0, 1, 2), (3, 3, 3), (4, 5, 6)]
    q = SEVEN + [(x + 10, y, z) for x, y, z in SEVEN] + [(20.5, 0.5, 0.0), (20.0, -1.0, 0.0), (20.0, 2.0, 0.0)]
    return case(v, t, q, 3.0)


def poisoned_case():
    """triangles with NaN or infinite corners among good ones, non-finite queries among finite ones"""
    m = region_mesh()
    v = m["vertices"].copy()
    v[3, 1], v[11, 0], v[20, 2] = NAN, INF, -INF
    q = m["points"].copy()
    q[5, 0], q[17, 2], q[40, 1], q[41] = NAN, INF, -INF, (NAN, NAN, NAN)
    return case(v, m["triangles"], q, 0.75)


def sphere_mesh():
    v, _, t = tsdf_meshes()["sphere"]
    return v, t


def sphere_points(n=2000, seed=5, radius=None):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (np.array(SPHERE["centre"]) + (SPHERE["radius"] if radius is None else radius) * d).astype(F)


def sphere_case(voxels, n=2000):
    v, t = sphere_mesh()
    return case(v, t, sphere_points(n), voxels * VOXEL)


def big_triangles_case():
    """two 1 m triangles over 2 cm cells: each lies in thousands of cells"""
    v = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.3)]
    rng = np.random.default_rng(9)
    q = np.concatenate([rng.uniform(-0.05, 1.05, (300, 3)) * (1, 1, 0.3), [(0.5, 0.5, 0.01), (0.5, 0.5, 0.02), (-0.01, -0.01, 0)]])
    return case(v, [(0, 1, 2), (1, 3, 2)], q, 0.02 / 1.0625)


@functools.lru_cache(maxsize=None)
def all_cases():
    unit = case(UNIT, [(0, 1, 2)], SEVEN, 2.0)
    return {"unit": unit, "regions": region_mesh(), "truncation": truncation_case(), "ties": tie_case(), "degenerate": degenerate_case(),
            "poisoned": poisoned_case(), "sphere_1": sphere_case(1, 700), "sphere_2": sphere_case(2, 700), "sphere_6": sphere_case(6, 700),
            "big_triangles": big_triangles_case(),
            "nobody_takes_part": case([(NAN, 0, 0), (0, 1, 0), (1, 0, 0)], [(0, 1, 2), (0, 0, 0)], SEVEN, 1.0),
            "no_triangles": case(UNIT, [], SEVEN, 1.0), "no_vertices": case([], [], SEVEN, 1.0)}


@functools.lru_cache(maxsize=None)
def mirrored(name):
    """the vectorised mirror's result of a case (with the grid's figures and the candidates), computed once and shared with the GPU tests"""
    m = all_cases()[name]
    r = DM.query(m["vertices"], m["triangles"], m["points"], m["d_max"])
    r["plan"] = DM.plan(m["vertices"], m["triangles"], m["d_max"])
    r["candidates"] = DM.candidates(r["plan"], m["points"])
    return r


# ---- mirror against loop --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unit", "regions", "truncation", "ties", "degenerate", "poisoned", "nobody_takes_part", "no_triangles", "no_vertices"])
def test_mirror_equals_the_loops(name):
    m, a = all_cases()[name], mirrored(name)
    b = DM.query_loop(m["vertices"], m["triangles"], m["points"], m["d_max"])
    assert DM.same(a, b) == [] and a["d2"].tobytes() == b["d2"].tobytes(), (name, DM.same(a, b))
    assert a["triangle"].dtype == U32 and a["distance"].dtype == F and a["closest"].dtype == F and a["region"].dtype == np.uint8
    lost = a["triangle"] == NONE
    assert (a["distance"][lost].view(U32) == DM.NAN_BITS).all() and (a["closest"][lost].view(U32) == DM.NAN_BITS).all() and (a["region"][lost] == 255).all()
    assert np.isfinite(a["distance"][~lost]).all() and (a["region"][~lost] <= 6).all()


def test_the_random_mesh_reaches_every_region():
    a = mirrored("regions")
    assert sorted(set(a["region"].tolist()) - {255}) == [0, 1, 2, 3, 4, 5, 6], np.bincount(a["region"])
    assert len(all_cases()["regions"]["triangles"]) == 41 and len(a["triangle"]) == 60


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------------
def test_unit_triangle():
    a = mirrored("unit")
    assert a["d2"].tolist() == [0.25, 2.0, 1.0, 0.5, 2.0, 1.0, 2.0]
    assert a["region"].tolist() == [6, 0, 3, 5, 1, 4, 2] and a["triangle"].tolist() == [0] * 7
    assert a["closest"].tolist() == [[.25, .25, 0], [0, 0, 0], [.5, 0, 0], [.5, .5, 0], [1, 0, 0], [0, .5, 0], [0, 1, 0]]
    assert a["distance"].tolist() == [F(np.sqrt(x)) for x in (0.25, 2.0, 1.0, 0.5, 2.0, 1.0, 2.0)]


def test_degenerate_triangles():
    a = mirrored("degenerate")
    assert a["d2"][:7].tolist() == [0.3125, 2, 1, 1, 1, 1.25, 5] and a["triangle"][:7].tolist() == [0] * 7
    assert a["d2"][7:14].tolist() == [0.375, 2, 1.25, 2, 5, 1.25, 5] and a["triangle"][7:14].tolist() == [1] * 7 and a["region"][7:14].tolist() == [0] * 7
    # a = b: beside the edge a c the region AB holds with v = 0 / 0, the point and d2 are NaN and the pair does not compete; before a and
    # behind c the vertex regions answer
    p, v, t = all_cases()["degenerate"]["points"], all_cases()["degenerate"]["vertices"].astype(F64), all_cases()["degenerate"]["triangles"]
    r, region = DM.closest_points(p[14:15].astype(F64), *(v[t[2, k]][None] for k in range(3)))
    assert region.tolist() == [3] and np.isnan(r).all()
    assert a["triangle"][14:].tolist() == [NONE, 2, 2] and a["region"][14:].tolist() == [255, 0, 2] and a["d2"][15:].tolist() == [1, 1]
    assert a["distance"][14:15].view(U32).tolist() == [DM.NAN_BITS]


def test_ties_go_to_the_smaller_index():
    a = mirrored("ties")
    assert a["triangle"].tolist() == [1] * 7 + [0]
    assert a["d2"][:7].tolist() == mirrored("unit")["d2"].tolist()
    # the rotated copy alone names the regions differently and gives the same distances
    m = all_cases()["ties"]
    b = DM.query(m["vertices"], m["triangles"][2:3], m["points"][:7], 4.0)
    assert b["d2"].tolist() == a["d2"][:7].tolist() and b["region"].tolist() != a["region"][:7].tolist()


def test_truncation_to_the_ulp():
    a = mirrored("truncation")
    won = (a["triangle"] != NONE).tolist()
    assert won == [True, False, True, False, True, False, True, True, False, True, True]
    assert a["d2"][[0, 2, 4, 6, 7]].tolist() == [0.0625] * 5 and a["distance"][[0, 2, 4, 6, 7]].tolist() == [0.25] * 5
    assert a["d2"][9] == 0 and a["region"][9] <= 2 and a["d2"][10] == 0.015625


@pytest.mark.parametrize("name", ["regions", "sphere_2"])
def test_vertices_lie_on_their_own_mesh(name):
    m = all_cases()[name]
    named = np.unique(m["triangles"])
    a = DM.query(m["vertices"], m["triangles"], m["vertices"][named], m["d_max"])
    assert (a["d2"] == 0).all() and (a["distance"] == 0).all() and (a["region"] <= 2).all()
    assert a["closest"].tobytes() == m["vertices"][named].tobytes()


def test_sphere_points_lie_within_the_voxel_diagonal():
    """test_cpu_tsdf.py asserts that the mesh is closed, encloses the centre and lies between the balls r -+ sqrt(3) voxel: a point on the
    analytic sphere is then within sqrt(3) voxel of the surface, and with d_max there every query is matched"""
    v, t = sphere_mesh()
    assert v.shape == (2002, 3) and t.shape == (4000, 3)
    bound = np.sqrt(3) * VOXEL
    q = sphere_points(2000)
    a = DM.query(v, t, q, bound)
    assert (a["triangle"] != NONE).all() and float(a["distance"].max()) <= bound
    print("sphere: distance of 2 000 analytic points: median %.5f max %.5f m (bound %.5f)" % (np.median(a["distance"]), a["distance"].max(), bound))
    b = mirrored("sphere_2")
    assert (b["triangle"] != NONE).all() and b["distance"].tobytes() == a["distance"][:700].tobytes()
    c = mirrored("sphere_1")
    assert c["distance"].tobytes() == np.where(a["distance"][:700] <= F(VOXEL), a["distance"][:700], np.array([DM.NAN_BITS], U32).view(F)).tobytes()


# ---- the grid --------------------------------------------------------------------------------------------------------------------------------
def test_grid_cover_on_adversarial_pairs():
    """DESIGN.md section 26's statement: a pair that passes step 3 has the triangle's cell range within one cell of the query's cell on
    every axis.  One axis, 3 M pairs: q at lo - d_max and hi + d_max and an ulp either side, on cell borders, cell indices up to 2^18,
    d_max from 2^-8 to 8."""
    rng = np.random.default_rng(15)
    n, bad, passed = 250_000, 0, 0
    for e in range(-8, 4):
        dm = F(2.0 ** e) * F(rng.uniform(1.0, 2.0)) if e % 2 else F(2.0 ** e)
        cell = dm * DM.CELL_FACTOR
        inv = F(1.0) / cell
        base = rng.integers(-(1 << 18) + 4, (1 << 18) - 4, n).astype(F64)
        lo = (base * float(cell)).astype(F)
        kind = rng.integers(0, 3, n)
        lo = np.where(kind == 0, lo, np.nextafter(lo, np.where(kind == 1, F(INF), F(-INF)))).astype(F)     # on a cell border and beside it
        hi = (lo + (rng.integers(0, 3, n) * rng.uniform(0, 2, n)).astype(F) * cell).astype(F)
        side = rng.integers(0, 2, n).astype(bool)
        q = np.where(side, lo - dm, hi + dm).astype(F)
        step = rng.integers(-2, 3, n)
        for _ in range(2):
            q = np.where(step > 0, np.nextafter(q, F(INF)), np.where(step < 0, np.nextafter(q, F(-INF)), q)).astype(F)
            step -= np.sign(step)
        q64 = q.astype(F64)
        ok = np.abs(q64 - np.minimum(np.maximum(q64, lo.astype(F64)), hi.astype(F64))) <= F64(dm)
        cq, clo, chi = np.floor(q * inv), np.floor(lo * inv), np.floor(hi * inv)
        keep = ok & (np.abs(clo) <= 1 << 18) & (np.abs(chi) <= 1 << 18)
        bad += int((keep & ~((clo <= cq + 1) & (chi >= cq - 1))).sum())
        passed += int(keep.sum())
    assert bad == 0 and passed > 1_000_000, (bad, passed)


@pytest.mark.parametrize("name", ["regions", "truncation", "poisoned", "big_triangles", "sphere_2"])
def test_grid_restatement_against_a_dictionary(name):
    m, pl = all_cases()[name], mirrored(name)["plan"]
    loop = DM.plan_loop(m["vertices"], m["triangles"], m["d_max"])
    assert pl["pairs"] == sum(len(x) for x in loop["cells"].values()) == len(pl["keys"]) and pl["cells"] == len(loop["cells"])
    assert pl["longest_run"] == max(len(x) for x in loop["cells"].values())
    d0, d1 = int(pl["div"][0]), int(pl["div"][1])
    for c in range(pl["cells"]):
        key = int(pl["ukeys"][c])
        ijk = tuple(int(x) for x in np.array([key % d0, key // d0 % d1, key // (d0 * d1)]) + pl["min_b"])
        run = pl["tris"][pl["starts"][c]:pl["starts"][c + 1]].tolist()
        assert run == loop["cells"][ijk] and run == sorted(run)           # ascending triangle index
    rng = np.random.default_rng(3)
    lo, hi = np.nanmin(np.where(np.isfinite(m["vertices"]), m["vertices"], NAN), 0), np.nanmax(np.where(np.isfinite(m["vertices"]), m["vertices"], NAN), 0)
    far = rng.uniform(lo - 3 * float(pl["inv"]) ** -1, hi + 3 * float(pl["inv"]) ** -1, (300, 3)).astype(F)
    q = np.concatenate([m["points"], far, [(NAN, 0, 0), (INF, 0, 0), (3e38, 3e38, 3e38), (-3e38, 0, 0)]]).astype(F)
    assert DM.candidates(pl, q).tolist() == DM.candidates_loop(loop, q).tolist()
    assert mirrored(name)["candidates"].tolist() == DM.candidates_loop(loop, m["points"]).tolist()


def test_a_match_is_always_among_the_candidates():
    """the cover statement end to end: the brute-force winner's triangle lies in one of the 27 runs its query walks"""
    for name in ("regions", "truncation", "big_triangles", "sphere_6"):
        m, a = all_cases()[name], mirrored(name)
        loop = DM.plan_loop(m["vertices"], m["triangles"], m["d_max"])
        for p, t in zip(m["points"], a["triangle"]):
            if t != NONE:
                i, j, k = (int(x) for x in np.floor(p * loop["inv"]))
                assert any(int(t) in loop["cells"].get((i + a_, j + b_, k + c_), ()) for a_ in (-1, 0, 1) for b_ in (-1, 0, 1) for c_ in (-1, 0, 1))


def test_pair_count_and_its_refusal():
    v = [(0.1, 0.1, 0.5), (4.9, 0.1, 0.5), (0.1, 3.9, 0.5), (NAN, 0, 0)]
    pl = DM.plan(v, [(0, 1, 2), (0, 1, 3)], 0.5, cell=1.0)                 # 5 x 4 x 1 cells; the second triangle takes no part
    assert pl["pairs"] == 20 and pl["participating"] == 1 and pl["cells"] == 20 and pl["longest_run"] == 1 and pl["grid"].tolist() == [0, 0, 0, 5, 4, 1]
    assert DM.plan(v, [(0, 1, 2)], 0.5, cell=1.0, max_pairs=20)["pairs"] == 20
    with pytest.raises(ValueError) as e:
        DM.plan(v, [(0, 1, 2)], 0.5, cell=1.0, max_pairs=19)
    assert e.value.args[1] == 20
    b = mirrored("big_triangles")["plan"]
    assert b["pairs"] > 4096 and b["longest_run"] == 2 and b["participating"] == 2
    for bad in (dict(cell=0.5), dict(cell=NAN), dict(cell=INF), dict(cell=0.53)):
        with pytest.raises(ValueError):
            DM.plan(v, [(0, 1, 2)], 0.5, **bad)
    with pytest.raises(ValueError):
        DM.plan([(0, 0, 0), (1e6, 0, 0), (0, 1, 0)], [(0, 1, 2)], 1.0)           # 2^18 cells of 1.0625 m end at 278 km
    with pytest.raises(ValueError):
        DM.plan(UNIT, [(0, 1, 3)], 1.0)


# ---- the Python checkers, one by one -------------------------------------------------------------------------------------------------------
def test_capacity_distance_and_cell_checkers():
    assert MD.capacity_arg(1, 1, 1, 1) == (1, 1, 1, 1) and MD.capacity_arg(1 << 31, 2, np.int64(1 << 31), 1 << 31) == (1 << 31, 2, 1 << 31, 1 << 31)
    good = [1, 1, 1, 1]
    for k in range(4):
        for bad in (0, (1 << 31) + 1, -1, 1.0, "1", None, True):
            with pytest.raises(ValueError):
                MD.capacity_arg(*(good[:k] + [bad] + good[k + 1:]))
    assert MD.distance_arg(0.1) == float(F(0.1)) and MD.distance_arg(2.0 ** -60) == 2.0 ** -60 and MD.distance_arg(F(2.0) ** 60) == 2.0 ** 60
    for d in (0, -1, NAN, INF, -INF, 2.0 ** -61, 2.0 ** 61, 1e-50, 1e39, "0.1", None, True, (1, 2)):
        with pytest.raises(ValueError):
            MD.distance_arg(d)
    assert MD.cell_arg(None, 0.5) == 0.53125 and MD.cell_arg(0.53125, 0.5) == 0.53125 and MD.cell_arg(1, 0.5) == 1.0
    assert MD.cell_arg(None, 0.1) == float(F(0.1) * F(1.0625)) == float(DM.cell_size(0.1))
    for c in (0.5, 0.53, 0, -1, NAN, INF, "1", True, (1, 2), 1e39):
        with pytest.raises(ValueError):
            MD.cell_arg(c, 0.5)
    with pytest.raises(ValueError):
        MD.cell_arg(1.0, NAN)
    assert MD.outputs_arg(("distance", "triangle")) == ("triangle", "distance") and MD.outputs_arg("closest") == ("closest",)
    assert MD.outputs_arg(MD.OUTPUTS[::-1]) == MD.OUTPUTS
    for o in ((), ("depth",), ("distance", "distance"), None, 3, (1,), ("distance", None)):
        with pytest.raises(ValueError):
            MD.outputs_arg(o)


def test_tensor_checkers_need_cuda_tensors():
    hv, ht = torch.zeros((5, 3), dtype=torch.float32), torch.zeros((4, 3), dtype=torch.int32)
    for v, t in ((hv, ht), (hv.numpy(), ht), (None, ht), (hv, None), ([[0.0, 1.0, 2.0]], ht)):
        with pytest.raises(ValueError):
            MD.mesh_arg(v, t)
    for p in (hv, hv.numpy(), None, [[0.0, 0.0, 0.0]]):
        with pytest.raises(ValueError):
            MD.points_arg(p)
    for r in (torch.zeros((4, 32), dtype=torch.uint8), torch.zeros((4, 32)), np.zeros((4, 32), np.uint8), None):
        with pytest.raises(ValueError):
            MD.records_arg(r)


def test_checks_come_before_the_library():
    for caps in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, (1 << 31) + 1, 1)):
        with pytest.raises(ValueError):
            MD.Distance(None, *caps)

    class Ctx:
        device = 0
    d = MD.Distance.__new__(MD.Distance)
    d.ctx, d.max_vertices, d.max_triangles, d.max_pairs, d.max_queries, d.planned, d.needed_pairs = Ctx(), 10, 10, 10, 10, None, None
    for dm in (0, NAN, -1.0, "x"):
        with pytest.raises(ValueError):
            d.plan(None, None, dm)
    with pytest.raises(ValueError):
        d.plan(None, None, 1.0, cell=1.0)                           # below 1.0625
    with pytest.raises(ValueError):
        d.plan(np.zeros((3, 3), F), np.zeros((1, 3), np.int32), 0.1)
    with pytest.raises(ValueError):
        d.query(None)
    with pytest.raises(ValueError):
        d.query_records(None)
    with pytest.raises(ValueError):
        d.query(None, outputs=("nothing",))
    d._h = None
    for f in (lambda: MD.mesh_deviation(None, None, None, None, None, 0.1), lambda: MD.cloud_deviation(None, None, None, None, 0.1),
              lambda: MD.point_deviation(None, None, None, None, 0.1)):
        with pytest.raises(ValueError):
            f()
    assert "vertex-sampled" in MD.mesh_deviation.__doc__ and "truncated" in MD.mesh_deviation.__doc__


def test_summary_on_a_hand_made_tensor():
    nan = float("nan")
    s = MD.summary(torch.tensor([3.0, nan, 1.0, 2.0, nan, 4.0, 0.0, 0.0, 6.0, 4.0, 10.0, 0.0], dtype=torch.float32))
    assert s == dict(queries=12, matched=10, mean=3.0, rms=float(np.sqrt(182 / 10)), median=2.0, p90=6.0, max=10.0)
    e = MD.summary(torch.tensor([nan, nan], dtype=torch.float32))
    assert e["queries"] == 2 and e["matched"] == 0 and all(np.isnan(e[k]) for k in ("mean", "rms", "median", "p90", "max"))
    assert MD.summary(torch.zeros(0, dtype=torch.float32))["matched"] == 0
    assert MD.summary(torch.tensor([0.5], dtype=torch.float32)) == dict(queries=1, matched=1, mean=0.5, rms=0.5, median=0.5, p90=0.5, max=0.5)
    for bad in (np.zeros(3, F), torch.zeros(3, dtype=torch.float64), torch.zeros((3, 1))):
        with pytest.raises(ValueError):
            MD.summary(bad)
    assert "3 of 4 matched" in MD.summary_line(dict(queries=4, matched=3, mean=1, rms=1, median=1, p90=1, max=1))


# ---- the boundary ------------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_meshdist.c"
    src.write_text('#include "rgbid_meshdist.h"\n'
                   "int use(rgbid_meshdist* h, rgbid_ctx* ctx, const float* v, const uint32_t* tris, const float* q, const rgbid_cloud_point* rec,\n"
                   "        uint32_t* to, float* d, float* c, uint8_t* r, uint32_t* n) {\n"
                   "  long long grid[6]; unsigned long long stats[4]; float ms[5];\n"
                   "  return rgbid_meshdist_create(&h, ctx, RGBID_MESHDIST_MAX_VERTICES, RGBID_MESHDIST_MAX_TRIANGLES, RGBID_MESHDIST_MAX_PAIRS,\n"
                   "                               RGBID_MESHDIST_MAX_QUERIES)\n"
                   "       + rgbid_meshdist_plan(h, 10, v, 5, tris, RGBID_MESHDIST_MIN_DISTANCE, RGBID_MESHDIST_MAX_DISTANCE * RGBID_MESHDIST_CELL_FACTOR, grid, stats)\n"
                   "       + rgbid_meshdist_query(h, 7, q, to, d, c, r, n) + rgbid_meshdist_query_records(h, 7, rec, to, d, c, r, n)\n"
                   "       + rgbid_meshdist_set_query_sort(h, 0) + rgbid_meshdist_timing(h, 1, ms) + rgbid_meshdist_destroy(h)\n"
                   "       + (to[0] == RGBID_MESHDIST_NONE) + (r[0] == RGBID_MESHDIST_NO_REGION) + (grid[0] > RGBID_MESHDIST_MAX_CELL); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_meshdist.h")).read()
    for name, value in (("MAX_VERTICES", MD.MAX_VERTICES), ("MAX_TRIANGLES", MD.MAX_TRIANGLES), ("MAX_PAIRS", MD.MAX_PAIRS), ("MAX_QUERIES", MD.MAX_QUERIES)):
        assert int(re.search(r"RGBID_MESHDIST_%s\s+(\d+)ull" % name, txt).group(1)) == value == 1 << 31
    assert int(re.search(r"RGBID_MESHDIST_NONE\s+0x([0-9A-F]+)u", txt).group(1), 16) == MD.NONE == DM.NONE
    assert int(re.search(r"RGBID_MESHDIST_NO_REGION\s+(\d+)", txt).group(1)) == MD.NO_REGION == DM.NO_REGION
    assert int(re.search(r"RGBID_MESHDIST_MAX_CELL\s+(\d+)", txt).group(1)) == MD.MAX_CELL == DM.MAX_CELL
    assert F(re.search(r"RGBID_MESHDIST_CELL_FACTOR\s+([0-9.]+)f", txt).group(1)) == MD.CELL_FACTOR == DM.CELL_FACTOR
    assert float(re.search(r"RGBID_MESHDIST_MIN_DISTANCE\s+([0-9.e-]+)f", txt).group(1)) == MD.MIN_DISTANCE == DM.MIN_DISTANCE
    assert float(re.search(r"RGBID_MESHDIST_MAX_DISTANCE\s+([0-9.e-]+)f", txt).group(1)) == MD.MAX_DISTANCE == DM.MAX_DISTANCE
    render = open(os.path.join(ROOT, "include", "rgbid_render.h")).read()
    assert int(re.search(r"RGBID_RENDER_NAN_BITS\s+0x([0-9A-F]+)u", render).group(1), 16) == DM.NAN_BITS


def test_library_exports_meshdist_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_meshdist.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_meshdist_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(MD.MESHDIST_EXPORTS) and len(declared) == 7, set(declared) ^ set(MD.MESHDIST_EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    L.rgbid_meshdist_create.argtypes = [c.c_void_p, c.c_void_p] + [c.c_ulonglong] * 4
    L.rgbid_meshdist_plan.argtypes = [c.c_void_p, c.c_ulonglong, c.c_void_p, c.c_ulonglong, c.c_void_p, c.c_float, c.c_float, c.c_void_p, c.c_void_p]
    L.rgbid_meshdist_query.argtypes = [c.c_void_p, c.c_ulonglong] + [c.c_void_p] * 6
    L.rgbid_meshdist_query_records.argtypes = [c.c_void_p, c.c_ulonglong] + [c.c_void_p] * 6
    L.rgbid_meshdist_set_query_sort.argtypes = [c.c_void_p, c.c_int]
    L.rgbid_meshdist_timing.argtypes = [c.c_void_p, c.c_int, c.c_void_p]
    L.rgbid_meshdist_destroy.argtypes = [c.c_void_p]
    h = c.c_void_p()
    assert L.rgbid_meshdist_create(c.byref(h), None, 10, 10, 10, 10) == -1 and not h.value and L.rgbid_meshdist_create(None, None, 10, 10, 10, 10) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    big = (1 << 31) + 1
    for caps in ((0, 10, 10, 10), (10, 0, 10, 10), (10, 10, 0, 10), (10, 10, 10, 0), (big, 10, 10, 10), (10, big, 10, 10), (10, 10, big, 10), (10, 10, 10, big)):
        assert L.rgbid_meshdist_create(c.byref(h), fake, *caps) == -1 and not h.value
    assert L.rgbid_meshdist_plan(None, 0, None, 0, None, 0.1, 0.0, None, None) == -1
    assert L.rgbid_meshdist_query(None, 0, None, *([None] * 5)) == -1 and L.rgbid_meshdist_query_records(None, 0, None, *([None] * 5)) == -1
    assert L.rgbid_meshdist_set_query_sort(None, 1) == -1
    assert L.rgbid_meshdist_timing(None, 0, None) == -1 and L.rgbid_meshdist_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-deviation", "0.1"], "need --mesh"), (["--mesh-reference", "x.ply"], "need --mesh"),
                      (mesh_opt + ["--mesh-deviation", "0.1"], "--mesh-deviation needs at least one of"),
                      (mesh_opt + ["--mesh-simplify", "0.1", "--mesh-deviation", "0"], "d_max must be finite and > 0"),
                      (mesh_opt + ["--mesh-simplify", "0.1", "--mesh-deviation", "nan"], "d_max must be finite and > 0"),
                      (mesh_opt + ["--mesh-simplify", "0.1", "--mesh-deviation", "x"], "invalid float value"),
                      (mesh_opt + ["--mesh-reference-distance", "0.1"], "--mesh-reference-distance needs --mesh-reference"),
                      (mesh_opt + ["--mesh-reference", str(tmp_path / "absent.ply")], "--mesh-reference: cannot read"),
                      (mesh_opt + ["--mesh-reference", __file__, "--mesh-reference-distance", "-1"], "d_max must be finite and > 0")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()
    tool = os.path.join(ROOT, "tools", "mesh_compare.py")
    a = str(tmp_path / "a.ply")
    for bad, word in (([a], "the following arguments are required"), ([a, a], "--max-distance"), ([a, a, "--max-distance", "0"], "d_max must be finite and > 0"),
                      ([a, a, "--max-distance", "1", "--cell", "0.5"], "cell must be at least"), ([a, a, "--max-distance", "1"], "cannot read")):
        r = subprocess.run([sys.executable, tool] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
