"""CPU checks of the hole-filling stage (include/rgbid_holes.h, rgbid.holes): the vectorised numpy restatement the GPU tests compare the
kernels against (tests/holes_mirror.py) against its scalar loops on every mesh below, and by hand what each mesh is about: section 19's
sphere whole and punched, with the figures of the issue; flat annuli as built and with their vertices renumbered (the order of the centre's
sum); the open tetrahedron; the meshes of the component filter's tests; a hand-built mesh with holes that touch, edges named twice and
three times, degenerate triangles, non-finite vertices, a non-finite owner, loops either side of max_edges, colours that round at .5 and
normals that cancel; idempotence; the Python argument checks one by one; the header as C99; the library's exports; the command line's
option errors; a filled mesh through the PLY writer."""
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
from rgbid import holes as HO
from rgbid import tsdf as TS
from tests import holes_mirror as HM
from tests.test_cpu_mesh import hard_meshes, tsdf_meshes
from tests.test_cpu_simplify import signed_volume

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U32, U8 = np.float32, np.uint32, np.uint8
NAN, INF = float("nan"), float("inf")
ANNULI = (3, 4, 63, 64, 65, 2048)


def mesh(vertices, triangles, colours=None, normals=None):
    return dict(vertices=np.array(vertices, F).reshape(-1, 3), triangles=np.array(triangles, U32).reshape(-1, 3), colours=colours, normals=normals)


# ---- the meshes: name -> dict(vertices float32 [n_v, 3], triangles uint32 [n_t, 3], colours, normals) --------------------------------------
def annulus(k, inner=1.0, outer=2.0, centre=(0.0, 0.0, 0.0)):
    """k vertices on each of two circles in the plane z = centre_z and 2 k triangles, counter-clockwise seen from +z: the inner circle is a
    hole (vertices 0 .. k - 1), the outer one the sheet's edge"""
    ang = 2.0 * np.pi * np.arange(k) / k
    ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(k)], 1)
    pos = (np.concatenate([inner * ring, outer * ring]) + np.array(centre)).astype(F)
    i = np.arange(k)
    j = (i + 1) % k
    return mesh(pos, np.concatenate([np.stack([i, k + i, k + j], 1), np.stack([i, k + j, j], 1)]))


def permuted(m, seed):
    """the same mesh with its vertices renumbered by a seeded permutation"""
    n = len(m["vertices"])
    perm = np.random.default_rng(seed).permutation(n)
    out = {k: None if m[k] is None else np.empty_like(m[k]) for k in ("vertices", "colours", "normals")}
    for k, a in out.items():
        if a is not None:
            a[perm] = m[k]
    return dict(out, triangles=perm[m["triangles"].astype(np.int64)].astype(U32))


def punched(m, centres):
    """the mesh without the triangles that name one of the vertices `centres` -> (mesh, triangles removed)"""
    gone = np.isin(m["triangles"], centres).any(1)
    return dict(m, triangles=np.ascontiguousarray(m["triangles"][~gone])), int(gone.sum())


def join(*parts):
    """meshes side by side, the indices of each shifted behind the vertices before it -> (mesh, the first vertex of every part)"""
    first = np.concatenate([[0], np.cumsum([len(p["vertices"]) for p in parts])])
    return mesh(np.concatenate([p["vertices"] for p in parts]),
                np.concatenate([p["triangles"].astype(np.int64) + o for p, o in zip(parts, first)])), [int(x) for x in first[:-1]]


def hand_mesh():
    """max_edges = 4 is what this mesh is about"""
    flat = lambda n, x: [(x + i, i % 2, 0) for i in range(n)]
    parts = [annulus(3),                                                              # 0 - 5: a hole of 3 (0 1 2) in a sheet (3 4 5)
             mesh(flat(5, 10), [(0, 1, 2), (0, 3, 4)]),                               # 6 - 10: two outlines that share vertex 6
             mesh(flat(4, 20), [(0, 1, 2), (0, 1, 3)]),                               # 11 - 14: the edge 11 -> 12 named twice in one direction
             mesh(flat(5, 30), [(0, 1, 2), (1, 0, 3), (0, 1, 4)]),                    # 15 - 19: the edge 15 16 in three triangles
             mesh(flat(3, 40), [(0, 0, 1), (2, 2, 2)]),                               # 20 - 22: (a, a, b) and (a, a, a)
             mesh([(NAN, 0, 0), (51, 0, 0), (50, 1, 0)], [(0, 1, 2)]),                # 23 - 25: a NaN on a loop
             mesh([(60, 0, 0), (61, -INF, 0), (60, 1, 0)], [(0, 1, 2)]),              # 26 - 28: an inf on a loop
             annulus(3, centre=(70, 0, 0)),                                           # 29 - 34: a hole of 3 whose owners name the NaN vertex 32
             annulus(4, centre=(80, 0, 0)),                                           # 35 - 42: a hole of exactly max_edges
             annulus(5, centre=(90, 0, 0))]                                           # 43 - 52: a hole of max_edges + 1
    m, first = join(*parts)
    assert first == [0, 6, 11, 15, 20, 23, 26, 29, 35, 43] and len(m["vertices"]) == 53
    m["vertices"][32, 1] = NAN
    col = np.full((53, 3), 7, U8)
    col[35:39] = [(1, 0, 255), (2, 0, 255), (2, 0, 255), (1, 1, 254)]                 # means 1.5, 0.25, 254.75 -> 2, 0, 255
    nrm = np.tile(np.array([0, 0, 1], F), (53, 1))
    nrm[35:39] = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)]                       # they cancel
    nrm[0:3] = [(0, 0, 2), (0, 3, 0), (0, 0, 2)]                                      # (0, 3, 4) / 5
    return dict(m, colours=col, normals=nrm)


def random_positions(n_v, seed):
    return np.random.default_rng(900 + seed).uniform(-1, 1, (n_v, 3)).astype(F)


def attributes(n_v, seed):
    rng = np.random.default_rng(300 + seed)
    return rng.integers(0, 256, (n_v, 3), dtype=U8), rng.normal(0, 1, (n_v, 3)).astype(F)


@functools.lru_cache(maxsize=None)
def all_cases():
    ts, hard = tsdf_meshes(), hard_meshes()
    sphere = mesh(ts["sphere"][0], ts["sphere"][2])
    cases = {"hand": hand_mesh(), "no_triangles": mesh([(0.1, 0.2, 0.3), (4, 5, 6), (NAN, 1, 2)], []), "no_vertices": mesh([], []),
             "sphere": sphere, "sphere_1": punched(sphere, [100])[0], "sphere_3": punched(sphere, [100, 900, 1500])[0],
             "sphere_40": punched(sphere, np.arange(0, 2002, 40))[0],
             "tetrahedron": mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], [(0, 2, 1), (0, 1, 3), (0, 3, 2)]),
             "noise": mesh(ts["noise"][0], ts["noise"][2]), "cut": mesh(ts["cut"][0], ts["cut"][2]),
             "strip": mesh(random_positions(hard["strip"][1], 1), hard["strip"][0]), "fan": mesh(random_positions(hard["fan"][1], 2), hard["fan"][0]),
             "many": mesh(random_positions(hard["many"][1], 3), hard["many"][0])}
    for k in ANNULI:
        cases[f"annulus_{k}"] = annulus(k)
        cases[f"annulus_{k}_permuted"] = permuted(annulus(k), k)
    for seed, (name, m) in enumerate(sorted(cases.items())):
        if m["colours"] is None:
            m["colours"], m["normals"] = attributes(len(m["vertices"]), seed)
    return cases


@functools.lru_cache(maxsize=None)
def table_of(name):
    """the vectorised mirror's loop table of a case, computed once and shared with the GPU tests"""
    m = all_cases()[name]
    return HM.plan(m["triangles"], len(m["vertices"]))


@functools.lru_cache(maxsize=None)
def selected(name, max_edges=64, any_facing=False):
    return HM.select(table_of(name), all_cases()[name]["vertices"], max_edges, any_facing)


@functools.lru_cache(maxsize=None)
def filled(name, max_edges=64, any_facing=False):
    """-> (vertices, colours, normals, triangles) with both attributes"""
    m = all_cases()[name]
    return HM.emit(table_of(name), selected(name, max_edges, any_facing), m["vertices"], m["colours"], m["normals"])


def figures(name, max_edges=64, any_facing=False):
    return dict(table_of(name)["counts"], **selected(name, max_edges, any_facing)["counts"])


def closed(tri):
    """-> (boundary half-edges, V - E + F over the vertices that are named) of a mesh"""
    t = HM.plan(tri, int(tri.max()) + 1 if len(tri) else 0)
    e = np.sort(np.concatenate([tri[:, (0, 1)], tri[:, (1, 2)], tri[:, (2, 0)]]).astype(np.int64), 1)
    return t["counts"]["boundary_half_edges"], len(np.unique(tri)) - len(np.unique(e, axis=0)) + len(tri)


# ---- mirror against loop ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(all_cases()))
def test_mirror_equals_the_loops(name):
    m = all_cases()[name]
    a, b = table_of(name), HM.plan_loop(m["triangles"], len(m["vertices"]))
    assert HM.same(a, b) == [], (name, HM.same(a, b), a["counts"], b["counts"])
    c = a["counts"]
    assert c["loop_edges"] + c["blocked"] == c["boundary_half_edges"] and len(a["vertices"]) == c["loop_edges"] and len(a["offsets"]) == c["loops"] + 1
    for max_edges, any_facing in ((64, False), (64, True), (3, False), (8, True)) if name != "many" else ((64, False),):      # 200 000 loops: one pass of the scalar form
        sa, sb = selected(name, max_edges, any_facing), HM.select_loop(b, m["vertices"], max_edges, any_facing)
        assert HM.same(sa, sb) == [], (name, max_edges, any_facing, HM.same(sa, sb), sa["counts"], sb["counts"])
        ea, eb = filled(name, max_edges, any_facing), HM.emit_loop(b, sb, m["vertices"], m["colours"], m["normals"])
        assert HM.same(ea, eb) == [], (name, max_edges, any_facing, HM.same(ea, eb))
        assert len(ea[0]) == len(m["vertices"]) + sa["counts"]["filled"] and len(ea[3]) == len(m["triangles"]) + sa["counts"]["new_triangles"]


def test_one_shot_without_attributes():
    m = all_cases()["sphere_3"]
    v, c, t, n, fig = HM.fill(m["vertices"], None, m["triangles"], None, 16)
    assert c is None and n is None and fig == figures("sphere_3", 16)
    assert v.tobytes() == filled("sphere_3", 16)[0].tobytes() and t.tobytes() == filled("sphere_3", 16)[3].tobytes()
    for bad in (2, 1 << 31):
        with pytest.raises(ValueError):
            HM.select(table_of("sphere_3"), m["vertices"], bad)
    for bad in ((0, 1, 2002), (0, 1, -1)):
        with pytest.raises(ValueError):
            HM.plan([bad], 2002)
        with pytest.raises(ValueError):
            HM.plan_loop([bad], 2002)


# ---- section 19's sphere -------------------------------------------------------------------------------------------------------------------
def test_the_sphere_as_it_is():
    m = all_cases()["sphere"]
    assert len(m["vertices"]) == 2002 and len(m["triangles"]) == 4000
    assert figures("sphere") == dict(directed_edges=12000, boundary_half_edges=0, boundary_vertices=0, non_simple=0, loops=0, loop_edges=0, blocked=0,
                                     longest=0, too_long=0, not_finite=0, outlines=0, filled=0, new_triangles=0)
    v, c, n, t = filled("sphere")
    assert v.tobytes() == m["vertices"].tobytes() and t.tobytes() == m["triangles"].tobytes() and c.tobytes() == m["colours"].tobytes()
    assert n.tobytes() == m["normals"].tobytes()


def test_one_vertex_removed():
    sphere = all_cases()["sphere"]
    assert punched(sphere, [100])[1] == 7
    f = figures("sphere_1", 16)
    assert (f["loops"], f["longest"], f["filled"], f["new_triangles"], f["blocked"], f["non_simple"]) == (1, 7, 1, 7, 0, 0)
    v, _, _, t = filled("sphere_1", 16)
    assert closed(t) == (0, 2) and len(t) == 4000 and len(v) == 2003
    vol, whole = signed_volume(v, t), signed_volume(sphere["vertices"], sphere["triangles"])
    print("signed volume: filled", vol, "closed sphere", whole)               # measured: 0.1115171 against 0.1115180
    assert abs(vol - 0.1115171) < 5e-8 and abs(whole - 0.1115180) < 5e-8


def test_three_vertices_removed():
    tab, f = table_of("sphere_3"), figures("sphere_3", 16)
    assert sorted(np.diff(tab["offsets"].astype(np.int64)).tolist()) == [6, 6, 7] and (f["filled"], f["new_triangles"]) == (3, 19)
    assert closed(filled("sphere_3", 16)[3]) == (0, 2)


def test_every_40th_vertex_removed():
    assert punched(all_cases()["sphere"], np.arange(0, 2002, 40))[1] == 310 and len(np.arange(0, 2002, 40)) == 51
    f = figures("sphere_40", 16)
    assert (f["boundary_half_edges"], f["boundary_vertices"] - f["non_simple"], f["non_simple"]) == (304, 298, 3)
    assert (f["loops"], f["loop_edges"], f["filled"], f["new_triangles"], f["blocked"], f["outlines"], f["too_long"]) == (42, 257, 42, 257, 47, 0, 0)
    assert closed(filled("sphere_40", 16)[3])[0] == 47                          # the blocked ones, where two holes touch, stay


@pytest.mark.parametrize("name", ["sphere_1", "sphere_3", "sphere_40", "hand", "noise"])
def test_filling_again_fills_nothing_more(name):
    v, c, n, t = filled(name, 16)
    tab = HM.plan(t, len(v))
    sel = HM.select(tab, v, 16)
    first = figures(name, 16)
    assert tab["counts"]["loops"] == first["loops"] - first["filled"] and tab["counts"]["blocked"] == first["blocked"]
    if name.startswith("sphere"):
        assert sel["counts"]["filled"] == 0 and tab["counts"]["loops"] == 0
    again = HM.emit(tab, sel, v, c, n)
    if sel["counts"]["filled"] == 0:
        assert HM.same(again, (v, c, n, t)) == []


# ---- annuli and the tetrahedron --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ANNULI)
def test_annulus(k):
    for name in (f"annulus_{k}", f"annulus_{k}_permuted"):
        tab, m = table_of(name), all_cases()[name]
        assert tab["counts"] == dict(directed_edges=6 * k, boundary_half_edges=2 * k, boundary_vertices=2 * k, non_simple=0, loops=2, loop_edges=2 * k,
                                     blocked=0, longest=k)
        assert selected(name, max(k, 3))["counts"] == dict(too_long=0, not_finite=0, outlines=1, filled=1, new_triangles=k)
        assert selected(name, max(k, 3), True)["counts"] == dict(too_long=0, not_finite=0, outlines=0, filled=2, new_triangles=2 * k)
        if k > 3:
            assert selected(name, k - 1, True)["counts"] == dict(too_long=2, not_finite=0, outlines=0, filled=0, new_triangles=0)
        v, _, _, t = filled(name, max(k, 3))
        radius = np.linalg.norm(m["vertices"][tab["vertices"][tab["offsets"][selected(name, max(k, 3))["status"].argmin()]]])
        assert abs(radius - 1.0) < 1e-6                                          # the inner circle is the one that is filled
        assert np.abs(v[-1]).max() < 1e-6 and HM.plan(t, len(v))["counts"]["loops"] == 1
        new = v[t[-k:].astype(np.int64)].astype(np.float64)                      # the fan faces +z as the sheet does
        assert (np.cross(new[:, 1] - new[:, 0], new[:, 2] - new[:, 0])[:, 2] > 0).all()


def test_the_order_of_the_centre_sum_shows():
    """the same circle summed from another first vertex and in the same direction has other bits: what the permuted cases are for"""
    a, b = selected("annulus_64", 64, True), selected("annulus_64_permuted", 64, True)
    print("centres as built", a["centres"].tolist(), "permuted", b["centres"].tolist())
    assert a["centres"].tobytes() != b["centres"].tobytes() and np.abs(a["centres"]).max() < 1e-15 and np.abs(b["centres"]).max() < 1e-15


def test_open_tetrahedron():
    assert figures("tetrahedron") == dict(directed_edges=9, boundary_half_edges=3, boundary_vertices=3, non_simple=0, loops=1, loop_edges=3, blocked=0,
                                          longest=3, too_long=0, not_finite=0, outlines=1, filled=0, new_triangles=0)
    assert figures("tetrahedron", 64, True)["filled"] == 1 and closed(filled("tetrahedron", 64, True)[3]) == (0, 2)
    assert table_of("tetrahedron")["vertices"].tolist() == [1, 3, 2] and table_of("tetrahedron")["owners"].tolist() == [4, 7, 1]


# ---- the meshes of the other stages ---------------------------------------------------------------------------------------------------------
def test_many_separate_triangles():
    f = figures("many")
    assert (f["loops"], f["outlines"], f["filled"], f["longest"], f["blocked"]) == (200000, 200000, 0, 3, 0)
    f = figures("many", 64, True)
    v, _, _, t = filled("many", 64, True)
    assert (f["filled"], f["new_triangles"]) == (200000, 600000) and len(v) == 800000 and len(t) == 800000


def test_noise_cut_strip_and_fan():
    f = figures("noise")
    assert (f["boundary_half_edges"], f["non_simple"], f["loops"], f["longest"]) == (2572, 30, 207, 56)
    assert (f["outlines"], f["filled"], f["new_triangles"], f["too_long"]) == (204, 3, 32, 0)
    f = figures("noise", 8)
    assert (f["too_long"], f["outlines"], f["filled"], f["new_triangles"]) == (69, 136, 2, 12)
    assert np.diff(table_of("cut")["offsets"].astype(np.int64)).tolist() == [78, 78] and figures("cut")["too_long"] == 2
    for name, half_edges in (("strip", 5002), ("fan", 12288)):
        c = table_of(name)["counts"]
        assert c["loops"] == 0 and c["blocked"] == c["boundary_half_edges"] == half_edges and c["non_simple"] > 0
    assert table_of("no_triangles")["counts"] == dict.fromkeys(HM.PLAN_COUNTS, 0) and table_of("no_vertices")["offsets"].tolist() == [0]


# ---- the hand-built mesh -------------------------------------------------------------------------------------------------------------------
def test_hand_built_loops():
    tab = table_of("hand")
    # the directed edges: 6 + 8 + 10 triangles of the annuli, 2 + 2 + 3 + 1 + 1 others, three each; the degenerate two give none
    assert tab["counts"] == dict(directed_edges=3 * (6 + 6 + 8 + 10 + 9), boundary_half_edges=6 + 6 + 4 + 6 + 3 + 3 + 6 + 8 + 10, boundary_vertices=53 - 3,
                                 non_simple=1 + 2 + 2, loops=10, loop_edges=6 + 3 + 3 + 6 + 8 + 10, blocked=6 + 4 + 6, longest=5)
    off, lv = tab["offsets"].tolist(), tab["vertices"].tolist()
    loops = [lv[a:b] for a, b in zip(off, off[1:])]
    assert loops == [[0, 2, 1], [3, 4, 5], [23, 24, 25], [26, 27, 28], [29, 31, 30], [32, 33, 34], [35, 38, 37, 36], [39, 40, 41, 42],
                     [43, 47, 46, 45, 44], [48, 49, 50, 51, 52]]
    # the owners: the hole's edge 0 -> 2 belongs to the triangle (2, 3 + 2, 0) ... of the second half, corner 2; the lone triangles own theirs
    tri = all_cases()["hand"]["triangles"].reshape(-1).tolist()
    for l, k in zip(loops, tab["owners"].tolist()[:0] or [tab["owners"].tolist()[a:b] for a, b in zip(off, off[1:])]):
        for i, v in enumerate(l):
            c = k[i]
            assert tri[c] == v and tri[3 * (c // 3) + (c % 3 + 1) % 3] == l[(i + 1) % len(l)]
    assert tab["owners"].tolist()[6:12] == [3 * 15, 3 * 15 + 1, 3 * 15 + 2, 3 * 16, 3 * 16 + 1, 3 * 16 + 2]


def test_hand_built_select_and_emit():
    O, T, N, FL = HM.OUTLINE, HM.TOO_LONG, HM.NOT_FINITE, HM.FILLED
    sel = selected("hand", 4)
    assert sel["status"].tolist() == [FL, O, N, N, O, N, FL, O, T, T]           # the non-finite owner makes loop 4 an outline
    assert sel["counts"] == dict(too_long=2, not_finite=3, outlines=3, filled=2, new_triangles=7)
    assert selected("hand", 4, True)["status"].tolist() == [FL, FL, N, N, FL, N, FL, FL, T, T]
    assert selected("hand", 5)["status"].tolist() == [FL, O, N, N, O, N, FL, O, FL, O] and selected("hand", 3)["status"].tolist()[6:] == [T] * 4
    m = all_cases()["hand"]
    v, c, n, t = filled("hand", 4)
    assert len(v) == 55 and len(t) == len(m["triangles"]) + 7
    assert t[-7:].tolist() == [[2, 0, 53], [1, 2, 53], [0, 1, 53], [38, 35, 54], [37, 38, 54], [36, 37, 54], [35, 36, 54]]
    assert np.abs(v[53]).max() < 1e-7 and np.abs(v[54] - np.array([80, 0, 0], F)).max() < 1e-5
    assert c[53].tolist() == [7, 7, 7] and c[54].tolist() == [2, 0, 255]         # 1.5 rounds up, 0.25 down, 254.75 up
    assert n[54].tolist() == [0, 0, 0] and n[53].tolist() == [0, F(0.6), F(0.8)]
    assert v[:53].tobytes() == m["vertices"].tobytes() and t[:-7].tobytes() == m["triangles"].tobytes()


# ---- the Python checkers, one by one ------------------------------------------------------------------------------------------------------
def test_checkers():
    assert HO.capacity_arg(1, 1) == (1, 1) and HO.capacity_arg(1 << 31, np.int64(1 << 29)) == (1 << 31, 1 << 29)
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 1), (1, (1 << 29) + 1), (-1, 1), (1.0, 1), (1, "1"), (None, 1), (True, 1)):
        with pytest.raises(ValueError):
            HO.capacity_arg(v, t)
    assert HO.max_edges_arg(3) == 3 and HO.max_edges_arg(np.int64((1 << 31) - 1)) == (1 << 31) - 1
    for n in (2, 0, -1, 1 << 31, 64.0, "64", None, True):
        with pytest.raises(ValueError):
            HO.max_edges_arg(n)
    assert HO.fill_holes_arg(None) is None and HO.fill_holes_arg(16) == dict(max_edges=16, any_facing=False)
    assert HO.fill_holes_arg(dict(max_edges=3, any_facing=True)) == dict(max_edges=3, any_facing=True)
    for bad in (2, 1 << 31, 1.5, "3", dict(any_facing=True), dict(max_edges=8, facing=1), dict(max_edges=8, any_facing=1), dict(max_edges=2)):
        with pytest.raises(ValueError):
            HO.fill_holes_arg(bad)


def test_mesh_and_attribute_checkers_need_cuda_tensors():
    import torch
    ht = torch.zeros((4, 3), dtype=torch.int32)
    for t, n in ((ht, 5), (ht.numpy(), 5), (None, 5)):
        with pytest.raises(ValueError):
            HO.mesh_arg(t, n)
    hv = torch.zeros((4, 3), dtype=torch.float32)
    for args in ((hv, None, None, 4), (None, None, None, 0), (hv.numpy(), None, None, 4)):
        with pytest.raises(ValueError):
            HO.attributes_arg(*args)


def test_checks_come_before_the_library():
    for v, t in ((0, 1), (1, 0), ((1 << 31) + 1, 4), (4, (1 << 29) + 1)):
        with pytest.raises(ValueError):
            HO.Filler(None, v, t)

    class Ctx:
        device = 0
    fl = HO.Filler.__new__(HO.Filler)
    fl.ctx, fl.max_vertices, fl.max_triangles, fl._triangles, fl.counts, fl.n_vertices, fl.selected = Ctx(), 10, 10, None, None, 0, None
    with pytest.raises(ValueError):
        fl.plan(np.zeros((1, 3), np.int32), 3)
    for call in (lambda: fl.select(None), lambda: fl.loops(), lambda: fl.loops(status=True), lambda: fl.emit(None, None)):
        with pytest.raises(ValueError):
            call()                                                  # nothing is planned
    fl._triangles = np.zeros((1, 3), np.int32)
    for call in (lambda: fl.loops(status=True), lambda: fl.emit(None, None)):
        with pytest.raises(ValueError):
            call()                                                  # nothing is selected
    for k in (2, 1 << 31, 8.0):
        with pytest.raises(ValueError):
            fl.select(None, k)
        with pytest.raises(ValueError):
            HO.fill_holes(None, None, None, None, None, k)
    with pytest.raises(ValueError):
        HO.fill_holes(None, None, None, None, None)                 # no tensors
    fl._h = None
    kf = [dict(R=np.eye(3), t=np.zeros(3), depthinv=None)]
    for f in (2, 1.5, dict(any_facing=True), dict(max_edges=8, any_facing=3)):
        with pytest.raises(ValueError):
            TS.fuse(None, kf, (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), fill_holes=f)
    vol = TS.Volume.__new__(TS.Volume)
    vol.ctx, vol.max_views, vol.max_voxels = Ctx(), 2, 1000
    for f in (2, dict(max_edges=1 << 31)):
        with pytest.raises(ValueError):
            vol.extract(1, fill_holes=f)
    vol._h = None


def test_nothing_is_imported_without_the_option():
    """fuse checks its options before it looks at the keyframes: without fill_holes the module is not imported, with it it is"""
    code = ("import sys; sys.path[:0] = [%r, %r]; from rgbid import tsdf as TS\n"
            "def fuse(**kw):\n"
            "    try:\n"
            "        TS.fuse(None, [], (60.0, 58.0, 31.5, 23.5), 48, 64, bounds=(0, 0, 0, 1, 1, 1), **kw)\n"
            "    except ValueError as e:\n"
            "        assert 'no keyframes' in str(e), e\n"
            "fuse(); fuse(fill_holes=None, smooth=None); assert 'rgbid.holes' not in sys.modules\n"
            "fuse(fill_holes=3); assert 'rgbid.holes' in sys.modules\n") % (ROOT, os.path.join(ROOT, "rgbid-slam_amd"))
    subprocess.check_call([sys.executable, "-c", code])


# ---- the boundary -------------------------------------------------------------------------------------------------------------------------
def _lib_handle():
    _lib.build()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_compiles_as_c99(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler on this machine")
    src = tmp_path / "use_holes.c"
    src.write_text('#include "rgbid_holes.h"\n'
                   "int use(rgbid_holes* h, rgbid_ctx* ctx, const float* v, const uint8_t* c, const float* n, const uint32_t* tris, float* vo, uint8_t* co,\n"
                   "        float* no, uint32_t* to, uint32_t* off, uint32_t* lv, uint32_t* lo, uint8_t* st) {\n"
                   "  unsigned long long counts[8], chosen[5]; float ms[3];\n"
                   "  return rgbid_holes_create(&h, ctx, RGBID_HOLES_MAX_VERTICES, RGBID_HOLES_MAX_TRIANGLES)\n"
                   "       + rgbid_holes_plan(h, 10, 5, tris, counts)\n"
                   "       + rgbid_holes_select(h, v, RGBID_HOLES_MAX_EDGES, RGBID_HOLES_ANY_FACING, chosen)\n"
                   "       + rgbid_holes_loops(h, off, lv, lo, st, counts[5])\n"
                   "       + rgbid_holes_emit(h, v, c, n, tris, vo, co, no, to, 10 + chosen[3], 5 + chosen[4])\n"
                   "       + rgbid_holes_timing(h, 1, ms) + rgbid_holes_destroy(h)\n"
                   "       + (int)(RGBID_HOLES_FILLED + RGBID_HOLES_TOO_LONG + RGBID_HOLES_NOT_FINITE + RGBID_HOLES_OUTLINE + RGBID_HOLES_MIN_EDGES); }\n")
    subprocess.check_call([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    txt = open(os.path.join(ROOT, "include", "rgbid_holes.h")).read()
    num = lambda name, suffix: int(re.search(r"RGBID_HOLES_%s\s+(\d+)%s" % (name, suffix), txt).group(1))
    assert num("MAX_VERTICES", "ull") == HO.MAX_VERTICES == HM.MAX_VERTICES == 1 << 31
    assert num("MAX_TRIANGLES", "ull") == HO.MAX_TRIANGLES == HM.MAX_TRIANGLES == 1 << 29
    assert num("MIN_EDGES", "u") == HO.MIN_EDGES == 3 and num("MAX_EDGES", "u") == HO.MAX_EDGES == (1 << 31) - 1 and num("ANY_FACING", "u") == HO.ANY_FACING
    for name in ("FILLED", "TOO_LONG", "NOT_FINITE", "OUTLINE"):
        assert num(name, "u") == getattr(HO, name) == getattr(HM, name)
    assert HO.PLAN_COUNTS == HM.PLAN_COUNTS and HO.SELECT_COUNTS == HM.SELECT_COUNTS


def test_library_exports_holes_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rgbid_holes.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rgbid_holes_[a-z0-9_]+)\s*\(", txt)))
    assert set(declared) == set(HO.EXPORTS) and len(declared) == 7, set(declared) ^ set(HO.EXPORTS)
    L = _lib_handle()
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing


def test_refusals_before_any_device_call():
    L = _lib_handle()
    c = ctypes
    for name, types in HO.SIGNATURES.items():
        getattr(L, name).argtypes = list(types)
    h = c.c_void_p()
    assert L.rgbid_holes_create(c.byref(h), None, 10, 10) == -1 and not h.value and L.rgbid_holes_create(None, None, 10, 10) == -1
    fake = c.c_void_p(8)                                    # never dereferenced: the capacities are refused first
    for v, t in ((0, 10), (10, 0), ((1 << 31) + 1, 10), (10, (1 << 29) + 1)):
        assert L.rgbid_holes_create(c.byref(h), fake, v, t) == -1 and not h.value
    assert L.rgbid_holes_plan(None, 0, 0, None, None) == -1 and L.rgbid_holes_loops(None, None, None, None, None, 0) == -1
    assert L.rgbid_holes_select(None, None, 64, 0, None) == -1
    assert L.rgbid_holes_emit(None, None, None, None, None, None, None, None, None, 0, 0) == -1
    assert L.rgbid_holes_timing(None, 0, None) == -1 and L.rgbid_holes_destroy(None) == 0


def test_cli_option_errors(tmp_path):
    tool = os.path.join(ROOT, "tools", "track_dataset.py")
    mesh_opt = ["--mesh", str(tmp_path / "m.ply")]
    for bad, word in ((["--mesh-fill-holes", "16"], "--mesh-fill-holes needs --mesh"),
                      (mesh_opt + ["--mesh-fill-any-facing"], "--mesh-fill-any-facing needs --mesh-fill-holes"),
                      (mesh_opt + ["--mesh-fill-holes", "2"], "max_edges must lie in"), (mesh_opt + ["--mesh-fill-holes", "2147483648"], "max_edges must lie in"),
                      (mesh_opt + ["--mesh-fill-holes", "x"], "invalid int value")):
        r = subprocess.run([sys.executable, tool, str(tmp_path)] + bad, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and word in r.stderr, (bad, r.stderr[-500:])
    assert not (tmp_path / "m.ply").exists()


def test_filled_mesh_through_the_ply_writer(tmp_path):
    v, c, n, t = filled("sphere_40", 16)
    path = tmp_path / "filled.ply"
    TS.write_mesh_ply(str(path), v, c, t, n)
    pv, pc, pt, pn = TS.read_mesh_ply(path.read_bytes())
    assert pv.tobytes() == v.tobytes() and pc.tobytes() == c.tobytes() and pt.tobytes() == t.tobytes() and pn.tobytes() == n.tobytes()
    assert len(pt) == 4000 - 310 + 257 and len(pv) == 2002 + 42
